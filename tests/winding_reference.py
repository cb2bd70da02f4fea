"""K40 restated in numpy (the comment of K40 in include/gens_hip.h is the definition): the exact generalised winding number as a
np.longdouble sum of Van Oosterom-Strackee solid angles over all faces, the moments of the leaves (64 faces of the plan order) and nodes
(64 leaves) in float64 in the kernel's order, and the far-field traversal with its bound -- decisions in float64 as the kernel takes them,
sums in longdouble.  Shared by tests/test_winding_cpu.py and tests/test_hip_winding.py, which also take their shapes and queries from here.

The rounding bracket of a float64 result, per query:  tol = 16 * 2^-53 * sum_f (1 + 4 |A||B||C| / hypot(num_f, den_f)) / (4 pi), in
longdouble.  atan2(num, den) moves by at most |d num| |den| + |d den| |num| over num^2 + den^2 <= (|d num| + |d den|) / hypot; num and
den are sums of a few products of magnitude <= |A||B||C| each carrying a handful of roundings, so their absolute errors are a small multiple
of 2^-53 |A||B||C| -- the second term, with room for about ten roundings --; the first term covers atan2's own rounding and the face's share
of the accumulation (each |Omega| <= 2 pi, each partial sum of the tree is rounded once per addition)."""
import math

import numpy as np

LEAF = 64
LD = np.longdouble
FOUR_PI = 4.0 * np.arctan2(LD(0.0), LD(-1.0))


def face_valid(vertices, triangles):
    nv = len(np.asarray(vertices).reshape(-1, 3))
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    return ((t >= 0) & (t < nv)).all(axis=1) & (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 2] != t[:, 0])


def omegas(vertices, triangles, queries, block=64):
    """-> (omega (n, T) longdouble: every face's solid angle at every query, 0 for faces that are not valid; term (n, T) longdouble: the
    face's summand of the rounding bracket, 0 likewise).  Queries must be finite."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3).astype(LD)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    q = np.asarray(queries, dtype=np.float64).reshape(-1, 3).astype(LD)
    ok = face_valid(vertices, triangles)
    omega = np.zeros((len(q), len(t)), dtype=LD)
    term = np.zeros((len(q), len(t)), dtype=LD)
    if not ok.any():
        return omega, term
    corners = [v[t[ok, k]] for k in range(3)]
    for s in range(0, len(q), block):
        a, b, c = (x[None] - q[s:s + block, None] for x in corners)
        la, lb, lc = (np.sqrt((x * x).sum(-1)) for x in (a, b, c))
        num = (a * np.cross(b, c)).sum(-1)
        den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
        omega[s:s + block, ok] = 2.0 * np.arctan2(num, den)
        hyp = np.hypot(num, den)
        with np.errstate(divide="ignore", invalid="ignore"):
            term[s:s + block, ok] = np.where(hyp > 0, 1.0 + 4.0 * la * lb * lc / hyp, np.inf)
    return omega, term


def bracket(term):
    """The rounding bracket (n) float64 from omegas()' terms."""
    return np.asarray(16.0 * LD(2.0) ** -53 * term.sum(axis=1) / FOUR_PI, dtype=np.float64)


def exact(vertices, triangles, queries):
    """-> (w (n) longdouble, tol (n) float64): the exact winding number and the rounding bracket of a float64 evaluation.  NaN for a query
    that is not finite."""
    q = np.asarray(queries, dtype=np.float64).reshape(-1, 3)
    fin = np.isfinite(q).all(axis=1)
    w = np.full(len(q), np.nan, dtype=LD)
    tol = np.full(len(q), np.nan)
    if fin.any():
        omega, term = omegas(vertices, triangles, q[fin])
        w[fin] = omega.sum(axis=1) / FOUR_PI
        tol[fin] = bracket(term)
    return w, tol


def _cross(u, v):
    return np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]])


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _centre(area, s, m, count):
    return s / area if area > 0.0 else m / float(count)


def moments(vertices, triangles, face_order):
    """The leaves' and nodes' moments over the given order, float64 in the kernel's order of operations -> dict: leaf_count (L) int32,
    leaf_area (L), leaf_normal (L, 3), leaf_centre (L, 3), leaf_radius2 (L), the same as node_*, and node_true_radius (K): the largest
    distance from the node's centre to a corner of its valid faces."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    order = np.asarray(face_order, dtype=np.int64).reshape(-1)
    ok = face_valid(v, t)
    nt = len(t)
    nl = -(-nt // LEAF)
    nk = -(-nl // LEAF)
    out = {"leaf_count": np.zeros(nl, np.int32), "leaf_area": np.zeros(nl), "leaf_normal": np.zeros((nl, 3)), "leaf_centre": np.zeros((nl, 3)),
           "leaf_radius2": np.zeros(nl), "node_count": np.zeros(nk, np.int32), "node_area": np.zeros(nk), "node_normal": np.zeros((nk, 3)),
           "node_centre": np.zeros((nk, 3)), "node_radius2": np.zeros(nk), "node_true_radius": np.zeros(nk)}
    for l in range(nl):
        area, normal, s, m, count, corners = 0.0, np.zeros(3), np.zeros(3), np.zeros(3), 0, []
        for f in order[LEAF * l:LEAF * (l + 1)]:
            if not (0 <= f < nt and ok[f]):
                continue
            a, b, c = v[t[f, 0]], v[t[f, 1]], v[t[f, 2]]
            n = _cross(b - a, c - a)
            af = 0.5 * math.sqrt(_dot(n, n))
            g = ((a + b) + c) / 3.0
            area, normal, s, m, count = area + af, normal + 0.5 * n, s + af * g, m + g, count + 1
            corners += [a, b, c]
        out["leaf_count"][l] = count
        if count:
            p = _centre(area, s, m, count)
            out["leaf_area"][l], out["leaf_normal"][l], out["leaf_centre"][l] = area, normal, p
            out["leaf_radius2"][l] = max(_dot(x - p, x - p) for x in corners)
    for k in range(nk):
        leaves = [l for l in range(LEAF * k, min(LEAF * (k + 1), nl)) if out["leaf_count"][l] > 0]
        area, normal, s, m, count = 0.0, np.zeros(3), np.zeros(3), np.zeros(3), 0
        for l in leaves:
            al, pl, cl = out["leaf_area"][l], out["leaf_centre"][l], int(out["leaf_count"][l])
            area, normal, s, m, count = area + al, normal + out["leaf_normal"][l], s + al * pl, m + float(cl) * pl, count + cl
        out["node_count"][k] = count
        if count:
            p = _centre(area, s, m, count)
            out["node_area"][k], out["node_normal"][k], out["node_centre"][k] = area, normal, p
            r = max(math.sqrt(_dot(out["leaf_centre"][l] - p, out["leaf_centre"][l] - p)) + math.sqrt(out["leaf_radius2"][l]) for l in leaves)
            out["node_radius2"][k] = r * r
            faces = [f for l in leaves for f in order[LEAF * l:LEAF * (l + 1)] if 0 <= f < nt and ok[f]]
            out["node_true_radius"][k] = max(float(np.linalg.norm(v[t[f]] - p, axis=1).max()) for f in faces)
    return out


def _far(q, beta2, area, normal, centre, radius2):
    """One cluster against all queries, float64 as the kernel: -> (accepted (n) bool, dipole (n), err (n), margin (n))."""
    d = centre[None] - q
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    far = d2 > beta2 * radius2
    with np.errstate(divide="ignore", invalid="ignore"):
        margin = np.abs(d2 - beta2 * radius2) / d2
        dist, r = np.sqrt(d2), math.sqrt(radius2)
        g = dist - r
        dipole = ((normal[0] * d[:, 0] + normal[1] * d[:, 1]) + normal[2] * d[:, 2]) / (d2 * dist)
        err = (area * r) / (2.0 * math.pi * ((g * g) * g))
    return far, dipole, err, margin


def traverse(omega, face_order, m, queries, beta):
    """K40's traversal over a plan that is GIVEN (face_order and the moments m, e.g. read back from the device): omega = omegas()[0] of the
    same mesh and (finite) queries.  The accept decisions in float64 as the kernel takes them, the sums in longdouble.
    -> dict: w (n) longdouble, bound (n) float64, far (n): clusters accepted, margin (n): the smallest |d2 - beta2 r2| / d2 over the tests
    made (inf if none), node_accepts and leaf_accepts (n)."""
    q = np.asarray(queries, dtype=np.float64).reshape(-1, 3)
    order = np.asarray(face_order, dtype=np.int64).reshape(-1)
    n, nt = len(q), omega.shape[1]
    beta2 = float(beta) * float(beta)
    total, bound = np.zeros(n, dtype=LD), np.zeros(n)
    node_acc, leaf_acc, margin = np.zeros(n, np.int64), np.zeros(n, np.int64), np.full(n, np.inf)
    nl = len(m["leaf_count"])
    for k in range(len(m["node_count"])):
        if m["node_count"][k] <= 0:
            continue
        part = np.zeros(n, dtype=LD)
        open_ = np.ones(n, dtype=bool)
        if beta2 > 0.0:
            far, dipole, err, mg = _far(q, beta2, m["node_area"][k], m["node_normal"][k], m["node_centre"][k], m["node_radius2"][k])
            margin = np.minimum(margin, mg)
            part[far], open_ = dipole[far], ~far
            bound[far] = bound[far] + err[far]
            node_acc += far
        for l in range(LEAF * k, min(LEAF * (k + 1), nl)):
            if m["leaf_count"][l] <= 0 or not open_.any():
                continue
            near = open_.copy()
            leaf = np.zeros(n, dtype=LD)
            if beta2 > 0.0:
                far, dipole, err, mg = _far(q, beta2, m["leaf_area"][l], m["leaf_normal"][l], m["leaf_centre"][l], m["leaf_radius2"][l])
                far &= open_
                margin[open_] = np.minimum(margin[open_], mg[open_])
                leaf[far], near = dipole[far], open_ & ~far
                bound[far] = bound[far] + err[far]
                leaf_acc += far
            faces = [f for f in order[LEAF * l:LEAF * (l + 1)] if 0 <= f < nt]
            if near.any():
                leaf[near] = omega[np.ix_(near, faces)].sum(axis=1)
            part[open_] = part[open_] + leaf[open_]
        total = total + part
    return {"w": total / FOUR_PI, "bound": bound, "far": node_acc + leaf_acc, "margin": margin, "node_accepts": node_acc, "leaf_accepts": leaf_acc}


def inside(w, bound):
    """ops.mesh_inside's rule -> (n) int8."""
    w, bound = np.asarray(w, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    out = np.full(len(w), -1, dtype=np.int8)
    out[w - bound >= 0.5] = 1
    out[w + bound < 0.5] = 0
    return out


def morton_order(vertices, triangles):
    """A plan order by the definition's (3), for CPU-only checks of the traversal: stable sort of 30-bit Morton keys, faces that are not valid last."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    ok = face_valid(v, t)
    key = np.full(len(t), 1 << 30, dtype=np.int64)
    if ok.any():
        g = ((v[t[ok, 0]] + v[t[ok, 1]]) + v[t[ok, 2]]) / 3.0
        lo, span = g.min(axis=0), g.max(axis=0) - g.min(axis=0)
        span = np.where(span > 0, span, 1.0)
        cell = np.clip(np.floor((g - lo) / span * 1024.0), 0, 1023).astype(np.int64)
        bits = np.zeros(len(g), dtype=np.int64)
        for b in range(10):
            for axis in range(3):
                bits |= ((cell[:, axis] >> b) & 1) << (3 * b + 2 - axis)
        key[ok] = bits
    return np.argsort(key, kind="stable").astype(np.int32)


# ------------------------------------------------------------------------------------------------ shapes and queries
def planar_strip(n):
    """n triangles in the plane z = 0, alternating so that all normals point to +z."""
    v = np.array([[0.5 * i, float(i % 2), 0.0] for i in range(n + 2)])
    return v, np.array([(i, i + 1, i + 2) if i % 2 == 0 else (i + 1, i, i + 2) for i in range(n)], dtype=np.int32)


def without_cap(mesh, z=0.5):
    """The mesh without the faces whose centroid lies above z."""
    v, t = mesh
    return v, t[v[t].mean(axis=1)[:, 2] <= z].copy()


def query_stream(vertices, seed):
    """An endless seeded stream of blocks of 256 uniform points in 1.5 x the bounding box of the vertices about its centre; an axis along
    which the box is thinner than a tenth of its diagonal is widened to that, so that the queries of a planar mesh do not lie in its plane
    (where the sign of a zero decides between +-2 pi)."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    lo, hi = (v.min(axis=0), v.max(axis=0)) if len(v) else (np.zeros(3), np.ones(3))
    diag = float(np.linalg.norm(hi - lo)) or 1.0
    half = 0.75 * np.maximum(hi - lo, 0.1 * diag)
    mid = 0.5 * (lo + hi)
    rng = np.random.default_rng(seed)
    while True:
        yield mid + rng.uniform(-1.0, 1.0, size=(256, 3)) * half


def queries_with_bracket(vertices, triangles, n, seed, limit=1e-9):
    """n queries of query_stream whose rounding bracket is below `limit` (the reference alone decides; a query that breaks it is replaced by
    the next of the stream) -> (queries (n, 3), omega (n, T), tol (n))."""
    stream = query_stream(vertices, seed)
    qs, oms, tols, have = [], [], [], 0
    for _ in range(64):
        block = next(stream)
        omega, term = omegas(vertices, triangles, block)
        tol = bracket(term)
        keep = tol < limit
        qs.append(block[keep]), oms.append(omega[keep]), tols.append(tol[keep])
        have += int(keep.sum())
        if have >= n:
            break
    assert have >= n, "the query stream does not yield enough queries inside the bracket"
    return np.concatenate(qs)[:n].copy(), np.concatenate(oms)[:n].copy(), np.concatenate(tols)[:n].copy()
