"""K39 restated in numpy / Python float64 (the comment of K39 in include/gens_hip.h is the definition): the neighbour lists, the uniform and
cotangent weights, the vertex Laplacian, a step, Laplacian and Taubin smoothing with its stats, and the dihedral roughness, as brute force
with dicts and loops -- every operation rounded on its own, in the order written.  Shared by tests/test_mesh_smooth_cpu.py and
tests/test_hip_mesh_smooth.py, which take their shapes from here, from mesh_repair_reference.py and from mesh_topology_reference.py."""
import math

import numpy as np

from . import mesh_topology_reference as TR

STAT_KEYS = ("iterations", "weights", "pinned", "moved", "displacement_max", "displacement_mean", "displacement_rms")
MEASURE_KEYS = ("area_before", "area_after", "volume_before", "volume_after", "roughness_before", "roughness_after")
NAN = float("nan")


def neighbours(edges, n_vertices):
    """Definition 1 -> (nbr_start (V + 1) int32, nbr_vertex (2 E) int32, nbr_edge (2 E) int32)."""
    at = [{} for _ in range(n_vertices)]
    for e, (lo, hi) in enumerate(np.asarray(edges).reshape(-1, 2).tolist()):
        at[lo][hi] = e
        at[hi][lo] = e
    start, vertex, edge = [0], [], []
    for i in range(n_vertices):
        for j in sorted(at[i]):
            vertex.append(j)
            edge.append(at[i][j])
        start.append(len(vertex))
    return (np.array(start, dtype=np.int32).reshape(-1), np.array(vertex, dtype=np.int32).reshape(-1), np.array(edge, dtype=np.int32).reshape(-1))


def corner_cot(vertices, triangles, face_valid):
    """Definition 2 -> cot (3 T) float64."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3).tolist()
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3).tolist()
    cot = np.zeros(3 * len(t))
    for f, face in enumerate(t):
        if not face_valid[f]:
            continue
        for k in range(3):
            p, q, r = v[face[(k + 2) % 3]], v[face[k]], v[face[(k + 1) % 3]]
            u = [q[a] - p[a] for a in range(3)]
            w = [r[a] - p[a] for a in range(3)]
            d = (u[0] * w[0] + u[1] * w[1]) + u[2] * w[2]
            n = [u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]]
            with np.errstate(all="ignore"):
                ln = float(np.sqrt(np.float64((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])))
                c = float(np.float64(d) / np.float64(ln)) if ln > 0.0 else 0.0
            cot[3 * f + k] = c if math.isfinite(c) else 0.0
    return cot


def edge_weights(topo, cot=None, kind="uniform"):
    """Definition 2 -> (weight (E) float64, the sum of |cot_h| per edge, which bounds the rounding of the ordered sum)."""
    ne = len(topo["edges"])
    if kind == "uniform":
        return np.ones(ne), np.zeros(ne)
    w, mag = [0.0] * ne, [0.0] * ne
    for h, e in enumerate(topo["edge_of_halfedge"].tolist()):          # ascending h: the order of an edge's uses
        if e >= 0:
            with np.errstate(all="ignore"):
                w[e] = float(np.float64(w[e]) + np.float64(cot[h]))
            mag[e] += abs(float(cot[h]))
    return np.array([x if x > 0.0 else 0.0 for x in w], dtype=np.float64).reshape(-1), np.array(mag, dtype=np.float64).reshape(-1)


def laplacian(points, nbrs, weight):
    """Definition 3: points (V, 3), nbrs = neighbours(), weight (E) -> (delta (V, 3), weight_sum (V), has (V) bool: W > 0 and finite)."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3).tolist()
    start, vertex, edge = (x.tolist() for x in nbrs)
    w_e = np.asarray(weight, dtype=np.float64).tolist()
    delta, wsum, has = np.zeros((len(p), 3)), np.zeros(len(p)), np.zeros(len(p), dtype=bool)
    for i, pi in enumerate(p):
        s, big = [0.0, 0.0, 0.0], 0.0
        for j in range(start[i], start[i + 1]):
            w, pj = w_e[edge[j]], p[vertex[j]]
            big = big + w
            for a in range(3):
                s[a] = s[a] + w * (pj[a] - pi[a])
        wsum[i] = big
        if big > 0.0 and math.isfinite(big):
            has[i] = True
            with np.errstate(all="ignore"):
                delta[i] = [float(np.float64(s[a]) / np.float64(big)) for a in range(3)]
    return delta, wsum, has


def step(points, nbrs, weight, pinned, factor):
    """Definition 4 -> the new points; pinned vertices and those without a positive finite weight sum keep their bits."""
    p = np.array(points, dtype=np.float64).reshape(-1, 3)
    delta, _, has = laplacian(p, nbrs, weight)
    out = p.copy()
    factor = np.float64(factor)
    with np.errstate(all="ignore"):
        for i in range(len(p)):
            if has[i] and not pinned[i]:
                out[i] = [p[i, a] + factor * delta[i, a] for a in range(3)]
    return out


def dihedral(topo):
    """Definition 7 -> angle (E) float64 from topology(..., normals=True)."""
    angle = np.full(len(topo["edges"]), NAN)
    for e in range(len(angle)):
        if topo["edge_class"][e] != 2:
            continue
        n1, n2 = (topo["face_normal"][int(h) // 3] for h in topo["edge_halfedges"][e])
        if not n1.any() or not n2.any():
            continue
        c = TR._cross(n1, n2)
        angle[e] = np.arctan2(np.sqrt(TR._dot(c, c)), TR._dot(n1, n2))
    return angle


def roughness_report(angle):
    a = angle[np.isfinite(angle)]
    if not len(a):
        return {"edges": 0, "mean": NAN, "rms": NAN, "max": NAN}
    return {"edges": len(a), "mean": float(a.sum() / len(a)), "rms": float(np.sqrt((a * a).sum() / len(a))), "max": float(a.max())}


def roughness(vertices, triangles):
    return roughness_report(dihedral(TR.topology(vertices, triangles, normals=True)))


def check_request(iterations=10, lam=0.5, mu=-0.53, weights="uniform"):
    """Definition 6's accepted ranges."""
    ok = isinstance(iterations, int) and not isinstance(iterations, bool) and 0 <= iterations <= 1000
    ok = ok and 0.0 < lam <= 1.0 and (mu == 0 or -2.0 <= mu < -lam) and weights in ("uniform", "cotangent")
    if not ok:
        raise ValueError((iterations, lam, mu, weights))


def smooth(vertices, triangles, iterations=10, lam=0.5, mu=-0.53, weights="uniform", fix_boundary=True, pinned=None, measure=False,
           weight_override=None, topology=None):
    """Definitions 5, 6 and 8 -> {"vertices", "triangles", "stats", "pinned" (V) bool, "nbr_start", "nbr_vertex", "nbr_edge", "weight" (E),
    "weight_bound" (E), "topology"}.  weight_override (E): weights to step with in place of the restatement's own (the device's cotangent
    sums).  topology: TR.topology(vertices, triangles, normals=True) if the caller has it."""
    check_request(iterations, lam, mu, weights)
    v = np.array(vertices, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(triangles).reshape(-1, 3)
    topo = TR.topology(v, t, normals=measure) if topology is None else topology
    nbrs = neighbours(topo["edges"], len(v))
    weight, mag = edge_weights(topo, corner_cot(v, t, topo["face_valid"]) if weights == "cotangent" else None, weights)
    used = weight if weight_override is None else np.asarray(weight_override, dtype=np.float64)
    fixed = np.zeros(len(v), dtype=bool) if pinned is None else np.array(pinned, dtype=bool).reshape(-1)
    if fix_boundary:
        fixed = fixed | ((topo["vertex_flags"] & 2) != 0)
    cur = v.copy()
    for _ in range(iterations):
        cur = step(cur, nbrs, used, fixed, lam)
        if mu != 0:
            cur = step(cur, nbrs, used, fixed, mu)
    free = ~fixed & ((topo["vertex_flags"] & 1) != 0)
    d = cur - v
    dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[free]
    moved = int((cur.view(np.int64).reshape(-1, 3) != v.view(np.int64).reshape(-1, 3)).any(axis=1).sum())
    stats = {"iterations": iterations, "weights": weights, "pinned": int(fixed.sum()), "moved": moved,
             "displacement_max": float(dist.max()) if len(dist) else NAN, "displacement_mean": float(dist.sum() / len(dist)) if len(dist) else NAN,
             "displacement_rms": float(np.sqrt((dist * dist).sum() / len(dist))) if len(dist) else NAN}
    if measure:
        after = TR.topology(cur, t, normals=True)
        stats.update(area_before=topo["report"]["area"], area_after=after["report"]["area"], volume_before=topo["report"]["volume"],
                     volume_after=after["report"]["volume"], roughness_before=roughness_report(dihedral(topo)),
                     roughness_after=roughness_report(dihedral(after)))
    return {"vertices": cur, "triangles": np.array(triangles), "stats": stats, "pinned": fixed, "nbr_start": nbrs[0], "nbr_vertex": nbrs[1],
            "nbr_edge": nbrs[2], "weight": weight, "weight_bound": 8.0 * 2.0 ** -52 * mag, "topology": topo}


# ------------------------------------------------------------------------------------------------ shapes
def lattice_sheet(n=9):
    """An n x n integer lattice sheet in the plane z = 0, every cell cut by the same diagonal."""
    v = np.array([[float(x), float(y), 0.0] for y in range(n) for x in range(n)])
    t = []
    for y in range(n - 1):
        for x in range(n - 1):
            a, b, c, d = y * n + x, y * n + x + 1, (y + 1) * n + x, (y + 1) * n + x + 1
            t += [(a, b, d), (a, d, c)]
    return v, np.array(t, dtype=np.int32)


def icosphere(subdivisions=3):
    """The unit icosphere: 10 * 4^s + 2 vertices, 20 * 4^s faces, outward winding."""
    g = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    v = [list(np.array(p, dtype=np.float64) / math.sqrt(1.0 + g * g)) for p in v]
    t = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, out = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = (np.array(v[a]) + np.array(v[b])) / 2.0
                v.append(list(m / math.sqrt(float(m @ m))))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in t:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        t = out
    return np.array(v, dtype=np.float64), np.array(t, dtype=np.int32)


def noisy_icosphere(subdivisions=3, sigma=0.02, seed=7):
    """The icosphere with every vertex moved along its normal (its own position) by N(0, sigma) -> (noisy vertices, triangles, clean vertices)."""
    v, t = icosphere(subdivisions)
    noise = np.random.default_rng(seed).normal(0.0, sigma, size=len(v))
    return v * (1.0 + noise)[:, None], t, v


def unreferenced_tail(n=257):
    """A strip over the first vertices of n, the rest referenced by no face (and one face with an index out of range)."""
    v, t = TR.strip(20)
    rng = np.random.default_rng(3)
    tail = rng.uniform(-1.0, 1.0, size=(n - len(v), 3))
    tail[0] = [-0.0, 0.0, -0.0]
    return np.concatenate([v, tail]), np.concatenate([t, [[0, 1, n + 4]]]).astype(np.int32)
