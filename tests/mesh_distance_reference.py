"""K36 restated in numpy (the comment of K36 in include/gens_hip.h is the definition): the per-face rule operation for operation in float64,
the result of a query as brute force over ALL faces, the summary dict of ops.mesh_distance -- and a second, independent formulation in
np.longdouble (foot on the plane, three half-plane tests, else the nearest of three clamped segments) to hold the rule against.  Shared by
tests/test_mesh_distance_cpu.py and tests/test_hip_mesh_distance.py, which also take their meshes from here."""
import numpy as np

from . import mesh_simplify_reference as SR

NO_REGION = 255
QUANTILES = (("q50", 50), ("q90", 90), ("q99", 99))


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _xyz(p):
    return [p[..., 0], p[..., 1], p[..., 2]]


def _segment(q, p0, e, w):
    """The degenerate path's segment p0 + t e, w = q - p0 -> (d2, s): lists of component arrays."""
    ln = _dot(e, e)
    ok = ln > 0.0
    t = np.where(ok, _dot(w, e) / np.where(ok, ln, 1.0), 0.0)
    t = np.where(t > 0.0, t, 0.0)
    t = np.where(t > 1.0, 1.0, t)
    s = [p0[k] + t * e[k] for k in range(3)]
    u = [q[k] - s[k] for k in range(3)]
    return _dot(u, u), s


def face_rule(q, a, b, c):
    """Rule (a).  q, a, b, c: float64 arrays (..., 3) that broadcast -> (d2 (...), p (..., 3), region (...) uint8)."""
    q, a, b, c = (np.asarray(x, dtype=np.float64) for x in (q, a, b, c))
    shape = np.broadcast_shapes(q.shape, a.shape, b.shape, c.shape)
    q, a, b, c = (_xyz(np.broadcast_to(x, shape)) for x in (q, a, b, c))
    with np.errstate(all="ignore"):
        ab = [b[k] - a[k] for k in range(3)]
        ac = [c[k] - a[k] for k in range(3)]
        ap = [q[k] - a[k] for k in range(3)]
        n = [ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]]
        flat = (n[0] == 0.0) & (n[1] == 0.0) & (n[2] == 0.0)
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = [q[k] - b[k] for k in range(3)]
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        cp = [q[k] - c[k] for k in range(3)]
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e, g = d4 - d3, d5 - d6
        tests = [(d1 <= 0.0) & (d2 <= 0.0), (d3 >= 0.0) & (d4 <= d3), (vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0), (d6 >= 0.0) & (d5 <= d6),
                 (vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0), (va <= 0.0) & (e >= 0.0) & (g >= 0.0), (va >= 0.0) & (vb >= 0.0) & (vc >= 0.0)]
        which = np.full(d1.shape, 7, dtype=np.int64)            # the index of the first test that holds; 7: none
        for k in range(6, -1, -1):
            which = np.where(tests[k], k, which)
        which = np.where(flat, 7, which)
        dens = {2: d1 - d3, 4: d2 - d6, 5: e + g, 6: (va + vb) + vc}
        for k, den in dens.items():
            which = np.where((which == k) & ~(den > 0.0), 7, which)
        safe = {k: np.where(den > 0.0, den, 1.0) for k, den in dens.items()}
        v_ab = d1 / safe[2]
        w_ca = d2 / safe[4]
        w_bc = e / safe[5]
        v_in, w_in = vb / safe[6], vc / safe[6]
        bc = [c[k] - b[k] for k in range(3)]
        cands = {0: a, 1: b, 2: [a[k] + v_ab * ab[k] for k in range(3)], 3: c, 4: [a[k] + w_ca * ac[k] for k in range(3)],
                 5: [b[k] + w_bc * bc[k] for k in range(3)], 6: [(a[k] + v_in * ab[k]) + w_in * ac[k] for k in range(3)]}
        codes = {0: 1, 1: 2, 2: 4, 3: 3, 4: 6, 5: 5, 6: 0}
        p = [np.zeros(d1.shape) for _ in range(3)]
        region = np.full(d1.shape, 7, dtype=np.uint8)
        for k, cand in cands.items():
            hit = which == k
            region = np.where(hit, np.uint8(codes[k]), region)
            p = [np.where(hit, cand[j], p[j]) for j in range(3)]
        u = [q[k] - p[k] for k in range(3)]
        dist2 = _dot(u, u)
        # the degenerate path: the segments ab, bc, ca, the first on ties
        ca = [a[k] - c[k] for k in range(3)]
        s_d2, s_p = _segment(q, a, ab, ap)
        for p0, ee, w in ((b, bc, bp), (c, ca, cp)):
            t_d2, t_p = _segment(q, p0, ee, w)
            better = t_d2 < s_d2
            s_d2 = np.where(better, t_d2, s_d2)
            s_p = [np.where(better, t_p[k], s_p[k]) for k in range(3)]
        deg = which == 7
        dist2 = np.where(deg, s_d2, dist2)
        p = [np.where(deg, s_p[k], p[k]) for k in range(3)]
    return dist2, np.stack(p, axis=-1), region


def closest(vertices, triangles, queries, max_dist=np.inf, chunk=256):
    """Rule (b) as brute force: every query against every face -> dict(dist2 (n) float64, face (n) int32, point (n, 3) float64, region (n)
    uint8)."""
    v, t = np.asarray(vertices, dtype=np.float64).reshape(-1, 3), np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    q = np.asarray(queries, dtype=np.float64).reshape(-1, 3)
    n = len(q)
    out = {"dist2": np.full(n, np.inf), "face": np.full(n, -1, np.int32), "point": np.full((n, 3), np.nan), "region": np.full(n, NO_REGION, np.uint8)}
    finite = np.isfinite(q).all(axis=1)
    out["dist2"][~finite] = np.nan
    if len(t) == 0 or n == 0:
        return out
    a, b, c = v[t[:, 0]][None], v[t[:, 1]][None], v[t[:, 2]][None]
    cap2 = np.float64(max_dist) * np.float64(max_dist)
    for s in range(0, n, chunk):
        rows = np.arange(s, min(s + chunk, n))
        d2, p, region = face_rule(q[rows][:, None, :], a, b, c)
        key = np.where(np.isnan(d2), np.inf, d2)
        best = key.min(axis=1)
        face = np.argmax(key == best[:, None], axis=1)            # the first, hence the smallest, face index among equal d2
        pick = (np.arange(len(rows)), face)
        found = finite[rows] & np.isfinite(best) & (best <= cap2)
        sel = rows[found]
        out["dist2"][sel] = d2[pick][found]
        out["face"][sel] = face[found].astype(np.int32)
        out["point"][sel] = p[pick][found]
        out["region"][sel] = region[pick][found]
    return out


def exact_distance(q, a, b, c):
    """The independent formulation in np.longdouble: the foot of q on the face's plane if the three edge half-planes hold it, else the nearest
    of the three clamped segments; a face without a plane has only the segments -> the distance (not squared), longdouble (...)."""
    ld = np.longdouble
    q, a, b, c = (np.asarray(x, dtype=np.float64).astype(ld) for x in (q, a, b, c))
    shape = np.broadcast_shapes(q.shape, a.shape, b.shape, c.shape)
    q, a, b, c = (np.broadcast_to(x, shape) for x in (q, a, b, c))
    dot = lambda u, w: (u * w).sum(axis=-1)  # noqa: E731
    with np.errstate(all="ignore"):
        n = np.cross(b - a, c - a)
        nn = dot(n, n)
        has_plane = nn > 0
        h = dot(q - a, n) / np.where(has_plane, nn, ld(1))
        foot = q - h[..., None] * n
        inside = has_plane
        for p0, p1 in ((a, b), (b, c), (c, a)):
            inside = inside & (dot(np.cross(p1 - p0, foot - p0), n) >= 0)
        best = np.full(shape[:-1], np.inf, dtype=ld)
        for p0, p1 in ((a, b), (b, c), (c, a)):
            e = p1 - p0
            ln = dot(e, e)
            t = np.clip(np.where(ln > 0, dot(q - p0, e) / np.where(ln > 0, ln, ld(1)), ld(0)), 0, 1)
            r = q - (p0 + t[..., None] * e)
            best = np.minimum(best, np.sqrt(dot(r, r)))
        plane = np.abs(h) * np.sqrt(nn)
    return np.where(inside, plane, best)


def exact_closest(vertices, triangles, queries, chunk=64):
    """min over all faces of exact_distance -> (n) longdouble."""
    v, t = np.asarray(vertices, dtype=np.float64), np.asarray(triangles, dtype=np.int64)
    q = np.asarray(queries, dtype=np.float64).reshape(-1, 3)
    a, b, c = v[t[:, 0]][None], v[t[:, 1]][None], v[t[:, 2]][None]
    return np.concatenate([exact_distance(q[s:s + chunk, None, :], a, b, c).min(axis=1) for s in range(0, len(q), chunk)])


# ------------------------------------------------------------------------------------------------------------------------------------
# the summary of ops.mesh_distance
# ------------------------------------------------------------------------------------------------------------------------------------
def mesh_area(vertices, triangles):
    v, t = np.asarray(vertices, dtype=np.float64), np.asarray(triangles, dtype=np.int64)
    if len(t) == 0:
        return 0.0
    n = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    return float(0.5 * np.sqrt((n * n).sum(axis=1)).sum())


def direction_stats(dist2):
    """One direction's figures from the squared distances of its samples: +inf entries (nothing under the cap) are counted in `unmatched` and
    left out of everything else; q_p = the order statistic at index (p m) // 100 of the m matched distances in ascending order; with m = 0
    every figure is NaN."""
    d2 = np.asarray(dist2, dtype=np.float64)
    keep = np.isfinite(d2)
    m = int(keep.sum())
    out = {"n": int(len(d2)), "unmatched": int(len(d2) - m)}
    if m == 0:
        out.update({k: float("nan") for k in ("mean", "rms", "max", "q50", "q90", "q99")})
        return out
    d = np.sort(np.sqrt(d2[keep]))
    out.update(mean=float(d.sum() / m), rms=float(np.sqrt(d2[keep].sum() / m)), max=float(d[-1]))
    for name, p in QUANTILES:
        out[name] = float(d[min(m - 1, (p * m) // 100)])
    return out


def summary(a_to_b, b_to_a, density_a, density_b):
    ha, hb = a_to_b["max"], b_to_a["max"]
    return {"a_to_b": a_to_b, "b_to_a": b_to_a, "hausdorff": float("nan") if ha != ha or hb != hb else max(ha, hb),
            "chamfer": 0.5 * (a_to_b["mean"] + b_to_a["mean"]), "density_a": float(density_a), "density_b": float(density_b)}


def mesh_distance(va, ta, vb, tb, samples_a, samples_b, density_a, density_b, max_dist=np.inf):
    """The dict of ops.mesh_distance from the SAME samples (K24's sampler is restated in its own tests, not here)."""
    ab = closest(vb, tb, samples_a, max_dist)["dist2"]
    ba = closest(va, ta, samples_b, max_dist)["dist2"]
    return summary(direction_stats(ab), direction_stats(ba), density_a, density_b)


# ------------------------------------------------------------------------------------------------------------------------------------
# inputs the CPU and the GPU tests share
# ------------------------------------------------------------------------------------------------------------------------------------
TRIANGLE = (np.array([[0.5, 0.25, 1.0], [2.5, 0.5, 1.25], [0.75, 2.0, 0.5]]), np.array([[0, 1, 2]], np.int32))


def noise_mesh():
    """The ragged white-noise lattice of tests/test_marching_cubes.py at its threshold (K33's tests use the same)."""
    from gens_amd import mc_tables
    from oracle import mc_oracle
    u = np.random.default_rng(2).standard_normal((7, 19, 66)).astype(np.float32)
    v, t = mc_oracle.marching_cubes(u, 0.25, mc_tables.TRI_TABLE, mc_tables.TRI_COUNT)
    return v, t.astype(np.int32)


def sphere_mesh():
    return SR.lattice_mesh(SR.sphere_field)


def fan_mesh():
    return SR.fan_mesh()


def degenerate_mesh():
    """Three equal points; a zero edge; three collinear points -- and one plain triangle so that the mesh has an extent on every axis."""
    v = np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0],
                  [3.0, 1.0, 0.5], [3.0, 1.0, 0.5], [4.0, 2.0, 0.5],
                  [0.0, 4.0, 2.0], [1.0, 4.5, 2.0], [3.0, 5.5, 2.0],
                  [6.0, 6.0, 3.0], [7.0, 6.0, 3.0], [6.0, 7.0, 3.5]])
    return v, np.arange(12, dtype=np.int32).reshape(4, 3)


def tie_mesh():
    """A duplicated face (0 and 2, with face 1 between them), and a pair mirrored in the plane x = 2 (faces 3 and 4): a query with x = 2 is
    equally far from both, in exactly representable coordinates -> (vertices, triangles)."""
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0],          # 0 1 2
                  [0.0, 0.0, 3.0], [1.0, 0.0, 3.0], [0.0, 1.0, 3.5],          # 3 4 5: far from the duplicated pair
                  [1.5, 4.0, 1.0], [1.0, 5.0, 1.0], [1.25, 4.5, 2.0],         # 6 7 8: left of x = 2
                  [2.5, 4.0, 1.0], [3.0, 5.0, 1.0], [2.75, 4.5, 2.0]])        # 9 10 11: its mirror image
    t = np.array([[0, 1, 2], [3, 4, 5], [0, 1, 2], [9, 10, 11], [6, 7, 8]], np.int32)
    return v, t


def two_clusters_mesh():
    """Two small patches 40 units apart: the cells between them are empty, so a query there walks many rings."""
    gv, gt = SR.grid_mesh(3, 3, 0.5)
    far = gv[:, [2, 0, 1]] + np.array([40.0, 3.0, 1.0])
    return np.concatenate([gv, far]), np.concatenate([gt, gt + len(gv)]).astype(np.int32)


def region_queries():
    """Queries of TRIANGLE in all seven regions, above and below the plane, then on the vertices, on the edges and in the plane ->
    (queries, expected region codes)."""
    v = TRIANGLE[0]
    a, b, c = v
    n = np.cross(b - a, c - a)
    n = n / np.linalg.norm(n)
    mid = lambda p, r, s: p + s * (r - p)  # noqa: E731
    out_ab, out_bc, out_ca = np.cross(b - a, n), np.cross(c - b, n), np.cross(a - c, n)
    base = [((a + b + c) / 3, 0), (a - 0.5 * (b - a) - 0.5 * (c - a), 1), (b + 0.5 * (b - a) + 0.3 * (b - c), 2), (c + 0.5 * (c - a) + 0.5 * (c - b), 3),
            (mid(a, b, 0.4) + 0.3 * out_ab, 4), (mid(b, c, 0.6) + 0.3 * out_bc, 5), (mid(c, a, 0.3) + 0.3 * out_ca, 6)]
    q, r = [], []
    for p, code in base:
        for h in (0.7, -0.4):
            q.append(p + h * n)
            r.append(code)
    return np.array(q), np.array(r, np.uint8)


def zero_queries():
    """Points OF the triangle whose d2 must be exactly 0: the vertices, dyadic points of the edges and of the interior of a triangle with
    dyadic coordinates (every product in the rule is exact there)."""
    a, b, c = TRIANGLE[0]
    pts = [a, b, c, a + 0.5 * (b - a), b + 0.25 * (c - b), c + 0.5 * (a - c), a + 0.25 * (b - a) + 0.25 * (c - a), a + 0.5 * (b - a) + 0.125 * (c - a)]
    return np.array(pts)
