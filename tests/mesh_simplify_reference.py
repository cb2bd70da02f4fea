"""K33 restated with numpy, straight from its definition (include/gens_hip.h, K33): the cell keys, the triangles' cluster ranks, the quadrics,
the representatives and the source vertices.  float64 throughout, every operation a numpy operation of its own (numpy rounds each on its
own and never fuses), in the order the definition writes; the sums that the definition orders (a cluster's quadric over its triangles, the
mean over its members) are plain loops in that order.  The GPU tests compare the kernels with this file bit for bit; the CPU tests check what
the rule promises on analytic meshes.  Nothing here is derived from the kernels' source.
"""
import numpy as np

AXIS_CELLS = 1 << 21
REG = 1e-3


def cells(vertices, cell, origin):
    """Step 1 -> (V, 3) int64 cell coordinates; ValueError where one is outside 0 .. 2^21 - 1 or not a number."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    c = np.floor((v - np.asarray(origin, dtype=np.float64)[None, :]) / np.float64(cell))
    if not ((c >= 0) & (c < AXIS_CELLS)).all():
        raise ValueError("mesh_simplify_reference: a vertex's cell is outside 0 .. 2^21 - 1 on some axis")
    return c.astype(np.int64)


def keys(vertices, cell, origin):
    c = cells(vertices, cell, origin)
    return (c[:, 2] << 42) + (c[:, 1] << 21) + c[:, 0]


def key_cell(key):
    key = np.asarray(key, dtype=np.int64)
    return np.stack([key & (AXIS_CELLS - 1), (key >> 21) & (AXIS_CELLS - 1), (key >> 42) & (AXIS_CELLS - 1)], axis=-1)


def default_origin(vertices, cell):
    """ops.simplify_mesh's origin=None: per axis cell floor(min_a / cell)."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    return np.float64(cell) * np.floor(v.min(axis=0) / np.float64(cell))


def cluster_triangles(triangles, vertex_cluster):
    """Step 2's per-triangle part -> ranks (T, 3) int32, survive (T,) bool, triple (T, 3) int32 (the ranks ascending)."""
    t = np.asarray(triangles).reshape(-1, 3)
    ranks = np.asarray(vertex_cluster, dtype=np.int32)[t]
    survive = (ranks[:, 0] != ranks[:, 1]) & (ranks[:, 1] != ranks[:, 2]) & (ranks[:, 0] != ranks[:, 2])
    return ranks, survive, np.sort(ranks, axis=1)


def solve_cluster(q_tris, q_members, reg):
    """Steps 3 to 5 for one cluster.  q_tris: a list of (3, 3) arrays, the cluster's surviving triangles in ascending index, rows q0, q1, q2 in
    cell units about the cluster's centre; q_members (k, 3): its members in ascending vertex index -> (x (3,), the member's position in
    q_members, fell_back, m (3,))."""
    A = np.zeros(6, np.float64)                                # A00 A01 A02 A11 A12 A22
    b = np.zeros(3, np.float64)
    for q in q_tris:
        q0, q1, q2 = q[0], q[1], q[2]
        e1, e2 = q1 - q0, q2 - q0
        n = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]], dtype=np.float64)
        d = -((n[0] * q0[0] + n[1] * q0[1]) + n[2] * q0[2])
        A[0] += n[0] * n[0]
        A[1] += n[0] * n[1]
        A[2] += n[0] * n[2]
        A[3] += n[1] * n[1]
        A[4] += n[1] * n[2]
        A[5] += n[2] * n[2]
        b[0] += n[0] * d
        b[1] += n[1] * d
        b[2] += n[2] * d
    s = np.zeros(3, np.float64)
    for q in q_members:
        s = s + q
    m = s / np.float64(len(q_members))
    x, fell = m, True
    tr = (A[0] + A[3]) + A[5]
    if tr > 0:
        lam = np.float64(reg) * tr
        M00, M11, M22, M01, M02, M12 = A[0] + lam, A[3] + lam, A[5] + lam, A[1], A[2], A[4]
        r0, r1, r2 = lam * m[0] - b[0], lam * m[1] - b[1], lam * m[2] - b[2]
        c00 = M11 * M22 - M12 * M12
        c01 = M02 * M12 - M01 * M22
        c02 = M01 * M12 - M02 * M11
        c11 = M00 * M22 - M02 * M02
        c12 = M01 * M02 - M00 * M12
        c22 = M00 * M11 - M01 * M01
        det = (M00 * c00 + M01 * c01) + M02 * c02
        with np.errstate(all="ignore"):
            y = np.array([((c00 * r0 + c01 * r1) + c02 * r2) / det, ((c01 * r0 + c11 * r1) + c12 * r2) / det,
                          ((c02 * r0 + c12 * r1) + c22 * r2) / det], dtype=np.float64)
        if det > 0 and bool((np.abs(y) <= 0.5).all()):
            x, fell = y, False
    best, src = None, -1
    for k, q in enumerate(q_members):
        dq = q - x
        dist = (dq[0] * dq[0] + dq[1] * dq[1]) + dq[2] * dq[2]
        if src < 0 or dist < best:
            best, src = dist, k
    return x, src, fell, m


def simplify(vertices, triangles, cell, origin=None, reg=REG, use_mean=False):
    """The whole rule -> dict: vertices (V', 3) float64, triangles (T', 3) int32, source (V',) int64, and what the kernels' intermediate
    outputs are compared with: keys (V,) int64, cluster_keys (C,) int64, vertex_cluster (V,) int32, ranks, survive, triple, out_clusters
    (V',) int32, fell_back (V',) bool, means (V', 3) (the cluster means m as world points), stats.  use_mean=True: every representative is
    its cluster's mean m (plain vertex clustering: what the quadric is measured against)."""
    v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
    t = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
    cell = np.float64(cell)
    if not (cell > 0 and np.isfinite(cell)) or not (reg > 0 and np.isfinite(reg)):
        raise ValueError("mesh_simplify_reference: cell and reg are positive and finite")
    if not np.isfinite(v).all():
        raise ValueError("mesh_simplify_reference: a vertex is not finite")
    if t.size and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError("mesh_simplify_reference: a triangle index is outside the vertices")
    origin = (default_origin(v, cell) if len(v) else np.zeros(3)) if origin is None else np.asarray(origin, dtype=np.float64).reshape(3)
    key = keys(v, cell, origin)
    cluster_keys, vertex_cluster = np.unique(key, return_inverse=True)
    vertex_cluster = vertex_cluster.astype(np.int32).reshape(-1)
    n_c = len(cluster_keys)
    ranks, survive, triple = cluster_triangles(t, vertex_cluster)
    # duplicates: the smallest surviving index of every set of three clusters
    seen, kept = set(), []
    for i in np.nonzero(survive)[0]:
        k = tuple(int(r) for r in triple[i])
        if k not in seen:
            seen.add(k)
            kept.append(int(i))
    kept = np.array(kept, dtype=np.int64)
    used = np.zeros(n_c, bool)
    used[ranks[kept].reshape(-1)] = True
    out_clusters = np.nonzero(used)[0].astype(np.int32)
    new_index = np.cumsum(used) - 1
    out_triangles = new_index[ranks[kept]].astype(np.int32).reshape(-1, 3)
    # segments, in the definition's orders
    members = [[] for _ in range(n_c)]
    for i, c in enumerate(vertex_cluster):
        members[c].append(i)
    tris_of = [[] for _ in range(n_c)]
    for i in np.nonzero(survive)[0]:
        for c in ranks[i]:
            tris_of[c].append(int(i))                          # three different clusters: each triangle once per cluster, ascending
    out_v = np.zeros((len(out_clusters), 3), np.float64)
    means = np.zeros((len(out_clusters), 3), np.float64)
    source = np.zeros(len(out_clusters), np.int64)
    fell = np.zeros(len(out_clusters), bool)
    cc = key_cell(cluster_keys).astype(np.float64)
    for j, c in enumerate(out_clusters):
        ctr = origin + (cc[c] + 0.5) * cell
        q_tris = [(v[t[i]] - ctr[None, :]) / cell for i in tris_of[c]]
        q_members = (v[members[c]] - ctr[None, :]) / cell
        x, src, fb, m = solve_cluster([] if use_mean else q_tris, q_members, reg)
        out_v[j] = ctr + x * cell
        means[j] = ctr + m * cell
        source[j] = members[c][src]
        fell[j] = fb
    n_s = int(survive.sum())
    stats = {"input_vertices": len(v), "input_triangles": len(t), "output_vertices": len(out_clusters), "output_triangles": len(kept),
             "collapsed_triangles": len(t) - n_s, "duplicate_triangles": n_s - len(kept), "fell_back": int(fell.sum())}
    return {"vertices": out_v, "triangles": out_triangles, "source": source, "keys": key, "cluster_keys": cluster_keys,
            "vertex_cluster": vertex_cluster, "ranks": ranks, "survive": survive, "triple": triple.astype(np.int32), "out_clusters": out_clusters,
            "fell_back": fell, "means": means, "stats": stats, "origin": origin}


# ------------------------------------------------------------------------------------------------------------------------------------
# inputs the CPU and the GPU tests share
# ------------------------------------------------------------------------------------------------------------------------------------
CENTRE = np.array([15.7, 16.2, 16.4])
SPHERE_RADIUS = 11.3
BOX_HALF = np.array([9.3, 7.1, 10.2])


def sphere_field(p):
    """Signed distance to the sphere (negative inside), p (..., 3)."""
    return np.sqrt(((np.asarray(p, dtype=np.float64) - CENTRE) ** 2).sum(axis=-1)) - SPHERE_RADIUS


def box_field(p):
    """Signed distance to the axis-aligned box (negative inside)."""
    d = np.abs(np.asarray(p, dtype=np.float64) - CENTRE) - BOX_HALF
    return np.sqrt((np.maximum(d, 0.0) ** 2).sum(axis=-1)) + np.minimum(d.max(axis=-1), 0.0)


def lattice_mesh(field, n=33):
    """The marching-cubes mesh (oracle/mc_oracle.py, the product's triangle table) of u = -field on the n^3 lattice, index coordinates ->
    (vertices (V, 3) float64, triangles (T, 3) int32)."""
    from gens_amd import mc_tables
    from oracle import mc_oracle
    g = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).astype(np.float64)
    v, t = mc_oracle.marching_cubes((-field(g)).astype(np.float32), 0.0, mc_tables.TRI_TABLE, mc_tables.TRI_COUNT)
    return v, t.astype(np.int32)


def grid_mesh(nx, ny, spacing=1.0):
    """A flat nx x ny grid of vertices in z = 0, two triangles per square -> (vertices, triangles)."""
    ix, iy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    v = np.stack([ix.reshape(-1) * spacing, iy.reshape(-1) * spacing, np.zeros(nx * ny)], axis=1).astype(np.float64)
    idx = (ix * ny + iy)
    a, b, c, d = idx[:-1, :-1].reshape(-1), idx[1:, :-1].reshape(-1), idx[1:, 1:].reshape(-1), idx[:-1, 1:].reshape(-1)
    t = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.int32)
    return v, t


FAN_CELL = 0.04


def fan_mesh(n=300, radius=3.0):
    """n triangles around the vertex 0 at (4.5, 4.5, 4.5) (slightly coned and waved, so that the planes differ).  With cell FAN_CELL (below
    the rim vertices' spacing 2 pi radius / n = 0.063 divided by sqrt(2)) every rim vertex has a cell of its own, every triangle survives
    and the hub's cluster has an entry segment of n triangles."""
    ang = 2 * np.pi * np.arange(n) / n
    rim = np.stack([4.5 + radius * np.cos(ang), 4.5 + radius * np.sin(ang), 4.5 + 0.2 * np.cos(3 * ang) - 0.4], axis=1)
    v = np.concatenate([[[4.5, 4.5, 4.5]], rim]).astype(np.float64)
    t = np.stack([np.zeros(n, np.int64), 1 + np.arange(n), 1 + (np.arange(n) + 1) % n], axis=1).astype(np.int32)
    return v, t


def planted_mesh():
    """One small mesh with every special input of the rule, cell 1, origin (-2, -2, -2) -> (vertices, triangles, cell, origin):
    a triangle with a repeated index; duplicate and reversed duplicate triangles (other vertices, the same three clusters); unreferenced
    vertices (one alone in its cell, one in a used cell); vertices exactly on cell boundaries; a zero-area surviving triangle (tr = 0: the
    mean); negative coordinates."""
    v = np.array([
        [-1.5, -1.5, -1.5], [-0.4, -1.6, -1.3], [-1.4, -0.5, -1.2],        # 0 1 2: a plain triangle, negative coordinates
        [-1.6, -1.4, -1.7], [-0.6, -1.4, -1.4], [-1.3, -0.6, -1.6],        # 3 4 5: other vertices in the same three cells
        [0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 1.0, 1.0],  # 6 .. 9: exactly on cell boundaries
        [2.5, 2.5, 2.5],                                                 # 10: unreferenced, alone in its cell
        [-1.45, -1.55, -1.5],                                            # 11: unreferenced, in vertex 0's cell: it counts in m
        [3.25, 0.5, 0.5], [4.25, 0.5, 0.5], [5.25, 0.5, 0.5],              # 12 13 14: collinear: a surviving triangle of area 0
        [0.5, 3.5, 0.5], [0.6, 3.6, 0.5], [1.5, 3.5, 0.5],                 # 15 16 17: 15 and 16 share a cell: collapsed
    ], dtype=np.float64)
    t = np.array([
        [0, 1, 2], [3, 4, 5], [5, 4, 3], [2, 1, 0], [1, 2, 0],           # one kept, a duplicate, two reversed ones, a rotated one
        [6, 7, 8], [7, 9, 8], [6, 8, 9],                                 # boundary vertices
        [6, 6, 7], [8, 9, 8],                                            # repeated indices: never survive
        [12, 13, 14],                                                    # zero area, three clusters: survives, tr = 0
        [15, 16, 17],                                                    # two vertices in one cluster: collapsed
        [0, 6, 12], [4, 7, 13],
    ], dtype=np.int32)
    return v, t, 1.0, np.array([-2.0, -2.0, -2.0])


def clusters_mesh(n_clusters):
    """A strip of triangles whose vertices fall into exactly n_clusters cells of edge 1 (two rows of cells along x), three vertices per cell
    -> (vertices, triangles, cell 1.0, origin zeros)."""
    half = (n_clusters + 1) // 2
    rng = np.random.default_rng(n_clusters)
    cells_xy = [(i, 0) for i in range(half)] + [(i, 1) for i in range(n_clusters - half)]
    v = np.concatenate([np.array([cx, cy, 0.0]) + rng.uniform(0.1, 0.9, (3, 3)) for cx, cy in cells_xy]).astype(np.float64)
    tris = []
    first = {c: 3 * k for k, c in enumerate(cells_xy)}
    for i in range(half - 1):                                  # (row 1 has half or half - 1 cells: (i, 1) exists for every i here)
        for a in range(3):
            tris.append([first[(i, 0)] + a, first[(i + 1, 0)] + (a + 1) % 3, first[(i, 1)] + (a + 2) % 3])
        if (i + 1, 1) in first:
            for a in range(2):
                tris.append([first[(i + 1, 0)] + a, first[(i + 1, 1)] + a, first[(i, 1)] + a])
    return v, np.array(tris, dtype=np.int32), 1.0, np.zeros(3)


def field_error(field, vertices, triangles, seed=0, samples=6):
    """The mean |field| over `samples` barycentric points per triangle, fixed seed."""
    rng = np.random.default_rng(seed)
    w = rng.dirichlet(np.ones(3), size=(len(triangles), samples))                  # (T, samples, 3)
    p = np.einsum("tsk,tkd->tsd", w, np.asarray(vertices)[np.asarray(triangles)])
    return float(np.abs(field(p)).mean())
