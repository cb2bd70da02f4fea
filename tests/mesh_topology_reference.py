"""K37 restated in numpy float64 (the comment of K37 in include/gens_hip.h is the definition): the edge table, the classes of edges and
vertices, the fans, the components, the report, the pseudonormals and the sign of K36's distance, as brute force with dicts and loops -- and
an independent truth for the sign: the winding number of a closed mesh at a point, as the Van Oosterom-Strackee solid-angle sum over all
faces.  Shared by tests/test_mesh_topology_cpu.py and tests/test_hip_mesh_topology.py, which also take their shapes from here."""
import math

import numpy as np

from . import mesh_distance_reference as DR

NO_SIGN_FLAGS = 0x1E


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _cross(u, v):
    return np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]])


class _Sets:
    """Union-find whose root is the smallest member."""

    def __init__(self, n):
        self.parent = list(range(n))

    def find(self, x):
        while self.parent[x] != x:
            x = self.parent[x]
        return x

    def join(self, a, b):
        a, b = self.find(a), self.find(b)
        if a != b:
            self.parent[max(a, b)] = min(a, b)

    def labels(self):
        return np.array([self.find(x) for x in range(len(self.parent))], dtype=np.int32).reshape(-1)


def topology(vertices, triangles, normals=True):
    """-> dict of numpy arrays named as ops.MeshTopology's fields, plus "report"."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    nv, nt = len(v), len(t)
    valid = np.array([all(0 <= int(i) < nv for i in f) and len({int(i) for i in f}) == 3 for f in t], dtype=bool).reshape(-1)
    uses = {}                                       # (lo, hi) -> [(h, forward)] in ascending h
    for f in range(nt):
        if not valid[f]:
            continue
        for k in range(3):
            a, b = int(t[f, k]), int(t[f, (k + 1) % 3])
            uses.setdefault((min(a, b), max(a, b)), []).append((3 * f + k, a < b))
    keys = sorted(uses)
    ne = len(keys)
    edges = np.array(keys, dtype=np.int32).reshape(-1, 2)
    edge_count = np.array([len(uses[k]) for k in keys], dtype=np.int32).reshape(-1)
    edge_forward = np.array([sum(1 for _, fw in uses[k] if fw) for k in keys], dtype=np.int32).reshape(-1)
    edge_halfedges = np.full((ne, 2), -1, dtype=np.int32)
    edge_class = np.zeros(ne, dtype=np.uint8)
    edge_of_halfedge = np.full(3 * nt, -1, dtype=np.int32)
    for e, k in enumerate(keys):
        hs = [h for h, _ in uses[k]]
        for j, h in enumerate(hs[:2]):
            edge_halfedges[e, j] = h
        for h in hs:
            edge_of_halfedge[h] = e
        edge_class[e] = 1 if len(hs) == 1 else 4 if len(hs) > 2 else 2 if edge_forward[e] == 1 else 3
    corners = _Sets(3 * nt)
    faces = _Sets(nt)
    for e in range(ne):
        if edge_class[e] not in (2, 3):
            continue
        f0, f1 = int(edge_halfedges[e, 0]) // 3, int(edge_halfedges[e, 1]) // 3
        faces.join(f0, f1)
        for end in edges[e]:
            c0 = 3 * f0 + [int(i) for i in t[f0]].index(int(end))
            c1 = 3 * f1 + [int(i) for i in t[f1]].index(int(end))
            corners.join(c0, c1)
    corner_label = corners.labels()
    face_component = faces.labels()
    valence, fans, flags = np.zeros(nv, np.int32), np.zeros(nv, np.int32), np.zeros(nv, np.uint8)
    at = [[] for _ in range(nv)]                    # the corners of each vertex in ascending corner id
    for f in range(nt):
        if valid[f]:
            for k in range(3):
                at[int(t[f, k])].append(3 * f + k)
    bit_of = {1: 2, 4: 4, 3: 8}
    for x in range(nv):
        valence[x] = len(at[x])
        fans[x] = len({int(corner_label[c]) for c in at[x]})
        bits = 1 if at[x] else 0
        for c in at[x]:
            f, k = divmod(c, 3)
            for h in (c, 3 * f + (k + 2) % 3):
                bits |= bit_of.get(int(edge_class[edge_of_halfedge[h]]), 0)
        if fans[x] > 1:
            bits |= 16
        flags[x] = bits
    out = {"edges": edges, "edge_count": edge_count, "edge_forward": edge_forward, "edge_halfedges": edge_halfedges, "edge_class": edge_class,
           "edge_of_halfedge": edge_of_halfedge, "face_valid": valid, "valence": valence, "fans": fans, "vertex_flags": flags,
           "corner_label": corner_label, "face_component": face_component}
    # the report
    n_valid = int(valid.sum())
    n_ref = int((flags & 1 != 0).sum())
    cls = [int((edge_class == k).sum()) for k in range(5)]
    rim = _Sets(nv)
    for e in range(ne):
        if edge_class[e] == 1:
            rim.join(int(edges[e, 0]), int(edges[e, 1]))
    rim_label = rim.labels()
    sizes = {}
    for f in range(nt):
        if valid[f]:
            sizes[int(face_component[f])] = sizes.get(int(face_component[f]), 0) + 1
    area = volume = 0.0
    for f in range(nt):
        if valid[f]:
            a, b, c = (v[int(i)] for i in t[f])
            area += 0.5 * math.sqrt(float(_dot(_cross(b - a, c - a), _cross(b - a, c - a))))
            volume += float(_dot(a, _cross(b, c)))
    rep = {"vertices": nv, "vertices_referenced": n_ref, "faces": nt, "faces_invalid": nt - n_valid, "edges": ne, "edges_boundary": cls[1],
           "edges_manifold": cls[2], "edges_flipped": cls[3], "edges_nonmanifold": cls[4], "vertices_pinched": int((flags & 16 != 0).sum()),
           "vertices_nonmanifold": int(((flags & 1 != 0) & (flags & 20 != 0)).sum()), "components": len(sizes),
           "largest_component_faces": max(sizes.values()) if sizes else 0,
           "boundary_components": len({int(rim_label[x]) for x in range(nv) if flags[x] & 2}), "euler": n_ref - ne + n_valid}
    rep["closed"] = cls[1] == 0 and cls[4] == 0 and n_valid > 0
    rep["oriented"] = cls[3] == 0
    rep["manifold"] = cls[4] == 0 and rep["vertices_pinched"] == 0
    rep["watertight"] = rep["closed"] and rep["oriented"] and rep["manifold"]
    rep["genus"] = (2 * rep["components"] - rep["euler"]) // 2 if rep["watertight"] else None
    rep["area"], rep["volume"] = area, volume / 6.0
    out["report"] = rep
    if normals:
        with np.errstate(all="ignore"):
            face_normal = np.zeros((nt, 3))
            for f in range(nt):
                if valid[f]:
                    a, b, c = (v[int(i)] for i in t[f])
                    n = _cross(b - a, c - a)
                    ln = np.sqrt(_dot(n, n))
                    if ln > 0.0 and np.isfinite(ln):
                        face_normal[f] = n / ln
            edge_normal, edge_weight = np.zeros((ne, 3)), np.zeros(ne)
            for e, k in enumerate(keys):
                for h, _ in uses[k]:
                    edge_normal[e] = edge_normal[e] + face_normal[h // 3]
                    edge_weight[e] += 1.0
            vertex_normal, vertex_weight = np.zeros((nv, 3)), np.zeros(nv)
            for x in range(nv):
                for c in at[x]:
                    f, k = divmod(c, 3)
                    p, q, r = v[int(t[f, k])], v[int(t[f, (k + 1) % 3])], v[int(t[f, (k + 2) % 3])]
                    n = _cross(q - p, r - p)
                    angle = np.arctan2(np.sqrt(_dot(n, n)), _dot(q - p, r - p))
                    if not np.isfinite(angle):
                        continue
                    vertex_normal[x] = vertex_normal[x] + angle * face_normal[f]
                    vertex_weight[x] += angle
        out.update(face_normal=face_normal, edge_normal=edge_normal, vertex_normal=vertex_normal, edge_weight=edge_weight,
                   vertex_weight=vertex_weight)
    return out


def sign_normals(topo, triangles, near):
    """The normal the sign rule picks per query of `near` (DR.closest's dict) -> (n (m, 3), has (m) bool)."""
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    m = len(near["face"])
    n, has = np.zeros((m, 3)), np.zeros(m, dtype=bool)
    for i in range(m):
        f, r = int(near["face"][i]), int(near["region"][i])
        if f < 0 or f >= len(t) or r > 6:
            continue
        if r == 0:
            n[i], has[i] = topo["face_normal"][f], True
        elif r <= 3:
            x = int(t[f, r - 1])
            if 0 <= x < len(topo["vertex_flags"]) and not topo["vertex_flags"][x] & NO_SIGN_FLAGS:
                n[i], has[i] = topo["vertex_normal"][x], True
        else:
            e = int(topo["edge_of_halfedge"][3 * f + r - 4])
            if e >= 0 and topo["edge_class"][e] == 2:
                n[i], has[i] = topo["edge_normal"][e], True
    return n, has


def signed_distance(topo, triangles, queries, near):
    """The sign rule on DR.closest's results -> (signed (m) float64, dot (m): (q - p) . n, 0 where there is no n)."""
    q = np.asarray(queries, dtype=np.float64).reshape(-1, 3)
    n, has = sign_normals(topo, triangles, near)
    d2 = near["dist2"]
    with np.errstate(all="ignore"):
        u = q - near["point"]
        dot = np.where(has, (u[:, 0] * n[:, 0] + u[:, 1] * n[:, 1]) + u[:, 2] * n[:, 2], 0.0)
        d = np.sqrt(d2)
        ok = (near["face"] >= 0) & np.isfinite(d2) & (d2 >= 0.0)
        out = np.full(len(q), np.nan)
        out = np.where(ok & has & (dot > 0.0), d, out)
        out = np.where(ok & has & (dot < 0.0), -d, out)
        out = np.where(ok & (d2 == 0.0), 0.0, out)
    return out, dot


def winding_number(vertices, triangles, queries):
    """Sum over all faces of the solid angle the face subtends at the query (Van Oosterom and Strackee, 1983), over 4 pi: +1 inside a closed
    mesh whose normals point outwards, 0 outside."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    q = np.asarray(queries, dtype=np.float64).reshape(-1, 3)
    a, b, c = (v[t[:, k]][None] - q[:, None] for k in range(3))
    la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (a, b, c))
    num = (a * np.cross(b, c)).sum(-1)
    den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
    return (2.0 * np.arctan2(num, den)).sum(axis=1) / (4.0 * np.pi)


# ------------------------------------------------------------------------------------------------ shapes
def tetrahedron():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float64)
    return v, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], dtype=np.int32)


def cube():
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=np.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]      # outward
    return v, np.array([tri for a, b, c, d in quads for tri in ((a, b, c), (a, c, d))], dtype=np.int32)


def octahedron():
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)
    t = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    return v, np.array(t, dtype=np.int32)


def torus(nu=8, nw=6, big=2.0, small=0.7):
    v = np.array([[(big + small * math.cos(2 * math.pi * j / nw)) * math.cos(2 * math.pi * i / nu),
                   (big + small * math.cos(2 * math.pi * j / nw)) * math.sin(2 * math.pi * i / nu), small * math.sin(2 * math.pi * j / nw)]
                  for i in range(nu) for j in range(nw)])
    idx = lambda i, j: (i % nu) * nw + (j % nw)  # noqa: E731
    t = [tri for i in range(nu) for j in range(nw)
         for tri in ((idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)))]
    return v, np.array(t, dtype=np.int32)


def l_prism(height=1.0):
    """An L-shaped hexagon times a height: non-convex (the corner at (1, 1) is reflex), watertight, normals outwards.  The two arms end in
    slanted faces that meet the outer walls at 45 degrees: at such a sharp edge the normals of the two faces are more than a right angle apart,
    so a query whose closest point is on the edge can lie behind the plane of one of them -- where the closest face's normal gives the wrong
    sign and the pseudonormal does not."""
    poly = [(0, 0), (3, 0), (2, 1), (1, 1), (1, 2), (0, 3)]                      # counter-clockwise, area 4
    v = np.array([[x, y, z] for z in (0.0, height) for x, y in poly], dtype=np.float64)
    fan = [(0, 1, 2), (0, 2, 3), (0, 3, 4), (0, 4, 5)]                          # vertex 0 sees the whole L
    t = [(a, c, b) for a, b, c in fan] + [(a + 6, b + 6, c + 6) for a, b, c in fan]
    for i in range(6):
        j = (i + 1) % 6
        t += [(i, j, j + 6), (i, j + 6, i + 6)]
    return v, np.array(t, dtype=np.int32)


def joined(a, b, shared):
    """Mesh a and mesh b with b's vertices `shared` (a dict b-index -> a-index) merged into a's."""
    (va, ta), (vb, tb) = a, b
    remap, extra = {}, []
    for i in range(len(vb)):
        if i in shared:
            remap[i] = shared[i]
        else:
            remap[i] = len(va) + len(extra)
            extra.append(vb[i])
    v = np.concatenate([va, np.array(extra).reshape(-1, 3)])
    return v, np.concatenate([ta, np.vectorize(remap.get)(tb).astype(np.int32)])


def two_tetrahedra_vertex():
    a = tetrahedron()
    b = (-a[0], a[1][:, ::-1].copy())               # the point reflection, re-wound to point outwards; shares the origin
    return joined(a, b, {0: 0})


def two_tetrahedra_edge():
    a = tetrahedron()
    vb = a[0] * np.array([1.0, -1.0, -1.0])         # rotated half a turn about the x axis: shares the edge (0, 1), wound as a is
    return joined(a, (vb, a[1].copy()), {0: 0, 1: 1})


def bipyramid(n):
    ring = [[math.cos(2 * math.pi * i / n), math.sin(2 * math.pi * i / n), 0.0] for i in range(n)]
    v = np.array(ring + [[0, 0, 1.0], [0, 0, -1.0]])
    t = [(i, (i + 1) % n, n) for i in range(n)] + [((i + 1) % n, i, n + 1) for i in range(n)]
    return v, np.array(t, dtype=np.int32)


def strip(n):
    v = np.array([[0.5 * i, float(i % 2), 0.01 * i * i] for i in range(n + 2)])
    return v, np.array([(i, i + 1, i + 2) if i % 2 == 0 else (i + 1, i, i + 2) for i in range(n)], dtype=np.int32)


def book(n):
    """n faces on one edge."""
    v = np.array([[0, 0, 0], [0, 0, 1.0]] + [[math.cos(0.09 * i), math.sin(0.09 * i), 0.5] for i in range(n)])
    return v, np.array([(0, 1, 2 + i) for i in range(n)], dtype=np.int32)


def mc_sphere(n=17, radius=None):
    from gens_amd import mc_tables
    from oracle import mc_oracle
    radius = 0.31 * (n - 1) if radius is None else radius
    g = np.arange(n, dtype=np.float64) - 0.5 * (n - 1) - 0.123
    x, y, z = np.meshgrid(g, g + 0.21, g - 0.37, indexing="ij")
    u = (np.sqrt(x * x + y * y + z * z) - radius).astype(np.float32)
    v, t = mc_oracle.marching_cubes(u, 0.0, mc_tables.TRI_TABLE, mc_tables.TRI_COUNT)
    return np.asarray(v, dtype=np.float64), np.asarray(t, dtype=np.int32)


def reversed_faces(mesh):
    return mesh[0], mesh[1][:, ::-1].copy()


def hand_shapes():
    """name -> (vertices, triangles): the shapes whose answers are known by hand."""
    cv, ct = cube()
    tv, tt = tetrahedron()
    odd = np.array([[0, 1, 2], [0, 1, 2], [3, 3, 4], [0, 2, 9], [-1, 2, 3], [1, 3, 2]], dtype=np.int32)
    return {
        "triangle": (tv[:3], np.array([[0, 1, 2]], dtype=np.int32)),
        "two_consistent": (tv, np.array([[0, 1, 2], [1, 0, 3]], dtype=np.int32)),
        "two_flipped": (tv, np.array([[0, 1, 2], [0, 1, 3]], dtype=np.int32)),
        "three_on_edge": book(3),
        "tetrahedron": (tv, tt), "cube": (cv, ct), "octahedron": octahedron(), "cube_reversed": reversed_faces((cv, ct)),
        "torus": torus(), "tetrahedra_vertex": two_tetrahedra_vertex(), "tetrahedra_edge": two_tetrahedra_edge(),
        "cube_open": (cv, ct[2:]), "l_prism": l_prism(),
        "odd_faces": (np.concatenate([tv, [[2.0, 2.0, 2.0], [3.0, 3.0, 3.0]]]), odd),
        "empty": (np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int32)),
        "no_faces": (tv, np.zeros((0, 3), dtype=np.int32)),
    }


WATERTIGHT = ("tetrahedron", "cube", "octahedron", "cube_reversed", "torus", "l_prism")


def sign_queries(vertices, triangles, seed, n=2000, offset=0.05):
    """`n` seeded random points in 1.5 x the bounding box, plus a point along the outward bisector of every edge and vertex: the
    normalised pseudonormal, `offset` x the diagonal away (only where the table has one: class-2 edges, vertices without flag bits 1 - 4)."""
    v = np.asarray(vertices, dtype=np.float64)
    topo = topology(v, triangles)
    lo, hi = v.min(0), v.max(0)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    diag = float(np.linalg.norm(hi - lo))
    rng = np.random.default_rng(seed)
    pts = [mid + 1.5 * half * rng.uniform(-1.0, 1.0, size=(n, 3))]
    for e in range(len(topo["edges"])):
        nrm = topo["edge_normal"][e]
        if topo["edge_class"][e] == 2 and np.linalg.norm(nrm) > 0:
            pts.append((0.5 * (v[topo["edges"][e, 0]] + v[topo["edges"][e, 1]]) + offset * diag * nrm / np.linalg.norm(nrm))[None])
    for x in range(len(v)):
        nrm = topo["vertex_normal"][x]
        if topo["vertex_flags"][x] & 1 and not topo["vertex_flags"][x] & NO_SIGN_FLAGS and np.linalg.norm(nrm) > 0:
            pts.append((v[x] + offset * diag * nrm / np.linalg.norm(nrm))[None])
    return np.concatenate(pts), diag


def precondition(queries, near, dot, normals, diag):
    """Every query at least 1e-6 x diagonal from the mesh and (q - p) . n at least 1e-6 |q - p| |n| from zero."""
    u = np.asarray(queries) - near["point"]
    return bool((np.sqrt(near["dist2"]) >= 1e-6 * diag).all() and
                (np.abs(dot) >= 1e-6 * np.linalg.norm(u, axis=1) * np.linalg.norm(normals, axis=1)).all())
