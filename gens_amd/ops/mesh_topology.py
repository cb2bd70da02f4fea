"""K37: the undirected edge table of a triangle mesh on the device (mesh_topology), the topology report built from it (closed, oriented,
manifold, Euler characteristic, genus, boundary loops, pinched vertices, area, signed volume), Baerentzen-Aanaes pseudonormals and the exact
sign of K36's distance (signed_distance_to_mesh).  The definitions are the comment of K37 in include/gens_hip.h;
tests/mesh_topology_reference.py restates them in numpy with dicts and loops.

Part of gens_amd.ops (see ops/__init__.py)."""
from .base import *  # noqa: F401,F403
from .geometry import MeshGrid, face_components
from .mesh_distance import mesh_closest_dist2
from .winding import WINDING_SIGNS, WindingPlan, mesh_inside, winding_beta, winding_sign

_f64, _i32, _i64, _u8 = torch.float64, torch.int32, torch.int64, torch.uint8
EDGE_BOUNDARY, EDGE_MANIFOLD, EDGE_FLIPPED, EDGE_NONMANIFOLD = 1, 2, 3, 4
VERTEX_REFERENCED, VERTEX_BOUNDARY, VERTEX_NONMANIFOLD_EDGE, VERTEX_FLIPPED_EDGE, VERTEX_PINCHED = 1, 2, 4, 8, 16
_EDGE_SENTINEL = 2 ** 63 - 1           # the key of a half-edge of a face that is not valid

topology_section_hook = None           # a callable(name), called where a part of mesh_topology begins (scripts/mesh_topology_bench.py records HIP events there)


def _topology_section(name):
    if topology_section_hook is not None:
        topology_section_hook(name)


def _union_labels(pairs, n):
    """K23's union-find over `n` nodes: pairs (P, 2) int32 -> labels (n) int32, the smallest member of each node's set."""
    parent = torch.arange(n, device=pairs.device, dtype=_i32)
    label = torch.empty(n, device=pairs.device, dtype=_i32)
    if n == 0:
        return label
    if pairs.shape[0]:
        L.call("gens_face_cc_hook", L.ptr(pairs, _i32), pairs.shape[0], L.ptr(parent, _i32), n, L.stream())
    L.call("gens_face_cc_compress", L.ptr(parent, _i32), n, L.ptr(label, _i32), L.stream())
    return label


def area_volume(vertices, triangles, valid):
    """The area and the signed volume of report(), as 0-d device tensors: vertices (V, 3) float64, triangles (T, 3) int32 with T > 0, valid (T)
    bool (K37's face_valid; other faces add nothing).  volume = sum of a . (b x c) / 6.  No read-back."""
    a, b, c = (vertices[torch.where(valid, triangles[:, k], torch.zeros_like(triangles[:, k])).long()] for k in range(3))
    keep = valid.to(_f64)
    area = (0.5 * torch.linalg.cross(b - a, c - a).square().sum(dim=1).sqrt() * keep).sum()
    volume = ((a * torch.linalg.cross(b, c)).sum(dim=1) * keep).sum() / 6.0
    return area, volume


class MeshTopology:
    """What ops.mesh_topology found, as device tensors (E edges, T faces, V vertices; the definitions: include/gens_hip.h, K37):
        edges (E, 2) int32 (lo, hi) in ascending order; edge_count (E) int32; edge_forward (E) int32: uses that run lo -> hi;
        edge_halfedges (E, 2) int32: the two smallest half-edges, -1 where there is none; edge_class (E) uint8: 1 boundary, 2 manifold,
        3 flipped, 4 non-manifold; edge_of_halfedge (3 T) int32, -1 for faces that are not valid; face_valid (T) bool;
        valence (V) int32; fans (V) int32; vertex_flags (V) uint8: bit 0 referenced, 1 on a boundary edge, 2 on a non-manifold edge, 3 on a
        flipped edge, 4 pinched; corner_label (3 T) int32; face_component (T) int32: ops.face_components over the pairs of the class-2 and
        class-3 edges; with normals=True: face_normal (T, 3), edge_normal (E, 3), vertex_normal (V, 3) float64 (the sums, not normalised),
        else None; edge_start (E + 1) int32 and halfedge_order (3 T) int32: the edges' runs in the half-edges stably sorted by edge key, and
        corner_start (V + 1), corner_order (3 T): the vertices' corner segments (K38 and K39 walk them again).  report(): the figures as Python
        numbers, in one read-back."""

    def __init__(self, vertices, triangles):
        self.vertices, self.triangles = vertices, triangles
        self.n_vertices, self.n_faces, self.n_edges = vertices.shape[0], triangles.shape[0], 0
        self.face_normal = self.edge_normal = self.vertex_normal = None
        self._report = None

    @property
    def has_normals(self):
        return self.face_normal is not None

    def report(self):
        """-> {"vertices", "vertices_referenced", "faces", "faces_invalid", "edges", "edges_boundary", "edges_manifold", "edges_flipped",
        "edges_nonmanifold", "vertices_pinched", "vertices_nonmanifold", "components", "largest_component_faces", "boundary_components",
        "euler", "closed", "oriented", "manifold", "watertight", "genus" (None unless watertight), "area", "volume"}: Python numbers.
        volume = sum of a . (b x c) / 6 over the valid faces: meaningful when watertight, negative for an inside-out mesh."""
        if self._report is not None:
            return dict(self._report)
        dev, nv, nt, ne = self.vertices.device, self.n_vertices, self.n_faces, self.n_edges
        zero = torch.zeros((), device=dev, dtype=_f64)
        flags = self.vertex_flags
        # (counts by comparison and sizes by sort and search, not torch.bincount: on a closed manifold mesh every edge has one class and every
        # face one component, and a histogram's atomics all land on one address -- 12 ms for 930 000 faces; nor anything whose result's SIZE
        # depends on the data, which would read it back: the figures' copy below is the only read-back)
        classes = torch.stack([(self.edge_class == k).sum() for k in range(5)]).to(_f64)
        valid = self.face_valid
        referenced = (flags & VERTEX_REFERENCED) != 0
        pinched = (flags & VERTEX_PINCHED) != 0
        bad_vertex = referenced & ((flags & (VERTEX_NONMANIFOLD_EDGE | VERTEX_PINCHED)) != 0)
        if nt:
            components = ((self.face_component == torch.arange(nt, device=dev, dtype=_i32)) & valid).sum().to(_f64)
            label = torch.sort(torch.where(valid, self.face_component, torch.full_like(self.face_component, nt)))[0]     # (not valid: last, under T)
            size = torch.searchsorted(label, label, right=True) - torch.searchsorted(label, label)                      # each face's component's size
            largest = torch.where(label < nt, size, torch.zeros_like(size)).max().to(_f64)
            area, volume = area_volume(self.vertices, self.triangles, valid)
        else:
            components = largest = area = volume = zero
        if nv:
            rim = _c(torch.where((self.edge_class == EDGE_BOUNDARY)[:, None], self.edges, torch.full_like(self.edges, -1)))     # (the hook skips ids below 0)
            loops = _union_labels(rim, nv)
            boundary = ((loops == torch.arange(nv, device=dev, dtype=_i32)) & ((flags & VERTEX_BOUNDARY) != 0)).sum().to(_f64)
        else:
            boundary = zero
        figures = torch.stack([referenced.sum().to(_f64), valid.sum().to(_f64), classes[1], classes[2], classes[3], classes[4],
                               pinched.sum().to(_f64), bad_vertex.sum().to(_f64), components, largest, boundary, area, volume]).cpu().tolist()
        n_ref, n_valid, e1, e2, e3, e4, n_pinched, n_bad, n_comp, n_largest, n_loops = (int(x) for x in figures[:11])
        out = {"vertices": nv, "vertices_referenced": n_ref, "faces": nt, "faces_invalid": nt - n_valid, "edges": ne, "edges_boundary": e1,
               "edges_manifold": e2, "edges_flipped": e3, "edges_nonmanifold": e4, "vertices_pinched": n_pinched, "vertices_nonmanifold": n_bad,
               "components": n_comp, "largest_component_faces": n_largest, "boundary_components": n_loops, "euler": n_ref - ne + n_valid}
        out["closed"] = e1 == 0 and e4 == 0 and n_valid > 0
        out["oriented"] = e3 == 0
        out["manifold"] = e4 == 0 and n_pinched == 0
        out["watertight"] = out["closed"] and out["oriented"] and out["manifold"]
        out["genus"] = (2 * n_comp - out["euler"]) // 2 if out["watertight"] else None
        out["area"], out["volume"] = float(figures[11]), float(figures[12])
        self._report = out
        return dict(out)


def _check_mesh(who, vertices, triangles):
    for name, t, dtype in (("vertices", vertices, _f64), ("triangles", triangles, _i32)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError(f"{who}: {name} is not a tensor on the device (gens_amd kernels have no CPU path)")
        if t.dtype != dtype or t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{who}: {name} is {tuple(t.shape)} {t.dtype}, expected (n, 3) {dtype}")
    if triangles.device != vertices.device:
        raise ValueError(f"{who}: vertices on {vertices.device}, triangles on {triangles.device}")
    if vertices.shape[0] >= 2 ** 31 or 3 * triangles.shape[0] >= 2 ** 31:
        raise ValueError(f"{who}: {vertices.shape[0]} vertices, {triangles.shape[0]} triangles (V and 3 T below 2^31)")


def mesh_topology(vertices, triangles, normals=False):
    """K37.  vertices (V, 3) float64, triangles (T, 3) int32 on the device -> MeshTopology: the edge table, the classes of edges and
    vertices, the fans, the face components and, with normals=True, the face normals and the edge and vertex pseudonormals.  Any indices
    are accepted: a face with an index outside the vertices or a repeated one is counted (report()["faces_invalid"]) and takes part in
    nothing else.  Two sorts (half-edges by edge, corners by vertex), run lengths and prefix sums in torch; the rest in K37's kernels and
    K23's union-find.  Deterministic.  ValueError before any launch for anything but such tensors, or a `normals` that is no bool."""
    who = "mesh_topology"
    _check_mesh(who, vertices, triangles)
    if not isinstance(normals, bool):
        raise ValueError(f"{who}: normals = {normals!r}: True or False")
    v, t = _c(vertices.detach()), _c(triangles.detach())
    dev, nv, nt = v.device, v.shape[0], t.shape[0]
    nh = 3 * nt
    topo = MeshTopology(v, t)
    _topology_section("keys")
    key = torch.empty(nh, device=dev, dtype=_i64)
    forward = torch.empty(nh, device=dev, dtype=_u8)
    if nt:
        L.call("gens_mesh_edge_keys", L.ptr(t, _i32), nt, nv, L.ptr(key, _i64), L.ptr(forward, _u8), L.stream(), nbytes=nt * 12 + nh * 9)
    _topology_section("edge_sort")
    key, order = torch.sort(key, stable=True)
    order = order.to(_i32)
    edge_key, counts = torch.unique_consecutive(key, return_counts=True)
    ne = int((edge_key != _EDGE_SENTINEL).sum()) if nt else 0
    edge_key = _c(edge_key[:ne])
    seg_start = torch.zeros(ne + 1, device=dev, dtype=_i32)
    seg_start[1:] = torch.cumsum(counts[:ne], 0).to(_i32)
    del key, counts
    topo.edge_start, topo.halfedge_order = seg_start, order                    # (the edges' half-edge runs: K39's cotangent weights walk them again)
    _topology_section("edge_classify")
    topo.n_edges = ne
    topo.edges = torch.empty(ne, 2, device=dev, dtype=_i32)
    topo.edge_count, topo.edge_forward = torch.empty(ne, device=dev, dtype=_i32), torch.empty(ne, device=dev, dtype=_i32)
    topo.edge_halfedges = torch.empty(ne, 2, device=dev, dtype=_i32)
    topo.edge_class = torch.empty(ne, device=dev, dtype=_u8)
    topo.edge_of_halfedge = torch.empty(nh, device=dev, dtype=_i32)
    if nt:
        L.call("gens_mesh_edge_classify", L.ptr(edge_key, _i64), L.ptr(seg_start, _i32), L.ptr(order, _i32), L.ptr(forward, _u8), ne, nh,
               L.ptr(topo.edges, _i32), L.ptr(topo.edge_count, _i32), L.ptr(topo.edge_forward, _i32), L.ptr(topo.edge_halfedges, _i32),
               L.ptr(topo.edge_class, _u8), L.ptr(topo.edge_of_halfedge, _i32), L.stream(), nbytes=ne * 33 + nh * 9)
    topo.face_valid = topo.edge_of_halfedge.view(nt, 3)[:, 0] >= 0
    _topology_section("fans")
    pairs = torch.empty(2 * ne, 2, device=dev, dtype=_i32)
    if ne:
        L.call("gens_mesh_fan_pairs", L.ptr(t, _i32), nt, L.ptr(topo.edges, _i32), L.ptr(topo.edge_halfedges, _i32), L.ptr(topo.edge_class, _u8), ne,
               L.ptr(pairs, _i32), L.stream(), nbytes=ne * 57)
    topo.corner_label = _union_labels(pairs, nh)
    del pairs
    _topology_section("corner_sort")
    corner_vertex = torch.where(topo.edge_of_halfedge >= 0, t.reshape(-1), torch.full((nh,), nv, device=dev, dtype=_i32))
    corner_order = torch.sort(corner_vertex, stable=True)[1].to(_i32)
    corner_start = torch.zeros(nv + 1, device=dev, dtype=_i32)
    if nt and nv:
        corner_start[1:] = torch.cumsum(torch.bincount(corner_vertex.long(), minlength=nv + 1)[:nv], 0).to(_i32)
    del corner_vertex
    topo.corner_order, topo.corner_start = corner_order, corner_start          # (the vertices' corner segments: K38's split walks them again)
    _topology_section("vertex_classify")
    topo.valence, topo.fans = torch.empty(nv, device=dev, dtype=_i32), torch.empty(nv, device=dev, dtype=_i32)
    topo.vertex_flags = torch.empty(nv, device=dev, dtype=_u8)
    if nv:
        L.call("gens_mesh_vertex_classify", L.ptr(corner_order, _i32), L.ptr(corner_start, _i32), L.ptr(topo.corner_label, _i32),
               L.ptr(topo.edge_of_halfedge, _i32), L.ptr(topo.edge_class, _u8), nv, nh, ne, L.ptr(topo.valence, _i32), L.ptr(topo.fans, _i32),
               L.ptr(topo.vertex_flags, _u8), L.stream(), nbytes=nv * 13 + nh * 16)
    _topology_section("components")
    if ne:
        across = (topo.edge_class == EDGE_MANIFOLD) | (topo.edge_class == EDGE_FLIPPED)
        face_pairs = _c(torch.div(topo.edge_halfedges[across], 3, rounding_mode="floor").to(_i32))
    else:
        face_pairs = torch.zeros(0, 2, device=dev, dtype=_i32)
    topo.face_component = face_components(t, nv, pairs=face_pairs)
    if normals:
        _topology_section("normals")
        topo.face_normal = torch.empty(nt, 3, device=dev, dtype=_f64)
        topo.edge_normal = torch.empty(ne, 3, device=dev, dtype=_f64)
        topo.vertex_normal = torch.empty(nv, 3, device=dev, dtype=_f64)
        if nt or nv:
            L.call("gens_mesh_pseudonormals", L.ptr(v, _f64), L.ptr(t, _i32), nv, nt, ne, L.ptr(seg_start, _i32), L.ptr(order, _i32),
                   L.ptr(corner_start, _i32), L.ptr(corner_order, _i32), L.ptr(topo.face_normal, _f64), L.ptr(topo.edge_normal, _f64),
                   L.ptr(topo.vertex_normal, _f64), L.stream(), nbytes=nt * 108 + ne * 24 + nv * 24 + nh * 32)
    _topology_section("end")
    return topo


def _check_sign_topology(who, grid, topology):
    if not isinstance(grid, MeshGrid):
        raise ValueError(f"{who}: grid is {type(grid).__name__}, expected ops.build_mesh_grid's MeshGrid")
    if not isinstance(topology, MeshTopology):
        raise ValueError(f"{who}: topology is {type(topology).__name__}, expected ops.mesh_topology's MeshTopology")
    if not topology.has_normals:
        raise ValueError(f"{who}: the topology was built without normals (ops.mesh_topology(vertices, triangles, normals=True))")
    if topology.n_vertices != grid.vertices.shape[0] or topology.n_faces != grid.n_faces:
        raise ValueError(f"{who}: the topology is of another mesh ({topology.n_vertices} vertices, {topology.n_faces} faces; the grid's mesh has "
                         f"{grid.vertices.shape[0]} and {grid.n_faces})")
    if topology.vertices.device != grid.vertices.device:
        raise ValueError(f"{who}: the topology on {topology.vertices.device}, the grid on {grid.vertices.device}")


def distance_sign(queries, dist2, face, point, region, topology):
    """gens_mesh_distance_sign: K36's results for `queries` against the mesh of `topology` (built with normals) -> signed (n) float64."""
    n = queries.shape[0]
    signed = torch.full((n,), float("nan"), device=queries.device, dtype=_f64)
    if n == 0 or topology.n_faces == 0:
        return signed
    tp = topology
    L.call("gens_mesh_distance_sign", L.ptr(queries, _f64), n, L.ptr(dist2, _f64), L.ptr(face, _i32), L.ptr(point, _f64), L.ptr(region, _u8),
           L.ptr(tp.triangles, _i32), tp.n_faces, tp.n_vertices, tp.n_edges, L.ptr(tp.face_normal, _f64), L.ptr(tp.edge_normal, _f64),
           L.ptr(tp.vertex_normal, _f64), L.ptr(tp.edge_of_halfedge, _i32), L.ptr(tp.edge_class, _u8), L.ptr(tp.vertex_flags, _u8),
           L.ptr(signed, _f64), L.stream(), nbytes=n * 69)
    return signed


def _winding_signed_distance(who, queries, grid, winding, beta, max_dist, chunk):
    """signed_distance_to_mesh's sign="winding" route: K36's distance, K40's inside test."""
    if not isinstance(grid, MeshGrid):
        raise ValueError(f"{who}: grid is {type(grid).__name__}, expected ops.build_mesh_grid's MeshGrid")
    if not isinstance(winding, WindingPlan):
        raise ValueError(f"{who}: winding is {type(winding).__name__}, expected ops.build_winding_plan's WindingPlan of the grid's mesh "
                         f"(sign=\"winding\" takes its sign from it)")
    if winding.n_vertices != grid.vertices.shape[0] or winding.n_faces != grid.n_faces:
        raise ValueError(f"{who}: the winding plan is of another mesh ({winding.n_vertices} vertices, {winding.n_faces} faces; the grid's mesh "
                         f"has {grid.vertices.shape[0]} and {grid.n_faces})")
    if winding.vertices.device != grid.vertices.device:
        raise ValueError(f"{who}: the winding plan on {winding.vertices.device}, the grid on {grid.vertices.device}")
    winding_beta(who, beta)
    dist2, face, _, _ = mesh_closest_dist2(queries, grid, max_dist, False, False, chunk)
    return winding_sign(dist2, mesh_inside(queries, winding, beta, chunk, who=who)), face


def signed_distance_to_mesh(queries, grid, topology=None, max_dist=float("inf"), chunk=None, sign="pseudonormal", winding=None, beta=None):
    """K36's distance with K37's sign.  queries (n, 3) float64 on the device, grid = ops.build_mesh_grid(vertices, triangles), topology =
    ops.mesh_topology(vertices, triangles, normals=True) of the same mesh -> (signed (n) float64, face (n) int32).  |signed| is
    closest_point_on_mesh's distance; the sign is that of (q - closest point) . n with n the face normal, or the angle-weighted vertex
    normal, or the sum of the edge's two face normals, by where on the face the closest point lies: positive on the side the face normals
    point to, so negative inside a mesh whose normals point outwards.  Exact for a watertight mesh.  +0 on the mesh.
    NaN where there is no sign: nothing within max_dist, a closest point on a boundary, flipped or non-manifold edge or on a vertex of
    such an edge or a pinched one, a degenerate closest face, a query at right angles to the normal.  One K36 launch per chunk and one sign
    launch.  sign="winding" (K40; the default route issues not one more launch and is what it was, bit for bit): the sign comes from the
    generalised winding number instead -- winding = ops.build_winding_plan(vertices, triangles) of the same mesh, beta as ops.mesh_inside
    takes it (None: exact), `topology` is not needed -- -d where mesh_inside says 1, +d where it says 0, NaN where it is undecided or
    nothing lies within max_dist, +0 on the mesh.  It has a sign where K37 has none (a closest point on a rim, a pinch, a fold; a soup) and
    says whether the query is inside the OBJECT, not on which side of the nearest sheet it lies; inside an inside-out mesh nothing is
    (ops.repair_mesh re-orients).  ValueError before any launch for what closest_point_on_mesh refuses, a topology without normals or of
    another mesh, a sign that is neither name, a winding plan or beta without sign="winding", a plan of another mesh, a bad beta."""
    who = "signed_distance_to_mesh"
    if sign not in WINDING_SIGNS:
        raise ValueError(f"{who}: sign = {sign!r}: one of {', '.join(WINDING_SIGNS)}")
    if sign == "winding":
        return _winding_signed_distance(who, queries, grid, winding, beta, max_dist, chunk)
    if winding is not None or beta is not None:
        raise ValueError(f"{who}: winding and beta go with sign=\"winding\"")
    _check_sign_topology(who, grid, topology)
    dist2, face, point, region = mesh_closest_dist2(queries, grid, max_dist, True, True, chunk)
    return distance_sign(_c(queries.detach()), dist2, face, point, region, topology), face


__all__ = [n_ for n_ in dir() if not n_.startswith("__")]
