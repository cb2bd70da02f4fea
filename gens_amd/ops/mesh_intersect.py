"""K41: the self-intersections of a triangle mesh -- which pairs of its faces intersect, each pair decided exactly or reported as undecided,
never guessed (mesh_self_intersections over K23's grid; self_intersections_of for a mesh with any indices).  A report only: nothing is
removed or repaired.  The definitions are the comment of K41 in include/gens_hip.h; tests/mesh_intersect_reference.py
decides the same question in rational arithmetic.

Part of gens_amd.ops (see ops/__init__.py)."""
import ctypes as C

from .base import *  # noqa: F401,F403
from .geometry import MeshGrid, build_mesh_grid

_f64, _i32, _i64, _u8 = torch.float64, torch.int32, torch.int64, torch.uint8
FACE_INVALID, FACE_ORDINARY, FACE_DEGENERATE, FACE_UNCERTAIN = 0, 1, 2, 3
PAIR_INTERSECTING, PAIR_UNDECIDED = 1, 2
SELF_INTERSECTION_KEYS = ("faces", "invalid_faces", "degenerate_faces", "uncertain_faces", "duplicate_pairs", "candidates", "intersecting",
                          "undecided", "faces_intersecting", "faces_undecided")

intersect_section_hook = None          # a callable(name), called where a part of mesh_self_intersections begins (scripts/mesh_intersect_bench.py)


def _section(name):
    if intersect_section_hook is not None:
        intersect_section_hook(name)


class SelfIntersections:
    """What ops.mesh_self_intersections found: counts (a dict of Python ints: SELF_INTERSECTION_KEYS, and "plane_separated": the
    candidates one strict plane separation decided alone); face_flags (T) uint8 on the device: bit 0 for a face of an intersecting pair,
    bit 1 of an undecided one; face_class (T) uint8: 0 not valid, 1 ordinary, 2 degenerate, 3 uncertain; with pairs=True: pairs (n, 2)
    int32 ascending by (s, t), s < t, and kinds (n) uint8: 1 intersecting, 2 undecided -- else None."""

    def __init__(self, counts, face_flags, face_class, pairs=None, kinds=None):
        self.counts, self.face_flags, self.face_class, self.pairs, self.kinds = counts, face_flags, face_class, pairs, kinds


def check_intersect_request(who, pairs=True, max_pairs=None):
    """The keywords of mesh_self_intersections, checked on the host."""
    if not isinstance(pairs, bool):
        raise ValueError(f"{who}: pairs = {pairs!r}: True or False")
    if max_pairs is not None and (isinstance(max_pairs, bool) or not isinstance(max_pairs, int) or max_pairs < 1):
        raise ValueError(f"{who}: max_pairs = {max_pairs!r}: a positive whole number of pairs, or None")


def mesh_self_intersections(grid, pairs=True, max_pairs=None):
    """K41.  grid = ops.build_mesh_grid(vertices, triangles) -> SelfIntersections.  Every pair of valid, non-degenerate faces that share
    fewer than three vertex indices and whose closed AABBs overlap is a candidate, met once in the cell of K23's grid that holds the lower
    corner of the two boxes' intersection, and decided INTERSECTING, DISJOINT or UNDECIDED by predicates whose signs are certified in
    float64 (a static error bound, else a check that every operation was exact) -- sharing is by index: faces that touch at two unwelded
    copies of a vertex intersect.  counts is always complete; pairs=False launches no emit; max_pairs keeps the pairs with the smallest
    (s, t).  The result depends on neither the grid nor the order inside a cell, and a pair's verdict not on the faces' numbering.  A mesh
    without faces launches nothing.  Two read-backs (the lists' size, the counts).  ValueError before any launch for a grid that is no
    MeshGrid, a pairs that is no bool, a max_pairs that is no positive int or None; RuntimeError for 2^31 or more pairs to emit."""
    who = "mesh_self_intersections"
    if not isinstance(grid, MeshGrid):
        raise ValueError(f"{who}: grid is {type(grid).__name__}, expected ops.build_mesh_grid's MeshGrid")
    check_intersect_request(who, pairs, max_pairs)
    dev, nt, nv = grid.vertices.device, grid.n_faces, grid.vertices.shape[0]
    counts = dict.fromkeys(SELF_INTERSECTION_KEYS + ("plane_separated",), 0)
    counts["faces"] = nt
    empty = (torch.zeros(0, 2, device=dev, dtype=_i32), torch.zeros(0, device=dev, dtype=_u8)) if pairs else (None, None)
    if nt == 0:
        return SelfIntersections(counts, torch.zeros(0, device=dev, dtype=_u8), torch.zeros(0, device=dev, dtype=_u8), *empty)
    _section("faces")
    face_class = torch.empty(nt, device=dev, dtype=_u8)
    face_box = torch.empty(nt, 6, device=dev, dtype=_f64)
    L.call("gens_mesh_isect_faces", L.ptr(grid.vertices, _f64), nv, L.ptr(grid.triangles, _i32), nt, L.ptr(face_class, _u8), L.ptr(face_box, _f64),
           L.stream(), nbytes=nt * (12 + 72 + 49))
    cells = grid.dims[0] * grid.dims[1] * grid.dims[2]
    lists = grid.cell_start[1:] - grid.cell_start[:-1]
    n_entries, longest = (int(x) for x in torch.stack([grid.cell_start[-1], lists.max()]).cpu())
    _section("count")
    cell_counts = torch.zeros(cells, 2, device=dev, dtype=_i32)
    totals = torch.zeros(3, device=dev, dtype=_i64)
    flags = torch.zeros(4 * ((nt + 3) // 4), device=dev, dtype=_u8)
    args = grid.args()
    L.call("gens_mesh_isect_count", C.byref(args), nv, n_entries, longest, L.ptr(face_class, _u8), L.ptr(face_box, _f64), L.ptr(cell_counts, _i32),
           L.ptr(totals, _i64), L.ptr(flags, _u8), L.stream(), nbytes=n_entries * 4 + nt * 64)
    _section("figures")
    face_flags = flags[:nt]
    per_class = cell_counts.sum(dim=0, dtype=_i64)
    figures = torch.cat([totals, per_class, torch.stack([(face_class == k).sum() for k in (0, 2, 3)]),
                         torch.stack([((face_flags & 1) != 0).sum(), ((face_flags & 2) != 0).sum()])]).cpu().tolist()
    (counts["candidates"], counts["duplicate_pairs"], counts["plane_separated"], counts["intersecting"], counts["undecided"],
     counts["invalid_faces"], counts["degenerate_faces"], counts["uncertain_faces"], counts["faces_intersecting"],
     counts["faces_undecided"]) = (int(x) for x in figures)
    if not pairs:
        return SelfIntersections(counts, face_flags, face_class)
    n_out = counts["intersecting"] + counts["undecided"]
    if n_out >= 2 ** 31:
        raise RuntimeError(f"{who}: {n_out} pairs to emit (below 2^31; pairs=False still counts them)")
    if n_out == 0:
        return SelfIntersections(counts, face_flags, face_class, *empty)
    _section("emit")
    out_start = torch.zeros(cells + 1, device=dev, dtype=_i32)
    out_start[1:] = torch.cumsum(cell_counts.sum(dim=1, dtype=_i64), 0).to(_i32)
    cursor = torch.zeros(cells, device=dev, dtype=_i32)
    out_pairs = torch.empty(n_out, 2, device=dev, dtype=_i32)
    kinds = torch.empty(n_out, device=dev, dtype=_u8)
    L.call("gens_mesh_isect_emit", C.byref(args), nv, n_entries, longest, L.ptr(face_class, _u8), L.ptr(face_box, _f64), L.ptr(out_start, _i32),
           L.ptr(cursor, _i32), n_out, L.ptr(out_pairs, _i32), L.ptr(kinds, _u8), L.stream(), nbytes=n_entries * 4 + nt * 64 + n_out * 9)
    _section("sort")
    order = torch.sort((out_pairs[:, 0].to(_i64) << 32) | out_pairs[:, 1].to(_i64))[1]
    if max_pairs is not None:
        order = order[:max_pairs]
    _section("end")
    return SelfIntersections(counts, face_flags, face_class, _c(out_pairs[order]), _c(kinds[order]))


def self_intersections_of(vertices, triangles, pairs=True, max_pairs=None, who="self_intersections_of"):
    """mesh_self_intersections for a mesh with ANY indices: vertices (V, 3) float64, triangles (T, 3) int32 on the device.  K23's grid takes
    indices inside the vertices only, so a face with an index outside them -- not valid, it takes part in nothing -- is handed on as the row
    (0, 0, 0), which is not valid either; with no vertices at all every face is not valid and nothing is launched.  ValueError for anything but such tensors, and
    build_mesh_grid's for a vertex some face uses (vertex 0 included, once a row was replaced) that is not finite."""
    check_intersect_request(who, pairs, max_pairs)
    for name, t, dtype in (("vertices", vertices, _f64), ("triangles", triangles, _i32)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError(f"{who}: {name} is not a tensor on the device (gens_amd kernels have no CPU path)")
        if t.dtype != dtype or t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{who}: {name} is {tuple(t.shape)} {t.dtype}, expected (n, 3) {dtype}")
    nv, nt = vertices.shape[0], triangles.shape[0]
    if nv == 0 or nt == 0:
        dev = triangles.device
        counts = dict.fromkeys(SELF_INTERSECTION_KEYS + ("plane_separated",), 0)
        counts["faces"] = counts["invalid_faces"] = nt
        empty = (torch.zeros(0, 2, device=dev, dtype=_i32), torch.zeros(0, device=dev, dtype=_u8)) if pairs else (None, None)
        return SelfIntersections(counts, torch.zeros(nt, device=dev, dtype=_u8), torch.zeros(nt, device=dev, dtype=_u8), *empty)
    inside = ((triangles >= 0) & (triangles < nv)).all(dim=1, keepdim=True)
    return mesh_self_intersections(build_mesh_grid(vertices, torch.where(inside, triangles, torch.zeros_like(triangles))), pairs, max_pairs)


def self_intersection_counts(vertices, triangles, who="self_intersection_counts"):
    """The counts alone (SELF_INTERSECTION_KEYS) of a device mesh with any indices: self_intersections_of(pairs=False), no emit."""
    found = self_intersections_of(vertices, triangles, pairs=False, who=who)
    return {k: found.counts[k] for k in SELF_INTERSECTION_KEYS}


__all__ = [n_ for n_ in dir() if not n_.startswith("__")]
