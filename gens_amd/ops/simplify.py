"""K33: mesh simplification by vertex clustering with quadric-optimal representatives (simplify_mesh).  The definition is the comment of K33
in include/gens_hip.h; tests/mesh_simplify_reference.py restates it in numpy.  Works on any triangle mesh on the
device: an extracted one, a cleaned one, a file's.

Part of gens_amd.ops (see ops/__init__.py)."""
import ctypes as C

import numpy as np

from .base import *  # noqa: F401,F403
from .lookup import compact_valid

_f64, _i32, _i64, _u8 = torch.float64, torch.int32, torch.int64, torch.uint8
SIMPLIFY_AXIS_CELLS = 1 << 21        # cells per axis that a key holds
SIMPLIFY_REG = 1e-3


section_hook = None                  # a callable(name), called where a part of simplify_mesh begins (scripts/mesh_simplify_bench.py records HIP events there)


def _section(name):
    if section_hook is not None:
        section_hook(name)


def simplify_request(who, cell, reg=SIMPLIFY_REG):
    """cell and reg, checked on the host -> (cell, reg) floats.  ValueError unless both are positive and finite."""
    try:
        cell_f, reg_f = (float("nan") if isinstance(cell, bool) else float(cell)), (float("nan") if isinstance(reg, bool) else float(reg))
    except (TypeError, ValueError):
        raise ValueError(f"{who}: cell = {cell!r}, reg = {reg!r}: two numbers") from None
    if not (cell_f > 0.0 and math.isfinite(cell_f)):
        raise ValueError(f"{who}: cell = {cell!r}, the cell edge: positive and finite")
    if not (reg_f > 0.0 and math.isfinite(reg_f)):
        raise ValueError(f"{who}: reg = {reg!r}, the regulariser: positive and finite")
    return cell_f, reg_f


def simplify_origin(lowest, cell):
    """The default origin: per axis cell floor(lowest_a / cell) in float64, so that the grid is aligned to world multiples of `cell` whatever
    the mesh's extent.  lowest: the three per-axis minima of the vertices."""
    return [float(np.float64(cell) * np.floor(np.float64(v) / np.float64(cell))) for v in lowest]


def _compacted(mask, n):
    """The ascending indices of the n set entries of mask (n known on the host; compact_valid's rescue of an empty mask is not a list)."""
    if n == 0:
        return torch.empty(0, device=mask.device, dtype=_i64)
    return compact_valid(mask)[0][:n]


def simplify_mesh(vertices, triangles, cell, origin=None, reg=SIMPLIFY_REG):
    """K33.  vertices (V, 3) float64 and triangles (T, 3) int32 on the device; cell: the edge of the clustering cells, in the vertices' units;
    origin (3): a corner of the cell grid, at or below every vertex (None: per axis cell floor(min_a / cell), computed on the host in
    float64: the grid is aligned to world multiples of `cell`); reg: the weight, relative to the quadric's trace, that pulls a representative
    towards its cluster's mean along directions the cluster's triangles leave free.
    -> (vertices' (V', 3) float64, triangles' (T', 3) int32, source (V',) int64, stats) on the device: one vertex per cluster of input
    vertices that a kept triangle references, in ascending cell order (z, then y, then x), placed where the planes of the cluster's triangles
    meet (within the cell; else at the mean of the cluster's vertices); the triangles that join three different clusters, one per set of
    three clusters, in their input order and orientation; source: per output vertex the input vertex nearest to it within its cluster --
    gather per-vertex arrays with it (normals[source]), attributes are never averaged.  stats: input and output counts, `clusters` (None
    for vertices without triangles: nothing is launched, so they are not counted), `collapsed_triangles`, `duplicate_triangles` and
    `fell_back` (clusters placed at their mean).
    Deterministic: the same input gives the same bits.  Guaranteed: every output vertex lies in its cluster's cell, hence within sqrt(3) cell
    of vertices[source].  NOT guaranteed: topology (sheets less than a cell apart are pinched together, edges can end up with other than two
    faces, components smaller than a cell vanish) and any distance to the true surface.
    The sorts, segment boundaries and the duplicate removal run on the device through torch (stable sorts) and ops.compact_valid; the sizes
    of the outputs are read back (three small host reads).  ValueError before any launch: tensors not on the device or of other types or
    shapes, non-finite vertices, triangle indices outside the vertices, cell or reg not positive and finite, a vertex below origin,
    (max - origin) / cell >= 2^21, V or 3 T >= 2^31."""
    who = "simplify_mesh"
    for name, t, dtype in (("vertices", vertices, _f64), ("triangles", triangles, _i32)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError(f"{who}: {name} is not a tensor on the device (gens_amd kernels have no CPU path)")
        if t.dtype != dtype or t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{who}: {name} is {tuple(t.shape)} {t.dtype}, expected (n, 3) {dtype}")
    if triangles.device != vertices.device:
        raise ValueError(f"{who}: vertices on {vertices.device}, triangles on {triangles.device}")
    cell, reg = simplify_request(who, cell, reg)
    if origin is not None:
        origin = [float(o) for o in (origin.detach().cpu().tolist() if torch.is_tensor(origin) else np.asarray(origin, dtype=np.float64).reshape(-1).tolist())]
        if len(origin) != 3 or not all(math.isfinite(o) for o in origin):
            raise ValueError(f"{who}: origin = {origin!r}: three finite numbers")
    vertices, triangles = _c(vertices.detach()), _c(triangles.detach())
    dev = vertices.device
    n_v, n_t = vertices.shape[0], triangles.shape[0]
    if n_v >= 2 ** 31 or 3 * n_t >= 2 ** 31:
        raise ValueError(f"{who}: {n_v} vertices, {n_t} triangles (V and 3 T below 2^31)")
    # --- the host checks: one read of the extent and the index range
    _section("checks")
    if n_v:
        lo_d, hi_d = vertices.amin(dim=0), vertices.amax(dim=0)      # (a NaN propagates into both)
        lo, hi = lo_d.cpu().tolist(), hi_d.cpu().tolist()
        if not all(math.isfinite(v) for v in lo + hi):
            raise ValueError(f"{who}: a vertex is not finite")
    if n_t:
        t_lo, t_hi = int(triangles.min()), int(triangles.max())
        if t_lo < 0 or t_hi >= n_v:
            raise ValueError(f"{who}: triangle indices {t_lo} .. {t_hi} outside the {n_v} vertices")
    if origin is None:
        origin = simplify_origin(lo, cell) if n_v else [0.0, 0.0, 0.0]
    if n_v:
        for ax in range(3):
            if lo[ax] < origin[ax] or not math.floor((lo[ax] - origin[ax]) / cell) >= 0:
                raise ValueError(f"{who}: a vertex lies below origin on axis {ax} ({lo[ax]!r} < {origin[ax]!r})")
            if not (hi[ax] - origin[ax]) / cell < SIMPLIFY_AXIS_CELLS:
                raise ValueError(f"{who}: (max - origin) / cell = {(hi[ax] - origin[ax]) / cell!r} on axis {ax}: a key holds 2^21 cells per axis")
    stats = {"input_vertices": n_v, "input_triangles": n_t, "clusters": 0, "output_vertices": 0, "output_triangles": 0, "collapsed_triangles": n_t,
             "duplicate_triangles": 0, "fell_back": 0, "cell": cell, "origin": list(origin), "reg": reg}
    empty = (torch.empty(0, 3, device=dev, dtype=_f64), torch.empty(0, 3, device=dev, dtype=_i32), torch.empty(0, device=dev, dtype=_i64))
    if n_v == 0 or n_t == 0:
        if n_v:
            stats["clusters"] = None                               # (not counted: nothing is launched for a mesh without triangles)
        return (*empty, stats)
    # --- 1. keys, clusters, members
    _section("keys")
    keys = torch.empty(n_v, device=dev, dtype=_i64)
    L.call("gens_cluster_keys", L.ptr(vertices, _f64), n_v, origin[0], origin[1], origin[2], cell, L.ptr(keys, _i64), L.stream(), nbytes=n_v * 32)
    _section("sorts")
    sorted_keys, members = torch.sort(keys, stable=True)
    cluster_keys, counts = torch.unique_consecutive(sorted_keys, return_counts=True)
    n_c = int(cluster_keys.shape[0])
    stats["clusters"] = n_c
    member_start = torch.zeros(n_c + 1, device=dev, dtype=_i32)
    member_start[1:] = torch.cumsum(counts, 0)
    first = torch.ones(n_v, device=dev, dtype=_i64)
    first[1:] = sorted_keys[1:] != sorted_keys[:-1]
    vertex_cluster = torch.empty(n_v, device=dev, dtype=_i32)
    vertex_cluster[members] = (torch.cumsum(first, 0) - 1).to(_i32)
    members = members.to(_i32)
    # --- 2. triangles: ranks, survivors, one per set of three clusters
    _section("triangles")
    ranks = torch.empty(n_t, 3, device=dev, dtype=_i32)
    survive = torch.empty(n_t, device=dev, dtype=_u8)
    triple = torch.empty(n_t, 3, device=dev, dtype=_i32)
    L.call("gens_cluster_triangles", L.ptr(triangles, _i32), n_t, L.ptr(vertex_cluster, _i32), n_v, L.ptr(ranks, _i32), L.ptr(survive, _u8),
           L.ptr(triple, _i32), L.stream(), nbytes=n_t * 49)
    _section("duplicates")
    n_s = int(survive.sum())
    stats["collapsed_triangles"] = n_t - n_s
    if n_s == 0:
        return (*empty, stats)
    alive = _compacted(survive, n_s)                               # ascending triangle index
    tr = triple[alive].to(_i64)
    low = tr[:, 1] * (1 << 31) + tr[:, 2]                          # two stable sorts = the lexicographic order of the triples, ties in index order
    order = torch.sort(low, stable=True)[1]
    order = order[torch.sort(tr[order, 0], stable=True)[1]]
    tr = tr[order]
    head = torch.ones(n_s, device=dev, dtype=torch.bool)
    head[1:] = (tr[1:] != tr[:-1]).any(dim=1)
    kept_mask = torch.zeros(n_t, device=dev, dtype=_u8)
    kept_mask[alive[order[head]]] = 1
    n_k = int(head.sum())
    stats["duplicate_triangles"] = n_s - n_k
    kept = _compacted(kept_mask, n_k)
    # --- the output clusters: those a kept triangle references, ascending
    used = torch.zeros(n_c, device=dev, dtype=_u8)
    used[ranks[kept].reshape(-1).to(_i64)] = 1
    new_index = (torch.cumsum(used, 0, dtype=_i64) - 1).to(_i32)
    n_o = int(new_index[-1]) + 1
    out_clusters = _compacted(used, n_o).to(_i32)
    out_triangles = new_index[ranks[kept].to(_i64)]
    # --- 3. the entry segments: 3 t + k sorted stably by cluster
    _section("sorts")
    flat = ranks.reshape(-1)
    entries = torch.sort(flat, stable=True)[1].to(_i32)
    entry_start = torch.zeros(n_c + 1, device=dev, dtype=_i32)
    entry_start[1:] = torch.cumsum(torch.bincount(flat, minlength=n_c), 0)
    # --- 3 to 5. one thread per output cluster
    _section("solve")
    out_vertices = torch.empty(n_o, 3, device=dev, dtype=_f64)
    source = torch.empty(n_o, device=dev, dtype=_i32)
    fell = torch.empty(n_o, device=dev, dtype=_u8)
    args = L.ClusterSolveArgs(L.ptr(vertices, _f64), L.ptr(triangles, _i32), L.ptr(survive, _u8), L.ptr(cluster_keys, _i64), L.ptr(entries, _i32),
                              L.ptr(entry_start, _i32), L.ptr(members, _i32), L.ptr(member_start, _i32), L.ptr(out_clusters, _i32), n_v, n_t, n_c, n_o,
                              (C.c_double * 3)(*origin), cell, reg, L.ptr(out_vertices, _f64), L.ptr(source, _i32), L.ptr(fell, _u8))
    L.call("gens_cluster_solve", C.byref(args), L.stream(), nbytes=n_o * 37 + 3 * n_s * 76 + 2 * n_v * 28)
    stats.update(output_vertices=n_o, output_triangles=n_k, fell_back=int(fell.sum()))
    _section("end")
    return out_vertices, out_triangles, source.to(_i64), stats


__all__ = [n_ for n_ in dir() if not n_.startswith("__")]
