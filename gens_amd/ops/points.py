"""K24: the three hot steps of the reference's DTU scoring (evaluation/dtu_eval.py) -- mesh sampling, radius down-sampling, nearest
neighbour with a cap -- on float64 device tensors.

Part of gens_amd.ops (see ops/__init__.py); citations are relative to the reference tree (prstrive/GenS)."""
import numpy as np

from .base import *  # noqa: F401,F403

_f64 = torch.float64
POINT_GRID_MAX_CELLS = 1 << 27          # 512 MB of int32 counts; a grid that would be finer gets larger cells


def _need_device(name, *tensors):
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError(f"{name}: gens_amd kernels need device tensors (no CPU path)")


# ------------------------------------------------------------------------------------------------------------------
# mesh sampling (dtu_eval.py:11-20, 61-78)
# ------------------------------------------------------------------------------------------------------------------
def sample_mesh_points(vertices, triangles, density):
    """vertices (V,3), triangles (F,3) device tensors -> (V + S,3) float64: the vertices, then the lattice points of every triangle of
    non-zero area in the script's order (triangle by triangle, i major, j minor), bit for bit the script's float64 values."""
    _need_device("sample_mesh_points", vertices, triangles)
    dev = vertices.device
    v = _c(vertices.detach().to(_f64)).reshape(-1, 3)
    t = _c(triangles.detach().to(device=dev, dtype=torch.int32)).reshape(-1, 3)
    nv, nt = v.shape[0], t.shape[0]
    if nt == 0:
        return v.clone()
    lim = torch.stack([t.min(), t.max()]).cpu()
    if int(lim[0]) < 0 or int(lim[1]) >= nv:
        raise ValueError("sample_mesh_points: triangle index out of range")
    counts = torch.empty(nt, device=dev, dtype=torch.int64)
    L.call("gens_mesh_sample_count", L.ptr(v, _f64), nv, L.ptr(t, torch.int32), nt, float(density), L.ptr(counts, torch.int64), L.stream())
    ends = torch.cumsum(counts, 0)
    total = int(ends[-1])
    if nv + total >= 2 ** 31:
        raise RuntimeError(f"sample_mesh_points: {total} samples (a triangle with more than 2^20 lattice steps along an edge, or more than "
                           "2^31 points in all): the density is too fine for this mesh")
    out = torch.empty(nv + total, 3, device=dev, dtype=_f64)
    out[:nv] = v
    if total:
        offsets = ends - counts
        L.call("gens_mesh_sample_emit", L.ptr(v, _f64), nv, L.ptr(t, torch.int32), nt, float(density), L.ptr(offsets, torch.int64), total,
               C.c_void_p(out.data_ptr() + 24 * nv), L.stream())
    return out


# ------------------------------------------------------------------------------------------------------------------
# point grid
# ------------------------------------------------------------------------------------------------------------------
class PointGrid:
    """A point cloud on the device with K24's uniform grid over it: points (n,3) float64; cell_start (cells + 1) int32, cell_points (n)
    int32 = the point ids cell by cell, sorted (n,3) = their coordinates in that order; box = (lo_x, lo_y, lo_z, cell), dims = (nx, ny, nz)."""

    def __init__(self, points, sorted_points, cell_start, cell_points, box, dims):
        self.points, self.sorted, self.cell_start, self.cell_points = points, sorted_points, cell_start, cell_points
        self.box, self.dims = tuple(float(b) for b in box), tuple(int(d) for d in dims)

    @property
    def n(self):
        return self.points.shape[0]

    def args(self):
        i32 = torch.int32
        return L.PointGridArgs(L.ptr(self.points, _f64), L.ptr(self.sorted, _f64), L.ptr(self.cell_start, i32), L.ptr(self.cell_points, i32),
                               self.n, *self.box, *self.dims)


def _point_grid_box(pmin, pmax, cell, max_cells=POINT_GRID_MAX_CELLS):
    """Box and dims of a grid of cubic cells of edge >= `cell` over [pmin, pmax]: padded by a thousandth of a cell and a millionth of the
    coordinates' magnitude, so that no point is clamped; the edge grows until the grid has at most max_cells cells."""
    pmin, pmax = np.asarray(pmin, dtype=np.float64), np.asarray(pmax, dtype=np.float64)
    while True:
        pad = 1e-3 * cell + 1e-6 * max(float(np.abs(pmin).max()), float(np.abs(pmax).max()))
        lo = pmin - pad
        dims = np.maximum(np.ceil((pmax + pad - lo) / cell), 1.0)
        if float(np.prod(dims)) <= max_cells:
            return (float(lo[0]), float(lo[1]), float(lo[2]), float(cell)), tuple(int(d) for d in dims)
        cell = max(cell * 1.25, float(np.prod(pmax + pad - lo) / max_cells) ** (1.0 / 3.0))


def build_point_grid(points, cell):
    """points (n,3) float64 device tensor, n >= 1 -> PointGrid with cubic cells of edge >= cell (counting sort: count, exclusive scan, fill)."""
    dev = points.device
    p = _c(points.detach().to(_f64)).reshape(-1, 3)
    n = p.shape[0]
    ext = torch.stack([p.amin(0), p.amax(0)]).cpu().numpy()
    if not np.isfinite(ext).all():
        raise ValueError("build_point_grid: non-finite point")
    box, dims = _point_grid_box(ext[0], ext[1], float(cell))
    cells = dims[0] * dims[1] * dims[2]
    i32 = torch.int32
    counts = torch.zeros(cells, device=dev, dtype=i32)
    grid = PointGrid(p, torch.empty(n, 3, device=dev, dtype=_f64), torch.zeros(cells + 1, device=dev, dtype=i32),
                     torch.empty(n, device=dev, dtype=i32), box, dims)
    L.call("gens_point_grid_count", C.byref(grid.args()), L.ptr(counts, i32), L.stream())
    torch.cumsum(counts, 0, dtype=i32, out=grid.cell_start[1:])
    counts.zero_()                              # (now the fill's cursor)
    L.call("gens_point_grid_fill", C.byref(grid.args()), L.ptr(counts, i32), L.stream())
    return grid


# ------------------------------------------------------------------------------------------------------------------
# radius down-sampling (dtu_eval.py:94-102)
# ------------------------------------------------------------------------------------------------------------------
ROUNDS_PER_READBACK = 4
last_downsample_rounds = 0          # the rounds the last radius_downsample call needed (scripts/dtu_eval_bench.py reports it)


def radius_downsample(points, radius, order=None):
    """The mask of the script's sequential loop: visiting the points in `order` (order[k] = the index of the k-th point visited; None: index
    order), a point is kept iff no earlier-visited kept point lies within `radius` of it (d^2 <= radius^2 in float64).  points (n,3) device
    tensor -> (n,) bool.  Decided in rounds on the device (see k24_point_eval.hip); exactly the sequential result, the same on every call."""
    global last_downsample_rounds
    _need_device("radius_downsample", points)
    radius = float(radius)
    if not (radius > 0.0 and np.isfinite(radius)):
        raise ValueError(f"radius_downsample: radius {radius} (must be positive and finite)")
    dev = points.device
    n = points.reshape(-1, 3).shape[0]
    last_downsample_rounds = 0
    if n == 0:
        return torch.zeros(0, device=dev, dtype=torch.bool)
    if n >= 2 ** 31:
        raise RuntimeError(f"radius_downsample: {n} points")
    i32, u8 = torch.int32, torch.uint8
    if order is None:
        rank = torch.arange(n, device=dev, dtype=i32)
    else:
        order = order.detach().to(device=dev, dtype=torch.int64).reshape(-1)
        if order.shape[0] != n:
            raise ValueError("radius_downsample: order must visit every point once")
        rank = torch.full((n,), -1, device=dev, dtype=i32)
        rank[order] = torch.arange(n, device=dev, dtype=i32)
        if bool((rank < 0).any()):
            raise ValueError("radius_downsample: order must visit every point once")
    grid = build_point_grid(points, radius * (1.0 + 2.0 ** -20))
    slot_rank = _c(rank[grid.cell_points.long()])
    state, other = torch.zeros(n, device=dev, dtype=u8), torch.empty(n, device=dev, dtype=u8)
    args = grid.args()
    rounds = 0
    while True:
        left = torch.zeros(ROUNDS_PER_READBACK, device=dev, dtype=i32)
        for k in range(ROUNDS_PER_READBACK):
            L.call("gens_radius_downsample_round", C.byref(args), L.ptr(slot_rank, i32), radius, L.ptr(state, u8), L.ptr(other, u8),
                   C.c_void_p(left.data_ptr() + 4 * k), L.stream())
            state, other = other, state
        left = left.cpu().tolist()
        if 0 in left:
            rounds += left.index(0) + 1
            break
        rounds += ROUNDS_PER_READBACK
        if rounds > n + ROUNDS_PER_READBACK:           # (every round decides the earliest undecided point)
            raise RuntimeError("radius_downsample: the rounds did not end")
    last_downsample_rounds = rounds
    mask = torch.empty(n, device=dev, dtype=torch.bool)
    mask[grid.cell_points.long()] = state == 1
    return mask


# ------------------------------------------------------------------------------------------------------------------
# nearest neighbour with a cap (dtu_eval.py:127-130, 140-142)
# ------------------------------------------------------------------------------------------------------------------
def nearest_distance(queries, targets, max_dist=float("inf")):
    """queries (Q,3), targets (T,3) device tensors -> (dist (Q,) float64, index (Q,) int32): the distance to the nearest target and its
    index (the smallest among equal distances); +inf and -1 where no target is closer than max_dist (the script discards those:
    `dist < max_dist`), also for every query when there are no targets."""
    _need_device("nearest_distance", queries, targets)
    max_dist = float(max_dist)
    if not max_dist > 0.0:
        raise ValueError(f"nearest_distance: max_dist {max_dist} (must be positive)")
    dev = queries.device
    q = _c(queries.detach().to(_f64)).reshape(-1, 3)
    t = targets.detach().to(device=dev).reshape(-1, 3)
    nq, nt = q.shape[0], t.shape[0]
    dist = torch.full((nq,), float("inf"), device=dev, dtype=_f64)
    index = torch.full((nq,), -1, device=dev, dtype=torch.int32)
    if nq == 0 or nt == 0:
        return dist, index
    if nt >= 2 ** 31 or nq >= 2 ** 31:
        raise RuntimeError(f"nearest_distance: {nq} queries, {nt} targets")
    # cells of about two targets if the cloud filled its box, but no finer than an eighth of the cap: a query with nothing within the cap
    # walks at most ten shells before it gives up
    tt = _c(t.to(_f64))
    ext = (tt.amax(0) - tt.amin(0)).cpu().numpy()
    if not np.isfinite(ext).all():
        raise ValueError("nearest_distance: non-finite target")
    span = np.maximum(ext, 1e-3 * max(float(ext.max()), 1e-30))
    cell = (float(np.prod(span)) * 2.0 / nt) ** (1.0 / 3.0)
    if np.isfinite(max_dist):
        cell = max(cell, max_dist / 8.0)
    grid = build_point_grid(tt, cell)
    L.call("gens_nearest_point", C.byref(grid.args()), L.ptr(q, _f64), nq, max_dist, L.ptr(dist, _f64), L.ptr(index, torch.int32), L.stream())
    return dist, index


__all__ = [n_ for n_ in dir() if not n_.startswith("__")]      # private helpers travel too: the package namespace is the old module's
