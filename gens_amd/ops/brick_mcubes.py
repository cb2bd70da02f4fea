"""K29: marching cubes on the bricks of the two-level lattice (K28, ops.lattice) -- the mesh ops.marching_cubes returns for the lattice
ops.sparse_lattice builds, without that lattice: device memory and work follow the surface, and the resolution limit is C^3 < 2^31 on the
coarse lattice instead of R^3 < 2^31.

Part of gens_amd.ops (see ops/__init__.py)."""
from .base import *  # noqa: F401,F403
from .lattice import _box, _lattice_device, _values, sparse_lattice_margin
from .lookup import compact_valid

BRICK_MC_MAX = 8           # the largest brick edge of K29: (B + 1)^3 corner values and B^3 threads per workgroup


def brick_mc_dims(resolution, brick):
    """-> (C, P) as ops.sparse_lattice_dims under K29's limits: 2 <= B <= 8, C^3 < 2^31 and P^3 < 2^31.  ValueError for what the kernels
    refuse."""
    r, b = int(resolution), int(brick)
    if r < 2:
        raise ValueError(f"brick_marching_cubes: resolution = {r}, at least 2 points per axis (GENS_EINVAL)")
    if not 2 <= b <= BRICK_MC_MAX:
        raise ValueError(f"brick_marching_cubes: brick = {b}, 2 to {BRICK_MC_MAX} cells (GENS_EINVAL)")
    c, p = (r + b - 2) // b + 1, (r + b - 1) // b
    if max(c, p) ** 3 >= 1 << 31:
        raise ValueError(f"brick_marching_cubes: resolution = {r}, brick = {b}: {c}^3 coarse points and {p}^3 point bricks must stay below 2^31 "
                         "(GENS_ELIMIT)")
    return c, p


def brick_coarse_points(lo, hi, resolution, brick, first, count, device):
    """ops.sparse_coarse_points under K29's limits: coarse points first .. first + count - 1 (C order of the C^3 grid) -> (count, 3)."""
    pts = torch.empty(count, 3, device=device, dtype=_f32)
    L.call("gens_brick_coarse_points", (C.c_float * 3)(*lo), (C.c_float * 3)(*hi), int(resolution), int(brick), int(first), int(count), L.ptr(pts),
           L.stream(), nbytes=12 * count)
    return pts


def brick_points(lo, hi, resolution, brick, bricks, first, count):
    """ops.sparse_brick_points under K29's limits: the points of the point bricks bricks[first : first + count] -> (count * B^3, 3)."""
    pts = torch.empty(count * int(brick) ** 3, 3, device=bricks.device, dtype=_f32)
    L.call("gens_brick_points", (C.c_float * 3)(*lo), (C.c_float * 3)(*hi), int(resolution), int(brick), L.ptr(bricks, torch.int64), bricks.shape[0],
           int(first), int(count), L.ptr(pts), L.stream(), nbytes=12 * pts.shape[0] + 8 * count)
    return pts


def brick_active(uc, resolution, brick, threshold, margin):
    """ops.sparse_classify under K29's limits: uc (C^3) float32 -> flags ((C - 1)^3) uint8."""
    c, _ = brick_mc_dims(resolution, brick)
    uc = _c(uc.reshape(-1))
    if uc.numel() != c ** 3:
        raise ValueError(f"brick_active: {uc.numel()} coarse values, expected {c}^3")
    flags = torch.empty((c - 1) ** 3, device=uc.device, dtype=torch.uint8)
    L.call("gens_brick_active", L.ptr(uc), int(resolution), int(brick), float(threshold), float(margin), L.ptr(flags, torch.uint8), L.stream(),
           nbytes=4 * c ** 3 + (c - 1) ** 3)
    return flags


def brick_emit_flags(flags, resolution, brick):
    """flags ((C - 1)^3) uint8 of the active bricks -> the emitting bricks: X emits if a brick of X + {0,1}^3 is active."""
    c, _ = brick_mc_dims(resolution, brick)
    flags = _c(flags.reshape(-1))
    if flags.numel() != (c - 1) ** 3:
        raise ValueError(f"brick_emit_flags: {flags.numel()} flags, expected {c - 1}^3")
    emit = torch.empty_like(flags)
    L.call("gens_brick_emit_flags", L.ptr(flags, torch.uint8), int(resolution), int(brick), L.ptr(emit, torch.uint8), L.stream(), nbytes=9 * flags.numel())
    return emit


def _point_brick_flags(flags, c, p):
    """ops.point_brick_flags on K29's dims: the flags of the (C - 1)^3 deciding bricks -> those of the P^3 point bricks (the plane R - 1 of
    (R - 1) % B == 0 takes the flag of the brick below it)."""
    nb = c - 1
    if p == nb:
        return flags
    at = torch.arange(p, device=flags.device).clamp_(max=nb - 1)
    return _c(flags.view(nb, nb, nb)[at][:, at][:, :, at]).reshape(-1)


def _slot_map(bricks, p, device):
    """Listed point bricks -> (P^3) int32: a brick's place in the list, -1 for the others."""
    slots = torch.full((p ** 3,), -1, device=device, dtype=torch.int32)
    slots[bricks] = torch.arange(bricks.shape[0], device=device, dtype=torch.int32)
    return slots


def brick_marching_cubes(evaluate, bound_min, bound_max, resolution, threshold, brick, lipschitz, chunk=1 << 21, device=None):
    """ops.marching_cubes(u_s, threshold) for the lattice u_s that ops.sparse_lattice(evaluate, ...) builds before any fallback -- the same
    vertices and triangles in the same order -- without u_s: `evaluate` sees the coarse points and the points of the ACTIVE bricks, whose
    values stay brick by brick; marching cubes runs on the point bricks decided by EMITTING bricks (a brick of X + {0,1}^3 active), which
    hold every cell and every crossing edge of u_s, each corner reading its brick's stored value or the fill from the coarse lattice.
    -> (vertices (V, 3) float64 in index coordinates, triangles (T, 3) int32, stats): ops.sparse_lattice's stats and `emitting_bricks`;
    fell_back is always False: the function never falls back, `leaks` (ops.sparse_lattice's count) is the caller's to act on.
    Limits: 2 <= brick <= 8, C^3 and P^3 below 2^31 (resolution up to about 5000 at brick 4), V and T below 2^31.  Three host reads."""
    r, b = int(resolution), int(brick)
    c, p = brick_mc_dims(r, b)
    lo, hi = _box(bound_min, bound_max)
    if not float(lipschitz) > 0.0 or math.isinf(float(lipschitz)):
        raise ValueError(f"brick_marching_cubes: lipschitz = {lipschitz!r}, a positive finite bound")
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"brick_marching_cubes: chunk = {chunk}")
    from .geometry import _mc_tables
    dev = _lattice_device(bound_min, device)
    table, tri_count = _mc_tables(dev)
    margin = sparse_lattice_margin(lo, hi, r, b, lipschitz)
    b3, n_coarse = b ** 3, c ** 3
    uc = torch.empty(n_coarse, device=dev, dtype=_f32)
    for first in range(0, n_coarse, chunk):
        count = min(chunk, n_coarse - first)
        uc[first:first + count] = -_values(evaluate, brick_coarse_points(lo, hi, r, b, first, count, dev))
    flags = brick_active(uc, r, b, threshold, margin)
    emit = brick_emit_flags(flags, r, b)
    pflags, pemit = _point_brick_flags(flags, c, p), _point_brick_flags(emit, c, p)
    # (counted from the flags: compact_valid's rescue lists 10 bricks when none is set)
    active, emitting, n_eval, n_emit = (int(v) for v in torch.stack([flags.sum(), emit.sum(), pflags.sum(), pemit.sum()]).cpu())
    stats = {"coarse_points": n_coarse, "bricks": (c - 1) ** 3, "active_bricks": active, "evaluated_points": n_coarse + n_eval * b3, "leaks": 0,
             "fell_back": False, "emitting_bricks": emitting}
    vertices = torch.empty(0, 3, device=dev, dtype=torch.float64)
    triangles = torch.empty(0, 3, device=dev, dtype=torch.int32)
    if n_emit == 0:
        return vertices, triangles, stats
    store = torch.empty(max(n_eval, 1) * b3, device=dev, dtype=_f32)
    bricks = compact_valid(pflags)[0][:n_eval]
    per = max(1, chunk // b3)
    for first in range(0, n_eval, per):
        count = min(per, n_eval - first)
        store[first * b3:(first + count) * b3] = -_values(evaluate, brick_points(lo, hi, r, b, bricks, first, count))
    pslot = _slot_map(bricks, p, dev)
    listed = _c(compact_valid(pemit)[0][:n_emit])
    eslot = _slot_map(listed, p, dev)
    u8, i32, i64 = torch.uint8, torch.int32, torch.int64
    vmask = torch.empty(n_emit * b3, device=dev, dtype=u8)
    cases = torch.empty(n_emit * b3, device=dev, dtype=u8)
    rank = torch.empty(n_emit * b3, device=dev, dtype=torch.int16)           # (the kernels' uint16: at most 1536)
    counts = torch.empty(3, n_emit, device=dev, dtype=i32)
    field = (L.ptr(uc), L.ptr(store), L.ptr(pslot, i32))
    L.call("gens_brick_mc_classify", *field, L.ptr(flags, u8), r, b, L.ptr(listed, i64), n_emit, float(threshold), L.ptr(tri_count, u8), L.ptr(vmask, u8),
           L.ptr(cases, u8), L.ptr(rank, torch.int16), L.ptr(counts, i32), L.stream(), nbytes=n_emit * (4 * (b + 1) ** 3 + 4 * b3 + 20))
    ends = torch.cumsum(counts, 1, dtype=i64)
    nv, nt, leaks = (int(v) for v in ends[:, -1].cpu())
    stats["leaks"] = leaks
    if nv == 0:
        return vertices, triangles, stats
    if max(nv, nt) >= 1 << 31:
        raise RuntimeError(f"brick_marching_cubes: {nv} vertices and {nt} triangles exceed int32")
    voff, toff = ends[0] - counts[0], ends[1] - counts[1]          # exclusive scans over the brick list
    del ends
    vertices = torch.empty(nv, 3, device=dev, dtype=torch.float64)
    triangles = torch.empty(max(nt, 1), 3, device=dev, dtype=i32)
    vkey, tkey = torch.empty(nv, device=dev, dtype=i64), torch.empty(max(nt, 1), device=dev, dtype=i64)
    L.call("gens_brick_mc_emit", *field, L.ptr(eslot, i32), r, b, L.ptr(listed, i64), n_emit, float(threshold), L.ptr(table, torch.int8), table.shape[1],
           L.ptr(tri_count, u8), L.ptr(vmask, u8), L.ptr(cases, u8), L.ptr(rank, torch.int16), L.ptr(voff, i64), L.ptr(toff, i64),
           L.ptr(vertices, torch.float64), L.ptr(triangles, i32), L.ptr(vkey, i64), L.ptr(tkey, i64), L.stream(),
           nbytes=n_emit * (4 * (b + 1) ** 3 + 4 * b3 + 16) + nv * 32 + nt * 20)
    del vmask, cases, rank, store
    # K12's order: vertices by (lattice point in C order, axis), triangles by (cell in C order, table order) -- the keys, sorted stably
    order = torch.sort(vkey, stable=True)[1]
    del vkey
    vertices = vertices[order]
    new_id = torch.empty(nv, device=dev, dtype=i32)
    new_id[order] = torch.arange(nv, device=dev, dtype=i32)
    del order
    triangles, tkey = triangles[:nt], tkey[:nt]
    if nt and int(triangles.min()) < 0:
        raise RuntimeError("brick_marching_cubes: a triangle refers to a vertex outside the emitting bricks")
    triangles = _c(new_id[triangles.reshape(-1).long()].reshape(-1, 3)[torch.sort(tkey, stable=True)[1]])
    return vertices, triangles, stats


__all__ = [n_ for n_ in dir() if not n_.startswith("__")]
