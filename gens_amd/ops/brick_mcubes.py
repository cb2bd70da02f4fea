"""K29: marching cubes on the bricks of the two-level lattice (K28, ops.lattice) -- the mesh ops.marching_cubes returns for the lattice
ops.sparse_lattice builds, without that lattice: device memory and work follow the surface, and the resolution limit is C^3 < 2^31 on the
coarse lattice instead of R^3 < 2^31.

Part of gens_amd.ops (see ops/__init__.py)."""
from .base import *  # noqa: F401,F403
from .lattice import _K29, _front_end, brick_mc_dims
from .lookup import compact_valid


def brick_emit_flags(flags, resolution, brick):
    """flags ((C - 1)^3) uint8 of the active bricks -> the emitting bricks: X emits if a brick of X + {0,1}^3 is active."""
    c, _ = brick_mc_dims(resolution, brick)
    flags = _c(flags.reshape(-1))
    if flags.numel() != (c - 1) ** 3:
        raise ValueError(f"brick_emit_flags: {flags.numel()} flags, expected {c - 1}^3")
    emit = torch.empty_like(flags)
    L.call("gens_brick_emit_flags", L.ptr(flags, torch.uint8), int(resolution), int(brick), L.ptr(emit, torch.uint8), L.stream(), nbytes=9 * flags.numel())
    return emit


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
    def open_sink(f):
        if f.n_emit == 0:
            return None
        from .geometry import _mc_tables
        f.tables = _mc_tables(f.dev)
        f.store = torch.empty(max(f.n_eval, 1) * f.b ** 3, device=f.dev, dtype=_f32)

        def sink(first, count, sdf):
            f.store[first * f.b ** 3:(first + count) * f.b ** 3] = -sdf
        return sink

    f = _front_end(_K29, evaluate, bound_min, bound_max, resolution, threshold, brick, lipschitz, chunk, device, open_sink, brick_emit_flags)
    r, b, p, dev, stats, n_emit, b3 = f.r, f.b, f.p, f.dev, f.stats, f.n_emit, f.b ** 3
    vertices = torch.empty(0, 3, device=dev, dtype=torch.float64)
    triangles = torch.empty(0, 3, device=dev, dtype=torch.int32)
    if n_emit == 0:
        return vertices, triangles, stats
    (table, tri_count), uc, store, flags = f.tables, f.uc, f.store, f.flags
    pslot = _slot_map(f.bricks, p, dev)                      # (an emitting brick has an active one beside it: the list is not empty)
    listed = _c(compact_valid(f.pemit)[0][:n_emit])
    del f                                                    # (it holds the store, which is released before the sort)
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
