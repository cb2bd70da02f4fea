"""K28: the two-level lattice of extract_geometry (implicit_surface.py:407-427) -- the SDF is evaluated at every brick-th lattice point and
inside the bricks that can contain the iso-surface; every other point takes a lattice value of the right sign.  Under a Lipschitz bound on the
field the mesh marching cubes extracts equals the dense lattice's bit for bit; a leak count checks the bound after the fact (DESIGN.md,
section 5e).

K29 (ops.brick_mcubes) works on the same lattice under other limits.  Whatever the two share is written once, here, for two FAMILIES of
entry points: the dimensions, the point and classify launches behind both families' public names, and the front end of ops.sparse_lattice
and ops.brick_marching_cubes (_front_end).

Part of gens_amd.ops (see ops/__init__.py); file:line citations are the reference's."""
import collections
import types
import warnings

from .base import *  # noqa: F401,F403
from .geometry import lattice_points
from .lookup import compact_valid


BRICK_MC_MAX = 8           # the largest brick edge of K29: (B + 1)^3 corner values and B^3 threads per workgroup

# A family of entry points: the prefix of its error messages, its brick edges (with the codes the kernels refuse others by), and the names of
# its coarse-point, brick-point and classify entry points and of the classify operator.
_Family = collections.namedtuple("_Family", "who bricks codes coarse points classify classify_op")
_K28 = _Family("sparse_lattice", (1, 1024), "GENS_EINVAL / GENS_ELIMIT", "gens_sparse_coarse_points", "gens_sparse_brick_points", "gens_sparse_classify",
               "sparse_classify")
_K29 = _Family("brick_marching_cubes", (2, BRICK_MC_MAX), "GENS_EINVAL", "gens_brick_coarse_points", "gens_brick_points", "gens_brick_active",
               "brick_active")


def _grid(r, b):
    """-> (C, P): coarse points per axis, C = ceil((R - 1) / B) + 1 (so (C - 1)^3 bricks), and point bricks per axis, P = ceil(R / B)."""
    return (r + b - 2) // b + 1, (r + b - 1) // b


def _dims(fam, resolution, brick):
    """-> (C, P) under the limits of a family: K28's R^3 < 2^31, K29's C^3 < 2^31 and P^3 < 2^31.  ValueError for what the kernels refuse."""
    r, b = int(resolution), int(brick)
    if r < 2:
        raise ValueError(f"{fam.who}: resolution = {r}, at least 2 points per axis (GENS_EINVAL)")
    if not fam.bricks[0] <= b <= fam.bricks[1]:
        raise ValueError(f"{fam.who}: brick = {b}, {fam.bricks[0]} to {fam.bricks[1]} cells ({fam.codes})")
    c, p = _grid(r, b)
    if fam is _K28 and r ** 3 >= 1 << 31:
        raise ValueError(f"{fam.who}: resolution = {r}: resolution^3 must stay below 2^31 (GENS_ELIMIT)")
    if fam is _K29 and max(c, p) ** 3 >= 1 << 31:
        raise ValueError(f"{fam.who}: resolution = {r}, brick = {b}: {c}^3 coarse points and {p}^3 point bricks must stay below 2^31 (GENS_ELIMIT)")
    return c, p


def sparse_lattice_dims(resolution, brick):
    """-> (C, P) of the two-level lattice (include/gens_hip.h, K28).  ValueError for what the kernels refuse."""
    return _dims(_K28, resolution, brick)


def brick_mc_dims(resolution, brick):
    """-> (C, P) as ops.sparse_lattice_dims under K29's limits: 2 <= B <= 8, C^3 < 2^31 and P^3 < 2^31.  ValueError for what the kernels
    refuse."""
    return _dims(_K29, resolution, brick)


def sparse_lattice_margin(bound_min, bound_max, resolution, brick, lipschitz):
    """lipschitz * ||(B + 1) h||_2 with h the three lattice spacings, as the smallest float32 that is not below the float64 value: how far
    from the threshold a corner of a brick must be for the whole brick -- and one cell around it -- to stay on its side."""
    import numpy as np
    h = [(float(hi) - float(lo)) / (int(resolution) - 1) for lo, hi in zip(bound_min, bound_max)]
    m = float(lipschitz) * math.sqrt(sum(((int(brick) + 1) * v) ** 2 for v in h))
    m32 = np.float32(m)
    if float(m32) < m:
        m32 = np.nextafter(m32, np.float32(np.inf))
    return float(m32)


def _box(bound_min, bound_max):
    lo = bound_min.tolist() if torch.is_tensor(bound_min) else [float(v) for v in bound_min]
    hi = bound_max.tolist() if torch.is_tensor(bound_max) else [float(v) for v in bound_max]
    if len(lo) != 3 or len(hi) != 3:
        raise ValueError("sparse_lattice: bound_min / bound_max hold three values each")
    return lo, hi


def _values(evaluate, pts):
    """evaluate(pts) as a flat float32 row of len(pts) values; anything else is the caller's mistake."""
    sdf = evaluate(pts)
    if sdf.numel() != pts.shape[0]:
        raise ValueError(f"sparse_lattice: evaluate returned {tuple(sdf.shape)} for {pts.shape[0]} points, expected (n, 1)")
    return _c(sdf.detach().reshape(-1).to(_f32))


def dense_lattice(evaluate, bound_min, bound_max, resolution, chunk=1 << 21, device=None):
    """u = -evaluate(p) at every point of the resolution^3 lattice (K11's points, `chunk` at a time) -> (R, R, R) float32 on the device."""
    lo, hi = _box(bound_min, bound_max)
    r = int(resolution)
    dev = _lattice_device(bound_min, device)
    total = r ** 3
    u = torch.empty(total, device=dev, dtype=_f32)
    for first in range(0, total, chunk):
        count = min(chunk, total - first)
        u[first:first + count] = -_values(evaluate, lattice_points(lo, hi, r, first, count, dev))
    return u.reshape(r, r, r)


def _lattice_device(bound_min, device):
    if device is not None:
        return torch.device(device)
    if torch.is_tensor(bound_min) and bound_min.is_cuda:
        return bound_min.device
    return torch.device("cuda", torch.cuda.current_device())


def _coarse_points(fam, lo, hi, resolution, brick, first, count, device):
    pts = torch.empty(count, 3, device=device, dtype=_f32)
    L.call(fam.coarse, (C.c_float * 3)(*lo), (C.c_float * 3)(*hi), int(resolution), int(brick), int(first), int(count), L.ptr(pts), L.stream(),
           nbytes=12 * count)
    return pts


def _classify(fam, uc, resolution, brick, threshold, margin):
    c, _ = _dims(fam, resolution, brick)
    uc = _c(uc.reshape(-1))
    if uc.numel() != c ** 3:
        raise ValueError(f"{fam.classify_op}: {uc.numel()} coarse values, expected {c}^3")
    flags = torch.empty((c - 1) ** 3, device=uc.device, dtype=torch.uint8)
    L.call(fam.classify, L.ptr(uc), int(resolution), int(brick), float(threshold), float(margin), L.ptr(flags, torch.uint8), L.stream(),
           nbytes=4 * c ** 3 + (c - 1) ** 3)
    return flags


def _brick_points(fam, lo, hi, resolution, brick, bricks, first, count):
    pts = torch.empty(count * int(brick) ** 3, 3, device=bricks.device, dtype=_f32)
    L.call(fam.points, (C.c_float * 3)(*lo), (C.c_float * 3)(*hi), int(resolution), int(brick), L.ptr(bricks, torch.int64), bricks.shape[0], int(first),
           int(count), L.ptr(pts), L.stream(), nbytes=12 * pts.shape[0] + 8 * count)
    return pts


def sparse_coarse_points(lo, hi, resolution, brick, first, count, device):
    """Coarse lattice points first .. first + count - 1 (C order of the C^3 grid) -> (count, 3)."""
    return _coarse_points(_K28, lo, hi, resolution, brick, first, count, device)


def brick_coarse_points(lo, hi, resolution, brick, first, count, device):
    """ops.sparse_coarse_points under K29's limits."""
    return _coarse_points(_K29, lo, hi, resolution, brick, first, count, device)


def sparse_classify(uc, resolution, brick, threshold, margin):
    """uc (C^3) float32 -> flags ((C - 1)^3) uint8: 1 for a brick with a non-finite corner, a corner within `margin` of the threshold, or
    corners on both sides of it."""
    return _classify(_K28, uc, resolution, brick, threshold, margin)


def brick_active(uc, resolution, brick, threshold, margin):
    """ops.sparse_classify under K29's limits."""
    return _classify(_K29, uc, resolution, brick, threshold, margin)


def sparse_brick_points(lo, hi, resolution, brick, bricks, first, count):
    """The points of the point bricks bricks[first : first + count] (int64, device) -> (count * B^3, 3), indices past R - 1 clamped."""
    return _brick_points(_K28, lo, hi, resolution, brick, bricks, first, count)


def brick_points(lo, hi, resolution, brick, bricks, first, count):
    """ops.sparse_brick_points under K29's limits."""
    return _brick_points(_K29, lo, hi, resolution, brick, bricks, first, count)


def sparse_fill(uc, resolution, brick):
    """-> u (R^3) float32: every lattice point holds uc at the lowest corner of its deciding brick."""
    r = int(resolution)
    c, _ = sparse_lattice_dims(r, brick)
    uc = _c(uc.reshape(-1))
    if uc.numel() != c ** 3:
        raise ValueError(f"sparse_fill: {uc.numel()} coarse values, expected {c}^3")
    u = torch.empty(r ** 3, device=uc.device, dtype=_f32)
    L.call("gens_sparse_fill", L.ptr(uc), r, int(brick), L.ptr(u, align=16), L.stream(), nbytes=4 * r ** 3 + 4 * c ** 3)
    return u


def sparse_scatter(sdf, u, resolution, brick, bricks, first, count):
    """u[owned point] = -sdf[row] for the rows of sparse_brick_points(..., bricks, first, count), in place."""
    sdf = _c(sdf.reshape(-1))
    rows = count * int(brick) ** 3
    if sdf.numel() != rows or u.numel() != int(resolution) ** 3:
        raise ValueError(f"sparse_scatter: {sdf.numel()} values for {rows} rows, lattice of {u.numel()} points for resolution {resolution}")
    L.call("gens_sparse_scatter", L.ptr(sdf), int(resolution), int(brick), L.ptr(bricks, torch.int64), bricks.shape[0], int(first), int(count),
           L.ptr(u), L.stream(), nbytes=8 * rows + 8 * count)


def sparse_leaks(u, flags, resolution, brick, threshold):
    """-> one int64 on the device: the lattice edges that cross the threshold with an endpoint decided by a brick whose flag is clear."""
    r = int(resolution)
    c, _ = sparse_lattice_dims(r, brick)
    if u.numel() != r ** 3 or flags.numel() != (c - 1) ** 3:
        raise ValueError("sparse_leaks: u must hold R^3 values and flags (C - 1)^3 bytes")
    leaks = torch.empty(1, device=u.device, dtype=torch.int64)
    L.call("gens_sparse_leaks", L.ptr(_c(u.reshape(-1))), r, int(brick), L.ptr(_c(flags), torch.uint8), float(threshold), L.ptr(leaks, torch.int64),
           L.stream(), nbytes=4 * r ** 3)
    return leaks


def point_brick_flags(flags, resolution, brick):
    """flags ((C - 1)^3) of the deciding bricks -> the flags of the P^3 point bricks: the same tensor unless (R - 1) % B == 0, when the
    plane R - 1 is a point brick of its own and takes the flag of the brick below it.  (Either family's flags: whoever made them checked
    its limits.)"""
    c, p = _grid(int(resolution), int(brick))
    nb = c - 1
    if p == nb:
        return flags
    at = torch.arange(p, device=flags.device).clamp_(max=nb - 1)
    return _c(flags.view(nb, nb, nb)[at][:, at][:, :, at]).reshape(-1)


def lattice_leak_message(who, leaks, threshold, lipschitz, resolution, brick, then):
    """The warning of a refuted bound, K28's (here) and K29's (ImplicitSurface._brick_mesh); `then`: what the caller does about it."""
    return (f"{who}: {leaks} lattice edges cross the threshold {float(threshold)!r} next to an inactive brick, so the field is not "
            f"{float(lipschitz)!r}-Lipschitz on this lattice (resolution {resolution}, brick {brick}); {then}")


def _front_end(fam, evaluate, bound_min, bound_max, resolution, threshold, brick, lipschitz, chunk, device, open_sink, emit_flags=None):
    """What ops.sparse_lattice (K28) and ops.brick_marching_cubes (K29) do first: the argument checks, the margin, the coarse pass (`chunk`
    points at a time), the ACTIVE flags, with emit_flags (K29: ops.brick_emit_flags) the EMIT flags, every count in ONE host read, the list of
    the active point bricks and their evaluation, chunk // B^3 bricks at a time.  open_sink(f) is called once the counts are known and
    returns sink(first, count, values) for the evaluator's values at the points of bricks[first : first + count] -- or None: nothing is
    evaluated inside the bricks.  -> f: r, b, c, p, lo, hi, dev, uc, flags, emit / pemit / n_emit (with emit_flags), n_eval, bricks, stats."""
    f = types.SimpleNamespace(r=int(resolution), b=int(brick))
    f.c, f.p = _dims(fam, f.r, f.b)
    f.lo, f.hi = _box(bound_min, bound_max)
    if not float(lipschitz) > 0.0 or math.isinf(float(lipschitz)):
        raise ValueError(f"{fam.who}: lipschitz = {lipschitz!r}, a positive finite bound")
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"{fam.who}: chunk = {chunk}")
    f.dev = _lattice_device(bound_min, device)
    margin = sparse_lattice_margin(f.lo, f.hi, f.r, f.b, lipschitz)
    b3, n_coarse = f.b ** 3, f.c ** 3
    f.uc = torch.empty(n_coarse, device=f.dev, dtype=_f32)
    for first in range(0, n_coarse, chunk):
        count = min(chunk, n_coarse - first)
        f.uc[first:first + count] = -_values(evaluate, _coarse_points(fam, f.lo, f.hi, f.r, f.b, first, count, f.dev))
    f.flags = _classify(fam, f.uc, f.r, f.b, threshold, margin)
    pflags = point_brick_flags(f.flags, f.r, f.b)
    sums = [f.flags.sum(), pflags.sum()]
    if emit_flags is not None:
        f.emit = emit_flags(f.flags, f.r, f.b)
        f.pemit = point_brick_flags(f.emit, f.r, f.b)
        sums += [f.emit.sum(), f.pemit.sum()]
    # (counted from the flags: compact_valid's rescue lists 10 bricks when none is set)
    active, f.n_eval, *emitting = (int(v) for v in torch.stack(sums).cpu())
    f.stats = {"coarse_points": n_coarse, "bricks": (f.c - 1) ** 3, "active_bricks": active, "evaluated_points": n_coarse + f.n_eval * b3, "leaks": 0,
               "fell_back": False}
    if emitting:
        f.stats["emitting_bricks"], f.n_emit = emitting
    sink = open_sink(f)
    if sink is not None and f.n_eval:
        f.bricks = compact_valid(pflags)[0][:f.n_eval]
        per = max(1, chunk // b3)
        for first in range(0, f.n_eval, per):
            count = min(per, f.n_eval - first)
            sink(first, count, _values(evaluate, _brick_points(fam, f.lo, f.hi, f.r, f.b, f.bricks, first, count)))
    return f


def sparse_lattice(evaluate, bound_min, bound_max, resolution, threshold, brick, lipschitz, chunk=1 << 21, device=None):
    """u = -evaluate(p) on the resolution^3 lattice between bound_min and bound_max, evaluated only where marching cubes at `threshold` can
    look: at the coarse points (every `brick`-th index and the last), then at the points owned by ACTIVE bricks -- a corner non-finite or
    within lipschitz * ||(brick + 1) h|| of the threshold, or corners on both sides.  Every other point gets its brick's lowest-corner value.
    evaluate: callable on (n, 3) float32 device points -> (n, 1) signed distances (ImplicitSurface.sdf_grid passes its network call).
    -> (u (R, R, R) float32 on the device, stats): coarse_points, bricks, active_bricks, evaluated_points (rows handed to `evaluate`,
    clamped duplicates included), leaks, fell_back.  If |u(p) - u(q)| <= lipschitz * |p - q| holds between lattice points, u < threshold
    agrees with the dense lattice everywhere and the values agree on both endpoints of every crossing edge, so ops.marching_cubes returns
    the dense mesh; `leaks` counts the crossing edges next to an inactive brick, which that bound excludes.  leaks > 0: a RuntimeWarning, the
    dense lattice is evaluated and returned, fell_back is True.  Two host reads: the active count and the leak count."""
    def open_sink(f):
        f.u = sparse_fill(f.uc, f.r, f.b)
        return lambda first, count, sdf: sparse_scatter(sdf, f.u, f.r, f.b, f.bricks, first, count)      # (the scatter negates)

    f = _front_end(_K28, evaluate, bound_min, bound_max, resolution, threshold, brick, lipschitz, chunk, device, open_sink)
    r, stats = f.r, f.stats
    stats["leaks"] = leaks = int(sparse_leaks(f.u, f.flags, r, f.b, threshold))
    u = f.u.reshape(r, r, r)
    if leaks:
        warnings.warn(lattice_leak_message("sparse_lattice", leaks, threshold, lipschitz, r, f.b, "evaluating the dense lattice instead"),
                      RuntimeWarning, stacklevel=2)
        u = dense_lattice(evaluate, f.lo, f.hi, r, int(chunk), f.dev)
        stats["evaluated_points"] += r ** 3
        stats["fell_back"] = True
    return u, stats


__all__ = [n_ for n_ in dir() if not n_.startswith("__")]
