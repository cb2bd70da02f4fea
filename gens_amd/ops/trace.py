"""K31: sphere tracing of the surface sdf + threshold = 0 along rays -- the streaming launches between the evaluator's calls (begin, one
march round, one refine round, the gather of a round's points, the per-ray pack) and the loop around them (sphere_trace).  The definition
is the comment of K31 in include/gens_hip.h; tests/surface_trace_reference.py restates it in numpy.

Part of gens_amd.ops (see ops/__init__.py); file:line citations are the reference's."""
import types

from .base import *  # noqa: F401,F403
from .lattice import _box, _values
from .lookup import compact_valid

TRACE_LIVE, TRACE_HIT, TRACE_MISS, TRACE_INSIDE, TRACE_EXHAUSTED, TRACE_BAD, TRACE_BRACKET = range(7)
TRACE_STATUS_NAMES = {TRACE_HIT: "hit", TRACE_MISS: "miss", TRACE_INSIDE: "inside", TRACE_EXHAUSTED: "exhausted", TRACE_BAD: "bad"}
_STATE_F32 = ("t", "t_lo", "t_hi", "g_lo", "g_hi", "t_end", "dlen")


def _rays(who, rays_o, rays_d):
    for t in (rays_o, rays_d):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError(f"{who}: gens_amd kernels need device tensors (no CPU path)")
    o, d = _c(rays_o.detach().to(_f32)).reshape(-1, 3), _c(rays_d.detach().to(_f32)).reshape(-1, 3)
    if o.shape != d.shape:
        raise ValueError(f"{who}: {o.shape[0]} origins for {d.shape[0]} directions")
    return o, d


def trace_state(rays_o, rays_d, **given):
    """The per-ray state of K31 for rays (n, 3) on the device -> a namespace of device tensors (t, t_lo, t_hi, g_lo, g_hi, t_end, dlen float32;
    status, live uint8; steps int32; points (n, 3)) with .args, the gens_trace_state the entry points take.  given: tensors to use for
    some of them (tests upload a state made in numpy)."""
    o, d = _rays("trace_state", rays_o, rays_d)
    n, dev = o.shape[0], o.device
    s = types.SimpleNamespace(rays_o=o, rays_d=d, n=n)
    for k in _STATE_F32:
        setattr(s, k, torch.empty(n, device=dev, dtype=_f32))
    s.status, s.live = torch.empty(n, device=dev, dtype=torch.uint8), torch.empty(n, device=dev, dtype=torch.uint8)
    s.steps = torch.empty(n, device=dev, dtype=torch.int32)
    s.points = torch.empty(n, 3, device=dev, dtype=_f32)
    for k, v in given.items():
        want = getattr(s, k)
        if not v.is_cuda:
            raise RuntimeError("trace_state: gens_amd kernels need device tensors (no CPU path)")
        if v.shape != want.shape or v.dtype != want.dtype:
            raise ValueError(f"trace_state: {k} is {tuple(v.shape)} {v.dtype}, expected {tuple(want.shape)} {want.dtype}")
        setattr(s, k, _c(v))
    u8 = torch.uint8
    s.args = L.TraceState(L.ptr(o), L.ptr(d), *[L.ptr(getattr(s, k)) for k in _STATE_F32], L.ptr(s.status, u8), L.ptr(s.steps, torch.int32),
                          L.ptr(s.points), L.ptr(s.live, u8), n)
    return s


def trace_begin(state, near, far, bound_min, bound_max):
    """The begin rule: slab test against the box and [near, far] (one value each or one per ray, on the device) -> every field of `state`."""
    lo, hi = _box(bound_min, bound_max)
    nr, fr = _c(near.detach().to(_f32).reshape(-1)), _c(far.detach().to(_f32).reshape(-1))
    if nr.numel() != fr.numel() or nr.numel() not in (1, state.n):
        raise ValueError(f"trace_begin: near / far hold {nr.numel()} and {fr.numel()} values: one, or one per ray ({state.n})")
    L.call("gens_trace_begin", C.byref(state.args), L.ptr(nr), L.ptr(fr), 1 if nr.numel() == state.n and state.n > 1 else 0, (C.c_float * 3)(*lo),
           (C.c_float * 3)(*hi), L.stream(), nbytes=state.n * 70)


def _list(idx, m):
    if idx is None:
        return None
    if idx.dtype != torch.int64 or idx.numel() < m:
        raise ValueError(f"a ray list is int64 with at least {m} entries")
    return L.ptr(_c(idx), torch.int64)


def trace_march(state, sdf, idx, threshold, lipschitz, min_step, max_steps):
    """One march round: sdf (m values, flat or (m, 1)) at the points of the rays idx[:m] (int64 on the device; None: rays 0 .. m - 1)."""
    sdf = _c(sdf.detach().reshape(-1))
    m = sdf.numel()
    L.call("gens_trace_march", C.byref(state.args), L.ptr(sdf), _list(idx, m), m, float(threshold), float(lipschitz), float(min_step), int(max_steps),
           L.stream(), nbytes=m * 60)


def trace_refine(state, sdf, idx, threshold, final, m=None):
    """One refine round on the BRACKET rays of idx[:m]; sdf None: no bisection, the final interpolation only (then m says how many)."""
    if sdf is not None:
        sdf = _c(sdf.detach().reshape(-1))
        m = sdf.numel()
    L.call("gens_trace_refine", C.byref(state.args), L.ptr(sdf), _list(idx, m), int(m), float(threshold), 1 if final else 0, L.stream(), nbytes=int(m) * 60)


def trace_gather(points, idx, m):
    """points (n, 3), idx (>= m) int64 -> (m, 3): the rows idx[:m], the dense batch an evaluator takes."""
    out = torch.empty(m, 3, device=points.device, dtype=_f32)
    L.call("gens_trace_gather", L.ptr(points), _list(idx, m), m, points.shape[0], L.ptr(out), L.stream(), nbytes=m * 32)
    return out


def _trace_chunk(values, o, d, near, far, lo, hi, lipschitz, min_step, max_steps, refine, threshold):
    """sphere_trace for one chunk of rays -> (state, march rounds, rows evaluated)."""
    s = trace_state(o, d)
    trace_begin(s, near, far, lo, hi)
    rounds = evaluated = 0
    while rounds < max_steps:
        m = int(s.live.sum())                          # the round's one host read: it sizes the batch and ends the loop
        if m == 0:
            break
        idx = compact_valid(s.live)[0]
        trace_march(s, values(trace_gather(s.points, idx, m)), idx, threshold, lipschitz, min_step, max_steps)
        rounds += 1
        evaluated += m
    bracket = s.status == TRACE_BRACKET
    m = int(bracket.sum())
    if m:
        idx = compact_valid(bracket)[0]
        for k in range(refine):
            trace_refine(s, values(trace_gather(s.points, idx, m)), idx, threshold, final=k == refine - 1)
            evaluated += m
        if refine == 0:
            trace_refine(s, None, idx, threshold, final=True, m=m)
    return s, rounds, evaluated


def sphere_trace(evaluate, rays_o, rays_d, near, far, bound_min, bound_max, lipschitz, min_step, max_steps=256, refine=2, threshold=0.0, chunk=1 << 21):
    """Sphere tracing of the surface evaluate(p) + threshold = 0 along the rays o + t d inside the box (K31's definition, include/gens_hip.h).
    evaluate: callable on (m, 3) float32 device points -> (m, 1) signed distances, as ops.sparse_lattice takes it; rays_o / rays_d (n, 3),
    near / far (one value or one per ray): device tensors.  lipschitz: the assumed bound on |d sdf| per unit length -- a heuristic, the one of
    the sparse lattice: a field steeper than it can be stepped through, and so can a sheet thinner than min_step (world units).
    -> (t, status, steps, t_lo, t_hi, stats): per-ray device tensors (t: along d, the hit parameter where status is TRACE_HIT; steps: march
    evaluations) and stats: rays per final status ("hit", "miss", "inside", "exhausted", "bad"), "rays", "rounds" (march rounds, summed over
    the chunks) and "evaluated_points" (rows handed to `evaluate`).  Each round evaluates the compacted list of the rays that are still LIVE:
    a finished ray is never evaluated again.  One host read per round (the live count).  Rays are traced `chunk` at a time; with an
    evaluator whose values do not depend on the batch the result does not depend on `chunk`."""
    out, stats = trace_rays(evaluate, rays_o, rays_d, near, far, bound_min, bound_max, lipschitz, min_step, max_steps, refine, threshold, chunk)
    return out["t"], out["status"], out["steps"], out["t_lo"], out["t_hi"], stats


def trace_rays(evaluate, rays_o, rays_d, near, far, bound_min, bound_max, lipschitz, min_step, max_steps=256, refine=2, threshold=0.0, chunk=1 << 21):
    """sphere_trace with everything it holds per ray -> (dict of device tensors: t, t_lo, t_hi, status, steps, points (the hit points where
    status is TRACE_HIT), stats)."""
    o, d = _rays("sphere_trace", rays_o, rays_d)
    for name, v in (("near", near), ("far", far)):
        if not torch.is_tensor(v) or not v.is_cuda:
            raise RuntimeError(f"sphere_trace: {name}: gens_amd kernels need device tensors (no CPU path)")
    lo, hi = _box(bound_min, bound_max)
    lipschitz, min_step, max_steps, refine, chunk = float(lipschitz), float(min_step), int(max_steps), int(refine), int(chunk)
    if not lipschitz > 0.0 or math.isinf(lipschitz):
        raise ValueError(f"sphere_trace: lipschitz = {lipschitz!r}, a positive finite bound")
    if not min_step > 0.0 or math.isinf(min_step):
        raise ValueError(f"sphere_trace: min_step = {min_step!r}, a positive finite length")
    if max_steps < 1 or refine < 0 or chunk < 1:
        raise ValueError(f"sphere_trace: max_steps = {max_steps} (at least 1), refine = {refine} (at least 0), chunk = {chunk} (at least 1)")
    n, dev = o.shape[0], o.device
    near, far = near.detach().to(_f32).reshape(-1), far.detach().to(_f32).reshape(-1)
    if near.numel() != far.numel() or near.numel() not in (1, n):
        raise ValueError(f"sphere_trace: near / far hold {near.numel()} and {far.numel()} values: one, or one per ray ({n})")
    per_ray = near.numel() == n and n > 1
    values = lambda pts: _values(evaluate, pts)  # noqa: E731
    out = {k: torch.empty(n, device=dev, dtype=_f32) for k in ("t", "t_lo", "t_hi")}
    out["status"], out["steps"] = torch.empty(n, device=dev, dtype=torch.uint8), torch.empty(n, device=dev, dtype=torch.int32)
    out["points"] = torch.empty(n, 3, device=dev, dtype=_f32)
    rounds = evaluated = 0
    for first in range(0, n, chunk):
        e = min(first + chunk, n)
        s, r, ev = _trace_chunk(values, o[first:e], d[first:e], near[first:e] if per_ray else near, far[first:e] if per_ray else far, lo, hi, lipschitz,
                                min_step, max_steps, refine, threshold)
        for k in out:
            out[k][first:e] = getattr(s, k)
        rounds += r
        evaluated += ev
    counts = torch.bincount(out["status"].to(torch.int64), minlength=7).tolist() if n else [0] * 7
    stats = {name: counts[code] for code, name in TRACE_STATUS_NAMES.items()}
    stats.update(rays=n, rounds=rounds, evaluated_points=evaluated)
    return out, stats


def surface_pack(status, t, rays_d, rot, grad=None, color=None, vis=None, index=None, out=None):
    """The per-ray pack of K31.  status (n) uint8, t (n), rays_d (n, 3), rot (9 floats: inverse(c2ws[0][:3,:3]) row-major) on the device;
    grad (m, 3) = d sdf / dx, color (m, 3) and vis (m, S) at the hit points of the rays index[:m] (int64; None: m = n, row j is ray j).
    -> dict of device tensors: "depth" (n) = t (rot d)_z, "hit" (n) uint8; with grad "normal" (n, 3) (K30's unit normal) and "normal_img"
    (n, 3) = clip((rot normal) 128 + 128, 0, 255); with color "img" (n, 3) uint8 (K30's colour rule) and "seen" (n) uint8.  Everything is 0 for a
    ray that is not TRACE_HIT.  out: the dict of an earlier call to write into (the chunks of one image)."""
    for v in (status, t, rays_d, rot, grad, color, vis, index):
        if v is not None and (not torch.is_tensor(v) or not v.is_cuda):
            raise RuntimeError("surface_pack: gens_amd kernels need device tensors (no CPU path)")
    if color is not None and vis is None:
        raise ValueError("surface_pack: a colour comes with its in-frustum flags")
    status, t, rays_d = _c(status.reshape(-1)), _c(t.detach().reshape(-1)), _c(rays_d.detach().to(_f32)).reshape(-1, 3)
    rot = _c(rot.detach().to(_f32).reshape(-1))
    n, dev, u8 = status.shape[0], status.device, torch.uint8
    if t.shape[0] != n or rays_d.shape[0] != n or rot.numel() != 9:
        raise ValueError(f"surface_pack: {n} status bytes, {t.shape[0]} t, {rays_d.shape[0]} rays, {rot.numel()} rotation entries (9)")
    first = grad if grad is not None else color
    m = n if first is None else first.shape[0]
    if index is None and m != n:
        raise ValueError(f"surface_pack: {m} rows for {n} rays without an index")
    s = 0
    if grad is not None:
        grad = _c(grad.detach()).reshape(-1, 3)
    if color is not None:
        color = _c(color.detach()).reshape(-1, 3)
        s = vis.shape[-1] if vis.dim() > 1 else 1
        vis = _c(vis.detach()).reshape(-1, s)
        vis = vis.view(u8) if vis.dtype == torch.bool else vis
        if color.shape[0] != m or vis.shape[0] != m or s < 1:
            raise ValueError(f"surface_pack: {m} rows, {color.shape[0]} colours, {vis.shape[0]} rows of {s} flags")
    if out is None:                                # zeros: the rows no list entry names are rays that are not hits
        out = {"depth": torch.zeros(n, device=dev, dtype=_f32), "hit": torch.zeros(n, device=dev, dtype=u8)}
    if grad is not None and "normal" not in out:
        out["normal"], out["normal_img"] = torch.zeros(n, 3, device=dev, dtype=_f32), torch.zeros(n, 3, device=dev, dtype=_f32)
    if color is not None and "img" not in out:
        out["img"], out["seen"] = torch.zeros(n, 3, device=dev, dtype=u8), torch.zeros(n, device=dev, dtype=u8)
    args = L.SurfacePackArgs(L.ptr(grad), L.ptr(color), L.ptr(vis, u8), s, _list(index, m), m, n, L.ptr(status, u8), L.ptr(t), L.ptr(rays_d), L.ptr(rot),
                             L.ptr(out["depth"]), L.ptr(out.get("normal")), L.ptr(out.get("normal_img")), L.ptr(out.get("img"), u8),
                             L.ptr(out.get("seen"), u8), L.ptr(out["hit"], u8))
    L.call("gens_surface_pack", C.byref(args), L.stream(), nbytes=m * (30 + (36 if grad is not None else 0) + (16 + s if color is not None else 0)))
    return out


__all__ = [n_ for n_ in dir() if not n_.startswith("__")]
