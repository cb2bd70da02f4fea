"""GPU tests of the sphere-traced surface maps (K31): every kernel against its numpy restatement (tests/surface_trace_reference.py), bit for
bit; ops.sphere_trace around exactly rounded torch fields against the restated loop; ImplicitSurface.render_surface on a real network against
the restatement driven by the device evaluator; the bracket; the attributes at the hits; the mesh of the same surface; the defaults, the
refusals, validate and the writer.  The f16x2 overflow retry has no test here: the sparse-lattice tests have no way to make a real network
overflow either, and the retry is _lattice_passes' own loop."""
import json
import os

import numpy as np
import pytest
import torch

from . import surface_trace_reference as SR

gpu = pytest.mark.gpu
F = np.float32
LO, HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
K31 = {"gens_trace_begin", "gens_trace_march", "gens_trace_refine", "gens_trace_gather", "gens_surface_pack"}
SIZES = (0, 1, 63, 64, 65, 257, 3072)


def _bits(a):
    """The bit patterns of a float32 array, every NaN as one pattern (which NaN an operation returns is the hardware's choice)."""
    a = np.ascontiguousarray(a)
    if a.dtype != np.float32:
        return a
    return np.where(np.isnan(a), np.uint32(0x7fc00000), a.view(np.uint32))


def _upload(s):
    """A restated state -> ops.trace_state with the same bits."""
    from gens_amd import ops
    given = {k: torch.from_numpy(s[k].copy()).cuda() for k in SR.STATE}
    return ops.trace_state(torch.from_numpy(s["rays_o"]).cuda(), torch.from_numpy(s["rays_d"]).cuda(), **given)


def _assert_state(dev, s, what):
    for k in SR.STATE:
        got = getattr(dev, k).cpu().numpy()
        assert got.dtype == s[k].dtype and np.array_equal(_bits(got), _bits(s[k])), (what, k)


def _rays(n, seed=0):
    """n rays: the planted ones first, then pinhole rays (|d| = 1) and seeded rays of other lengths from seeded origins -> o, d, near, far."""
    po, pd, pn, pf, _, _ = SR.planted_rays()
    o, d = SR.pinhole_rays()
    rng = np.random.default_rng(seed)
    ro = rng.uniform(-2.5, 2.5, (1024, 3)).astype(F)
    rd = ((-ro + rng.uniform(-0.7, 0.7, (1024, 3))) * rng.uniform(0.2, 3.0, (1024, 1))).astype(F)
    rd[::17, rng.integers(0, 3)] = 0
    o, d = np.concatenate([po, ro, o])[:n], np.concatenate([pd, rd, d])[:n]
    near = np.concatenate([pn, rng.uniform(0.0, 1.5, 1024).astype(F), np.full(4000, 1.14, F)])[:n]
    far = np.concatenate([pf, rng.uniform(1.0, 6.0, 1024).astype(F), np.full(4000, 3.36, F)])[:n]
    return np.ascontiguousarray(o), np.ascontiguousarray(d), near, far


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. the kernels
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", SIZES)
def test_begin_equals_the_restatement(n):
    from gens_amd import ops
    o, d, near, far = _rays(n)
    want = SR.begin(o, d, near, far, LO, HI)
    dev = ops.trace_state(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda())
    ops.trace_begin(dev, torch.from_numpy(near).cuda(), torch.from_numpy(far).cuda(), LO, HI)
    _assert_state(dev, want, f"begin n={n}")
    if n >= 64:
        assert len(set(want["status"].tolist())) == 3
    if n:                                      # one near / far for all rays
        want = SR.begin(o, d, near[:1], far[:1], LO, HI)
        ops.trace_begin(dev, torch.from_numpy(near[:1]).cuda(), torch.from_numpy(far[:1]).cuda(), LO, HI)
        _assert_state(dev, want, f"begin n={n}, one near / far")


def _planted_march(n, max_steps, seed):
    """A state after begin with planted steps, t == t_end and finished rays, and planted g values -> (state, sdf (n))."""
    o, d, near, far = _rays(n, seed)
    s = SR.begin(o, d, near, far, LO, HI)
    rng = np.random.default_rng(seed)
    live = np.nonzero(s["status"] == SR.LIVE)[0]
    s["steps"][live] = rng.integers(1, 8, len(live))
    s["steps"][live[::5]] = 0                                   # first evaluations
    s["steps"][live[1::7]] = max_steps - 1                      # evaluation number max_steps
    s["t_lo"][live] = (s["t"][live] - F(0.01)).astype(F)
    s["g_lo"][live] = F(0.02)
    s["t"][live[2::9]] = s["t_end"][live[2::9]]                 # the exit point itself
    s["status"][live[3::11]] = SR.BRACKET                       # finished rays in the list are left alone
    s["live"][:] = s["status"] == SR.LIVE
    sdf = rng.normal(0.0, 0.05, n).astype(F)
    planted = F([np.nan, np.inf, -np.inf, 0.0, -0.0, np.finfo(F).tiny, np.finfo(F).smallest_subnormal, -np.finfo(F).tiny, 1e30])
    for k, v in enumerate(planted):
        sdf[k::23][:3] = v
    return s, sdf


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_march_equals_the_restatement(n):
    from gens_amd import ops
    max_steps, thr, lip, step = 16, 0.0, 2.0, 2.0 / 511
    s, sdf = _planted_march(n, max_steps, seed=n)
    dev = _upload(s)
    ops.trace_march(dev, torch.from_numpy(sdf).cuda(), None, thr, lip, step, max_steps)
    SR.march(s, sdf, None, thr, lip, step, max_steps)
    _assert_state(dev, s, f"march n={n}")
    if n >= 257:
        assert set(s["status"].tolist()) >= {SR.LIVE, SR.MISS, SR.INSIDE, SR.EXHAUSTED, SR.BAD, SR.BRACKET}
    # a second round through a list (the LIVE rays, in a seeded order that is not ascending), with a threshold
    idx = np.nonzero(s["live"])[0]
    idx = np.random.default_rng(n).permutation(idx).astype(np.int64)
    if len(idx):
        sdf2 = np.random.default_rng(n + 1).normal(0.03, 0.05, len(idx)).astype(F)
        ops.trace_march(dev, torch.from_numpy(sdf2).cuda(), torch.from_numpy(idx).cuda(), -0.01, lip, step, max_steps)
        SR.march(s, sdf2, idx, -0.01, lip, step, max_steps)
        _assert_state(dev, s, f"march n={n}, listed")
        got = ops.trace_gather(dev.points, torch.from_numpy(idx).cuda(), len(idx)).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(s["points"][idx]))


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_refine_equals_the_restatement(n):
    from gens_amd import ops
    s, sdf = _planted_march(n, 16, seed=100 + n)
    SR.march(s, sdf, None, 0.0, 2.0, 2.0 / 63, 16)
    dev = _upload(s)
    idx = np.nonzero(s["status"] == SR.BRACKET)[0].astype(np.int64)
    rng = np.random.default_rng(n)
    for final in (False, False, True):
        g = rng.normal(0.0, 0.01, len(idx)).astype(F)
        g[::5] = F([0.0, -0.0, np.nan, np.finfo(F).tiny, np.inf])[np.arange(len(g[::5])) % 5]
        if len(idx):
            ops.trace_refine(dev, torch.from_numpy(g).cuda(), torch.from_numpy(idx).cuda(), 0.0, final)
        SR.refine(s, g, idx, 0.0, final)
        _assert_state(dev, s, f"refine n={n} final={final}")
    assert n < 257 or (s["status"] == SR.HIT).sum() == len(idx) > 0
    # refine = 0: the interpolation alone, on every ray (no list)
    s2, sdf2 = _planted_march(n, 16, seed=200 + n)
    SR.march(s2, sdf2, None, 0.0, 2.0, 2.0 / 63, 16)
    dev2 = _upload(s2)
    if n:
        ops.trace_refine(dev2, None, None, 0.0, True, m=n)
    SR.refine(s2, None, np.arange(n), 0.0, True)
    _assert_state(dev2, s2, f"refine n={n}, final only")


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_surface_pack_equals_the_restatement(n):
    """depth bit-equal, colours and flags exact, normals within 2^-23 of the float64 restatement (K30's bar: one rounding of a correctly
    rounded double quotient), the normal image exactly the float32 expression of the normals the device wrote."""
    from gens_amd import ops
    from . import vertex_attrs_reference as VR
    rng = np.random.default_rng(n)
    eg, ec = VR.edge_rows()
    rg, rc, rv = VR.random_rows(max(n, 1), 3, seed=n)
    grad, color = np.concatenate([eg, rg])[:n], np.concatenate([ec, rc])[:n]
    vis = np.concatenate([VR.flag_rows(3)[np.arange(len(eg)) % 4], rv])[:n]
    status = rng.integers(0, 7, n).astype(np.uint8)
    status[::2] = SR.HIT
    t = rng.uniform(0.0, 4.0, n).astype(F)
    _, d, _, _ = _rays(n, seed=3)
    a = 0.3
    rot = F([[np.cos(a), 0, np.sin(a)], [0.1, 0.99, 0], [-np.sin(a), 0.05, np.cos(a)]])
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    out = {k: v.cpu().numpy() for k, v in ops.surface_pack(up(status), up(t), up(d), up(rot), up(grad), up(color), up(vis)).items()}
    want = SR.pack(status, t, d, rot, grad, color, vis, normal=out["normal"])
    assert np.array_equal(out["hit"].astype(bool), want["hit"])
    assert np.array_equal(_bits(out["depth"]), _bits(want["depth"]))
    err = np.abs(out["normal"].astype(np.float64) - want["normal64"])
    print(f"n={n}: largest normal error {err.max() if n else 0.0:.3e} (bound {2.0 ** -23:.3e})")
    assert n == 0 or err.max() <= 2.0 ** -23
    assert not out["normal"][~want["hit"]].any() and not out["normal"][~want["normal64"].any(axis=1)].any()
    assert np.array_equal(_bits(out["normal_img"]), _bits(want["normal_img"]))
    assert np.array_equal(out["img"], want["img"]) and np.array_equal(out["seen"].astype(bool), want["seen"])
    if n < 64:
        return
    # through a list: rows j of the inputs belong to ray idx[j]; the rays no entry names stay zero; depth alone
    idx = rng.permutation(n)[: n // 3].astype(np.int64)
    part = {k: v.cpu().numpy() for k, v in ops.surface_pack(up(status), up(t), up(d), up(rot), up(grad[idx]), up(color[idx]), up(vis[idx]), index=up(idx)).items()}
    named = np.zeros(n, bool)
    named[idx] = True
    for k in part:
        assert np.array_equal(_bits(part[k][named]), _bits(out[k][named])) and not part[k][~named].any(), k
    alone = ops.surface_pack(up(status), up(t), up(d), up(rot))
    assert sorted(alone) == ["depth", "hit"] and np.array_equal(_bits(alone["depth"].cpu().numpy()), _bits(want["depth"]))
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.surface_pack(up(status), torch.from_numpy(t), up(d), up(rot))


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. the loop
# ------------------------------------------------------------------------------------------------------------------------------------
def _torch_plane(p):
    a, b, c, e = (float(F(v)) for v in SR.PLANE)
    return (((p[:, 0] * a + p[:, 1] * b) + p[:, 2] * c) + e).reshape(-1, 1)


def _torch_poly(p):
    return (((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]) - 0.25).reshape(-1, 1)


@gpu
@pytest.mark.parametrize("name", ["plane", "poly"])
def test_sphere_trace_equals_the_restated_loop(name):
    """Evaluators of separate float32 torch multiplications and additions are exactly rounded on both sides, so t, status, steps and the
    number of evaluated rows are equal -- whatever the chunk."""
    from gens_amd import ops
    field, dev_field, lip = {"plane": (SR.plane_field, _torch_plane, 1.0), "poly": (SR.poly_field, _torch_poly, 3.5)}[name]
    o, d, near, far = _rays(3072 + 20 + 1024)
    step = 2.0 / 511
    s, stats = SR.trace(field, o, d, near, far, LO, HI, lip, step, max_steps=256, refine_rounds=2)
    print(name, stats)
    assert stats["hit"] > 0 and stats["miss"] > 0 and stats["bad"] > 0
    up = lambda x: torch.from_numpy(x).cuda()  # noqa: E731
    for chunk in (64, 1000, 1 << 21):
        t, status, steps, t_lo, t_hi, got = ops.sphere_trace(dev_field, up(o), up(d), up(near), up(far), LO, HI, lip, step, chunk=chunk)
        assert np.array_equal(status.cpu().numpy(), s["status"]), chunk
        assert np.array_equal(steps.cpu().numpy(), s["steps"]), chunk
        for k, v in (("t", t), ("t_lo", t_lo), ("t_hi", t_hi)):
            assert np.array_equal(_bits(v.cpu().numpy()), _bits(s[k])), (chunk, k)
        assert got["evaluated_points"] == stats["evaluated_points"] and all(got[k] == stats[k] for k in ("hit", "miss", "inside", "exhausted", "bad", "rays"))
        assert chunk < len(o) or got["rounds"] == stats["rounds"]
    # refine = 0 and a threshold
    s0, stats0 = SR.trace(field, o, d, near, far, LO, HI, lip, step, max_steps=40, refine_rounds=0, threshold=0.05)
    t, status, steps, _, _, got = ops.sphere_trace(dev_field, up(o), up(d), up(near), up(far), LO, HI, lip, step, max_steps=40, refine=0, threshold=0.05)
    assert np.array_equal(status.cpu().numpy(), s0["status"]) and np.array_equal(_bits(t.cpu().numpy()), _bits(s0["t"]))
    assert got["evaluated_points"] == stats0["evaluated_points"]
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.sphere_trace(dev_field, torch.from_numpy(o), up(d), up(near), up(far), LO, HI, lip, step)
    for bad in ({"lipschitz": 0.0}, {"min_step": 0.0}, {"max_steps": 0}):
        kw = {"lipschitz": lip, "min_step": step, **bad}
        with pytest.raises(ValueError):
            ops.sphere_trace(dev_field, up(o), up(d), up(near), up(far), LO, HI, **kw)


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. the model: the g23 surface and synthetic views of tests/test_hip_vertex_attrs.py
# ------------------------------------------------------------------------------------------------------------------------------------
RES = 128                     # min_step: the spacing of the R = 128 lattice the mesh test extracts
_TRACED = {}


def _model(precision):
    from .test_hip_vertex_attrs import _bounds, _scene, _surface
    from gens_amd import synthetic
    surf, vols = _surface(precision)
    sc, views = _scene(surf, 3)
    rays_o, rays_d = synthetic.make_rays(sc["intrs"].cpu(), sc["c2ws"].cpu(), 48, 64)
    lo, hi = _bounds()
    return surf, vols, sc, views, rays_o.cuda(), rays_d.cuda(), lo, hi


def _traced(precision):
    """render_surface of the 48 x 64 image, once per precision -> (its outputs, its stats)."""
    if precision not in _TRACED:
        surf, vols, sc, views, o, d, lo, hi = _model(precision)
        out = surf.render_surface(o, d, sc["near"], sc["far"], vols, lo, hi, sc["c2ws"], views=views, resolution=RES, hw=(48, 64))
        _TRACED[precision] = (out, dict(surf.last_surface_stats))
    return _TRACED[precision]


@gpu
@pytest.mark.parametrize("precision", ["f32", "f16x2"])
def test_render_surface_equals_the_restatement_driven_by_the_device_evaluator(precision):
    """(a) The network's values do not depend on the batch (asserted first, on the points of the trace), so the restated loop around
    ops.sdf_mlp must give the device's t, status and steps bit for bit."""
    from gens_amd import ops
    surf, vols, sc, views, o, d, lo, hi = _model(precision)
    out, stats = _traced(precision)
    print(f"{precision}: {stats}, {stats['evaluated_points'] / stats['rays']:.2f} evaluations per ray")
    assert stats["hit"] > 0 and stats["rays"] - stats["hit"] > 0 and stats["rays"] == 3072
    assert out["t"].shape == (48, 64) and out["normal_img"].shape == (48, 64, 3) and out["img"].dtype == np.uint8 and out["hit"].dtype == bool
    assert int(out["hit"].sum()) == stats["hit"] and np.array_equal(out["hit"], out["status"] == SR.HIT)
    packed = ops.VolumeSet.packed(vols)
    with torch.no_grad():
        plan = surf._fused_plan(packed)
    prec = surf._precision(plan)
    calls = []

    def evaluate(p):
        calls.append(len(p))
        if len(p) == 0:
            return np.zeros(0, F)
        with torch.no_grad():
            return ops.sdf_mlp(plan, packed, torch.from_numpy(np.ascontiguousarray(p)).cuda(), precision=prec)[:, 0].cpu().numpy()

    # batch independence on the hit points: one batch against a seeded permutation in batches of 101
    t = out["t"].reshape(-1)
    pts = SR.points_at(o.cpu().numpy(), d.cpu().numpy(), t)[out["hit"].reshape(-1)]
    whole = evaluate(pts)
    perm = np.random.default_rng(1).permutation(len(pts))
    again = np.empty_like(whole)
    for s in range(0, len(pts), 101):
        again[perm[s:s + 101]] = evaluate(pts[perm[s:s + 101]])
    assert np.array_equal(_bits(whole), _bits(again))
    h = 2.0 / (RES - 1)
    s, want = SR.trace(evaluate, o.cpu().numpy(), d.cpu().numpy(), sc["near"].cpu().numpy(), sc["far"].cpu().numpy(), LO, HI, surf.lattice_lipschitz,
                       h, max_steps=256, refine_rounds=2)
    assert not surf._split_half_overflowed()
    assert np.array_equal(out["status"].reshape(-1), s["status"])
    assert np.array_equal(out["steps"].reshape(-1), s["steps"])
    assert np.array_equal(_bits(out["t"].reshape(-1)), _bits(s["t"]))
    assert all(stats[k] == want[k] for k in want), (stats, want)


@gpu
@pytest.mark.parametrize("precision", ["f32", "f16x2"])
def test_every_hit_is_a_sign_bracket_of_the_network(precision):
    """(b) g(p(t_lo)) > 0 >= g(p(t_hi)) re-evaluated, and (t_hi - t_lo) |d| <= min_step 2^-refine plus 4 ulp of t_hi."""
    from gens_amd import ops
    surf, vols, sc, views, o, d, lo, hi = _model(precision)
    packed = ops.VolumeSet.packed(vols)
    h = 2.0 / (RES - 1)
    with torch.no_grad():
        plan = surf._fused_plan(packed)
        evaluate = lambda p: ops.sdf_mlp(plan, packed, p, precision=surf._precision(plan))  # noqa: E731
        t, status, steps, t_lo, t_hi, stats = ops.sphere_trace(evaluate, o, d, sc["near"], sc["far"], lo, hi, surf.lattice_lipschitz, h)
        hit = status == ops.TRACE_HIT
        g_lo = evaluate((o + t_lo[:, None] * d)[hit])[:, 0]
        g_hi = evaluate((o + t_hi[:, None] * d)[hit])[:, 0]
    assert np.array_equal(status.cpu().numpy(), _traced(precision)[0]["status"].reshape(-1))
    assert int(hit.sum()) > 0 and bool((g_lo > 0).all()) and bool((g_hi <= 0).all())
    width = ((t_hi.double() - t_lo.double()) * torch.linalg.norm(d.double(), dim=1))[hit].cpu().numpy()
    ulp = np.spacing(t_hi[hit].cpu().numpy()).astype(np.float64)
    print(f"{precision}: widest final bracket {width.max():.3e} (min_step / 4 = {h / 4:.3e})")
    assert (width > 0).all() and (width <= h / 4 + 4 * ulp).all()
    assert bool(((t >= t_lo) & (t <= t_hi))[hit].all())


@gpu
def test_attributes_at_the_hits_are_vertex_attributes_of_the_hit_points():
    """(c) normal, img and seen at HIT rays equal vertex_attributes of the hit points; everything is zero elsewhere."""
    surf, vols, sc, views, o, d, lo, hi = _model("f32")
    out, _ = _traced("f32")
    hit = out["hit"].reshape(-1)
    pts = SR.points_at(o.cpu().numpy(), d.cpu().numpy(), out["t"].reshape(-1))[hit]
    attrs = surf.vertex_attributes(pts, vols, views)
    assert np.array_equal(out["normal"].reshape(-1, 3)[hit], attrs["normals"])
    assert np.array_equal(out["img"].reshape(-1, 3)[hit], attrs["colors"])
    assert np.array_equal(out["seen"].reshape(-1)[hit], attrs["seen"])
    for k in ("depth", "normal", "normal_img", "img", "seen"):
        assert not out[k].reshape(len(hit), -1)[~hit].any(), k
    rot = np.linalg.inv(sc["c2ws"][0, :3, :3].cpu().numpy().astype(np.float64))
    depth = out["t"].reshape(-1)[hit] * (d.cpu().numpy().astype(np.float64)[hit] @ rot[2])
    assert np.abs(out["depth"].reshape(-1)[hit] - depth).max() < 1e-5 and (out["depth"].reshape(-1)[hit] > 0).all()
    # one output at a time, flat rays, no views for what needs none
    only = surf.render_surface(o, d, sc["near"], sc["far"], vols, lo, hi, sc["c2ws"], outputs="normals", resolution=RES)
    assert sorted(only) == ["hit", "normal", "normal_img", "status", "steps", "t"] and only["t"].shape == (3072,)
    assert np.array_equal(only["normal_img"], out["normal_img"].reshape(-1, 3))
    depth_only = surf.render_surface(o, d, sc["near"], sc["far"], vols, lo, hi, sc["c2ws"], outputs=("depth",), resolution=RES, chunk=1000)
    assert np.array_equal(depth_only["depth"], out["depth"].reshape(-1))


@gpu
def test_against_the_mesh_of_the_same_surface():
    """A measurement with one condition: the R = 128 mesh is cast with the same rays (ops.ray_mesh_first_hit).  For the rays hit on both
    routes |t_trace - t_mesh| |d . n| / h is printed (median, 99th percentile, max) with the share of rays whose hit flags differ, and
    recorded in profiles/ when GENS_RECORD_PROFILES is set; asserted: the rays hit on both routes are a majority of those hit on either."""
    from gens_amd import ops
    surf, vols, sc, views, o, d, lo, hi = _model("f32")
    out, stats = _traced("f32")
    vertices, triangles = surf.extract_geometry(vols, lo, hi, RES, 0.0)
    grid = ops.build_mesh_grid(torch.from_numpy(vertices).cuda(), torch.from_numpy(triangles).cuda())
    face, t_mesh = ops.ray_mesh_first_hit(o, d, grid)
    face, t_mesh = face.cpu().numpy(), t_mesh.cpu().numpy()
    hit_t, hit_m = out["hit"].reshape(-1), face >= 0
    both, either = hit_t & hit_m, hit_t | hit_m
    h = 2.0 / (RES - 1)
    n = out["normal"].reshape(-1, 3).astype(np.float64)
    cos = np.abs((d.cpu().numpy().astype(np.float64) * n).sum(axis=1))
    gap = np.abs(out["t"].reshape(-1).astype(np.float64) - t_mesh)[both] * cos[both] / h
    record = {"resolution": RES, "rays": int(len(hit_t)), "hit_trace": int(hit_t.sum()), "hit_mesh": int(hit_m.sum()), "hit_both": int(both.sum()),
              "flags_differ_share": float((hit_t != hit_m).mean()), "gap_over_h_median": float(np.median(gap)),
              "gap_over_h_p99": float(np.percentile(gap, 99)), "gap_over_h_max": float(gap.max()), "trace_stats": stats}
    print(json.dumps(record))
    if os.environ.get("GENS_RECORD_PROFILES"):
        with open(os.path.join(os.environ["GENS_RECORD_PROFILES"], "k31_trace_against_mesh.json"), "w") as f:
            json.dump(record, f, indent=1)
    assert 2 * both.sum() > either.sum()


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. defaults, refusals, validate and the writer
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_nothing_changes_when_the_option_is_unset_and_validate_adds_four_keys_when_set(tmp_path):
    from gens_amd import io as gio, lib as L
    from gens_amd.config import Conf, gens_model_conf
    from gens_amd.models.gens import GenS
    from gens_amd.models.modules.implicit_surface import ImplicitSurface
    from .test_hip_vertex_attrs import TODAYS_KEYS, _surface, _validate_args
    assert ImplicitSurface.surface_render is None
    surf, vols = _surface("f32")
    assert "surface_render" not in vars(surf)
    args = _validate_args(surf, vols)
    L.profile_begin(only=K31)
    torch.manual_seed(3)
    ref = surf.validate(*args, extract_geometry=True, mesh_resolution=33)
    torch.manual_seed(3)
    off = surf.validate(*args, extract_geometry=True, mesh_resolution=33, surface_render=False)
    assert not L.profile_end(raw=True)
    assert set(ref) == set(off) == TODAYS_KEYS
    L.profile_begin(only=K31)
    torch.manual_seed(3)
    out = surf.validate(*args, extract_geometry=True, mesh_resolution=33, surface_render=True)
    assert {k for k, *_ in L.profile_end(raw=True)} == K31
    new = {"surface_depth", "surface_normal_img", "surface_img", "surface_hit"}
    assert set(out) == TODAYS_KEYS | new
    for k in TODAYS_KEYS:
        assert torch.equal(torch.as_tensor(out[k]), torch.as_tensor(ref[k])) and torch.equal(torch.as_tensor(off[k]), torch.as_tensor(ref[k])), k
    assert out["surface_depth"].shape == (24, 32) and out["surface_normal_img"].shape == (24, 32, 3) and out["surface_img"].shape == (24, 32, 3)
    assert out["surface_hit"].shape == (24, 32) and out["surface_hit"].dtype == bool and 0 < out["surface_hit"].sum() < 24 * 32
    assert surf.last_surface_stats["hit"] == int(out["surface_hit"].sum())
    # the attribute does what the keyword does; a dict passes render_surface's keywords
    surf.surface_render = {"max_steps": 64, "refine": 1}
    try:
        torch.manual_seed(3)
        tuned = surf.validate(*args, extract_geometry=False)
        assert new <= set(tuned) and surf.last_surface_stats["rounds"] <= 64
    finally:
        del surf.surface_render
    # the writer: three more folders, only when the keys are there; pixels that are not hits are black
    inputs = {"scene": "scan1", "file_name": "scan1_view0", "scale_mat": torch.eye(4)}
    plain = gio.save_validation_outputs(str(tmp_path / "plain"), ref, inputs, "epoch0")
    assert not any(k.startswith("surface") for k in plain) and not (tmp_path / "plain" / "val_surface_depth").exists()
    paths = gio.save_validation_outputs(str(tmp_path / "set"), out, inputs, "epoch0")
    from PIL import Image
    for key, sub in (("surface_depth", "val_surface_depth"), ("surface_normal", "val_surface_normal"), ("surface_img", "val_surface_img")):
        assert os.path.dirname(paths[key]) == str(tmp_path / "set" / sub)
        img = np.asarray(Image.open(paths[key]))
        assert img.shape == (24, 32, 3) and not img[~out["surface_hit"]].any() and img[out["surface_hit"]].any()
    assert np.array_equal(np.asarray(Image.open(paths["surface_img"])), out["surface_img"])
    # the conf key reaches the attribute (and its absence leaves the class default)
    conf = gens_model_conf(volume_dims=(16, 8, 4), has_vol=True)
    assert "surface_render" not in vars(GenS(conf).implicit_surface)
    assert GenS(Conf({**conf, "surface_render": True})).implicit_surface.surface_render is True
    assert GenS(Conf({**conf, "surface_render": {"refine": 3}})).implicit_surface.surface_render == {"refine": 3}


@gpu
def test_refusals_come_before_any_launch():
    from gens_amd import lib as L, ops
    from .test_hip_vertex_attrs import NETWORK
    surf, vols, sc, views, o, d, lo, hi = _model("f32")
    six = ops.VolumeSet.packed([torch.zeros(1, 4, 4, 4, 4, device="cuda") for _ in range(6)])
    base = (o, d, sc["near"], sc["far"])
    L.profile_begin(only=K31 | NETWORK | {"gens_compact_valid"})
    with pytest.raises(ValueError, match="1 to 5 packed volume levels, not 6"):
        surf.render_surface(*base, six, lo, hi, sc["c2ws"], views=views)
    with pytest.raises(ValueError, match="needs the scene's views"):
        surf.render_surface(*base, vols, lo, hi, sc["c2ws"])
    with pytest.raises(ValueError, match="min_step"):
        surf.render_surface(*base, vols, lo, hi, sc["c2ws"], views=views, min_step=0.0)
    with pytest.raises(ValueError, match="min_step"):
        surf.render_surface(*base, vols, lo, hi, sc["c2ws"], views=views, min_step=-1.0)
    with pytest.raises(ValueError, match="lipschitz"):
        surf.render_surface(*base, vols, lo, hi, sc["c2ws"], views=views, lipschitz=0.0)
    with pytest.raises(ValueError, match="max_steps"):
        surf.render_surface(*base, vols, lo, hi, sc["c2ws"], views=views, max_steps=0)
    with pytest.raises(ValueError, match="the known ones are"):
        surf.render_surface(*base, vols, lo, hi, sc["c2ws"], views=views, outputs=("depth", "albedo"))
    assert not L.profile_end(raw=True)
