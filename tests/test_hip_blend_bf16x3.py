"""gens_blend_views_bf16x3 (k7b_blend_bf16x3.hip: the transposed blending kernel with three-term bfloat16 operands on
v_mfma_f32_16x16x32_bf16) against the float64 oracle, against gens_blend_views_t (k7t_blend.hip, float32 MFMA) on the edges of its waves,
on not-a-number inputs, and the selection between the two."""
import functools

import pytest
import torch

from .test_hip_blend import _setup

pytestmark = pytest.mark.gpu

# seeds of the accuracy scenes, picked on the CPU (the oracle side needs no GPU) so that the two-view case leaves out at most 2 %
SEEDS = {5: 100, 3: 103, 4: 100}
# max / mean colour error of "bf16x3" over that of "transposed", measured on an MI355X (profiles/r14_blend_bf16x3.txt)
MEASURED = {(5, 1000): (1.012, 1.000), (3, 333): (1.000, 1.005), (4, 250): (1.000, 1.003)}


def _cpu_net(n_levels, seed):
    """_setup's network with its perturbation drawn on the CPU: the same weights on every machine (the oracle side is then known here)"""
    from gens_amd.models.modules.blending_network import BlendingNetwork
    torch.manual_seed(seed)
    net = BlendingNetwork(d_feature=4 * n_levels)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return net


@functools.lru_cache(maxsize=None)
def _oracle_case(nv, n):
    """CPU only: the scene and points of _setup(nv, 5, SEEDS[nv], n), the float64 oracle's colours of the float32 weights, and the rows
    that are compared -- computed from the oracle's inputs alone:
      * a point no source view sees is left out (soft-max over -1e9 only: the colour is arbitrary);
      * blending_network.py:93-95: weight = (e - min e) * mask / (sum + 1e-8), e = exp(|s| (cos - 1)) ~ 1.  In float32 each e carries a
        rounding error of up to 2^-25, so sum -- with two source views ONE difference of two exponentials -- is uncertain by 2^-24 and
        the weight by A 2^-24, A = d w / d sum = 1e-8 / (sum + 1e-8)^2.  Where that exceeds 2e-5, the bound to which the suite holds
        the colours, the REFERENCE's float32 weights are noise and no float32 kernel can be judged: left out."""
    from oracle import gens_oracle as K
    from oracle import render_oracle as R
    from gens_amd import synthetic
    seed = SEEDS[nv]
    sc = synthetic.make_scene(nv=nv, h=48, w=64, n_levels=5, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    pts = torch.rand(n, 3, generator=g) * 2 - 1
    pts[:3] = torch.tensor([[0, 0, -3.0], [2.5, 0, -2.0], [0.9, 0.9, 0.9]])[:min(3, n)]
    net = _cpu_net(5, seed)
    d = lambda t: t.double()  # noqa: E731
    sd = {"color_network." + k: d(v.detach()) for k, v in net.state_dict().items()}
    fv, rd, mk = K.lookup_feature(d(pts), d(sc["imgs"]), d(sc["intrs"]), d(sc["c2ws"]), [d(f) for f in sc["features"]])
    assert fv.dtype == torch.float64
    ref = R.blend_mlp(sd, torch.nan_to_num(fv), torch.nan_to_num(rd), mk)
    live = mk.any(1)
    e = torch.exp(sd["color_network.s"].abs() * (torch.nan_to_num(rd[..., 3]) - 1))
    wsum = ((e - e.min(dim=1, keepdim=True)[0]) * mk).sum(1)
    amp = 1e-8 / (wsum + 1e-8) ** 2
    firm = (amp * 2.0 ** -24 <= 2e-5) | (wsum == 0)
    left_out = float((live & ~firm).sum()) / max(1, int(live.sum()))
    return sc, pts, net, ref, mk, live & firm, left_out


def test_left_out_share_of_the_accuracy_scenes():
    for nv, n in MEASURED:
        left_out = _oracle_case(nv, n)[-1]
        assert left_out <= 0.02, (nv, n, left_out)


def _views(ops, sc):
    return ops.SceneViews(sc["imgs"].cuda(), sc["intrs"].cuda(), sc["c2ws"].cuda(), [f.cuda() for f in sc["features"]])


@pytest.mark.parametrize("nv,n", list(MEASURED))
def test_bf16x3_is_as_accurate_as_the_float32_kernel_against_the_float64_oracle(nv, n, monkeypatch):
    """Max and mean colour error against the float64 oracle (oracle.gens_oracle.lookup_feature + oracle.render_oracle.blend_mlp on double
    inputs, the float32 weights taken to double), "bf16x3" over "transposed" on the same points.  Measured on an MI355X
    (max ratio, mean ratio; errors of "bf16x3" / "transposed"): S = 4, 1000 points: 1.012, 1.000 (max 5.02e-6 / 4.96e-6, mean 6.05e-7 /
    6.04e-7); S = 2, 333 points, 0.94 % left out: 1.000, 1.005 (3.26e-6 / 3.26e-6, 6.61e-7 / 6.58e-7); S = 3, 250 points: 1.000, 1.003
    (4.88e-6 / 4.88e-6, 5.93e-7 / 5.91e-7).  Bound: the measured ratio plus a quarter (the margin of the SDF test of the same kind), and
    never above 2: a dropped cross term is 2^-16 relative, tens of float32 roundings."""
    from gens_amd import ops
    sc, pts, net, ref, mk, keep, left_out = _oracle_case(nv, n)
    assert left_out <= 0.02, left_out
    views, plan = _views(ops, sc), ops.BlendPlan(net.cuda())
    err = {}
    for kind in ("bf16x3", "transposed"):
        monkeypatch.setattr(ops.kernels, "blend", kind)
        rgb, vis = ops.blend_views(plan, views, pts.cuda())
        assert torch.equal(vis.bool().cpu(), mk)
        e = (rgb.cpu().double() - ref)[keep].abs()
        err[kind] = (float(e.max()), float(e.mean()))
    r_max, r_mean = err["bf16x3"][0] / err["transposed"][0], err["bf16x3"][1] / err["transposed"][1]
    print(f"nv={nv} n={n} kept={int(keep.sum())} left_out={left_out:.4f} bf16x3 max/mean {err['bf16x3'][0]:.3e} {err['bf16x3'][1]:.3e} "
          f"transposed max/mean {err['transposed'][0]:.3e} {err['transposed'][1]:.3e} ratio max {r_max:.3f} mean {r_mean:.3f}")
    m_max, m_mean = MEASURED[(nv, n)]
    assert err["bf16x3"][0] < 2e-5, err
    assert r_max <= min(m_max + 0.25, 2.0) and r_mean <= min(m_mean + 0.25, 2.0), (r_max, r_mean)


@pytest.mark.parametrize("nv,n", [(5, 1), (5, 15), (5, 17), (4, 1), (4, 15), (4, 17), (3, 31), (3, 33)])
def test_bf16x3_on_the_edges_of_a_wave(nv, n, monkeypatch):
    """16 points per wave at S = 3, 4 and 32 at S = 2: one point, one short of a wave, one over.  A random index map and a device-side
    count of 3 n / 4 as implicit_surface.py:196-199 passes them: the flags equal gens_blend_views_t's, the colours agree to the 5e-6 that
    tests/test_hip_blend.py allows between two float32 kernels, untouched rows keep the caller's fill values in both outputs."""
    ops, net, views, pts = _setup(nv, 5, seed=40 + nv, n=n)
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(n)).cuda()
    count = torch.tensor([max(1, (3 * n) // 4)], dtype=torch.int32, device="cuda")
    plan = ops.BlendPlan(net)

    def run(kind):
        monkeypatch.setattr(ops.kernels, "blend", kind)
        rgb = torch.full((n, 3), -7.0, device="cuda")
        vis = torch.full((n, nv - 1), 9, dtype=torch.uint8, device="cuda")
        ops.blend_views(plan, views, pts, index=idx, rgb_out=rgb, vis_out=vis, count=count)
        return rgb, vis

    new, old = run("bf16x3"), run("transposed")
    live, dead = idx[:int(count)], idx[int(count):]
    assert torch.equal(new[1], old[1])
    assert (new[0][live] - old[0][live]).abs().max() < 5e-6
    assert (new[0][dead] == -7).all() and (new[1][dead] == 9).all()


@pytest.mark.parametrize("nv", [5, 3, 4])
def test_bf16x3_propagates_not_a_number_inputs_on_the_rows_the_float32_kernel_does(nv, monkeypatch):
    ops, net, views, pts = _setup(nv, 5, seed=9, n=3000)
    views.feat_tex[1][2, 6:18, 8:24, 1] = float("nan")             # view 2, level 1, channel 1
    pts[5, 1] = float("nan")
    plan = ops.BlendPlan(net)
    monkeypatch.setattr(ops.kernels, "blend", "transposed")
    want, vis_t = ops.blend_views(plan, views, pts)
    monkeypatch.setattr(ops.kernels, "blend", "bf16x3")
    got, vis_b = ops.blend_views(plan, views, pts)
    bad = torch.isnan(want).any(1)
    assert 1 < int(bad.sum()) < 2500 and bool(bad[5])
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(vis_b, vis_t)
    assert torch.isfinite(got[~bad]).all()


def test_selection_between_the_blend_kernels(monkeypatch):
    from gens_amd import lib as L
    from gens_amd.ops.base import KernelChoice
    assert KernelChoice(env={}).blend == "bf16x3"
    assert KernelChoice(env={"GENS_BLEND_F32_MFMA": "1"}).blend == "transposed"
    assert KernelChoice(env={"GENS_BLEND_ROWMAJOR": "1"}).blend == "rowmajor"
    assert KernelChoice(env={"GENS_BLEND_ROWMAJOR": "1", "GENS_BLEND_F32_MFMA": "1"}).blend == "rowmajor"
    ops, net, views, pts = _setup(5, 5, seed=3, n=300)
    plan = ops.BlendPlan(net)
    launched = []
    real_call = L.call
    monkeypatch.setattr(L, "call", lambda name, *a, **k: (launched.append(name) if "blend" in name else None, real_call(name, *a, **k))[1])
    # "transposed": gens_blend_views_t on the float32 stream, bit for bit what a direct call of the entry point returns
    monkeypatch.setattr(ops.kernels, "blend", "transposed")
    rgb_t, vis_t = ops.blend_views(plan, views, pts)
    assert launched == ["gens_blend_views_t"]
    feats = [ops.aligned16(f.detach()) for f in views.feat_tex]
    hw = [d for f in views.feat_tex for d in f.shape[1:3]]
    rgb_d, vis_d = torch.zeros(300, 3, device="cuda"), torch.zeros(300, 4, dtype=torch.uint8, device="cuda")
    real_call("gens_blend_views_t", L.ptr_table(feats, align=16), L.int_table(hw), 5, L.ptr(ops.aligned16(views.imgs_tex.detach()), align=16),
              L.ptr(views.w2c), L.ptr(views.intr), L.ptr(views.c2w), 5, L.ptr(plan.t_stream), L.ptr(plan.t_tab), plan.scalars, L.ptr(pts), None, 300,
              None, L.ptr(rgb_d), L.ptr(vis_d, torch.uint8), L.stream())
    assert torch.equal(rgb_t, rgb_d) and torch.equal(vis_t, vis_d)
    # the default: gens_blend_views_bf16x3, under its own name in the profile table
    monkeypatch.setattr(ops.kernels, "blend", KernelChoice(env={}).blend)
    del launched[:]
    L.profile_begin()
    rgb_b, vis_b = ops.blend_views(plan, views, pts)
    table = L.profile_end()
    assert launched == ["gens_blend_views_bf16x3"] and list(table) == ["gens_blend_views_bf16x3"]
    assert table["gens_blend_views_bf16x3"]["flops"] > 0 and table["gens_blend_views_bf16x3"]["bytes"] > 0
    assert torch.equal(vis_b, vis_t) and (rgb_b - rgb_t).abs().max() < 5e-6
    # six source views keep the row-major kernel under the new default
    del launched[:]
    ops7, net7, views7, pts7 = _setup(7, 3, seed=5, n=20)
    ops.blend_views(ops.BlendPlan(net7), views7, pts7)
    assert launched == ["gens_blend_views"]


def test_bf16x3_rejects_bad_arguments():
    from gens_amd import lib as L
    ops, net, views, pts = _setup(5, 5, seed=3, n=8)
    plan = ops.BlendPlan(net)
    feats = [ops.aligned16(f.detach()) for f in views.feat_tex]
    hw = [d for f in views.feat_tex for d in f.shape[1:3]]
    out = torch.zeros(8, 3, device="cuda")
    assert plan.b_stream.shape[0] == L.load().gens_blend_bf16x3_groups(5) + 2
    assert [L.load().gens_blend_bf16x3_groups(k) for k in (0, 6)] == [0, 0]

    def call(nv=5, n_levels=5, stream=plan.b_stream, feats=feats, hw=hw):
        L.call("gens_blend_views_bf16x3", L.ptr_table(feats, align=16), L.int_table(hw), n_levels, L.ptr(ops.aligned16(views.imgs_tex.detach()), align=16),
               L.ptr(views.w2c), L.ptr(views.intr), L.ptr(views.c2w), nv, L.ptr(stream, torch.int32), L.ptr(plan.t_tab), plan.scalars, L.ptr(pts), None, 8,
               None, L.ptr(out), None, L.stream())

    call()
    with pytest.raises(RuntimeError, match="null table"):
        call(stream=None)
    for nv in (2, 6):
        with pytest.raises(RuntimeError, match="two to four source views"):
            call(nv=nv)
    with pytest.raises(RuntimeError, match="at most 5 feature levels"):          # a level count without an instantiation
        call(n_levels=6, feats=feats + feats[:1], hw=hw + hw[:2])
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        call(stream=plan.b_stream.view(-1)[1:])
