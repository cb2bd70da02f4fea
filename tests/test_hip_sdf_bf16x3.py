"""GPU checks of the three-term bfloat16 SDF kernels (k6b_sdf_bf16x3.hip: gens_sdf_value_bf16x3 / gens_sdf_grad_bf16x3, the default "f32"
arithmetic at three and five volume levels): as accurate as the float32-MFMA kernels against the float64 oracle, one SDF for the sampling
passes and render_core, and the "transposed" generation still selectable."""
import pytest
import torch

from .test_hip_sdfmlp import _net

pytestmark = pytest.mark.gpu


def _points(n, seed):
    g = torch.Generator().manual_seed(seed)
    pts = torch.rand(n, 3, generator=g) * 2.4 - 1.2                          # inside and outside the cube (zero padding)
    return pts


def _run(ops, plan, packed, pts, gen, idx=None, count=None):
    ops.kernels.sdf_value = ops.kernels.sdf_grad = gen
    n = pts.shape[0]
    sdf, grad, val = torch.full((n, 1), 100.0, device="cuda"), torch.zeros(n, 3, device="cuda"), torch.full((n, 1), 100.0, device="cuda")
    ops.sdf_mlp(plan, packed, pts, index=idx, want_grad=True, sdf_out=sdf, grad_out=grad, count=count)
    ops.sdf_mlp(plan, packed, pts, index=idx, sdf_out=val, count=count)
    return sdf, grad, val


@pytest.mark.parametrize("n_levels,n", [(3, 4097), (5, 1531)])
def test_bf16x3_is_as_accurate_as_the_float32_mfma_kernels(n_levels, n, monkeypatch):
    """max and mean |sdf - oracle| and |grad - oracle| (float64 oracle: oracle/render_oracle.py::sdf_mlp, sdf_gradient) of the bf16x3 kernels
    against those of the float32-MFMA kernels on the same points; ragged count, index map and device-side count.  Both sit at float32
    round-off (~1e-7 mean); the bf16x3 value was measured up to 1.15 x the float32-MFMA figure at three levels (8.0e-7 against 7.6e-7 max,
    1.7e-7 against 1.5e-7 mean) and its gradient below it, so the bound is 1.25 x."""
    from gens_amd import ops, synthetic
    from oracle import render_oracle as R
    monkeypatch.setattr(ops.kernels, "sdf_value", ops.kernels.sdf_value)
    monkeypatch.setattr(ops.kernels, "sdf_grad", ops.kernels.sdf_grad)
    net, dims = _net(n_levels, seed=40 + n_levels)
    vols = synthetic.make_volumes(dims, seed=12)
    pts = _points(n, seed=n)
    sd = {"sdf_network." + k: v.detach().cpu().double() for k, v in net.state_dict().items()}
    vols64 = [v.double() * 2 for v in vols]
    ref = R.sdf_mlp(sd, pts.double(), vols64)[:, :1]
    ref_g, _ = R.sdf_gradient(sd, pts.double(), vols64, second=False)
    ref_g = ref_g.detach()
    packed = ops.VolumeSet.packed([(v * 2).cuda() for v in vols])
    plan = ops.SdfMlpPlan(net)
    assert plan.bf16x3_pieces is not None
    g = torch.Generator().manual_seed(7)
    idx = torch.randperm(n, generator=g).cuda()
    count = torch.tensor([n - 37], dtype=torch.int32, device="cuda")
    live = idx[:n - 37].cpu()
    errs = {}
    for gen in ("bf16x3", "transposed"):
        sdf, grad, val = _run(ops, plan, packed, pts.cuda(), gen, idx, count)
        sdf, grad, val = sdf.cpu().double(), grad.cpu().double(), val.cpu().double()
        dead = torch.ones(n, dtype=torch.bool)
        dead[live] = False
        assert (sdf[dead] == 100).all() and (val[dead] == 100).all() and (grad[dead] == 0).all()
        es, eg = (sdf[live] - ref[live]).abs(), (grad[live] - ref_g[live]).abs()
        errs[gen] = (float(es.max()), float(es.mean()), float(eg.max()), float(eg.mean()))
    print("bf16x3", errs["bf16x3"], "transposed", errs["transposed"])
    for a, b in zip(errs["bf16x3"], errs["transposed"]):
        assert a <= 1.25 * b, errs


@pytest.mark.parametrize("n_levels,n", [(3, 1), (3, 33), (3, 32768 + 129), (5, 4099)])
def test_bf16x3_value_and_gradient_kernels_return_the_same_sdf(n_levels, n, monkeypatch):
    """gens_sdf_value_bf16x3 runs the forward half of gens_sdf_grad_bf16x3: torch.equal values, with an index map and a device-side count."""
    from gens_amd import ops, synthetic
    monkeypatch.setattr(ops.kernels, "sdf_value", ops.kernels.sdf_value)
    monkeypatch.setattr(ops.kernels, "sdf_grad", ops.kernels.sdf_grad)
    net, dims = _net(n_levels, seed=50 + n_levels)
    packed = ops.VolumeSet.packed([(v * 2).cuda() for v in synthetic.make_volumes(dims, seed=13)])
    plan = ops.SdfMlpPlan(net)
    pts = _points(n, seed=n + 1).cuda()
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(n)).cuda()
    count = torch.tensor([max(1, (3 * n) // 4)], dtype=torch.int32, device="cuda")
    L_ = __import__("gens_amd.lib", fromlist=["lib"])
    L_.profile_begin()
    sdf, grad, val = _run(ops, plan, packed, pts, "bf16x3", idx, count)
    launched = set(L_.profile_end())
    assert {"gens_sdf_value_bf16x3", "gens_sdf_grad_bf16x3"} <= launched, launched
    assert torch.equal(sdf, val)
    assert torch.isfinite(grad).all()


def test_bf16x3_propagates_not_a_number_inputs(monkeypatch):
    """A NaN texel or point comes out as NaN in the value and the gradient, on the same rows as through the float32-MFMA kernels."""
    from gens_amd import ops, synthetic
    monkeypatch.setattr(ops.kernels, "sdf_value", ops.kernels.sdf_value)
    monkeypatch.setattr(ops.kernels, "sdf_grad", ops.kernels.sdf_grad)
    net, dims = _net(5, seed=6)
    vols = [v.cuda() for v in synthetic.make_volumes(dims, seed=6)]
    vols[2][0, 1, 2:4, 2:4, 2:4] = float("nan")
    packed = ops.VolumeSet.packed(vols)
    pts = (torch.rand(3000, 3, generator=torch.Generator().manual_seed(2)) * 2 - 1).cuda()
    pts[11, 0] = float("nan")
    plan = ops.SdfMlpPlan(net)
    new = _run(ops, plan, packed, pts, "bf16x3")
    old = _run(ops, plan, packed, pts, "transposed")
    bad = torch.isnan(old[0][:, 0])
    assert bad[11] and int(bad.sum()) > 1
    assert torch.equal(torch.isnan(new[0][:, 0]), bad) and torch.equal(torch.isnan(new[2][:, 0]), bad)
    assert torch.equal(torch.isnan(new[1]).any(1), torch.isnan(old[1]).any(1))
    assert (new[0][~bad] - old[0][~bad]).abs().max() < 2e-6


def test_transposed_generation_stays_selectable(monkeypatch):
    """kernels.sdf_value = kernels.sdf_grad = "transposed" launches today's float32-MFMA kernels (gens_sdf_value / gens_sdf_grad) and gives
    their numbers bit for bit; the environment switch GENS_SDF_F32_MFMA selects them at import."""
    from gens_amd import lib as L, ops, synthetic
    monkeypatch.setattr(ops.kernels, "sdf_value", ops.kernels.sdf_value)
    monkeypatch.setattr(ops.kernels, "sdf_grad", ops.kernels.sdf_grad)
    assert ops.KernelChoice({}).sdf_grad == "bf16x3" and ops.KernelChoice({"GENS_SDF_F32_MFMA": "1"}).sdf_value == "transposed"
    net, dims = _net(3, seed=9)
    packed = ops.VolumeSet.packed([v.cuda() for v in synthetic.make_volumes(dims, seed=9)])
    plan = ops.SdfMlpPlan(net)
    pts = _points(777, seed=3).cuda()
    L.profile_begin()
    sdf, grad, val = _run(ops, plan, packed, pts, "transposed")
    launched = set(L.profile_end())
    assert launched == {"gens_sdf_value", "gens_sdf_grad"}, launched
    s2, g2 = torch.empty_like(sdf), torch.empty_like(grad)
    L.call("gens_sdf_grad", packed.table, packed.dim_table, 3, L.ptr(plan.grad_stream), L.ptr(plan.grad_row), plan.b_last, plan.scale, L.ptr(pts),
           None, 777, None, L.ptr(s2), L.ptr(g2), L.ptr(ops.sdf_grad_stash(pts.device), torch.uint8), L.stream())
    assert torch.equal(sdf, s2) and torch.equal(grad, g2)


def test_bf16x3_kernels_reject_bad_arguments():
    from gens_amd import lib as L, ops, synthetic
    net, dims = _net(3, seed=1)
    packed = ops.VolumeSet.packed([v.cuda() for v in synthetic.make_volumes(dims, seed=4)])
    plan = ops.SdfMlpPlan(net)
    pts = torch.zeros(8, 3, device="cuda")
    out = torch.zeros(8, 1, device="cuda")
    with pytest.raises(RuntimeError, match="null weight stream"):
        L.call("gens_sdf_value_bf16x3", packed.table, packed.dim_table, 3, None, L.ptr(plan.grad_row), 0.0, 1.0, L.ptr(pts), None, 8, None,
               L.ptr(out), L.stream())
    with pytest.raises(RuntimeError, match="3 or 5 volume levels"):
        L.call("gens_sdf_grad_bf16x3", packed.table, packed.dim_table, 2, L.ptr(plan.bf16x3_pieces, torch.bfloat16), L.ptr(plan.grad_row), 0.0,
               1.0, L.ptr(pts), None, 8, None, L.ptr(out), L.ptr(torch.zeros(8, 3, device="cuda")),
               L.ptr(ops.sdf_grad_f16_stash(pts.device), torch.uint8), L.stream())
    assert L.load().gens_sdf_bf16x3_pieces(4) == 0 and L.load().gens_sdf_bf16x3_pieces(3) % 8 == 0
