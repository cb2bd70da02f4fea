"""GPU checks of the weight ring's chunk boundaries in the three-term bfloat16 SDF kernels (k6b_sdf_bf16x3.hip).  A wave refills the ring and
reads its A operands in the gaps between MFMAs; a boundary wait that is too small would read stale LDS bytes: wrong numbers, no fault.  The
workgroup's stream length does not depend on n, so the short shapes matter for the waves that are dead at the barrier.

One pool of 4 097 points per level count (the net, volumes and points of test_hip_sdf_bf16x3's accuracy test) is evaluated once and held
against the float64 oracle at that test's tolerance; every short shape then evaluates a slice of the pool and must return the pool's own
bits, so each of its points meets the same tolerance."""
import pytest
import torch

from .test_hip_sdf_bf16x3 import _points, _run
from .test_hip_sdfmlp import _net

pytestmark = pytest.mark.gpu

POOL = 4097
SHAPES = [1, 31, 32, 33, 127, 128, 129, 128 * 3 + 5]


@pytest.fixture(scope="module", params=[3, 5])
def pool(request):
    from gens_amd import ops, synthetic
    from oracle import render_oracle as R
    n_levels = request.param
    net, dims = _net(n_levels, seed=40 + n_levels)
    vols = synthetic.make_volumes(dims, seed=12)
    pts = _points(POOL, seed=POOL)
    sd = {"sdf_network." + k: v.detach().cpu().double() for k, v in net.state_dict().items()}
    vols64 = [v.double() * 2 for v in vols]
    ref = R.sdf_mlp(sd, pts.double(), vols64)[:, :1]
    ref_g = R.sdf_gradient(sd, pts.double(), vols64, second=False)[0].detach()
    packed = ops.VolumeSet.packed([(v * 2).cuda() for v in vols])
    plan = ops.SdfMlpPlan(net)
    assert plan.bf16x3_pieces is not None
    keep = ops.kernels.sdf_value, ops.kernels.sdf_grad
    try:
        new = _run(ops, plan, packed, pts.cuda(), "bf16x3")
        old = _run(ops, plan, packed, pts.cuda(), "transposed")
    finally:
        ops.kernels.sdf_value, ops.kernels.sdf_grad = keep
    return dict(n_levels=n_levels, plan=plan, packed=packed, pts=pts.cuda(), ref=ref, ref_g=ref_g, new=new, old=old)


def test_pool_meets_the_float64_oracle_at_the_bf16x3_tolerance(pool):
    """max and mean |sdf - oracle| and |grad - oracle| of the bf16x3 kernels within 1.25 x those of the float32-MFMA kernels on the same points
    (test_hip_sdf_bf16x3's bound), and one SDF from the value and the value + gradient kernel."""
    errs = {}
    for name in ("new", "old"):
        sdf, grad, val = (t.cpu().double() for t in pool[name])
        es, eg = (sdf - pool["ref"]).abs(), (grad - pool["ref_g"]).abs()
        errs[name] = (float(es.max()), float(es.mean()), float(eg.max()), float(eg.mean()))
    print("bf16x3", errs["new"], "transposed", errs["old"])
    assert torch.equal(pool["new"][0], pool["new"][2])
    for a, b in zip(errs["new"], errs["old"]):
        assert a <= 1.25 * b, errs


@pytest.mark.parametrize("n", SHAPES)
def test_short_shapes_return_the_pool_bits_wherever_a_point_lands(pool, n, monkeypatch):
    """n points of the pool (a slice that starts mid-workgroup, so every point changes workgroup, wave and lane): plain, through an index map,
    and with a device-side count below n.  The value kernel and the gradient kernel return the same float32 SDF bit for bit; every result
    equals the pool's for that point; and a second evaluation after permuting the points returns the same bits again."""
    from gens_amd import ops
    monkeypatch.setattr(ops.kernels, "sdf_value", ops.kernels.sdf_value)
    monkeypatch.setattr(ops.kernels, "sdf_grad", ops.kernels.sdf_grad)
    off = 517 + n
    assert off % 32 != 0 and off + n <= POOL
    pts = pool["pts"][off:off + n].contiguous()
    want_s, want_g = pool["new"][0][off:off + n], pool["new"][1][off:off + n]
    g = torch.Generator().manual_seed(n)
    perm = torch.randperm(n, generator=g).cuda()
    idx = torch.randperm(n, generator=g).cuda()
    few = max(1, (3 * n) // 4)
    count = torch.tensor([few], dtype=torch.int32, device="cuda")
    for p, back in ((pts, None), (pts[perm].contiguous(), perm)):
        for index, cnt, live in ((None, None, None), (idx, None, None), (idx, count, idx[:few])):
            sdf, grad, val = _run(ops, pool["plan"], pool["packed"], p, "bf16x3", index, cnt)
            assert torch.equal(sdf, val)
            if back is not None:                       # row r of the permuted run is point perm[r]
                s, gr = torch.empty_like(sdf), torch.empty_like(grad)
                s[back], gr[back] = sdf, grad
                rows = None if live is None else back[live]
            else:
                s, gr, rows = sdf, grad, live
            if rows is None:
                assert torch.equal(s, want_s) and torch.equal(gr, want_g)
            else:
                dead = torch.ones(n, dtype=torch.bool, device="cuda")
                dead[rows] = False
                assert torch.equal(s[rows], want_s[rows]) and torch.equal(gr[rows], want_g[rows])
                assert (s[dead] == 100).all() and (gr[dead] == 0).all()
