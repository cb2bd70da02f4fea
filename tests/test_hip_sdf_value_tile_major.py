"""GPU checks of the two-wave value kernel's stream (k6b_sdf_bf16x3.hip: sdf_bf16x3_k<3, false> on SdfMlpPlan.bf16x3_value_pieces) and of
layer 3's seven hidden blocks in the two three-level bf16x3 kernels.  The shipped library walks its layers block by block on the gradient
stream's forward prefix; under GENS_HIP_LIB=.../libgens_hip_k6b_tile_major.so (make k6b_tile_major) the same file checks the tile-major
build, which finishes a layer tile by tile on a value-only stream of its own: the plan packs what gens_sdf_bf16x3_layout says.
NOTE: the suite loads the shipped library only, so the kernel's tile-major branch (TM, GB_OP_CPH, GB_PREP_TM) and the plan's second stream
run on a GPU only when somebody sets GENS_HIP_LIB by hand; what the suite itself guards of that build is the stream's order, on the CPU
(tests/test_sdf_pack_tile_major_cpu.py).  Its last such run, and its registers (246, no scratch, two waves): profiles/r29_sdf_value_tile_major.txt.

Volumes of 16 / 8 / 4 cells a side.  One pool of points -- inside the cube, outside it, on its faces -- is evaluated ONCE by both kernels and
held to the float64 oracle with the bound of tests/test_hip_sdf_bf16x3.py (errors at most 1.25 x those of the float32-MFMA kernels on the same
points; its helpers `_run` and `_points` are imported).  A point's result does not depend on where it sits in a launch, so every case
below -- n = one lane, one wave, one workgroup and each plus one, plain, through an index map, and with a device-side count below n -- must
return the pool's bits for the rows it names and leave every other row alone; that carries the bound to every case."""
import ctypes as C
import inspect

import pytest
import torch

from . import test_hip_sdf_bf16x3 as B
from .test_hip_sdfmlp import _net

FILL = 100.0                      # what B._run pre-fills its outputs with
BOUND = 1.25                      # B's bound, which is a literal there: tied to its source below
POOL = {3: 4097, 5: 1531}         # B's point counts, at which that bound was set
DIMS = {3: (16, 8, 4), 5: None}   # None: _net's own
SIZES = [1, 32, 33, 128, 129, 257]


def test_the_bound_is_the_one_of_test_hip_sdf_bf16x3():
    assert f"a <= {BOUND} * b" in inspect.getsource(B.test_bf16x3_is_as_accurate_as_the_float32_mfma_kernels)
    assert f"{FILL}" in inspect.getsource(B._run)


def _pool_points(n):
    pts = B._points(n, seed=29)                                      # uniform in [-1.2, 1.2]^3
    first = torch.tensor([[0.3, -0.2, 0.1], [1.1, 0.2, -0.4], [1.0, 0.3, -0.2], [1.0, 1.0, 1.0], [-1.0, -1.0, 0.5], [0.25, -1.0, 0.0],
                          [-0.6, 0.7, 1.15], [1.0 / 15, -3.0 / 7, 1.0 / 3]])      # inside, outside, faces, a corner, an edge, cell planes
    pts[:len(first)] = first
    return pts


@pytest.fixture(scope="module")
def pools():
    """Per level count: (plan, volumes, pool points on the device, the pool's sdf, gradient and value-kernel sdf), computed once and left
    unchanged; the accuracy bound is asserted here."""
    from gens_amd import lib as L, ops, synthetic
    from oracle import render_oracle as R
    made = {}

    def get(n_levels):
        if n_levels in made:
            return made[n_levels]
        saved = ops.kernels.sdf_value, ops.kernels.sdf_grad
        try:
            net, dims = _net(n_levels, seed=70 + n_levels)
            dims = DIMS[n_levels] or dims
            vols = synthetic.make_volumes(dims, seed=15)
            pts = _pool_points(POOL[n_levels])
            inside = (pts.abs() < 1).all(1)
            face = ((pts.abs() == 1).any(1)) & (pts.abs() <= 1).all(1)
            assert inside[:32].any() and (~inside & ~face)[:32].any() and face[:32].any() and inside[0] and face[2]
            sd = {"sdf_network." + k: v.detach().cpu().double() for k, v in net.state_dict().items()}
            vols64 = [v.double() * 2 for v in vols]
            ref = R.sdf_mlp(sd, pts.double(), vols64)[:, :1]
            ref_g = R.sdf_gradient(sd, pts.double(), vols64, second=False)[0].detach()
            packed = ops.VolumeSet.packed([(v * 2).cuda() for v in vols])
            plan = ops.SdfMlpPlan(net)
            assert plan.bf16x3_pieces is not None and plan.bf16x3_value_pieces is not None
            layout = (C.c_int * 3)()
            assert L.load().gens_sdf_bf16x3_layout(n_levels, layout) == 0
            assert (plan.bf16x3_value_pieces is plan.bf16x3_pieces) == (layout[1] == 0) and plan.bf16x3_value_pieces.shape[0] >= layout[0]
            print("levels", n_levels, "layout", list(layout))
            errs, outs = {}, {}
            for gen in ("bf16x3", "transposed"):
                sdf, grad, val = outs[gen] = B._run(ops, plan, packed, pts.cuda(), gen)
                es, eg, ev = (sdf.cpu().double() - ref).abs(), (grad.cpu().double() - ref_g).abs(), (val.cpu().double() - ref).abs()
                errs[gen] = (float(es.max()), float(es.mean()), float(eg.max()), float(eg.mean()), float(ev.max()), float(ev.mean()))
            print("levels", n_levels, "bf16x3", errs["bf16x3"], "transposed", errs["transposed"])
            sdf, grad, val = outs["bf16x3"]
            assert torch.equal(sdf, val) and torch.isfinite(sdf).all() and torch.isfinite(grad).all() and (sdf != FILL).all()
            for a, b in zip(errs["bf16x3"], errs["transposed"]):
                assert a <= BOUND * b, errs
            made[n_levels] = (plan, packed, pts.cuda(), sdf, grad)
        finally:
            ops.kernels.sdf_value, ops.kernels.sdf_grad = saved
        return made[n_levels]
    return get


@pytest.fixture(autouse=True)
def _restore_generations(monkeypatch):
    from gens_amd import ops
    monkeypatch.setattr(ops.kernels, "sdf_value", ops.kernels.sdf_value)
    monkeypatch.setattr(ops.kernels, "sdf_grad", ops.kernels.sdf_grad)


def _check(pools, n_levels, n, mode):
    """mode "plain": the first n points of the pool; "index": n rows of the pool's first 300 in random order; "count": the same with a
    device-side count of n - 1."""
    from gens_amd import lib as L, ops
    plan, packed, pool, want, want_g = pools(n_levels)
    if mode == "plain":
        pts, idx, count, named = pool[:n], None, None, torch.arange(n, device="cuda")
    else:
        pts = pool[:300]
        idx = torch.randperm(300, generator=torch.Generator().manual_seed(n))[:n].cuda()
        count = torch.tensor([n - 1], dtype=torch.int32, device="cuda") if mode == "count" else None
        named = idx[:n - 1] if mode == "count" else idx
    L.profile_begin()
    sdf, grad, val = B._run(ops, plan, packed, pts, "bf16x3", idx, count)
    launched = set(L.profile_end())
    assert {"gens_sdf_value_bf16x3", "gens_sdf_grad_bf16x3"} <= launched, launched
    assert torch.equal(val, sdf)                                                       # the value kernel = the gradient kernel, bit for bit
    dead = torch.ones(pts.shape[0], dtype=torch.bool, device="cuda")
    dead[named] = False
    assert int(dead.sum()) == pts.shape[0] - named.shape[0]
    assert (val[dead] == FILL).all() and (sdf[dead] == FILL).all() and (grad[dead] == 0).all()
    assert torch.equal(val[named], want[named]) and torch.equal(grad[named], want_g[named])      # ... = the pool's, which met the bound


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["plain", "index", "count"])
@pytest.mark.parametrize("n", SIZES)
def test_value_kernel_returns_the_gradient_kernels_sdf(pools, n, mode):
    _check(pools, 3, n, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["plain", "index", "count"])
def test_five_level_kernels_still_agree(pools, mode):
    _check(pools, 5, 33, mode)


@pytest.mark.gpu
def test_a_nan_coordinate_poisons_its_own_point_only(pools):
    from gens_amd import ops
    plan, packed, pool, want, want_g = pools(3)
    n, bad = 129, [40, 97, 128]                    # a lane of each half of a wave's points, and the lone point of the second workgroup
    pts = pool[:n].clone()
    for k, row in enumerate(bad):
        pts[row, k] = float("nan")
    sdf, grad, val = B._run(ops, plan, packed, pts, "bf16x3")
    good = torch.ones(n, dtype=torch.bool, device="cuda")
    good[bad] = False
    assert torch.isnan(val[~good]).all() and torch.isnan(sdf[~good]).all() and torch.isnan(grad[~good]).all()
    assert torch.equal(val[good], want[:n][good]) and torch.equal(sdf[good], want[:n][good]) and torch.equal(grad[good], want_g[:n][good])
