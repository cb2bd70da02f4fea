"""GPU checks of gens_sdf_value_bf16x3's three-level kernel at TWO resident waves per SIMD (k6b_sdf_bf16x3.hip, the "diet" build of
sdf_bf16x3_k<3, false>).  Shipped shape: variant (a), two independent 256-thread workgroups per CU, each with its own 32 KB weight ring and
6 KB per wave of conditioning blocks behind it.

The gradient kernel is untouched code, so its SDF column is the bit pattern the value kernel had before: torch.equal with it pins the
two-wave kernel to the one-wave kernel it replaces.  gens_sdf_bf16x3_residency states the occupancy claim on the device."""
import ctypes as C

import pytest
import torch

from .test_hip_sdfmlp import _net

pytestmark = pytest.mark.gpu

FILL = 100.0
N_BIG = 65536 + 129      # 514 workgroups on 256 CUs: every CU holds two resident workgroups, and a ragged tail


def _points(n, seed):
    """Inside and outside the cube (zero padding), and -- where there is room -- points on the cube's faces, edges and corners and on
    voxel planes of the 16 / 12 / 8 lattices, where the look-up's corner masks change."""
    g = torch.Generator().manual_seed(seed)
    pts = torch.rand(n, 3, generator=g) * 2.4 - 1.2
    border = torch.tensor([[1.0, 0.3, -0.2], [-1.0, -1.0, 0.5], [1.0, 1.0, 1.0], [-1.0, 1.0, -1.0], [0.0, 0.0, 0.0], [1.0 / 15, -3.0 / 11, 5.0 / 7],
                           [1.0000001, 0.0, 0.0], [-0.99999994, 0.5, 1.2]])
    k = min(len(border), max(0, n - 1))
    pts[n - k:] = border[:k]
    return pts


@pytest.fixture(scope="module")
def scene():
    """One network, weight stream and volume set per level count, shared by every test of this file and left unchanged."""
    from gens_amd import ops, synthetic
    made = {}

    def get(n_levels):
        if n_levels not in made:
            net, dims = _net(n_levels, seed=60 + n_levels)
            packed = ops.VolumeSet.packed([(v * 2).cuda() for v in synthetic.make_volumes(dims, seed=14)])
            plan = ops.SdfMlpPlan(net)
            assert plan.bf16x3_pieces is not None
            made[n_levels] = (plan, packed)
        return made[n_levels]
    return get


def _both(scene, n_levels, pts, idx=None, count=None):
    """(SDF of the gradient kernel, SDF of the value kernel) on rows pre-filled with FILL; both launches are checked to be the bf16x3 ones."""
    from gens_amd import lib as L, ops
    plan, packed = scene(n_levels)
    n = pts.shape[0]
    sdf, grad, val = torch.full((n, 1), FILL, device="cuda"), torch.zeros(n, 3, device="cuda"), torch.full((n, 1), FILL, device="cuda")
    L.profile_begin()
    ops.sdf_mlp(plan, packed, pts, index=idx, want_grad=True, sdf_out=sdf, grad_out=grad, count=count)
    ops.sdf_mlp(plan, packed, pts, index=idx, sdf_out=val, count=count)
    launched = set(L.profile_end())
    assert {"gens_sdf_value_bf16x3", "gens_sdf_grad_bf16x3"} <= launched, launched
    return sdf, val


@pytest.fixture(autouse=True)
def _bf16x3(monkeypatch):
    from gens_amd import ops
    monkeypatch.setattr(ops.kernels, "sdf_value", "bf16x3")
    monkeypatch.setattr(ops.kernels, "sdf_grad", "bf16x3")


# 1 .. 33: a partial wave; 127 .. 129: the workgroup's edge; 255, 257: two workgroups; N_BIG: two resident workgroups on every CU
@pytest.mark.parametrize("n", [1, 31, 32, 33, 127, 128, 129, 255, 257, N_BIG])
def test_two_wave_value_kernel_returns_the_gradient_kernels_sdf(scene, n):
    pts = _points(n, seed=n + 3).cuda()
    sdf, val = _both(scene, 3, pts)
    assert torch.isfinite(sdf).all() and (sdf != FILL).all()
    assert torch.equal(sdf, val)


def test_two_wave_value_kernel_on_the_compacted_path(scene):
    """index = a random subset in random order, count = a device int below n_max: the rows named by index[:count] are written, bit-equal
    to the gradient kernel's, and every other row keeps its fill value."""
    n = 4099
    pts = _points(n, seed=5).cuda()
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(n)).cuda()
    k = 3001
    count = torch.tensor([k], dtype=torch.int32, device="cuda")
    sdf, val = _both(scene, 3, pts, idx, count)
    assert torch.equal(sdf, val)
    dead = torch.ones(n, dtype=torch.bool, device="cuda")
    dead[idx[:k]] = False
    assert int(dead.sum()) == n - k and (val[dead] == FILL).all() and (val[~dead] != FILL).all()
    full, _ = _both(scene, 3, pts)
    assert torch.equal(val[~dead], full[~dead])      # ... and they are the values of the rows they name


def test_five_level_value_kernel_returns_the_gradient_kernels_sdf(scene):
    pts = _points(1531, seed=8).cuda()
    sdf, val = _both(scene, 5, pts)
    assert torch.isfinite(sdf).all() and torch.equal(sdf, val)


def test_two_wave_value_kernel_is_deterministic_under_co_residence(scene):
    from gens_amd import ops
    plan, packed = scene(3)
    pts = _points(N_BIG, seed=9).cuda()
    a, b = torch.full((N_BIG, 1), FILL, device="cuda"), torch.full((N_BIG, 1), FILL, device="cuda")
    ops.sdf_mlp(plan, packed, pts, sdf_out=a)
    ops.sdf_mlp(plan, packed, pts, sdf_out=b)
    assert (a != FILL).all() and torch.equal(a, b)


def _residency(n_levels, grad):
    from gens_amd import lib as L
    out = (C.c_int * 4)()
    rc = L.load().gens_sdf_bf16x3_residency(n_levels, grad, out)
    assert rc == 0, L.load().gens_last_error()
    return {"regs": out[0], "scratch": out[1], "lds": out[2], "blocks": out[3]}


def test_residency_on_the_device():
    """Variant (a) shipped: the three-level value kernel has no scratch and TWO 256-thread workgroups per CU, two waves per SIMD.  The
    gradient kernels (160 KB of LDS) and the five-level value kernel (28 more conditioning registers) keep one, without scratch."""
    from gens_amd import lib as L
    v3 = _residency(3, 0)
    print("residency", {(nl, g): _residency(nl, g) for nl in (3, 5) for g in (0, 1)})
    assert v3["scratch"] == 0 and v3["blocks"] == 2 and 0 < v3["regs"] <= 256, v3
    assert v3["lds"] == 32768 + 4 * 6144 and 2 * v3["lds"] <= 160 * 1024, v3
    for nl in (3, 5):
        g = _residency(nl, 1)
        assert g["scratch"] == 0 and g["blocks"] == 1 and g["lds"] == 160 * 1024, (nl, g)
    v5 = _residency(5, 0)
    assert v5["scratch"] == 0 and v5["blocks"] == 1 and v5["lds"] == 32768, v5
    out = (C.c_int * 4)()
    assert L.load().gens_sdf_bf16x3_residency(4, 0, out) == -2 and b"3 or 5" in L.load().gens_last_error()
    assert L.load().gens_sdf_bf16x3_residency(3, 0, None) == -1
