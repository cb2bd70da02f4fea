"""The fused patch warp (gens_patch_warp_fwd / _bwd, k19_step.hip), the K9 read (gens_patch_sample_fwd / _bwd) and the warp features' up-sampling
(gens_upsample2d_into / _cat, k9_misc.hip) against the float64 references and bounds of tests/patch_warp_reference.py (pinned on the CPU by
test_patch_warp_reference_cpu.py).  The reference gets the kernel's own kinv_ref (SceneCams.kinv_ref copied back).  The texel tensors of every
forward, K9 and up-sampling case carry a NaN sentinel in their pad channels: no output of those kernels may depend on them.

    shape (R.SHAPES: views, h x w, channels, patch, rays)   what it exercises
    2, 2 x 2, 1, 1, 1         the smallest legal value of every argument: two samples on 64 lanes, three of the block's four waves without a ray
    3, 5 x 7, 3, 3, 4         exactly one full block; c = 3: the tail of one float4; every 3 x 3 patch touches the border
    3, 5 x 7, 5, 3, 5         a second block that holds one ray; c = 5: q4 = 2 with three pad channels
    5, 33 x 65, 12, 11, 70    the shipped form: 605 samples = nine passes of the lane loop + 29 lanes; 17 blocks + 2 rays
    11, 24 x 32, 12, 11, 33   the fine-tuning view count
    16, 9 x 12, 16, 15, 9     GENS_MAX_VIEWS, 4 * PW_MAX_Q4 channels, the largest patch (wider than the image)
    `exact`: 4, 33 x 65, 5, 5, 24   nothing rounds: kernel and reference agree bit for bit, ON every texel and image boundary

Classes: inside, border, outside, behind (q.z < 0), grazing, zero_normal, nonfinite, exact.  Run with -s for the share of the bound used."""
import numpy as np
import pytest
import torch

from tests import patch_warp_reference as R

pytestmark = pytest.mark.gpu

IDS = [R.case_id(s, c) for s, c in R.ALL_CASES]
BWD_CASES = [(s, c) for s in (1, 2, 3, 5) for c in R.BWD_CLASSES] + [(None, "exact")]
BWD_IDS = [R.case_id(s, c) for s, c in BWD_CASES]


@pytest.fixture(scope="module")
def ops():
    from gens_amd import ops
    return ops


def _bits(t):
    return t.view(torch.int32)


def _run(ops, case, grad=False, cot=None):
    """-> (ref, sampled, g_z or None, kinv) on the CPU, from fresh device copies.  The forward-only runs carry NaN in the pad channels; the runs
    with a backward pass carry zeros there, which is what the project's own producers write: patch_warp_bwd_k multiplies the pad channels by a
    zero cotangent, so a NaN there turns the sample's term into NaN and the sample is dropped (open: DESIGN.md)."""
    pad = 0.0 if grad else float("nan")
    cams = ops.SceneCams(case["intrs"].cuda(), case["c2ws"].cuda())
    assert torch.equal(cams.intr.cpu(), case["intrs"]) and torch.equal(cams.c2w.cpu(), case["c2ws"])
    z = case["z"].cuda().requires_grad_(grad)
    tex = R.texels(case["maps"], pad).cuda()
    ref, smp = ops.patch_warp(z, case["o"].cuda(), case["d"].cuda(), case["g0"].cuda(), cams, (tex, case["maps"].shape[1]), case["patch"])
    g_z = None
    if grad:
        (smp * (case["cot"] if cot is None else cot).cuda()).sum().backward()
        g_z = z.grad.cpu()
    return ref.detach().cpu(), smp.detach().cpu(), g_z, cams.kinv_ref.cpu().clone()


# ------------------------------------------------------------------------------------------------------------------ fused forward
@pytest.mark.parametrize("shape,cls", R.ALL_CASES, ids=IDS)
def test_forward_lies_inside_the_float64_bound(ops, shape, cls):
    case, _ = R.shape_case(shape, cls)
    got_ref, got_smp, _, kinv = _run(ops, case)
    case, ref = R.reference_for(shape, cls, kinv)
    s, b, p, c = case["c2ws"].shape[0] - 1, case["z"].shape[0], case["patch"] ** 2, case["maps"].shape[1]
    assert got_ref.shape == (1, b, p, c) and got_smp.shape == (s, b, p, c)
    res = R.check_forward(ref, got_ref, got_smp)
    print(f"{R.case_id(shape, cls)}: ref {res['use_ref']:.3f}, sampled {res['use_sampled']:.3f} of the bound; {res['n_free']} of {res['n_samples']} "
          f"samples free")
    assert res["use_ref"] <= 1, f"the reference patch uses {res['use_ref']:.3g} of the bound"
    assert res["use_sampled"] <= 1, f"the source patches use {res['use_sampled']:.3g} of the bound"
    assert res["finite"], "a free sample is not finite"
    assert res["zeros"], "a pinned zero (non-finite input) is not zero"
    if cls == "nonfinite":
        assert bool(ref["dead"].any()) and bool(ref["ref_dead"].any())
    if cls == "exact":
        assert torch.equal(kinv, case["kinv"]) and res["n_free"] == 0
        assert np.array_equal(got_ref.numpy().astype(np.float64), ref["ref"]) and np.array_equal(got_smp.numpy().astype(np.float64), ref["sampled"])


# ------------------------------------------------------------------------------------------------------------------ fused backward
@pytest.mark.parametrize("shape,cls", BWD_CASES, ids=BWD_IDS)
def test_backward_lies_inside_every_rays_bound(ops, shape, cls):
    case, _ = R.shape_case(shape, cls)
    _, _, g_z, kinv = _run(ops, case, grad=True)
    case, ref = R.reference_for(shape, cls, kinv)
    assert g_z.shape == case["z"].shape
    use = R.check_backward(ref["g_z"], ref["g_bound"], g_z)
    free = int(np.isinf(ref["g_bound"]).sum())
    print(f"{R.case_id(shape, cls)}: g_z uses {use:.3f} of the bound; {free} of {g_z.numel()} rays free")
    assert use <= 1, f"g_z uses {use:.3g} of a ray's bound"
    assert bool(torch.isfinite(g_z).all())
    bad_z = ~torch.isfinite(case["z"])
    assert bool((g_z[bad_z] == 0).all()) and bool((g_z[torch.from_numpy(ref["bad_ray"])] == 0).all())
    if cls == "nonfinite":
        assert bool(bad_z.any())
    if cls == "exact":
        assert free == 0 and np.array_equal(g_z.numpy().astype(np.float64), ref["g_z"])


def test_zero_points(ops):
    """ops.patch_sample with no point returns an empty tensor, and a backward pass through it runs.  (ops.patch_warp with no ray hands NULL
    pointers to an entry point that refuses them; open, with the pad channels of the fused backward: DESIGN.md.)"""
    m, _, _ = R.k9_case(1, 5, "inside")
    tex = R.texels(m[None])[0].cuda()
    xy = torch.zeros(0, 2, device="cuda", requires_grad=True)
    out = ops.patch_sample(tex, xy, 5)
    assert out.shape == (0, 5)
    out.sum().backward()
    assert xy.grad.shape == (0, 2)


@pytest.mark.parametrize("shape,cls", [(3, "border"), (5, "nonfinite")], ids=[R.case_id(3, "border"), R.case_id(5, "nonfinite")])
def test_the_same_call_twice_gives_the_same_bits(ops, shape, cls):
    case, _ = R.shape_case(shape, cls)
    first, second = _run(ops, case, grad=True), _run(ops, case, grad=True)
    for a, b in zip(first[:3], second[:3]):
        assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("shape,cls", [(2, "inside"), (2, "border"), (3, "inside"), (3, "border")],
                         ids=[R.case_id(s, c) for s in (2, 3) for c in ("inside", "border")])
def test_operator_by_operator_mirror_lies_inside_the_same_bound(ops, shape, cls):
    """projector.surface_patch_warp given pts = o + d z and the reference-camera normals, as render_core forms them."""
    from gens_amd.models.modules.projector import surface_patch_warp
    case, _ = R.shape_case(shape, cls)
    intrs, c2ws = case["intrs"].cuda(), case["c2ws"].cuda()
    pts = case["o"].cuda()[:, None, :] + case["d"].cuda()[:, None, :] * case["z"].cuda()[:, None, None]
    n = case["g0"].cuda().reshape(-1, 1, 3)
    nn = torch.linalg.norm(n, dim=-1, keepdim=True)
    n = n / torch.where(nn <= 0, torch.full_like(nn, 1e-8), nn)
    tex = R.texels(case["maps"]).cuda()
    got_ref, got_smp = surface_patch_warp(pts, n @ c2ws[0, :3, :3], (tex, case["maps"].shape[1]), intrs, c2ws, case["patch"])
    case, ref = R.reference_for(shape, cls, ops.SceneCams.of(intrs, c2ws).kinv_ref.cpu())
    res = R.check_forward(ref, got_ref.cpu(), got_smp.cpu())
    print(f"mirror {R.case_id(shape, cls)}: ref {res['use_ref']:.3f}, sampled {res['use_sampled']:.3f} of the bound")
    assert R.forward_ok(res), res


# ------------------------------------------------------------------------------------------------------------------ K9 direct
@pytest.mark.parametrize("cls", R.K9_CLASSES)
@pytest.mark.parametrize("c", R.K9_CHANNELS)
def test_k9_read_and_its_derivative(ops, c, cls):
    worst = [0.0, 0.0]
    for n in R.K9_POINTS:
        m, xy, cot = R.k9_case(n, c, cls)
        val, val_bound, g, g_bound = R.k9_reference(m, xy, cot)
        tex = R.texels(m[None])[0].cuda()
        xy_d = xy.cuda().requires_grad_(True)
        out = ops.patch_sample(tex, xy_d, c)
        assert out.shape == (n, c)
        (out * cot.cuda()).sum().backward()
        got, got_g = out.detach().cpu(), xy_d.grad.cpu()
        assert got_g.shape == (n, 2)
        if n == 0:
            continue
        worst = [max(worst[0], float(R.use(got, val, val_bound).max())), max(worst[1], float(R.use(got_g, g, g_bound).max()))]
        if cls == "on_grid":
            assert np.array_equal(got.numpy().astype(np.float64), val) and np.array_equal(got_g.numpy().astype(np.float64), g), n
    print(f"K9 c{c} {cls}: values {worst[0]:.3f}, d/d(xy) {worst[1]:.3f} of the bound")
    assert worst[0] <= 1 and worst[1] <= 1


# ------------------------------------------------------------------------------------------------------------------ up-sampling
@pytest.mark.parametrize("size", range(len(R.UP_SIZES)), ids=[f"{a[0]}x{a[1]}-to-{b[0]}x{b[1]}" for a, b in R.UP_SIZES])
@pytest.mark.parametrize("c", R.UP_CHANNELS)
def test_upsampling_into_a_channel_slice(c, size):
    from gens_amd import lib as L
    src, h, w = R.up_case(size, c)
    val, bound = R.upsample_reference(src, h, w)
    n, cpad, off = src.shape[0], c + 3, 2
    dst = torch.full((n, h, w, cpad), 0.5, device="cuda")
    s = src.cuda().contiguous()
    L.call("gens_upsample2d_into", L.ptr(s), n, c, src.shape[2], src.shape[3], L.ptr(dst), h, w, cpad, off, L.stream())
    got = dst.cpu()
    use = float(R.use(got[..., off:off + c].permute(0, 3, 1, 2), val, bound).max())
    print(f"gens_upsample2d_into {R.UP_SIZES[size]} c{c}: {use:.3f} of the bound")
    assert use <= 1
    assert bool((got[..., :off] == 0.5).all()) and bool((got[..., off + c:] == 0.5).all())              # outside the slice: untouched


@pytest.mark.parametrize("size", range(len(R.UP_SIZES)), ids=[f"{a[0]}x{a[1]}-to-{b[0]}x{b[1]}" for a, b in R.UP_SIZES])
@pytest.mark.parametrize("c,cpad", [(1, 5), (4, 12), (4, 9), (5, 13)], ids=["c1-generic", "c4-four", "c4-generic", "c5-generic"])
def test_upsampling_cat(c, cpad, size):
    """Two maps of the same source into one texel tensor: the FOUR form (every map four channels, C_pad a multiple of four) and the generic
    one; the pad channels are written as zeros."""
    from gens_amd import lib as L
    src, h, w = R.up_case(size, c)
    val, bound = R.upsample_reference(src, h, w)
    n = src.shape[0]
    maps = [src.cuda().contiguous(), src.cuda().contiguous()]
    dst = torch.full((n, h, w, cpad), float("nan"), device="cuda")
    chw = [d for f in maps for d in f.shape[1:]]
    L.call("gens_upsample2d_cat", L.ptr_table(maps), L.int_table(chw), 2, n, L.ptr(dst), h, w, cpad, L.stream())
    got = dst.cpu()
    use = max(float(R.use(got[..., k * c:(k + 1) * c].permute(0, 3, 1, 2), val, bound).max()) for k in range(2))
    print(f"gens_upsample2d_cat {R.UP_SIZES[size]} c{c} into {cpad}: {use:.3f} of the bound")
    assert use <= 1
    assert cpad > 2 * c and bool((got[..., 2 * c:] == 0).all())                                        # pad channels: zeros
    assert torch.equal(_bits(got[..., :c].contiguous()), _bits(got[..., c:2 * c].contiguous()))
