"""tests/patch_warp_reference.py pinned on the CPU: the recorded g7_patchwarp patches, the float32 oracle (with its autograd on `inside` and `border`)
and the clean float32 restatement lie inside the float64 bounds on every shape and class, every seeded defect leaves them on the class that is
named for it here, the caps on free samples and rays hold, every class is what it says, `exact` is bit-equal between float32 and float64, and the
bound is not vacuous.  The K9 read and the up-sampling references are pinned against the oracle's _bilinear and F.interpolate in float64.
Run with -s for the figures."""
import numpy as np
import pytest
import torch

from oracle import gens_oracle as K
from tests import patch_warp_reference as R

IDS = [R.case_id(s, c) for s, c in R.ALL_CASES]
BWD_CASES = [(s, c) for s, c in R.ALL_CASES if c in R.BWD_CLASSES + ("exact",)]
# the class that must notice each defect (on at least one shape); H_v does not change with the normal's length but for the 1e-10 beside disp, so
# normal_not_normalised shows only on the nearly-zero normals of `zero_normal`
CAUGHT_BY = dict(rows_cols_swapped="inside", offsets_from_zero="inside", tex_view_off_by_one="inside", intr_view_off_by_one="inside",
                 rel_transposed="inside", normal_not_rotated="inside", normal_not_normalised="zero_normal", align_corners_false="inside",
                 border_clamp="border", ref_through_homography="inside", no_h_du0="inside", no_dh="inside", dh_sign="inside", slopes_swapped="inside",
                 quotient_without_dq2="inside", border_slope_kept="border")


def _oracle_inputs(case):
    """pts = o + d z and the reference-camera normals as the caller of surface_patch_warp forms them, in float32."""
    z = case["z"].clone().requires_grad_(True)
    pts = case["o"][:, None, :] + case["d"][:, None, :] * z[:, None, None]
    n = case["g0"].reshape(-1, 1, 3)
    nn = torch.linalg.norm(n, dim=-1, keepdim=True)
    n = n / torch.where(nn <= 0, torch.full_like(nn, 1e-8), nn)
    return z, pts, (n @ case["c2ws"][0, :3, :3]).detach()


def test_recorded_patch_warp_lies_inside_the_bound(golden):
    g = golden("g7_patchwarp")
    b = g["pts"].shape[0]
    zero = torch.zeros(b)
    ref = R.reference(g["pts"][:, 0], torch.zeros(b, 3), zero, torch.ones(b, 3), g["c2ws"], g["intrs"], torch.inverse(g["intrs"])[0, :3, :3],
                      g["images"], 11, normals=g["normals"][:, 0])
    res = R.check_forward(ref, g["ref_val"], g["src_val"])
    print(f"g7_patchwarp: {res}")
    assert R.forward_ok(res)
    assert not bool(ref["free"][:, 1:].any()) and bool(np.isfinite(ref["bound"][:, 1:]).all())        # (ray 0 sits AT the reference centre)


@pytest.mark.parametrize("shape,cls", R.ALL_CASES, ids=IDS)
def test_float32_oracle_lies_inside_the_bound(shape, cls):
    case, _ = R.shape_case(shape, cls)
    ref = R.case_reference(case, torch.inverse(case["intrs"])[0, :3, :3])
    z, pts, normals = _oracle_inputs(case)
    o_ref, o_src = K.patch_warp(pts, normals, case["maps"], case["intrs"], case["c2ws"], case["patch"])
    res = R.check_forward(ref, o_ref.detach(), o_src.detach())
    msg = f"oracle {R.case_id(shape, cls)}: ref {res['use_ref']:.3f}, sampled {res['use_sampled']:.3f} of the bound"
    assert R.forward_ok(res), res
    if cls in ("inside", "border", "exact"):               # reverse mode: d/dpts contracted with rays_d (what autograd does for z itself)
        g_z = torch.autograd.grad((o_src * case["cot"]).sum(), z)[0]
        ratio = R.check_backward(ref["g_z"], ref["g_bound"], g_z)
        msg += f", reverse-mode g_z {ratio:.3f} of the forward-mode bound"
        assert ratio <= R.REVERSE_MODE_FACTOR
    print(msg)


@pytest.mark.parametrize("shape,cls", R.ALL_CASES, ids=IDS)
def test_float32_restatement_lies_inside_both_bounds(shape, cls):
    case, ref = R.shape_case(shape, cls)
    res = R.check_forward(ref, *R.patch_warp_f32(*R.case_args(case)))
    use_g = R.check_backward(ref["g_z"], ref["g_bound"], R.patch_warp_bwd_f32(*R.case_args(case), case["cot"]))
    print(f"patch_warp_f32 {R.case_id(shape, cls)}: ref {res['use_ref']:.3f}, sampled {res['use_sampled']:.3f}, g_z {use_g:.3f} of the bound")
    assert R.forward_ok(res) and use_g <= 1


@pytest.mark.parametrize("shape,cls", R.ALL_CASES, ids=IDS)
def test_caps_hold_and_the_case_is_what_its_class_says(shape, cls):
    case, ref = R.shape_case(shape, cls)
    n_free, n = int(ref["free"].sum() + ref["ref_free"].sum()), ref["free"].size + ref["ref_free"].size
    free_rays = int(np.isinf(ref["g_bound"]).sum())
    b = case["z"].shape[0]
    h, w = case["maps"].shape[2:]
    print(f"{R.case_id(shape, cls)}: {n_free} of {n} samples free, {free_rays} of {b} rays free in the backward")
    if cls == "grazing":
        assert n_free <= 0.5 * n
        ratio = np.abs(ref["disp"]) / np.linalg.norm((case["o"] + case["d"] * case["z"][:, None] - case["c2ws"][0, :3, 3]).numpy(), axis=-1)
        assert bool((ratio > 0.9e-3).all()) and bool((ratio < 0.11).all())
    else:
        assert n_free <= R.AMBIGUOUS_CAP * n
    if cls in ("inside", "border", "zero_normal", "exact"):
        assert free_rays <= R.BWD_FREE_CAP * b
    ix, iy, u0, v0 = ref["ix"], ref["iy"], ref["u0"], ref["v0"]
    half = max(case["patch"] // 2, 1)
    if cls == "inside":
        assert bool(((u0 > -0.01) & (u0 < w - 0.99) & (v0 > -0.01) & (v0 < h - 0.99)).all())
        assert bool((np.abs(ref["disp"]) > 0.45 * case["z"].numpy()).all())
    elif cls == "border":
        near = np.minimum(np.minimum(np.abs(u0), np.abs(u0 - (w - 1))), np.minimum(np.abs(v0), np.abs(v0 - (h - 1))))
        assert bool((near <= half + 0.01).all())
        if b >= 33:                                         # zero-padded taps on both sides, and reads beyond
            rx = ref["rix"]
            assert bool(((rx > -1) & (rx < 0)).any()) and bool(((rx > w - 1) & (rx < w)).any()) and bool((rx < -1).any()) and bool((rx > w).any())
            assert bool(((ix > -1) & (ix < 0)).any()) and bool(((ix > w - 1) & (ix < w)).any())
    elif cls == "outside":
        out = (ix + ref["e_ix"] < -1) | (ix - ref["e_ix"] > w) | (iy + ref["e_iy"] < -1) | (iy - ref["e_iy"] > h)
        assert bool(out.all()) and bool((ref["sampled"] == 0).all()) and (b < 9 or float(np.abs(ix).max()) > 20 * w)       # some far outside
    elif cls == "behind":
        assert bool((ref["q2"][0] < 0).all()) and bool((ref["q2"][1:] > 0).all() if ref["q2"].shape[0] > 1 else True)
    elif cls == "zero_normal":
        assert bool((case["g0"][::2] == 0).all()) and bool((ref["disp"][::2] == 0).all()) and not bool(ref["free"].any())
    elif cls == "nonfinite":
        bad = ref["bad_ray"]
        assert int(bad.sum()) == min(4, max(1, b - 1)) and bool(ref["dead"][:, bad].all()) and not bool(ref["dead"][:, ~bad].any())
        assert bool((ref["g_z"][bad] == 0).all()) and bool((ref["g_bound"][bad] == 0).all())
        z_bad = ~np.isfinite(case["z"].numpy())
        assert bool(ref["ref_dead"][:, z_bad].all()) and not bool(ref["ref_dead"][:, ~z_bad].any())
    elif cls == "exact":
        assert n_free == 0 and free_rays == 0
        for k in ("e_ix", "e_iy", "e_dgx", "e_dgy", "g_bound"):
            assert not bool(ref[k].any()), k                 # nothing rounds
        frac_x, frac_y = ix - np.floor(ix), iy - np.floor(iy)
        for v in (0.0, 0.25, 0.125, 0.0625):
            assert bool((frac_x == v).any()), v
        assert bool((frac_y == 0.5).any())
        for v in (-1.0, 0.0, w - 1.0, float(w), -2.0, -3.0):                                    # ON the boundaries, and beyond
            assert bool((ix[1] == v).any()), v
        assert bool((ix[2] > w + 30).any()) and bool((ref["dgx"] != 0).any()) and bool((ref["g_z"] != 0).any())
        assert torch.equal(case["kinv"], torch.tensor([[1 / 32, 0, -1], [0, 1 / 32, -0.5], [0, 0, 1]]))


def test_exact_is_bit_equal_between_float32_and_float64():
    case, ref = R.shape_case(None, "exact")
    r32, s32 = R.patch_warp_f32(*R.case_args(case))
    assert np.array_equal(r32.numpy().astype(np.float64), ref["ref"]) and np.array_equal(s32.numpy().astype(np.float64), ref["sampled"])
    g32 = R.patch_warp_bwd_f32(*R.case_args(case), case["cot"])
    assert np.array_equal(g32.numpy().astype(np.float64), ref["g_z"])
    z, pts, normals = _oracle_inputs(case)
    o_ref, o_src = K.patch_warp(pts, normals, case["maps"], case["intrs"], case["c2ws"], case["patch"])
    assert torch.equal(o_ref.detach() + 0.0, r32 + 0.0) and torch.equal(o_src.detach() + 0.0, s32 + 0.0)
    assert torch.equal(torch.inverse(case["intrs"])[0, :3, :3], case["kinv"])


@pytest.mark.parametrize("defect", R.DEFECTS + R.BWD_DEFECTS)
def test_each_defect_is_noticed_by_its_class(defect):
    caught = []
    for shape, cls in R.ALL_CASES:
        case, ref = R.shape_case(shape, cls)
        if defect in R.BWD_DEFECTS:
            if (shape, cls) not in BWD_CASES:
                continue
            ok = R.check_backward(ref["g_z"], ref["g_bound"], R.patch_warp_bwd_f32(*R.case_args(case), case["cot"], defect=defect)) <= 1
        else:
            ok = R.forward_ok(R.check_forward(ref, *R.patch_warp_f32(*R.case_args(case), defect=defect)))
        if not ok:
            caught.append(R.case_id(shape, cls))
    print(f"{defect}: noticed on {len(caught)} cases, {sum(c.endswith(CAUGHT_BY[defect]) for c in caught)} of them `{CAUGHT_BY[defect]}`")
    assert any(c.endswith(CAUGHT_BY[defect]) for c in caught)


def test_the_bound_is_not_vacuous():
    """On `inside` at the shipped shape the median value bound is below 1e-3 of the largest texel; the backward bound of every shape's decided
    rays is a small part of the gradient's scale."""
    case, ref = R.shape_case(3, "inside")
    top = float(case["maps"].abs().max())
    med = float(np.median(ref["bound"]))
    print(f"{R.SHAPE_IDS[3]}: median value bound {med:.2e}, largest texel {top:.2f}")
    assert bool(np.isfinite(ref["bound"]).all()) and med < 1e-3 * top
    for shape in range(len(R.SHAPES)):
        _, ref = R.shape_case(shape, "inside")
        scale = float(np.abs(ref["g_z"]).max())
        med = float(np.median(ref["g_bound"]))
        print(f"{R.SHAPE_IDS[shape]}: median g_z bound {med:.2e}, largest |g_z| {scale:.2e}")
        assert med < 0.05 * scale


# ------------------------------------------------------------------------------------------------------------------ K9 direct, up-sampling
@pytest.mark.parametrize("cls", R.K9_CLASSES)
@pytest.mark.parametrize("c", R.K9_CHANNELS)
def test_k9_reference_against_the_oracle_read(c, cls):
    for n in R.K9_POINTS:
        m, xy, cot = R.k9_case(n, c, cls)
        val, val_bound, g, g_bound = R.k9_reference(m, xy, cot)
        assert val.shape == (n, c) and g.shape == (n, 2)
        if n == 0:
            continue
        xy_t = xy.clone().requires_grad_(True)
        o_val = K._bilinear(m, xy_t[:, 0], xy_t[:, 1]).t()
        o_g = torch.autograd.grad((o_val * cot).sum(), xy_t)[0]
        o_g = torch.where(torch.isfinite(xy).all(-1, keepdim=True), o_g, torch.zeros_like(o_g))     # (autograd leaves NaN at a non-finite coordinate)
        use_v = float(R.use(o_val.detach(), val, val_bound).max())
        use_m = float(R.use(R.patch_sample_f32(m, xy), val, val_bound).max())
        use_g = float(R.use(o_g, g, g_bound).max())
        assert max(use_v, use_m, use_g) <= 1, (n, use_v, use_m, use_g)
        if cls == "on_grid":
            assert np.array_equal(R.patch_sample_f32(m, xy).numpy().astype(np.float64), val) and np.array_equal(o_g.numpy().astype(np.float64), g)
            assert not bool(g_bound.any())
        if cls == "border" and n >= 255:
            x = xy[:, 0].numpy()
            assert bool(((x > -1) & (x < 0)).any()) and bool(((x > 11) & (x < 12)).any())


@pytest.mark.parametrize("size", range(len(R.UP_SIZES)))
@pytest.mark.parametrize("c", R.UP_CHANNELS)
def test_upsampling_reference_is_f_interpolate(c, size):
    src, h, w = R.up_case(size, c)
    val, bound = R.upsample_reference(src, h, w)
    want = torch.nn.functional.interpolate(src.double(), size=(h, w), mode="bilinear", align_corners=False).numpy()
    assert float(np.abs(val - want).max()) <= 1e-13
    got32 = torch.nn.functional.interpolate(src, size=(h, w), mode="bilinear", align_corners=False)
    ours = K.upsample_bilinear_half_pixel(src, h, w)
    use_t, use_o = float(R.use(got32, val, bound).max()), float(R.use(ours, val, bound).max())
    print(f"up-sampling {R.UP_SIZES[size]} c{c}: F.interpolate {use_t:.3f}, oracle {use_o:.3f} of the bound; median bound {np.median(bound):.2e}")
    assert use_t <= 1 and use_o <= 1 and float(np.median(bound)) < 1e-5
