"""tests/loss_reference.py pinned on the CPU: the float64 references hold the reference project's recorded results (g8_tv, g11_lncc, g19_loss) to
the criteria the device is held to, the float32 oracle and every clean float32 restatement meet them on every case, every seeded defect
fails them on at least one case, and the kept-ray cap of the LNCC gradient comparison holds.  Run with -s for the figures."""
import os

import numpy as np
import pytest
import torch

from oracle import gens_oracle as K
from tests import loss_reference as R

from .conftest import GOLDEN

LNCC_IDS = ["x".join(map(str, s)) for s in R.LNCC_SHAPES]
ALL_LNCC = [(i, c) for i in range(len(R.LNCC_SHAPES)) for c in R.LNCC_CLASSES]


# ------------------------------------------------------------------------------------------------------------------ recorded results
def test_recorded_tv_meets_the_criteria(golden):
    g = golden("g8_tv")
    vols, masks = [g["vol0"], g["vol1"]], [g["mask0"], g["mask1"]]
    ref = R.tv_reference(vols, masks)
    use_v, use_g, nan_ok = R.tv_check(ref, g["tv"], None, [g["gvol0"], g["gvol1"]])
    print(f"g8_tv: value use {use_v:.3f}, gradient use {use_g:.3f}")
    assert use_v <= 1 and use_g <= 1 and nan_ok


def test_recorded_lncc_meets_the_criteria(golden):
    g = golden("g11_lncc")
    keep_rays = torch.tensor([i for i in range(g["ref"].shape[1]) if i != 5])             # ray 5: constant patches (tests/test_lncc.py)
    ref, src, cot = g["ref"][:, keep_rays], g["src"][:, keep_rays], g["cot"][keep_rays]
    ok, text = R.lncc_value_ok(R.lncc_value_errors(ref, src, g["ncc"][keep_rays]))
    print("g11_lncc:", text)
    assert ok
    g_ref64, g_src64, keep = R.lncc_grads64(ref, src, cot)
    o_ref, o_src = R.lncc_grads_oracle32(ref, src, cot)
    for name, got, o32, want in (("g_ref", g["g_ref"][:, keep_rays], o_ref, g_ref64), ("g_src", g["g_src"][:, keep_rays], o_src, g_src64)):
        e, e32 = R.grad_error(got, want, keep), R.grad_error(o32, want, keep)
        print(f"g11_lncc {name}: recorded {e:.2e}, float32 oracle {e32:.2e}, {int(keep.sum())} of {keep.numel()} rays kept")
        assert e <= max(4 * e32, 1e-6)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_recorded_loss_meets_the_criteria(tag):
    raw = np.load(os.path.join(GOLDEN, "g19_loss.npz"))
    g = {k[2:]: torch.from_numpy(raw[k]) for k in raw.files if k.startswith(tag + ".")}
    preds = {k[5:]: v for k, v in g.items() if k.startswith("pred.")}
    targets = {k[7:]: v for k, v in g.items() if k.startswith("target.")}
    preds["ncc"] = K.lncc(preds.pop("ref_gray_val"), preds.pop("sampled_gray_val"))
    conf = g["conf"].tolist()
    case = dict(preds=preds, targets=targets, weights=conf[:8], scale=conf[8], cot=1.0)
    ref = R.loss_reference(case)
    out = {k: float(g["out." + k]) for k in R.LOSS_KEYS}
    grads = {k: g["grad." + k] for k in ref["grads"] if "grad." + k in g}
    for k in ref["grads"]:
        if k not in grads:                                     # ncc is an inner value of the recorded graph
            grads[k] = ref["grads"][k]
    use_v, use_g, text = R.loss_check(ref, out, grads)
    print(f"g19_loss {tag}: {text}")
    assert use_v <= 1 and use_g <= 1


# ------------------------------------------------------------------------------------------------------------------ LNCC
@pytest.mark.parametrize("shape,cls", ALL_LNCC, ids=[f"{LNCC_IDS[i]}-{c}" for i, c in ALL_LNCC])
def test_float32_oracle_and_restatement_meet_the_lncc_value_criteria(shape, cls):
    ref, src = R.lncc_case(shape, cls)
    for who, got in (("oracle32", K.lncc(ref, src)), ("restatement", R.lncc_f32(ref, src))):
        ok, text = R.lncc_value_ok(R.lncc_value_errors(ref, src, got))
        print(f"{who} {R.LNCC_SHAPES[shape]} {cls}: {text}")
        assert ok, who


def test_lncc_bound_is_not_vacuous_on_ordinary_cases():
    for shape in range(len(R.LNCC_SHAPES)):
        bound = R.lncc_bound(*R.lncc_case(shape, "ordinary"))
        print(f"{R.LNCC_SHAPES[shape]}: bound (a) {float(bound.min()):.1e} .. {float(bound.max()):.1e}")
        assert float(bound.max()) < 5e-3


@pytest.mark.parametrize("defect", R.LNCC_DEFECTS)
def test_each_lncc_defect_is_noticed(defect):
    caught = []
    for shape, cls in ALL_LNCC:
        ref, src = R.lncc_case(shape, cls)
        ok, _ = R.lncc_value_ok(R.lncc_value_errors(ref, src, R.lncc_f32(ref, src, defect=defect)))
        if not ok:
            caught.append(f"{LNCC_IDS[shape]}-{cls}")
    print(f"{defect}: noticed on {len(caught)} of {len(ALL_LNCC)} cases: {caught}")
    ordinary = [c for c in caught if c.endswith("ordinary")]
    assert len(ordinary) >= 1


def test_kept_rays_cap_holds_for_the_float64_reference():
    for shape in range(len(R.LNCC_SHAPES)):
        ref, src = R.lncc_case(shape, "ordinary")
        keep = R.lncc64(ref, src)[3]
        frac = float(keep.double().mean())
        print(f"{R.LNCC_SHAPES[shape]} ordinary: {100 * frac:.1f} % of the rays kept")
        assert frac >= 0.9


@pytest.mark.parametrize("shape", range(len(R.LNCC_SHAPES)), ids=LNCC_IDS)
def test_float32_oracle_gradients_are_a_usable_yardstick(shape):
    """e_oracle32 on the kept rays is small (the device may use four times it), and selecting other views is far outside it."""
    for cls in R.LNCC_GRAD_CLASSES:
        ref, src = R.lncc_case(shape, cls)
        cot = R.lncc_cot(shape)
        g_ref64, g_src64, keep = R.lncc_grads64(ref, src, cot)
        o_ref, o_src = R.lncc_grads_oracle32(ref, src, cot)
        e_ref, e_src = R.grad_error(o_ref, g_ref64, keep), R.grad_error(o_src, g_src64, keep)
        print(f"{R.LNCC_SHAPES[shape]} {cls}: e_oracle32 g_ref {e_ref:.2e}, g_src {e_src:.2e}, kept {int(keep.sum())} of {keep.numel()}")
        assert max(e_ref, e_src) < 1e-4
        if ref.shape[2] > 1:                                   # a gradient taken through the wrong views leaves the yardstick at once
            rolled = torch.roll(g_src64, 1, 0).float()
            assert R.grad_error(rolled, g_src64, keep) > 4 * max(e_src, 2.5e-7)


@pytest.mark.parametrize("kind", R.LNCC_NAN_KINDS)
def test_nan_follows_torch_in_the_reference_and_the_restatement(kind):
    ref, src, ref_clean, src_clean, ray = R.lncc_nan_case(kind)
    want = R.lncc64(ref, src)[0][:, 0]
    got, clean = R.lncc_f32(ref, src)[:, 0], R.lncc_f32(ref_clean, src_clean)[:, 0]
    assert bool(torch.isnan(want[ray])) == (kind != "one-view-of-4") and int(torch.isnan(want).sum()) == int(kind != "one-view-of-4")
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    others = torch.arange(want.numel()) != ray
    assert torch.equal(got[others], clean[others])
    assert torch.equal(torch.isnan(K.lncc(ref, src)[:, 0]), torch.isnan(want))            # float32 torch agrees with float64 torch
    ok, text = R.lncc_value_ok(R.lncc_value_errors(ref, src, got[:, None]))
    assert ok, text


# ------------------------------------------------------------------------------------------------------------------ TV
@pytest.mark.parametrize("name", list(R.TV_CASES))
def test_float32_restatement_meets_the_tv_criteria(name):
    vols, masks = R.tv_case(name)
    ref = R.tv_reference(vols, masks, cot=3.0)
    total, levels, grads = R.tv_f32(vols, masks, cot=3.0)
    use_v, use_g, nan_ok = R.tv_check(ref, total, levels, grads)
    o_total = K.tv_regularization(vols, masks)
    print(f"{name}: restatement value use {use_v:.3f}, gradient use {use_g:.3f}; float32 oracle value use {R.tv_value_use(o_total, ref['total']):.3f}")
    assert use_v <= 1 and use_g <= 1 and nan_ok
    assert R.tv_value_use(o_total, ref["total"]) <= 1
    if name == "l3-empty-middle":
        assert ref["levels"][1] == 0.0 and bool(torch.isnan(ref["grads"][1]).all()) and not bool(torch.isnan(ref["grads"][0]).any())


@pytest.mark.parametrize("defect", R.TV_DEFECTS)
def test_each_tv_defect_is_noticed(defect):
    caught = []
    for name in R.TV_CASES:
        vols, masks = R.tv_case(name)
        ref = R.tv_reference(vols, masks, cot=3.0)
        total, levels, grads = R.tv_f32(vols, masks, cot=3.0, defect=defect)
        use_v, use_g, nan_ok = R.tv_check(ref, total, levels, grads)
        if not (use_v <= 1 and use_g <= 1 and nan_ok):
            caught.append(name)
    print(f"{defect}: noticed on {len(caught)} of {len(R.TV_CASES)} cases: {caught}")
    assert caught
    if defect == "xy_swap":                                    # invisible on a level with X = Y, which is why the shapes are not cubes
        vols, masks = R.tv_case("v-4x4x8-cube-rand")
        clean, swapped = R.tv_f32(vols, masks, cot=3.0), R.tv_f32(vols, masks, cot=3.0, defect=defect)
        assert clean[:2] == swapped[:2] and torch.equal(clean[2][0], swapped[2][0]) and "v-4x4x8-cube-rand" not in caught
        assert any(c.startswith("v-") for c in caught) and any(c.startswith("s-") for c in caught)


# ------------------------------------------------------------------------------------------------------------------ fused loss
@pytest.mark.parametrize("name", list(R.LOSS_CASES))
def test_float32_restatement_meets_the_loss_criteria(name):
    case = R.loss_case(name)
    ref = R.loss_reference(case)
    out, grads = R.loss_f32(case)
    use_v, use_g, text = R.loss_check(ref, out, grads)
    print(f"{name}: {text}")
    assert use_v <= 1 and use_g <= 1


@pytest.mark.parametrize("defect", R.LOSS_DEFECTS)
def test_each_loss_defect_is_noticed(defect):
    caught = []
    for name in R.LOSS_CASES:
        case = R.loss_case(name)
        use_v, use_g, _ = R.loss_check(R.loss_reference(case), *R.loss_f32(case, defect=defect))
        if not (use_v <= 1 and use_g <= 1):
            caught.append(name)
    print(f"{defect}: noticed on {len(caught)} of {len(R.LOSS_CASES)} cases: {caught}")
    assert caught


def test_loss_cases_cover_the_listed_sizes_and_edges():
    specs = R.LOSS_CASES.values()
    assert {s["b"] for s in specs} == {1, 63, 65, 1023, 1024, 1025, 2500}
    assert {s["ns"] for s in specs} == {1, 1025, 16000} and {s["npz"] for s in specs} == {None, 1, 300, 3000}
    assert any((s["b"], s["ns"], s["npz"]) == (1, 1, 3000) for s in specs)
    big = R.loss_case("b2500-s1025-p3000-all")
    assert not big["preds"]["color_fine"].is_contiguous() and big["preds"]["valid_mask"].dtype == torch.bool
    assert big["preds"]["valid_mask"].shape == (2500, 1)
    p, t = big["preds"], big["targets"]
    assert bool((p["color_fine"] == t["color"]).any()) and bool((p["sparse_sdf"] == 0).any()) and bool((p["pseudo_sdf"] == 0).any())
    assert bool((t["pseudo_depth"] == 0).any()) and bool((t["pseudo_depth"] < 0).any()) and bool((p["render_depth"] == t["pseudo_depth"]).any())
    assert float(p["sparse_sdf"].abs().max()) * R.SPARSE_SCALE > 104                       # below exp's float32 range
    assert not bool(R.loss_case("b2500-s1-p1-invalid")["preds"]["valid_mask"].any())
    assert not bool((R.loss_case("b1025-s1025-p1-gated")["targets"]["depth"] > 0).any())
