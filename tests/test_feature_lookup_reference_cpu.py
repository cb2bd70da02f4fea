"""tests/feature_lookup_reference.py pinned on the CPU: the recorded g4_feature results, the float32 oracle with its autograd and the clean float32
restatement lie inside the float64 bound on every shape and class, every seeded defect leaves it (or flips a decided mask) on the class that is
named for it here, the cap on ambiguous items holds, `exact` is bit-equal between float32 and float64, and the bound is not vacuous.
Run with -s for the figures."""
import numpy as np
import pytest
import torch

from oracle import gens_oracle as K
from tests import feature_lookup_reference as R

IDS = [R.case_id(s, c) for s, c in R.ALL_CASES]
BWD_CASES = [(s, c) for s, c in R.ALL_CASES if c in ("inside", "border", "crowd", "exact")]
# the class that must notice each defect (on at least one shape); closed_pixel_test needs a coordinate exactly ON w or h and no_eps_in_norm a
# point exactly AT a camera centre: only `exact` has them
CAUGHT_BY = dict(align_corners="inside", level_size="inside", view_off_by_one="inside", closed_pixel_test="exact", border_clamp="border",
                 pair_mixup="inside", rgb_from_level1="inside", no_eps_in_norm="exact", taps_swapped="inside", bwd_level_scale="inside")


def _oracle_w2c(c2ws):
    w2c = torch.eye(4)[None].repeat(c2ws.shape[0], 1, 1)
    w2c[1:] = torch.inverse(c2ws[1:])                      # the inverse the float32 oracle and the reference project hold
    return w2c


def _args(case):
    return case["pts"], case["w2c"], case["intrs"], case["c2ws"], case["imgs"], case["feats"]


def test_recorded_feature_lookup_lies_inside_the_bound(golden):
    g = golden("g4_feature")
    feats = [g[f"feat{i}"] for i in range(5)]
    ref = R.reference(g["pts"], _oracle_w2c(g["c2ws"]), g["intrs"], g["c2ws"], g["imgs"], feats)
    res = R.check_forward(ref, g["feat_views"], g["ray_diff"], g["mask"], g["pts"])
    want, bounds = R.grads_reference(ref, [f.shape[2:] for f in feats], g["cot"])
    use_g = R.check_grads(want, bounds, [g[f"gfeat{i}"] for i in range(5)] + [g["gimgs"]])
    print(f"g4_feature: {res}, gradients use {use_g:.3f}")
    assert R.forward_ok(res) and use_g <= 1
    assert res["n_amb"] <= R.AMBIGUOUS_CAP * res["n_items"]
    assert all(bool(np.isfinite(b).all()) for b in bounds) and float(ref["mask_true"].mean()) > 0.2


@pytest.mark.parametrize("shape,cls", R.ALL_CASES, ids=IDS)
def test_float32_oracle_and_its_autograd_lie_inside_the_bound(shape, cls):
    case, _ = R.shape_case(shape, cls)
    ref = R.case_reference(case, _oracle_w2c(case["c2ws"]))
    feats = [f.clone().requires_grad_(True) for f in case["feats"]]
    imgs = case["imgs"].clone().requires_grad_(True)
    fv, rd, mk = K.lookup_feature(case["pts"], imgs, case["intrs"], case["c2ws"], feats)
    res = R.check_forward(ref, fv, rd, mk, case["pts"])
    want, bounds = R.grads_reference(ref, case["levels"], case["cot"])
    use_g = R.check_grads(want, bounds, torch.autograd.grad((fv * case["cot"]).sum(), feats + [imgs]))
    print(f"oracle {R.case_id(shape, cls)}: values {res['use_fv']:.3f}, ray_diff {res['use_rd']:.3f}, gradients {use_g:.3f}")
    assert R.forward_ok(res) and use_g <= 1


@pytest.mark.parametrize("shape,cls", R.ALL_CASES, ids=IDS)
def test_float32_restatement_lies_inside_the_bound(shape, cls):
    case, ref = R.shape_case(shape, cls)
    res = R.check_forward(ref, *R.lookup_f32(*_args(case)), case["pts"])
    want, bounds = R.shape_grads(shape, cls)
    use_g = R.check_grads(want, bounds, R.lookup_bwd_f32(case["pts"], case["w2c"], case["intrs"], case["levels"], case["cot"]))
    print(f"lookup_f32 {R.case_id(shape, cls)}: values {res['use_fv']:.3f}, ray_diff {res['use_rd']:.3f}, gradients {use_g:.3f}, "
          f"ambiguous {res['n_amb']} of {res['n_items']}, free masks {res['n_free_masks']}")
    assert R.forward_ok(res) and use_g <= 1


@pytest.mark.parametrize("shape,cls", R.ALL_CASES, ids=IDS)
def test_ambiguity_cap_holds_and_the_case_is_what_its_class_says(shape, cls):
    case, ref = R.shape_case(shape, cls)
    n_amb, n_items = R.ambiguous_share(ref)
    print(f"{R.case_id(shape, cls)}: {n_amb} of {n_items} items ambiguous, {int(ref['rd_amb'].sum())} ray differences")
    assert n_amb <= R.AMBIGUOUS_CAP * n_items and int(ref["rd_amb"].sum()) <= R.AMBIGUOUS_CAP * ref["rd_amb"].size
    assert max(w for _, w in case["levels"]) <= 65
    bad = ~np.isfinite(case["pts"].numpy()).all(-1)
    assert bool(ref["dead"][:, bad].all()) and not bool(np.isfinite(ref["px"][0][:, bad]).any())
    n = case["pts"].shape[0]
    target = (np.arange(n) % (case["c2ws"].shape[0] - 1), np.arange(n))                    # the view a point was aimed at
    if cls == "exact":
        assert n_amb == 0 and int(ref["rd_amb"].sum()) == 0
        assert all(not bool(e[~ref["dead"]].any()) for e in ref["e_ix"] + ref["e_iy"]) and not bool(ref["e_d"].any())       # nothing rounds
        px, py, d = ref["px"][0][0], ref["py"][0][0], ref["d"][0]
        for v in R.EXACT_PX:
            assert bool((px == v).any()), v
        for v in R.EXACT_PY:
            assert bool((py == v).any()), v
        for v in R.EXACT_D:
            assert bool((d == v).any()), v
        assert bool(np.isnan(px[-1])) and bool((ref["ray_diff"][:, 1, :3] == 0).all())     # AT view 1's centre; view 2 is the reference view
        assert 0 < int(ref["mask_true"].sum()) < ref["mask_true"].size and not bool((~ref["mask_true"] & ~ref["mask_false"]).any())
    elif cls == "behind":
        d = ref["d"][target]
        assert bool((d < 0).all()) and (n < 50 or float(np.abs(d).min()) < 3e-3)
    elif cls == "border":                                   # zero-padded taps: read positions within a texel of the image's edge
        ix, iy = ref["ix"][0][target], ref["iy"][0][target]
        h, w = case["levels"][0]
        edge = (ix < 0) | (ix > w - 1) | (iy < 0) | (iy > h - 1)
        assert float(edge.mean()) > 0.3 or n < 50
    elif cls == "crowd":
        assert len({(int(a), int(b)) for a, b in zip(np.floor(ref["px"][0][0]), np.floor(ref["py"][0][0]))}) == 1
    elif cls == "nonfinite":
        assert bool(bad.any()) and (n < 5 or int(bad.sum()) == 4)


def test_exact_is_bit_equal_between_float32_and_float64():
    case, ref = R.shape_case(None, "exact")
    fv, rd, mk = R.lookup_f32(*_args(case))
    assert np.array_equal(fv.numpy().astype(np.float64), ref["fv"]) and np.array_equal(mk.numpy(), ref["mask_true"])
    o_fv, _, o_mk = K.lookup_feature(case["pts"], case["imgs"], case["intrs"], case["c2ws"], case["feats"])
    assert torch.equal(torch.nan_to_num(o_fv), fv) and torch.equal(o_mk, mk)
    want, _ = R.shape_grads(None, "exact")
    for g32, g64 in zip(R.lookup_bwd_f32(case["pts"], case["w2c"], case["intrs"], case["levels"], case["cot"]), want):
        assert np.array_equal(g32.numpy().astype(np.float64), g64)
    inv = torch.eye(4)[None].repeat(3, 1, 1)
    inv[:, :3, 3] = -case["c2ws"][:, :3, 3]
    assert bool((case["w2c"] == inv).all()) and bool((_oracle_w2c(case["c2ws"])[1:] == inv[1:]).all())       # (== : a -0.0 is a 0.0)


@pytest.mark.parametrize("defect", R.DEFECTS + R.BWD_DEFECTS)
def test_each_defect_is_noticed_by_its_class(defect):
    caught = []
    for shape, cls in R.ALL_CASES:
        case, ref = R.shape_case(shape, cls)
        if defect in R.BWD_DEFECTS:
            if (shape, cls) not in BWD_CASES:
                continue
            want, bounds = R.shape_grads(shape, cls)
            got = R.lookup_bwd_f32(case["pts"], case["w2c"], case["intrs"], case["levels"], case["cot"], defect=defect)
            ok = R.check_grads(want, bounds, got) <= 1
        else:
            ok = R.forward_ok(R.check_forward(ref, *R.lookup_f32(*_args(case), defect=defect), case["pts"]))
        if not ok:
            caught.append(R.case_id(shape, cls))
    print(f"{defect}: noticed on {len(caught)} cases: {caught}")
    assert any(c.endswith(CAUGHT_BY[defect]) for c in caught)
    if defect == "closed_pixel_test":                      # (no_eps_in_norm: the 5e-7 it moves a unit vector by is 8 u, outside the bound anywhere)
        assert caught == ["exact"]


def test_the_bound_is_not_vacuous():
    for shape in range(len(R.SHAPES)):
        case, ref = R.shape_case(shape, "inside")
        bound = ref["fv_bound"][..., 3:]
        top = max(float(f.abs().max()) for f in case["feats"])
        med = float(np.median(bound))
        print(f"{R.SHAPE_IDS[shape]}: median value bound {med:.2e}, largest texel {top:.2f}")
        assert bool(np.isfinite(bound).all()) and med < 0.01 * top
