"""The source-view feature look-up (K4: gens_lookup_feature_fwd / _bwd / _bwd_idx, k4_feature.hip with k4_common.h and the tap code of common.h)
against the float64 reference and bound of tests/feature_lookup_reference.py (pinned on the CPU by test_feature_lookup_reference_cpu.py), at
the shapes where its forms and edges lie.  The reference gets the kernel's own w2c (SceneViews.w2c copied back) and intrinsics.

    shape (R.SHAPES)                        items    what it exercises
    2 views, one 2 x 2 level, 1 point           1    one item, whose pair partner is idle; S = 1: no multiply-high division
    3 views, 2 levels from 5 x 7, 85          170    the generic level loop with 2 levels
    4 views, 3 levels from 9 x 12, 85         255    one short of a block, an odd count, the unrolled 3-level form
    4 views, 3 levels from 9 x 12, 86         258    a second block of two rows: a span of 30 floats, so the float4 copy has a scalar tail
    5 views, 5 levels from 48 x 64, 1 622   6 488    25 blocks + 88 rows: GENS_K4_XCD_REMAP remaps 24 blocks and leaves 2; the unrolled 5-level form
    16 views, 4 levels from 30 x 41, 33       495    S = 15 (GENS_MAX_VIEWS), the generic level loop
    11 views, 5 levels from 24 x 32, 300    3 000    the fine-tuning view count, a pyramid that ends at 2 x 2
    9 views, 8 levels, 300                  2 400    GENS_MAX_LEVELS, maps that are not halvings of each other ((2, 2), (2, 3), (3, 2) last)
    `exact`: 3 views, 5 levels from 33 x 65   452    nothing rounds: kernel, oracle and reference agree bit for bit, ON every boundary

Classes: inside, border (zero-padded taps), behind (d < 0, |d| down to 1e-3), crowd (one texel), nonfinite (NaN / inf points), exact.
Run with -s for the worst share of the bound used per case."""
import numpy as np
import pytest
import torch

from oracle import gens_oracle as K
from tests import feature_lookup_reference as R

pytestmark = pytest.mark.gpu

IDS = [R.case_id(s, c) for s, c in R.ALL_CASES]
ITEMS_255, ITEMS_6488, S15 = 2, 4, 5
BWD_CASES = [(s, c) for s in (ITEMS_255, ITEMS_6488, S15) for c in ("inside", "border", "crowd")]
BWD_IDS = [R.case_id(s, c) for s, c in BWD_CASES]
SWITCHES = ("GENS_K4_NO_PAIRS", "GENS_K4_NO_UNROLL", "GENS_K4_PLAIN_COPY", "GENS_K4_XCD_REMAP")


@pytest.fixture(scope="module")
def ops():
    from gens_amd import ops
    return ops


def dev(t):
    if isinstance(t, (list, tuple)):
        return [dev(x) for x in t]
    return t.cuda()


def _views(ops, case, grad=()):
    """-> (views, feats, imgs): fresh device copies; grad: which of "feats" / "imgs" require a gradient."""
    feats = [dev(f).requires_grad_("feats" in grad) for f in case["feats"]]
    imgs = dev(case["imgs"]).requires_grad_("imgs" in grad)
    views = ops.SceneViews(imgs, dev(case["intrs"]), dev(case["c2ws"]), feats)
    assert torch.equal(views.intr.cpu(), case["intrs"]) and torch.equal(views.c2w.cpu(), case["c2ws"])
    return views, feats, imgs


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _grads(ops, case, cot, grad=("feats", "imgs"), pts=None):
    """-> (gradients [levels..., images] of those asked for, fv, views)."""
    views, feats, imgs = _views(ops, case, grad)
    fv, _, _ = ops.lookup_feature(dev(case["pts"] if pts is None else pts), views)
    inputs = (feats if "feats" in grad else []) + ([imgs] if "imgs" in grad else [])
    return [g.cpu() for g in torch.autograd.grad((fv * dev(cot)).sum(), inputs)], fv.detach().cpu(), views


def _reference(shape, cls, views):
    return R.reference_for(shape, cls, views.w2c)


def _grads_reference(shape, cls, ref, cot=None):
    case, own = R.shape_case(shape, cls)
    if ref is own and cot is None:
        return R.shape_grads(shape, cls)
    return R.grads_reference(ref, case["levels"], case["cot"] if cot is None else cot)


# ------------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("shape,cls", R.ALL_CASES, ids=IDS)
def test_forward_lies_inside_the_float64_bound(ops, shape, cls):
    case, _ = R.shape_case(shape, cls)
    views, _, _ = _views(ops, case)
    case, ref = _reference(shape, cls, views)
    fv, rd, mk = (t.cpu() for t in ops.lookup_feature(dev(case["pts"]), views))
    n, s = case["pts"].shape[0], case["c2ws"].shape[0] - 1
    assert fv.shape == (n, s, 3 + 4 * len(case["levels"])) and rd.shape == (n, s, 4) and mk.shape == (n, s) and mk.dtype == torch.bool
    res = R.check_forward(ref, fv, rd, mk, case["pts"])
    print(f"{R.case_id(shape, cls)}: values {res['use_fv']:.3f}, ray_diff {res['use_rd']:.3f} of the bound; {res['n_amb']} of {res['n_items']} "
          f"items ambiguous, {res['n_free_masks']} masks free")
    assert res["mask_bad"] == 0, f"{res['mask_bad']} decided masks differ"
    assert res["use_fv"] <= 1, f"values use {res['use_fv']:.3g} of the bound"
    assert res["use_rd"] <= 1, f"ray_diff uses {res['use_rd']:.3g} of the bound"
    assert res["n_amb"] <= R.AMBIGUOUS_CAP * res["n_items"]
    if cls == "exact":
        inv = torch.eye(4)[None].repeat(3, 1, 1)
        inv[:, :3, 3] = -case["c2ws"][:, :3, 3]
        assert bool((views.w2c.cpu() == inv).all())                                            # the exact inverse
        assert res["n_amb"] == 0 and res["n_free_masks"] == 0
        assert np.array_equal(torch.nan_to_num(fv).numpy().astype(np.float64), ref["fv"]) and np.array_equal(mk.numpy(), ref["mask_true"])
        o_fv, _, o_mk = K.lookup_feature(case["pts"], case["imgs"], case["intrs"], case["c2ws"], case["feats"])
        assert torch.equal(_bits(torch.nan_to_num(fv) + 0.0), _bits(torch.nan_to_num(o_fv) + 0.0)) and torch.equal(mk, o_mk)


@pytest.mark.parametrize("switch", SWITCHES)
@pytest.mark.parametrize("shape", [ITEMS_255, ITEMS_6488], ids=[R.SHAPE_IDS[ITEMS_255], R.SHAPE_IDS[ITEMS_6488]])
def test_forward_switches_leave_every_bit(ops, shape, switch, monkeypatch):
    """The lane-per-item read, the generic level loop, the element-wise copy and the contiguous block order give the default run's bits."""
    for cls in ("inside", "border", "nonfinite"):
        case, _ = R.shape_case(shape, cls)
        views, _, _ = _views(ops, case)
        pts = dev(case["pts"])
        monkeypatch.delenv(switch, raising=False)
        default = ops.lookup_feature(pts, views)
        monkeypatch.setenv(switch, "1")
        switched = ops.lookup_feature(pts, views)
        for a, b in zip(default, switched):
            assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), (switch, cls)
        assert 0 < int(default[2].sum()) < default[2].numel()


# ------------------------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("shape,cls", BWD_CASES + [(None, "exact")], ids=BWD_IDS + ["exact"])
def test_backward_lies_inside_the_per_texel_bound(ops, shape, cls):
    """Joint, images-only and features-only gradients; on `exact` the sums are exact, so all of them are the reference's bits."""
    case, _ = R.shape_case(shape, cls)
    joint, _, views = _grads(ops, case, case["cot"])
    case, ref = _reference(shape, cls, views)
    want, bounds = _grads_reference(shape, cls, ref)
    nl = len(case["levels"])
    only_feats, _, _ = _grads(ops, case, case["cot"], ("feats",))
    only_imgs, _, _ = _grads(ops, case, case["cot"], ("imgs",))
    use = [R.check_grads(want, bounds, joint), R.check_grads(want[:nl], bounds[:nl], only_feats), R.check_grads(want[nl:], bounds[nl:], only_imgs)]
    print(f"{R.case_id(shape, cls)}: gradients use {use[0]:.3f} (joint), {use[1]:.3f} (features only), {use[2]:.3f} (images only) of the bound")
    assert max(use) <= 1, use
    assert all(bool((g[0] == 0).all()) for g in joint)                                         # nothing for the reference view
    if cls == "exact":
        for g, w in zip(joint, want):
            assert np.array_equal(g.numpy().astype(np.float64), w)
        for a, b in zip(joint, only_feats + only_imgs):
            assert torch.equal(_bits(a + 0.0), _bits(b + 0.0))


@pytest.mark.parametrize("shape,cls", BWD_CASES, ids=BWD_IDS)
def test_backward_zero_cotangent_rows_add_nothing(ops, shape, cls):
    """Rows of exact zeros and of -0.0: the result is the reference of the remaining rows, and a texel that only such rows reach keeps the
    +0.0 it was allocated with."""
    case, _ = R.shape_case(shape, cls)
    cot = case["cot"].clone()
    cot[::2] = 0.0
    cot[1::4] = -0.0
    got, _, views = _grads(ops, case, cot)
    case, ref = _reference(shape, cls, views)
    want, bounds = R.grads_reference(ref, case["levels"], cot)
    assert R.check_grads(want, bounds, got) <= 1
    for g, b in zip(got, bounds):
        assert not bool(_bits(g)[torch.from_numpy(b == 0)].any())                              # +0.0, bit for bit


@pytest.mark.parametrize("shape,cls", BWD_CASES, ids=BWD_IDS)
def test_backward_nan_cotangent_stays_in_its_item_channel_and_level(ops, shape, cls):
    """One NaN in a level-1 feature column and one in a colour column: exactly the in-image taps of those items, channels and levels."""
    case, ref = R.shape_case(shape, cls)
    nl = len(case["levels"])
    cot = case["cot"].clone()
    expect = [np.zeros((case["c2ws"].shape[0], c, h, w), bool) for c, (h, w) in zip([4] * nl + [3], case["levels"] + (case["levels"][0],))]
    for lvl, ch, into in ((1, 2, 1), (0, 1, nl)):
        h, w = case["levels"][lvl]
        ix, iy = ref["ix"][lvl], ref["iy"][lvl]
        # an item whose four taps are in the image and decided: the read position at least 0.2 from a texel centre (e_ix is ~1e-5)
        good = (ix > 0.2) & (ix < w - 1.2) & (iy > 0.2) & (iy < h - 1.2) & (np.abs(ix - np.rint(ix)) > 0.2) & (np.abs(iy - np.rint(iy)) > 0.2)
        good &= (ref["e_ix"][lvl] < 0.01) & (ref["e_iy"][lvl] < 0.01)
        s, i = (int(a[0]) for a in np.nonzero(good))
        cot[i, s, (3 + 4 * lvl + ch) if into < nl else ch] = float("nan")
        y0, x0 = int(np.floor(iy[s, i])), int(np.floor(ix[s, i]))
        expect[into][s + 1, ch, y0:y0 + 2, x0:x0 + 2] = True
    got, _, _ = _grads(ops, case, cot)
    for g, e in zip(got, expect):
        assert np.array_equal(torch.isnan(g).numpy(), e) and int(e.sum()) in (0, 4)


@pytest.mark.parametrize("which", ["dense", "one-level", "one-view", "colour"])
@pytest.mark.parametrize("shape,cls", BWD_CASES, ids=BWD_IDS)
def test_backward_is_the_adjoint_of_the_kernels_own_forward(ops, shape, cls, which):
    """sum(fv * cot) = sum over maps of sum(map * grad), in float64 from the kernel's own outputs.  Both sides round the same exact sum of
    terms w * texel * cot when forward and backward project alike (project_src_base / project_src_level against project_src), so they differ
    by at most u sum over texels of (k + 12) sum|terms of the texel| (R.adjoint_tolerance): no projection error enters, which ties the two
    far tighter than the bound."""
    case, _ = R.shape_case(shape, cls)
    cot = case["cot"].clone()
    nl = len(case["levels"])
    if which == "one-level":
        keep = torch.zeros_like(cot)
        keep[..., 3 + 4 * (nl - 2):7 + 4 * (nl - 2)] = 1
        cot = cot * keep
    elif which == "one-view":
        cot[:, :-1] = 0.0
    elif which == "colour":
        cot[..., 3:] = 0.0
    got, fv, views = _grads(ops, case, cot)
    case, ref = _reference(shape, cls, views)
    lhs = float((fv.double() * cot.double()).sum())
    rhs = sum(float((m.double() * g.double()).sum()) for m, g in zip(case["feats"] + [case["imgs"]], got))
    tol, total = R.adjoint_tolerance(ref, case, cot)
    print(f"{R.case_id(shape, cls)} {which}: |lhs - rhs| = {abs(lhs - rhs):.3e}, {abs(lhs - rhs) / tol:.3f} of the rounding allowance {tol:.3e}; "
          f"sum|terms| = {total:.3e}")
    assert total > 0 and abs(lhs - rhs) <= tol


# ------------------------------------------------------------------------------------------------------------------ indexed backward
def _bwd_idx(views, case, pts, g_out, index, n, count, fill, want_feats=True, want_imgs=True):
    """gens_lookup_feature_bwd_idx as ops/blend.py calls it, into buffers prefilled with `fill`.  -> [levels..., images] (nv, C, h, w) on the
    CPU (texel layout undone; the images' padding channel must still hold `fill`)."""
    from gens_amd import lib as L
    hw = [d for lv in case["levels"] for d in lv]
    nv = case["c2ws"].shape[0]
    g_feats = [torch.full((nv, h, w, 4), fill, device="cuda") for h, w in case["levels"]] if want_feats else None
    g_imgs = torch.full((nv,) + tuple(case["levels"][0]) + (4,), fill, device="cuda") if want_imgs else None
    cnt = None if count is None else torch.tensor([count], device="cuda", dtype=torch.int32)
    L.call("gens_lookup_feature_bwd_idx", L.int_table(hw), len(case["levels"]), L.ptr(views.w2c), L.ptr(views.intr), nv, L.ptr(pts), L.ptr(g_out),
           L.ptr(index, torch.int64), n, L.ptr(cnt, torch.int32), L.ptr_table(g_feats), L.ptr(g_imgs), L.stream())
    torch.cuda.synchronize()
    out = [g.permute(0, 3, 1, 2).cpu() for g in (g_feats or [])]
    if want_imgs:
        assert bool((g_imgs[..., 3] == fill).all())
        out.append(g_imgs[..., :3].permute(0, 3, 1, 2).cpu())
    return out


def _index(case, seed):
    """A permuted selection of two thirds of the points (at least one), its second entry a repeat of the first."""
    n = case["pts"].shape[0]
    index = torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:max(1, 2 * n // 3)]
    if index.numel() > 1:
        index[1] = index[0]
    return index


@pytest.mark.parametrize("shape,cls", [(ITEMS_255, "inside"), (ITEMS_6488, "border"), (None, "exact")],
                         ids=[R.case_id(ITEMS_255, "inside"), R.case_id(ITEMS_6488, "border"), "exact"])
def test_indexed_backward_adds_the_gathered_rows(ops, shape, cls):
    """Compact g_out, a permuted index with a repeated point, a device count below, at and above n (only min(n, count) rows exist), buffers
    prefilled with 0.5: the reference of the gathered rows plus 0.5, inside the same bound; on `exact` the plain backward's bits."""
    case, _ = R.shape_case(shape, cls)
    views, _, _ = _views(ops, case)
    index = _index(case, 5)
    m = index.numel()
    pts, cot = dev(case["pts"]), dev(case["cot"][:m].contiguous())
    for count in (max(m - 3, 1), m, m + 5, None):
        rows = m if count is None else min(m, count)
        got = _bwd_idx(views, case, pts, cot, dev(index), m, count, 0.5)
        gathered = case["pts"][index[:rows]]
        ref = R.reference(gathered, views.w2c.cpu(), case["intrs"], case["c2ws"], case["imgs"], case["feats"])
        want, bounds = R.grads_reference(ref, case["levels"], case["cot"][:rows], base=0.5)
        use = R.check_grads(want, bounds, got)
        print(f"{R.case_id(shape, cls)} count {count} of n {m}: gradients use {use:.3f} of the bound")
        assert use <= 1
        if cls == "exact":
            plain, _, _ = _grads(ops, case, case["cot"][:rows], pts=gathered)
            for a, b in zip(got, plain):
                assert torch.equal(a - 0.5, b)
    only_imgs = _bwd_idx(views, case, pts, cot, dev(index), m, None, 0.5, want_feats=False)
    assert len(only_imgs) == 1 and R.check_grads(want[-1:], bounds[-1:], only_imgs) <= 1


@pytest.mark.parametrize("shape,cls", [(ITEMS_255, "inside")], ids=[R.case_id(ITEMS_255, "inside")])
def test_indexed_backward_without_rows_leaves_the_buffers(ops, shape, cls):
    case, _ = R.shape_case(shape, cls)
    views, _, _ = _views(ops, case)
    index = _index(case, 6)
    m = index.numel()
    pts, cot = dev(case["pts"]), dev(case["cot"][:m].contiguous())
    for n, count in ((m, 0), (0, 7), (0, None)):
        for g in _bwd_idx(views, case, pts, cot, dev(index), n, count, 0.25):
            assert bool((g == 0.25).all())
