"""The loss kernels on the device against the float64 references of tests/loss_reference.py (pinned on the CPU by test_loss_reference_cpu.py),
through the public wrappers, at the smallest shapes where they can go wrong:

    compute_LNCC        S*C = 64 (a full wavefront), C that does not divide 64, P = 9 and 1, 257 / 1 rays (idle waves), five data classes;
                        value criteria (a) and (b), gradients on the kept rays against four times the float32 oracle's own error; NaN as torch.
    tv_regularization   the all-levels launch, the four-voxel per-level form and the scalar form (Z % 4 != 0, GENS_TV_SCALAR, storage offset by
                        one float), each against float64 on non-cubic levels; an empty level's zero value and NaN gradient.
    _FusedLoss          b below, at and above the 1024-ray stride of loss_fwd_k, every one of b, n_sparse and n_pseudo as the backward's
                        grid size, absent targets, all-invalid batches, exact zeros in every sign(), expf underflow.

The criteria and their derivations are in the docstring of tests/loss_reference.py.  Run with -s for the tolerance use per case."""
import pytest
import torch

from tests import loss_reference as R

pytestmark = pytest.mark.gpu

LNCC_IDS = ["x".join(map(str, s)) for s in R.LNCC_SHAPES]
ALL_LNCC = [(i, c) for i in range(len(R.LNCC_SHAPES)) for c in R.LNCC_CLASSES]


@pytest.fixture(scope="module")
def ops():
    from gens_amd import ops
    return ops


# ------------------------------------------------------------------------------------------------------------------ LNCC
@pytest.mark.parametrize("shape,cls", ALL_LNCC, ids=[f"{LNCC_IDS[i]}-{c}" for i, c in ALL_LNCC])
def test_lncc_value_and_gradients_against_float64(shape, cls):
    from gens_amd.losses import compute_LNCC
    ref, src = R.lncc_case(shape, cls)
    ref_d, src_d = ref.cuda().requires_grad_(True), src.cuda().requires_grad_(True)
    out = compute_LNCC(ref_d, src_d)
    assert out.shape == (ref.shape[1], 1)
    ok, text = R.lncc_value_ok(R.lncc_value_errors(ref, src, out))
    print(f"lncc {R.LNCC_SHAPES[shape]} {cls}: {text}")
    assert ok, text
    if cls not in R.LNCC_GRAD_CLASSES and cls != "twin":
        return
    cot = R.lncc_cot(shape)
    g_ref, g_src = torch.autograd.grad((out * cot.cuda()).sum(), [ref_d, src_d])
    g_ref64, g_src64, keep = R.lncc_grads64(ref, src, cot, twins=cls == "twin")
    o_ref, o_src = R.lncc_grads_oracle32(ref, src, cot)
    if cls == "twin":                                          # which twin is selected is free; the sum of their gradients is not
        pairs = [("g_src[0] + g_src[1]", g_src.cpu()[:2].sum(0, keepdim=True), o_src[:2].sum(0, keepdim=True), g_src64[:2].sum(0, keepdim=True))]
    else:
        pairs = [("g_ref", g_ref, o_ref, g_ref64), ("g_src", g_src, o_src, g_src64)]
    for name, got, o32, want in pairs:
        e, e32 = R.grad_error(got, want, keep), R.grad_error(o32, want, keep)
        print(f"lncc {R.LNCC_SHAPES[shape]} {cls} {name}: device {e:.2e}, float32 oracle {e32:.2e}, limit {max(4 * e32, 1e-6):.2e}, "
              f"{int(keep.sum())} of {keep.numel()} rays kept")
        assert e <= max(4 * e32, 1e-6), name


def test_lncc_refuses_more_than_a_wavefront_and_a_single_view():
    from gens_amd.losses import compute_LNCC
    with pytest.raises(RuntimeError):                          # S*C = 65
        compute_LNCC(torch.rand(1, 1, 121, 13).cuda(), torch.rand(5, 1, 121, 13).cuda())
    with pytest.raises(RuntimeError):                          # S = 1: torch.topk(., 2) of the reference fails too
        compute_LNCC(torch.rand(1, 2, 121, 12).cuda(), torch.rand(1, 2, 121, 12).cuda())


@pytest.mark.parametrize("kind", R.LNCC_NAN_KINDS)
def test_lncc_propagates_nan_as_torch_does(kind):
    """A NaN in a patch must not read as a perfect score: the ray is NaN exactly where the float64 reference is (torch.clamp keeps NaN,
    torch.topk ranks it last), and no other ray changes by a bit."""
    from gens_amd.losses import compute_LNCC
    ref, src, ref_clean, src_clean, ray = R.lncc_nan_case(kind)
    got = compute_LNCC(ref.cuda(), src.cuda()).cpu()[:, 0]
    clean = compute_LNCC(ref_clean.cuda(), src_clean.cuda()).cpu()[:, 0]
    want = R.lncc64(ref, src)[0][:, 0]
    print(f"lncc NaN {kind}: device {got.tolist()}, float64 {[round(x, 6) for x in want.tolist()]}")
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    others = torch.arange(want.numel()) != ray
    assert torch.equal(got[others], clean[others])
    if not bool(torch.isnan(want[ray])):                       # one NaN view of four: the two smallest of the other three
        ok, text = R.lncc_value_ok(R.lncc_value_errors(ref, src, got[:, None]))
        assert ok, text


# ------------------------------------------------------------------------------------------------------------------ TV
def _tv_run(fn, vols, masks, cot):
    vs = [v.requires_grad_(True) for v in vols]
    out = fn(vs, masks)
    total, levels = out if isinstance(out, tuple) else (out, None)
    grads = torch.autograd.grad(total * cot, vs)
    return float(total.detach()), levels, grads


def _per_level(ops):
    def fn(vs, masks):
        levels = [ops._TVLevel.apply(v, m) for v, m in zip(vs, masks)]
        total = 0
        for lvl, t in enumerate(levels):
            total = total + t * 0.5 ** lvl
        return total, [float(t) for t in levels]
    return fn


def _offset_by_one_float(t):
    """The same values in contiguous storage that starts one float past a 16-byte boundary: the four-voxel forms must decline it."""
    flat = torch.empty(t.numel() + 1, device="cuda")
    flat[1:] = t.reshape(-1).cuda()
    view = flat[1:].view(t.shape)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view.detach()


def _tv_assert(name, form, ref, result):
    total, levels, grads = result
    use_v, use_g, nan_ok = R.tv_check(ref, total, levels, grads)
    print(f"tv {name} {form}: value use {use_v:.3f}, gradient use {use_g:.3f}")
    assert use_v <= 1 and use_g <= 1 and nan_ok, (name, form, use_v, use_g, nan_ok)


@pytest.mark.parametrize("name", list(R.TV_CASES))
def test_tv_forms_against_float64(ops, name, monkeypatch):
    vols, masks = R.tv_case(name)
    levels = R.TV_CASES[name][0]
    cot = 3.0
    ref = R.tv_reference(vols, masks, cot=cot)
    dev = lambda ts: [t.cuda() for t in ts]  # noqa: E731
    vec = R.tv_vectorisable(levels)
    assert ops.tv_levels_ok(dev(vols), dev(masks)) == vec
    _tv_assert(name, "all-levels launch" if vec else "tv_regularization (per level)", ref, _tv_run(ops.tv_regularization, dev(vols), dev(masks), cot))
    _tv_assert(name, "four-voxel per level" if vec else "scalar per level", ref, _tv_run(_per_level(ops), dev(vols), dev(masks), cot))
    if vec:
        _tv_assert(name, "scalar, storage offset by one float", ref,
                   _tv_run(_per_level(ops), [_offset_by_one_float(v) for v in vols], [_offset_by_one_float(m) for m in masks], cot))
        monkeypatch.setenv("GENS_TV_SCALAR", "1")
        _tv_assert(name, "scalar, GENS_TV_SCALAR", ref, _tv_run(_per_level(ops), dev(vols), dev(masks), cot))
    if name == "l3-empty-middle":
        assert ref["levels"][1] == 0.0 and bool(torch.isnan(ref["grads"][1]).all())


# ------------------------------------------------------------------------------------------------------------------ fused loss
def _fused(case):
    from gens_amd.losses.loss import _FusedLoss
    p, t = case["preds"], case["targets"]
    d = {k: v.cuda() for k, v in p.items()}
    if not p["color_fine"].is_contiguous():                    # keep the slice a slice on the device
        d["color_fine"] = torch.cat([p["color_fine"], torch.zeros(p["color_fine"].shape[0], 1)], 1).cuda()[:, :3]
        assert not d["color_fine"].is_contiguous()
    names = [k for k in R.LOSS_GRADS if k in d]
    for k in names:
        d[k] = d[k].detach().requires_grad_(True)
    tg = {k: v.cuda() for k, v in t.items()}
    loss, terms = _FusedLoss.apply(d["color_fine"], d["sparse_sdf"], d.get("pseudo_sdf"), d["ncc"], d["render_depth"], d["gradient_error"],
                                   d["smooth_error"], d["tv_reg"], tg["color"], d["valid_mask"], d["mid_inside_sphere"], tg.get("pseudo_depth"),
                                   tg.get("depth"), case["weights"], case["scale"])
    out = {k: float(terms[i]) for i, k in enumerate(R.LOSS_KEYS)}
    assert float(loss) == out["loss"]
    grads = dict(zip(names, torch.autograd.grad(loss * case["cot"], [d[k] for k in names], allow_unused=True)))
    return out, grads


@pytest.mark.parametrize("name", list(R.LOSS_CASES))
def test_fused_loss_against_float64(name):
    case = R.loss_case(name)
    ref = R.loss_reference(case)
    out, grads = _fused(case)
    use_v, use_g, text = R.loss_check(ref, out, grads)
    print(f"loss {name}: {text}")
    assert use_v <= 1 and use_g <= 1, text
    spec = R.LOSS_CASES[name]
    if spec["npz"] is not None and spec["npz"] > spec["b"]:    # every element of g_pseudo, past the rays too
        want = ref["grads"]["pseudo_sdf"]
        got = grads["pseudo_sdf"].cpu().double()
        assert got.shape == want.shape and bool(((got - want).abs() <= ref["grad_bound"]["pseudo_sdf"]).all())
        assert bool((got[want == 0] == 0).all()) and bool((got[spec["b"]:][want[spec["b"]:] != 0] != 0).all())
    if spec["valid"] == "none":                                # an all-invalid batch: zero colour and patch terms, zero gradients, exactly
        assert out["color_loss"] == 0.0 and out["mfc_loss"] == 0.0
        assert not bool(grads["color_fine"].any()) and not bool(grads["ncc"].any())


def test_loss_module_with_the_patch_statistic_fed_separately():
    """gens_amd.losses.Loss end to end equals compute_LNCC followed by the fused kernel, and its terms meet the criteria with that ncc."""
    from gens_amd.config import Conf
    from gens_amd.losses import Loss, compute_LNCC
    case = dict(R.loss_case("b65-s1-p1-depth-only"))
    ref_gray, src_gray = R.lncc_case(5, "ordinary")            # (6, 9, 7, 121): six rays are too few; tile them to the 65 of the case
    reps = -(-65 // ref_gray.shape[1])
    ref_gray, src_gray = ref_gray.repeat(1, reps, 1, 1)[:, :65].cuda(), src_gray.repeat(1, reps, 1, 1)[:, :65].cuda()
    ncc = compute_LNCC(ref_gray, src_gray)
    case["preds"] = dict(case["preds"], ncc=ncc.cpu())
    ref = R.loss_reference(case)
    out, grads = _fused(case)
    use_v, use_g, text = R.loss_check(ref, out, grads)
    print(f"loss module: {text}")
    assert use_v <= 1 and use_g <= 1, text
    keys = ("color_weight", "igr_weight", "sparse_weight", "mfc_weight", "smooth_weight", "tv_weight", "pseudo_sdf_weight", "pseudo_depth_weight")
    conf = Conf(dict(zip(keys, map(float, case["weights"])), sparse_scale_factor=float(case["scale"])))
    preds = {k: v.cuda() for k, v in case["preds"].items() if k != "ncc"}
    preds.update(ref_gray_val=ref_gray, sampled_gray_val=src_gray)
    res = Loss(conf)(preds, {k: v.cuda() for k, v in case["targets"].items()})
    assert tuple(res.keys()) == R.LOSS_KEYS
    for k in R.LOSS_KEYS:
        assert float(res[k]) == out[k], k
