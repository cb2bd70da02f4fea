"""GPU tests of GenS.filter_volume: the K26 kernel (gens_filter_masks) against the torch-operator chain on the same device and lattice,
exactly; the model method against the reference's own run (goldens g23 / g23c / g23d, tests/golden/make_golden_filter_volume.py); the bit
words that travel with the filtered masks; defaults, checkpoints and the captured fine-tune step."""
import os

import numpy as np
import pytest
import torch

from . import filter_volume_reference as FR

pytestmark = pytest.mark.gpu

THRESH = 0.1


def _lattice(d0, seed, kind="random"):
    g = torch.Generator().manual_seed(seed)
    if kind == "outside":
        return torch.full((d0, d0, d0), 5.0).cuda()
    if kind == "zero":                                    # the band is the open unit ball: the sphere test alone (D0 = 9 has points ON the sphere)
        return torch.zeros(d0, d0, d0).cuda()
    u = 0.15 * torch.randn(d0 ** 3, generator=g)
    t = torch.tensor(THRESH, dtype=torch.float32)
    below, above = torch.nextafter(t, torch.tensor(0.0)), torch.nextafter(t, torch.tensor(1.0))
    planted = [float("nan"), float("inf"), float("-inf"), float(t), -float(t), float(below), -float(below), float(above), -float(above), 0.0, -0.0]
    where = torch.randperm(d0 ** 3, generator=g)[:len(planted) * 6]
    u[where] = torch.tensor(planted, dtype=torch.float32).repeat(6)
    centre = (d0 // 2 * d0 + d0 // 2) * d0 + d0 // 2      # planted values inside the sphere too, whatever the permutation chose
    u[centre:centre + len(planted)] = torch.tensor(planted, dtype=torch.float32)
    return u.reshape(d0, d0, d0).cuda()


def _masks(dims, seed, binary=True):
    g = torch.Generator().manual_seed(seed)
    if binary:
        return [(torch.rand(1, 1, d, d, d, generator=g) < 0.7).float().cuda() for d in dims]
    return [(torch.rand(1, 1, d, d, d, generator=g) * 3 - 1).cuda() for d in dims]        # values in [-1, 2): kept by the float product


def _words_of(t):
    from gens_amd import lib as L
    flat = t.detach().reshape(-1).contiguous()
    w = torch.empty((flat.numel() + 31) // 32, device=t.device, dtype=torch.int32)
    L.call("gens_pack_mask_bits", L.ptr(flat), flat.numel(), L.ptr(w, torch.int32), L.stream())
    return w


def _check_against_chain(u, masks, thresh):
    from gens_amd import ops
    before = [m.clone() for m in masks]
    outs, n_band, n_dil, words = ops.filter_masks(u, masks, thresh, return_band=True)
    ref = FR.filter_chain(u, masks, thresh)
    assert torch.equal(FR.unpack_words(words, ref["band"].shape), ref["band"].cpu())
    assert all(torch.equal(m, b) for m, b in zip(masks, before))                         # the inputs are left alone
    assert int(n_band) == int(ref["band"].sum()) and int(n_dil) == int(ref["dilated"].sum())
    for l, (o, r) in enumerate(zip(outs, ref["masks"])):
        assert o.shape == masks[l].shape and torch.equal(o, r), l
        ver, words = o._gens_bits
        assert ver == o._version and words.dtype == torch.int32 and torch.equal(words, _words_of(o)), l
    return outs, ref


@pytest.mark.parametrize("dims", [(16, 8, 4), (20, 10, 5), (32, 16, 8), (64, 32), (9,), (8,)])
def test_kernel_equals_the_torch_chain_exactly(dims):
    for kind in ("random", "outside", "zero"):
        outs, ref = _check_against_chain(_lattice(dims[0], 11 + dims[0], kind), _masks(dims, 5), THRESH)
        if kind == "outside":
            assert all(float(o.abs().sum()) == 0.0 for o in outs)
        if kind == "zero":
            assert 0 < int(ref["band"].sum()) < dims[0] ** 3
    _check_against_chain(_lattice(dims[0], 3, "random"), _masks(dims, 6, binary=False), THRESH)
    _check_against_chain(_lattice(dims[0], 4, "random"), _masks(dims, 7), 0.05)


def _golden(name):
    from .conftest import GOLDEN
    raw = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: raw[k] for k in raw.files}


def _golden_model(dims, seed, sd):
    from gens_amd.config import gens_model_conf
    from gens_amd.models import gens
    saved = dict(gens._BACKBONES)
    gens._BACKBONES.clear()
    try:
        torch.manual_seed(seed)
        model = gens.GenS(gens_model_conf(volume_dims=dims)).train()
    finally:
        gens._BACKBONES.update(saved)
    model.implicit_surface.load_state_dict(sd, strict=True)
    return model.cuda()


@pytest.mark.parametrize("tag,name", [("a", "g23_filter_volume"), ("b", "g23_filter_volume"), ("c", "g23c_filter_volume")])
def test_filter_volume_against_the_reference_run(tag, name, capsys):
    """GenS.filter_volume on the golden's frozen volumes and masks: the device lattice within the g10 tolerance of the reference's; band
    bits equal outside the ambiguous set; final masks equal wherever no ambiguous voxel lies in the 3 x 3 x 3 level-0 neighbourhood (at
    least 99 % of every level, which the generator's 0.5 % cap guarantees: 27 x 0.5 % < 14 %, and the recorded counts are far below);
    the printed lines equal when nothing ambiguous flipped."""
    from gens_amd import ops
    g, main = _golden(name), _golden("g23_filter_volume")
    dims, thresh = tuple(int(d) for d in g[tag + ".dims"]), float(g[tag + ".thresh"])
    model = _golden_model(dims, int(main["seed"]), {k[3:]: torch.from_numpy(v) for k, v in main.items() if k.startswith("sd.")})
    vols = [torch.from_numpy(g[f"{tag}.volume{i}"]).cuda() for i in range(len(dims))]
    masks = [FR.unpack_bits(g[f"{tag}.mask{i}"], (1, 1, d, d, d)).cuda() for i, d in enumerate(dims)]
    u_ref = torch.from_numpy(g[tag + ".u"])
    d0 = dims[0]
    u = model.implicit_surface.sdf_grid(vols, torch.tensor([-1.0] * 3).cuda(), torch.tensor([1.0] * 3).cuda(), d0).cpu()
    err = (u - u_ref).abs() - (FR.LATTICE_ATOL + FR.LATTICE_RTOL * u_ref.abs())
    print(f"lattice: worst |du| {float((u - u_ref).abs().max()):.3e}, worst excess over the tolerance {float(err.max()):.3e}")
    assert float(err.max()) <= 0.0
    capsys.readouterr()
    given = list(masks)
    out = model.filter_volume(vols, given, thresh)
    lines = capsys.readouterr().out.splitlines()
    assert out is given and len(out) == len(dims)                       # the reference fills and returns the list it was handed
    amb = FR.ambiguous(u_ref, thresh)
    assert int(amb.sum()) == int(g[tag + ".ambiguous"])
    # band: the KERNEL's decision on the device lattice (the words its first launch leaves), against the reference's band outside the ambiguous set
    _, n_band, _, words = ops.filter_masks(u.cuda(), [torch.ones(1, 1, d0, d0, d0).cuda()], thresh, return_band=True)
    band_dev = FR.unpack_words(words, (d0, d0, d0))
    band_ref = FR.unpack_bits(g[tag + ".band"], (d0, d0, d0))
    assert torch.equal(band_dev[~amb], band_ref[~amb])
    assert int(n_band) == int(band_dev.sum())
    assert torch.equal(band_dev, FR.filter_chain(u.cuda(), [], thresh)["band"].cpu())       # and the torch chain decides the same on this lattice
    near = FR.near_ambiguous(amb)
    for l, d in enumerate(dims):
        want = FR.unpack_bits(g[f"{tag}.filtered{l}"], (d, d, d))
        sure = ~near[::1 << l, ::1 << l, ::1 << l]
        assert sure.shape == want.shape and float(sure.float().mean()) >= 0.99, l
        got = out[l].cpu()[0, 0]
        assert torch.equal(got[sure], want[sure]), l
    if torch.equal(band_dev, band_ref):
        assert lines == [str(s) for s in g[tag + ".lines"]]
    else:
        assert lines[0] == "Filtering sdf volume..." and lines[1].startswith("Survival ratio: tensor(") and len(lines) == 3


def test_init_volumes_with_a_threshold_then_a_finetune_step_matches_the_reference():
    """Case d: `init_volumes(..., filter_thresh=0.1)` on the device, then forward("finetune"), loss and backward against the reference's run
    with its filtered masks (golden g23d), at the tolerances tests/test_hip_training.py holds the unfiltered path to against g18.  The golden's
    model has no ambiguous voxel, so the filtered masks are compared at every voxel."""
    from gens_amd import synthetic
    from .test_hip_training import _check_grad_table
    g, main = _golden("g23d_filter_finetune"), _golden("g23_filter_volume")
    dims, seed, thresh = tuple(int(d) for d in g["dims"]), int(g["seed"]), float(g["thresh"])
    nl = len(dims)
    model = _golden_model(dims, seed, {k[3:]: torch.from_numpy(v) for k, v in main.items() if k.startswith("sd.")})
    sc = synthetic.make_scene(nv=4, h=64, w=96, n_levels=1, seed=seed + 1)
    assert torch.equal(sc["intrs"], torch.from_numpy(main["scene.intrs"])) and torch.equal(sc["c2ws"], torch.from_numpy(main["scene.c2ws"]))
    np.testing.assert_allclose(float(sc["imgs"].double().sum()), float(main["scene.imgs_sum"]), rtol=1e-9)
    t = lambda k: torch.from_numpy(g[k]).cuda()  # noqa: E731

    def rel(a, b):
        a, b = a.detach().cpu().double().reshape(-1), torch.from_numpy(b).double().reshape(-1)
        return ((a - b).abs().max() / b.abs().max().clamp_min(1e-8)).item()

    model.init_volumes({"imgs": sc["imgs"].cuda(), "intrs": sc["intrs"].cuda(), "c2ws": sc["c2ws"].cuda()}, filter_thresh=thresh)
    for i, d in enumerate(dims):
        assert rel(model.volumes[i], main[f"a.volume{i}"]) < 2e-4, i
        assert np.array_equal(FR.pack_bits(model.mask_volmes[i]), main[f"a.filtered{i}"]), i
        assert not model.mask_volmes[i].requires_grad and model.mask_volmes[i]._gens_bits[0] == model.mask_volmes[i]._version
    view_ids = g["in.view_ids"].tolist()
    ipts = {k[3:]: (view_ids if k == "in.view_ids" else t(k)) for k in g if k.startswith("in.")}
    ipts["imgs"] = sc["imgs"][view_ids].cuda()
    torch.manual_seed(seed + 3)
    out = model("finetune", ipts, cos_anneal_ratio=1.0, step=11)
    hit = out["mid_inside_sphere"].reshape(1, -1, 1, 1)
    loss = (out["color_fine"].abs().sum() + 0.1 * out["gradient_error"] + 0.01 * out["smooth_error"] + 0.01 * out["tv_reg"]
            + torch.exp(-out["sparse_sdf"].abs() * 100).mean() + (((out["sampled_gray_val"] - out["ref_gray_val"]) ** 2) * hit).mean()
            + 0.1 * out["render_depth"].sum() + out["pseudo_sdf"].abs().mean())
    loss.backward()
    errs = {k: rel(out[k[4:]], v) for k, v in g.items() if k.startswith("out.")}
    print({k: f"{e:.2e}" for k, e in errs.items()})
    bad = {k: e for k, e in errs.items() if e > (2e-3 if k == "out.weights" else 3e-4)}
    assert not bad, bad
    assert abs(float(loss) - float(g["loss"])) < 1e-4 * abs(float(g["loss"]))
    rows = [(f"volume{i}", rel(model.volumes[i].grad, g[f"grad.volume{i}"]), float(np.abs(g[f"grad.volume{i}"]).max())) for i in range(nl)]
    rows.append(("lin0.weight_v", rel(model.implicit_surface.sdf_network.lin0.weight_v.grad, g["grad.lin0"]), float(np.abs(g["grad.lin0"]).max())))
    params = dict(model.named_parameters())
    rows += [(k[5:], rel(params[k[5:]].grad, v), float(np.abs(v).max())) for k, v in g.items() if k.startswith("grad.implicit_surface.")]
    _check_grad_table(rows)


def _finetune_model(filter_thresh, auto=False, explicit_none=False):
    from tests.test_hip_ddp import _inputs, _model
    model = _model()
    ipts = _inputs(7, nv=3)
    kw = {"filter_thresh": filter_thresh} if filter_thresh is not None or explicit_none else {}
    model.init_volumes({k: ipts[k] for k in ("imgs", "intrs", "c2ws")}, **kw)
    model.auto_graph = auto
    return model


def _eager_step(model, seed=5):
    from tests.test_hip_auto_graph import _step_inputs
    torch.manual_seed(seed)
    return {k: v.detach() for k, v in model("finetune", _step_inputs(0)).items() if torch.is_tensor(v)}


def test_render_with_the_attached_bits_equals_a_render_with_fresh_tensors(capsys):
    from gens_amd import lib as L
    model = _finetune_model(THRESH)
    assert "Survival ratio after dilation: tensor(" in capsys.readouterr().out
    assert all(m._gens_bits[0] == m._version for m in model.mask_volmes)
    assert 0 < sum(float(m.sum()) for m in model.mask_volmes)
    L.profile_begin(only={"gens_pack_mask_bits"})
    a = _eager_step(model)
    assert not L.profile_end(raw=True)                               # the words came with the masks: no packing pass
    model.mask_volmes = torch.nn.ParameterList([torch.nn.Parameter(m.detach().clone(), requires_grad=False) for m in model.mask_volmes])
    assert not any(hasattr(m, "_gens_bits") for m in model.mask_volmes)
    b = _eager_step(model)
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), k
    assert any(torch.is_tensor(v) for v in a.values())


def test_defaults_leave_the_masks_as_they_were():
    from gens_amd.models.gens import GenS
    assert GenS.filter_thresh is None
    plain = _finetune_model(None)
    assert "filter_thresh" not in vars(plain)
    explicit = _finetune_model(None, explicit_none=True)
    by_attr = _finetune_model(None)
    for a, b in zip(plain.mask_volmes, explicit.mask_volmes):
        assert torch.equal(a, b)
    filtered = _finetune_model(THRESH)
    by_attr.filter_thresh = THRESH
    from tests.test_hip_ddp import _inputs
    ipts = _inputs(7, nv=3)
    by_attr.init_volumes({k: ipts[k] for k in ("imgs", "intrs", "c2ws")})
    for a, b, c in zip(filtered.mask_volmes, by_attr.mask_volmes, plain.mask_volmes):
        assert torch.equal(a, b) and float(a.sum()) < float(c.sum()) and bool(((a > 0) <= (c > 0)).all())


def test_checkpoint_round_trip_keeps_the_filtered_masks(tmp_path):
    model = _finetune_model(THRESH)
    path = str(tmp_path / "vol.pth")
    torch.save({"model": model.get_params_vol()}, path)
    other = _finetune_model(None)
    other.load_params_vol(path, "cuda")
    for a, b in zip(model.mask_volmes, other.mask_volmes):
        assert torch.equal(a, b)
    a, b = _eager_step(model), _eager_step(other)
    assert torch.equal(a["color_fine"], b["color_fine"])


def test_captured_finetune_step_after_filtering_matches_its_eager_step():
    from tests.test_hip_auto_graph import _compare, _runner_loop
    from tests.test_hip_ddp import _loss
    lrs = {"mlp_lr": 5e-4, "vol_lr": [1e-2, 1e-2, 1e-2]}
    runs = {}
    for auto in (False, True):
        model = _finetune_model(THRESH, auto=auto)
        opt = torch.optim.Adam(model.get_optim_params(lrs))
        torch.manual_seed(21)
        runs[auto] = (model, _runner_loop(model, opt, 5, _loss))
    model, graphed = runs[True]
    assert model._auto.stats["captured"] == 1 and model._auto.stats["replayed"] == 3, model._auto.stats
    _compare(runs[False][0], model, runs[False][1], graphed)
