"""GPU tests of K27 (gens_largest_component) and what is built on it: the kernel against the numpy restatement of utils/tools.py:34-50
(tests/clean_volume_reference.py), exactly -- bits, number of components, size, first voxel, label number -- for both connectivities;
ops.clean_volume's return contract; ops.filter_masks(keep_largest=True) against tests/filter_volume_reference.py's chain with the restatement
applied to the band before its dilation; GenS.init_volumes with and without the option.  No golden from the reference exists for this
function (skimage is not installed, clean_volume cannot be run): the pin is the restatement, which tests/test_clean_volume_cpu.py checks
against scipy.ndimage.label."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from . import clean_volume_reference as CR
from . import filter_volume_reference as FR

pytestmark = pytest.mark.gpu

THRESH = 0.1


def _random(shape, fill, seed):
    return np.random.default_rng(seed).random(shape) < fill


def _serpentine():
    """One path, one voxel thick, through a (32, 32, 32) volume: the full z rows at even x <= 28 and even y, joined end to end by single
    voxels (every second row in x and in y: rows any closer would touch under connectivity 3, so this is as long as such a path gets
    there, ~7.9 k voxels), and a 40-voxel blob three voxels away from it."""
    m = np.zeros((32, 32, 32), dtype=bool)
    rows = []
    for k, x in enumerate(range(0, 30, 2)):
        ys = list(range(0, 32, 2))
        rows += [(x, y) for y in (ys if k % 2 == 0 else ys[::-1])]
    end = 31                                                   # the z end at which the path leaves the current row
    for (x, y), nxt in zip(rows, rows[1:] + [None]):
        m[x, y, :] = True
        if nxt is not None:
            m[(x + nxt[0]) // 2, (y + nxt[1]) // 2, end] = True
            end = 31 - end
    path = int(m.sum())
    m[31, 10:15, 4:12] = True
    return m, path


def _two_equal(later_first):
    """Two components of 12 voxels each in (6, 9, 40), and one of 5; the 12-voxel one whose first voxel comes first must win.  later_first:
    the small one comes first of all in C order (the winner's label number is 2 then)."""
    m = np.zeros((6, 9, 40), dtype=bool)
    m[1, 2, 3:15] = True
    m[4, 6, 20:32] = True
    if later_first:
        m[0, 0, 0:5] = True
    else:
        m[5, 8, 35:40] = True
    return m


def _corner_cubes():
    m = np.zeros((7, 6, 5), dtype=bool)
    m[1:3, 1:3, 1:3] = True
    m[3:5, 3:5, 3:5] = True
    return m


def _long_rows():
    """(3, 5, 700): runs of set voxels along z that cross 32-bit words, 64-voxel waves and 256-thread workgroups (a row is 700 voxels, no
    multiple of any of them)."""
    return _random((3, 5, 700), 0.93, 4)


CASES = {
    "empty": lambda: np.zeros((5, 7, 3), dtype=bool),
    "single": lambda: np.pad(np.ones((1, 1, 1), dtype=bool), ((2, 2), (4, 2), (1, 1))),
    "full": lambda: np.ones((5, 7, 3), dtype=bool),
    "odd-0.1": lambda: _random((33, 17, 9), 0.1, 1),
    "odd-0.25": lambda: _random((33, 17, 9), 0.25, 2),
    "odd-0.6": lambda: _random((33, 17, 9), 0.6, 3),
    "odd-rows": lambda: np.pad(np.ones((29, 1, 9), dtype=bool), ((2, 2), (8, 8), (0, 0))) | _random((33, 17, 9), 0.05, 9),
    "cube-0.1": lambda: _random((64, 64, 64), 0.1, 5),
    "cube-0.25": lambda: _random((64, 64, 64), 0.25, 6),
    "cube-0.6": lambda: _random((64, 64, 64), 0.6, 7),
    "long-rows": _long_rows,
    "tie-later-second": lambda: _two_equal(False),
    "tie-later-first": lambda: _two_equal(True),
    "corner-cubes": _corner_cubes,
    "serpentine": lambda: _serpentine()[0],
}


@functools.lru_cache(maxsize=None)
def _case(name):
    m = CASES[name]()
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _expected(name, connectivity):
    """The restatement's answer, computed once per case: (bool volume of the largest region, (N, size, first index, label number))."""
    m = _case(name)
    out, info = CR.clean_volume(m, connectivity)
    keep = np.zeros(m.shape, dtype=bool) if info[0] < 1 else out > 0
    keep.setflags(write=False)
    return keep, info


def _run(m, connectivity):
    from gens_amd import ops
    vals = torch.from_numpy(m.astype(np.float32) * (0.5 + np.random.default_rng(0).random(m.shape, dtype=np.float32))).cuda()
    before = vals.clone()
    out, n, size, first, number = ops.largest_component(vals, connectivity, return_info=True)
    assert out.shape == vals.shape and out.dtype == vals.dtype and torch.equal(vals, before)
    assert all(t.dtype == torch.int64 and t.dim() == 0 and t.is_cuda for t in (n, size, first, number))
    return vals, out, (int(n), int(size), int(first), int(number))


@pytest.mark.parametrize("connectivity", [3, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_kernel_equals_the_restatement(name, connectivity):
    keep, info = _expected(name, connectivity)
    vals, out, got = _run(_case(name), connectivity)
    print(name, connectivity, "expected", info, "got", got)
    assert got == info
    want = torch.where(torch.from_numpy(keep.copy()).cuda(), vals, torch.zeros_like(vals))        # kept voxels unchanged, the others 0
    assert torch.equal(out, want)


def test_the_cases_are_what_they_claim():
    """The tie cases have two largest components of one size; the corner cubes are one component only through the diagonal; the serpentine is
    one long path that beats the blob; the 0.25 fill has many small components beside the large one."""
    for name, number in (("tie-later-second", 1), ("tie-later-first", 2)):
        lab, num = CR.label(_case(name), 3)
        sizes = np.bincount(lab.reshape(-1))[1:]
        assert num == 3 and sorted(sizes) == [5, 12, 12] and _expected(name, 3)[1] == (3, 12, int(np.flatnonzero(lab.reshape(-1) == number)[0]), number)
    assert _expected("corner-cubes", 3)[1][:2] == (1, 16) and _expected("corner-cubes", 1)[1][:2] == (2, 8)
    m, path = _serpentine()
    assert path > 7800
    for conn in (1, 3):
        assert _expected("serpentine", conn)[1] == (2, path, 0, 1)
    n, size, _, _ = _expected("cube-0.25", 1)[1]
    assert n > 5000 and size < 64 ** 3 // 8
    n, size, _, _ = _expected("cube-0.1", 3)[1]
    assert n > 1000


def test_sizes_and_component_count_on_the_quarter_fill():
    from gens_amd import ops
    m = _case("cube-0.25")
    for conn in (3, 1):
        keep, (n, size, first, number) = _expected("cube-0.25", conn)
        out, got_n, got_size, got_first, got_number = ops.largest_component(torch.from_numpy(m.copy()).cuda(), conn, return_info=True)
        assert out.dtype == torch.bool and torch.equal(out.cpu(), torch.from_numpy(keep.copy()))
        assert (int(got_n), int(got_size), int(got_first), int(got_number)) == (n, size, first, number)
        assert int(out.sum()) == size


def test_two_runs_give_identical_bits():
    from gens_amd import ops
    m = torch.from_numpy(_case("cube-0.25").copy()).cuda()
    for conn in (3, 1):
        a = ops.largest_component(m, conn, return_info=True)
        b = ops.largest_component(m, conn, return_info=True)
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_five_dim_input_keeps_its_shape():
    from gens_amd import ops
    m = _case("odd-0.25")
    keep, _ = _expected("odd-0.25", 3)
    out = ops.largest_component(torch.from_numpy(m.astype(np.float32))[None, None].cuda())
    assert out.shape == (1, 1) + m.shape and torch.equal(out[0, 0].cpu() > 0, torch.from_numpy(keep.copy()))


def test_clean_volume_return_contract(capsys):
    """utils/tools.py:38-50: the label-valued int64 volume (the winner's voxels hold its label number, not 1), the printed line, and the
    input object itself when nothing is set."""
    from gens_amd import ops
    for name in ("tie-later-first", "odd-0.1", "cube-0.1"):
        m = _case(name)
        want, (n, _, _, number) = CR.clean_volume(m, 3)
        vol = torch.from_numpy(m.astype(np.float32)).cuda()
        capsys.readouterr()
        got = ops.clean_volume(vol)
        assert capsys.readouterr().out == f"Num region: {n}\n"
        assert got.dtype == torch.int64 and got.shape == vol.shape and torch.equal(got.cpu(), torch.from_numpy(want))
        assert set(got.unique().tolist()) == {0, number}
    assert _expected("tie-later-first", 3)[1][3] == 2 and _expected("odd-0.1", 3)[1][3] > 1          # label numbers other than 1 were seen
    empty = torch.zeros(5, 7, 3).cuda()
    capsys.readouterr()
    assert ops.clean_volume(empty) is empty
    assert capsys.readouterr().out == "Num region: 0\n"


def _shell_lattice(d0):
    """u on linspace(-1, 1, d0)^3: a spherical shell 0.5 < |p| < 0.7 in the band, plus three blobs with u = 0 -- at the centre and at
    |p| ~ 0.87 on the x axis (both inside the unit sphere, both at least one clear voxel away from the shell), and in a corner (outside the
    unit sphere: the sphere test removes it before the components are looked at)."""
    axis = torch.linspace(-1, 1, d0)
    x, y, z = torch.meshgrid(axis, axis, axis, indexing="ij")
    u = torch.sqrt(x * x + y * y + z * z) - 0.6
    c = d0 // 2
    u[c - 1:c + 1, c - 1:c + 1, c - 1:c + 1] = 0.0
    hi = d0 - 2 if d0 == 16 else d0 - 3
    u[hi, c - 1:c + 1, c - 1:c + 1] = 0.0
    u[0:2, 0:2, 0:2] = 0.0
    return u.cuda()


def _chain_keeping_the_largest(u, masks, thresh):
    r = FR.filter_chain(u, masks, thresh)
    band = r["band"].cpu().numpy()
    kept, (n, size, _, _) = CR.clean_volume(band, 3)
    kept = torch.from_numpy((kept > 0).astype(np.float32)).to(u.device)
    cur = F.max_pool3d(kept[None, None], 3, 1, 1)
    dil = cur
    out = []
    for m in masks:
        out.append(m * cur)
        cur = F.interpolate(cur, scale_factor=0.5, mode="nearest")
    return {"band": r["band"], "kept": kept, "masks": out, "counts": (int(r["band"].sum()), int(dil.sum()), n, size)}


@pytest.mark.parametrize("dims", [(16, 8, 4), (32, 16, 8)])
def test_filter_masks_keeping_the_largest_region(dims):
    from gens_amd import ops
    from .test_hip_filter_volume import _masks, _words_of
    u, masks = _shell_lattice(dims[0]), _masks(dims, 5)
    ref = _chain_keeping_the_largest(u, masks, THRESH)
    assert ref["counts"][2] == 3 and ref["counts"][3] < ref["counts"][0]                           # shell + two blobs; the corner blob is no region
    outs, n_band, n_dil, n_regions, n_kept, words = ops.filter_masks(u, masks, THRESH, return_band=True, keep_largest=True)
    got = (int(n_band), int(n_dil), int(n_regions), int(n_kept))
    print(dims, "expected", ref["counts"], "got", got)
    assert got == ref["counts"]
    assert torch.equal(FR.unpack_words(words, ref["kept"].shape), ref["kept"].cpu())
    for l, (o, r) in enumerate(zip(outs, ref["masks"])):
        assert o.shape == masks[l].shape and torch.equal(o, r), l
        ver, w = o._gens_bits
        assert ver == o._version and w.dtype == torch.int32 and torch.equal(w, _words_of(o)), l
    assert len(ops.filter_masks(u, masks, THRESH, keep_largest=True)) == 5
    # keep_largest=False is the call without the argument, bit for bit
    a = ops.filter_masks(u, masks, THRESH, return_band=True)
    b = ops.filter_masks(u, masks, THRESH, return_band=True, keep_largest=False)
    assert len(a) == len(b) == 4
    for x, y in zip(a[0], b[0]):
        assert torch.equal(x, y) and torch.equal(x._gens_bits[1], y._gens_bits[1])
    assert all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))
    assert torch.equal(FR.unpack_words(a[3], ref["band"].shape), ref["band"].cpu())              # and its band is the whole band


def _finetune_model(**kw):
    from tests.test_hip_ddp import _inputs, _model
    model = _model()
    ipts = _inputs(7, nv=3)
    model.init_volumes({k: ipts[k] for k in ("imgs", "intrs", "c2ws")}, **kw)
    return model


def test_init_volumes_with_and_without_the_option(capsys):
    from gens_amd import lib as L, ops
    from .test_hip_filter_volume import _eager_step
    plain = _finetune_model()
    parent_path = _finetune_model(filter_thresh=THRESH)
    lines_parent = capsys.readouterr().out.splitlines()
    assert [s.split(":")[0] for s in lines_parent] == ["Filtering sdf volume...", "Survival ratio", "Survival ratio after dilation"]
    model = _finetune_model(filter_thresh=THRESH, filter_keep_largest=True)
    lines = capsys.readouterr().out.splitlines()
    assert lines[:3] == lines_parent and len(lines) == 5
    assert lines[3].startswith("Num region: ") and lines[4].startswith("Survival ratio of the largest region: tensor(")
    d0 = int(plain.volumes[0].shape[-1])
    lo, hi = torch.tensor([-1.0] * 3).cuda(), torch.tensor([1.0] * 3).cuda()
    u = plain.implicit_surface.sdf_grid([v.detach() for v in plain.volumes], lo, hi, d0)
    want, _, _, n_regions, _ = ops.filter_masks(u, list(plain.mask_volmes), THRESH, keep_largest=True)
    assert lines[3] == f"Num region: {int(n_regions)}"
    for a, b in zip(model.mask_volmes, want):
        assert torch.equal(a, b) and not a.requires_grad
    assert all(m._gens_bits[0] == m._version for m in model.mask_volmes)
    L.profile_begin(only={"gens_pack_mask_bits"})
    _eager_step(model)
    assert not L.profile_end(raw=True)                               # the words came with the masks: no packing pass
    # without the option: the parent commit's path, whichever way it is switched off
    old, _, _ = ops.filter_masks(u, list(plain.mask_volmes), THRESH)
    by_false = _finetune_model(filter_thresh=THRESH, filter_keep_largest=False)
    from gens_amd.models.gens import GenS
    try:
        GenS.filter_keep_largest = True                              # the class default turned on: an explicit False still wins
        by_attr = _finetune_model(filter_thresh=THRESH, filter_keep_largest=False)
        on_by_attr = _finetune_model(filter_thresh=THRESH)
    finally:
        GenS.filter_keep_largest = False
    for a, b, c, d, e, f in zip(parent_path.mask_volmes, old, by_false.mask_volmes, by_attr.mask_volmes, on_by_attr.mask_volmes, model.mask_volmes):
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d) and torch.equal(e, f)
