"""GenS.filter_volume without a GPU: the plain-torch restatement of the reference's chain (tests/filter_volume_reference.py) reproduces the
reference's own run (goldens g23 / g23c, tests/golden/make_golden_filter_volume.py) exactly from its stored lattice; the shapes the kernel
cannot serve are refused before anything touches a device; the goldens' recorded ambiguous counts respect the generator's caps."""
import os

import numpy as np
import pytest
import torch

from . import filter_volume_reference as FR
from .conftest import GOLDEN

CASES = [("a", "g23_filter_volume"), ("b", "g23_filter_volume"), ("c", "g23c_filter_volume")]


def load(name):
    raw = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: raw[k] for k in raw.files}


@pytest.mark.parametrize("tag,name", CASES)
def test_restatement_reproduces_the_reference_run_exactly(tag, name):
    g = load(name)
    dims, thresh = [int(d) for d in g[tag + ".dims"]], float(g[tag + ".thresh"])
    u = torch.from_numpy(g[tag + ".u"])
    masks = [FR.unpack_bits(g[f"{tag}.mask{i}"], (1, 1, d, d, d)) for i, d in enumerate(dims)]
    r = FR.filter_chain(u, masks, thresh)
    assert np.array_equal(FR.pack_bits(r["band"]), g[tag + ".band"])
    assert np.array_equal(FR.pack_bits(r["dilated"]), g[tag + ".dilated"])
    for i in range(len(dims)):
        assert np.array_equal(FR.pack_bits(r["masks"][i]), g[f"{tag}.filtered{i}"]), i
    assert FR.printed_lines(r["ratio"], r["ratio_dilated"]) == [str(s) for s in g[tag + ".lines"]]


@pytest.mark.parametrize("tag,name", CASES)
def test_recorded_ambiguous_counts_respect_the_caps(tag, name):
    g = load(name)
    u, thresh = torch.from_numpy(g[tag + ".u"]), float(g[tag + ".thresh"])
    n = int(FR.ambiguous(u, thresh).sum())
    assert n == int(g[tag + ".ambiguous"]) and n <= 0.005 * u.numel()
    if tag == "a":                                   # the model of the end-to-end case d: none, and none within the generator's margin
        d = load("g23d_filter_finetune")
        assert n == 0 and int(d["ambiguous"]) == 0 and int(d["seed"]) == int(g["seed"])
        assert int(FR.ambiguous(u, thresh, float(d["margin"])).sum()) == 0


def test_shapes_the_kernel_cannot_serve_are_refused():
    from gens_amd import lib as L, ops
    m = lambda *ds: [torch.ones(1, 1, d, d, d) for d in ds]  # noqa: E731
    assert ops.filter_mask_dims((16, 16, 16), [t.shape for t in m(16, 8, 4)]) == [16, 8, 4]
    assert ops.filter_mask_dims((20, 20, 20), [t.shape for t in m(20, 10, 5)]) == [20, 10, 5]
    with pytest.raises(ValueError, match="D0 >> 1"):
        ops.filter_masks(torch.zeros(16, 16, 16), m(16, 7, 4), 0.1)
    with pytest.raises(ValueError, match="multiple"):
        ops.filter_masks(torch.zeros(10, 10, 10), m(10, 5, 2), 0.1)
    with pytest.raises(ValueError, match="GENS_MAX_LEVELS"):
        ops.filter_masks(torch.zeros(512, 512, 512), [torch.ones(1, 1, 1, 1, 1)] * (L.MAX_LEVELS + 1), 0.1)
    with pytest.raises(ValueError, match="cube"):
        ops.filter_masks(torch.zeros(16, 16, 8), m(16), 0.1)
    with pytest.raises(ValueError):
        ops.filter_masks(torch.zeros(16, 16, 16), [], 0.1)


def test_entry_point_refuses_bad_arguments_before_any_launch():
    import ctypes as C
    from gens_amd import lib as L
    lib = L.load()
    one = (C.c_void_p * 3)(64, 64, 64)
    tab = C.cast(one, C.POINTER(C.c_void_p))
    p = C.c_void_p(64)
    assert lib.gens_filter_masks(None, 0.1, None, None, None, None, 1, None, None, None) == -1 and b"null" in lib.gens_last_error()
    assert lib.gens_filter_masks(p, 0.1, tab, tab, tab, L.int_table([8] * 9), 9, p, p, None) == -2 and b"GENS_MAX_LEVELS" in lib.gens_last_error()
    assert lib.gens_filter_masks(p, 0.1, tab, tab, tab, L.int_table([16, 8, 3]), 3, p, p, None) == -1 and b"dims[2]" in lib.gens_last_error()
    assert lib.gens_filter_masks(p, 0.1, tab, tab, tab, L.int_table([10, 5, 2]), 3, p, p, None) == -1 and b"multiple" in lib.gens_last_error()
    assert lib.gens_filter_masks(C.c_void_p(66), 0.1, tab, tab, tab, L.int_table([16, 8, 4]), 3, p, p, None) == -1 and b"misaligned" in lib.gens_last_error()
    assert lib.gens_filter_masks(p, 0.1, tab, tab, tab, L.int_table([16, 8, 4]), 3, p, C.c_void_p(68), None) == -1 and b"misaligned" in lib.gens_last_error()


def test_model_surface_of_the_feature():
    """The attribute, the conf key and the keyword exist and default to None; the method keeps the reference's signature."""
    import inspect
    from gens_amd.config import Conf, gens_model_conf
    from gens_amd.models.gens import GenS
    assert GenS.filter_thresh is None
    sig = inspect.signature(GenS.filter_volume)
    assert list(sig.parameters) == ["self", "volumes", "mask_volmes", "thresh"] and sig.parameters["thresh"].default == 0.1
    assert "filter_thresh" in inspect.signature(GenS.init_volumes).parameters
    conf = gens_model_conf(volume_dims=(16, 8, 4))
    assert GenS(conf).filter_thresh is None
    assert GenS(Conf({**conf, "filter_thresh": 0.05})).filter_thresh == 0.05
