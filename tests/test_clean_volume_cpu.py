"""clean_volume without a GPU: the numpy restatement (tests/clean_volume_reference.py) against scipy.ndimage.label -- partition, numbering
and the largest region; the shapes and dtypes the operators refuse before anything touches a device; the K27 entry points' argument checks;
what K26's surface accepted before still is accepted."""
import inspect

import numpy as np
import pytest
import torch

from . import clean_volume_reference as CR


def test_restatement_equals_scipy_label_on_random_volumes():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(27)
    for _ in range(20):
        shape = tuple(int(v) for v in rng.integers(3, 21, 3))
        m = rng.random(shape) < rng.uniform(0.05, 0.5)
        for conn in (1, 3):
            lab, num = CR.label(m, conn)
            want, n_want = ndimage.label(m, structure=ndimage.generate_binary_structure(3, conn))
            assert num == n_want and np.array_equal(lab, want), (shape, conn)           # same partition, same numbering
            out, (n, size, first, number) = CR.clean_volume(m, conn)
            if num < 1:
                assert out is m and (n, size, first, number) == (0, 0, -1, 0)
                continue
            areas = np.bincount(want.reshape(-1))[1:]
            big = int(np.argmax(areas)) + 1
            assert (n, size, number) == (num, int(areas.max()), big)
            assert np.array_equal(out, np.where(want == big, want, 0)) and out.dtype == np.int64
            assert first == int(np.flatnonzero(want.reshape(-1) == big)[0])
            assert number == 1 + len({int(v) for v in want.reshape(-1)[:first] if v})   # components whose first voxel comes before


def test_restatement_tie_goes_to_the_earlier_first_voxel_and_diagonals_need_connectivity_3():
    m = np.zeros((4, 5, 6), dtype=bool)
    m[0, 0, 0:2] = True
    m[3, 4, 4:6] = True
    out, info = CR.clean_volume(m)
    assert info == (2, 2, 0, 1) and out[0, 0, 0] == 1 and out[3, 4, 5] == 0
    m[0, 0, 0] = False
    m[2, 0, 0:2] = True                                     # three regions; the two of size 2 tie, the single voxel (label 1) does not win
    out, info = CR.clean_volume(m)
    assert info == (3, 2, 2 * 30, 2) and out[2, 0, 1] == 2 and out[0, 0, 1] == 0
    c = np.zeros((4, 4, 4), dtype=bool)
    c[:2, :2, :2] = True
    c[2:, 2:, 2:] = True
    assert CR.clean_volume(c, 3)[1] == (1, 16, 0, 1) and CR.clean_volume(c, 1)[1] == (2, 8, 0, 1)
    with pytest.raises(ValueError):
        CR.label(c, 2)


def test_operators_refuse_bad_shapes_and_dtypes_before_touching_a_device():
    from gens_amd import ops
    with pytest.raises(ValueError, match="three positive extents"):
        ops.largest_component(torch.ones(4, 4))
    with pytest.raises(ValueError, match="three positive extents"):
        ops.largest_component(torch.ones(2, 1, 4, 4, 4))
    with pytest.raises(ValueError, match="three positive extents"):
        ops.largest_component(torch.ones(4, 0, 4))
    with pytest.raises(ValueError, match="connectivity"):
        ops.largest_component(torch.ones(4, 4, 4), connectivity=2)
    with pytest.raises(TypeError, match="float or bool"):
        ops.largest_component(torch.ones(4, 4, 4, dtype=torch.int64))
    with pytest.raises(TypeError):
        ops.largest_component(np.ones((4, 4, 4)))
    with pytest.raises(RuntimeError, match="device"):
        ops.largest_component(torch.ones(4, 4, 4))                          # no CPU path
    with pytest.raises(TypeError, match="float or bool"):
        ops.clean_volume(torch.ones(4, 4, 4, dtype=torch.uint8))
    m = lambda *ds: [torch.ones(1, 1, d, d, d) for d in ds]  # noqa: E731
    with pytest.raises(ValueError, match="D0 >> 1"):
        ops.filter_masks(torch.zeros(16, 16, 16), m(16, 7, 4), 0.1, keep_largest=True)
    with pytest.raises(ValueError, match="cube"):
        ops.filter_masks(torch.zeros(16, 16, 8), m(16), 0.1, keep_largest=True)
    with pytest.raises(RuntimeError, match="float32"):
        ops.filter_masks(torch.zeros(16, 16, 16, dtype=torch.float64), m(16), 0.1, keep_largest=True)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    import ctypes as C
    from gens_amd import lib as L
    lib = L.load()
    p, odd = C.c_void_p(64), C.c_void_p(66)
    q = C.c_void_p(128)
    cc = lib.gens_largest_component
    assert cc(None, 4, 4, 4, 3, q, p, p, None) == -1 and b"null" in lib.gens_last_error()
    assert cc(p, 4, 4, 4, 3, q, None, p, None) == -1 and b"null" in lib.gens_last_error()
    assert cc(p, 4, 0, 4, 3, q, p, p, None) == -1 and b"positive" in lib.gens_last_error()
    assert cc(p, -1, 4, 4, 3, q, p, p, None) == -1 and b"positive" in lib.gens_last_error()
    assert cc(p, 2048, 1024, 1024, 3, q, p, p, None) == -2 and b"2^31" in lib.gens_last_error()
    assert cc(p, 65536, 65536, 1, 3, q, p, p, None) == -2 and b"2^31" in lib.gens_last_error()
    assert cc(p, 4, 4, 4, 2, q, p, p, None) == -1 and b"connectivity = 2" in lib.gens_last_error()
    assert cc(odd, 4, 4, 4, 3, q, p, p, None) == -1 and b"misaligned" in lib.gens_last_error()
    assert cc(p, 4, 4, 4, 1, q, C.c_void_p(68), p, None) == -1 and b"misaligned" in lib.gens_last_error()
    assert cc(p, 4, 4, 4, 1, q, p, C.c_void_p(68), None) == -1 and b"misaligned" in lib.gens_last_error()
    assert cc(p, 4, 4, 4, 3, p, p, p, None) == -1 and b"bits_in" in lib.gens_last_error()
    assert lib.gens_components_scratch_bytes(256, 256, 256) == 16 + 4 * 256 ** 3
    assert lib.gens_components_scratch_bytes(5, 7, 3) == 16 + 4 * 105
    assert lib.gens_components_scratch_bytes(0, 7, 3) == 0 and lib.gens_components_scratch_bytes(2048, 1024, 1024) == 0
    assert lib.gens_unpack_mask_bits(None, 8, p, None) == -1 and b"null" in lib.gens_last_error()
    assert lib.gens_unpack_mask_bits(p, 0, p, None) == -1 and b"n = 0" in lib.gens_last_error()
    assert lib.gens_unpack_mask_bits(odd, 8, p, None) == -1 and b"misaligned" in lib.gens_last_error()
    # K26's two launches one at a time: the checks of gens_filter_masks
    tab = C.cast((C.c_void_p * 3)(64, 64, 64), C.POINTER(C.c_void_p))
    assert lib.gens_filter_band(None, 0.1, 16, p, p, None) == -1 and b"null" in lib.gens_last_error()
    assert lib.gens_filter_band(p, 0.1, 0, p, p, None) == -1 and b"d0 = 0" in lib.gens_last_error()
    assert lib.gens_filter_band(odd, 0.1, 16, p, p, None) == -1 and b"misaligned" in lib.gens_last_error()
    assert lib.gens_filter_levels(None, None, None, None, 1, None, None, None) == -1 and b"null" in lib.gens_last_error()
    assert lib.gens_filter_levels(tab, tab, tab, L.int_table([8] * 9), 9, p, p, None) == -2 and b"GENS_MAX_LEVELS" in lib.gens_last_error()
    assert lib.gens_filter_levels(tab, tab, tab, L.int_table([16, 8, 3]), 3, p, p, None) == -1 and b"dims[2]" in lib.gens_last_error()
    assert lib.gens_filter_levels(tab, tab, tab, L.int_table([16, 8, 4]), 3, None, p, None) == -1 and b"null" in lib.gens_last_error()
    assert lib.gens_filter_levels(tab, tab, tab, L.int_table([16, 8, 4]), 3, odd, p, None) == -1 and b"misaligned" in lib.gens_last_error()
    assert lib.gens_abi_version() == 12


def test_the_surface_k26_had_is_still_accepted():
    from gens_amd import ops
    from gens_amd.config import Conf, gens_model_conf
    from gens_amd.models.gens import GenS
    m = lambda *ds: [torch.ones(1, 1, d, d, d) for d in ds]  # noqa: E731
    assert ops.filter_mask_dims((16, 16, 16), [t.shape for t in m(16, 8, 4)]) == [16, 8, 4]
    assert ops.filter_mask_dims((20, 20, 20), [t.shape for t in m(20, 10, 5)]) == [20, 10, 5]
    sig = inspect.signature(ops.filter_masks)
    assert list(sig.parameters) == ["u", "masks", "thresh", "return_band", "keep_largest"]
    assert sig.parameters["return_band"].default is False and sig.parameters["keep_largest"].default is False
    assert list(inspect.signature(ops.largest_component).parameters) == ["mask", "connectivity", "return_info"]
    assert inspect.signature(ops.largest_component).parameters["connectivity"].default == 3
    assert list(inspect.signature(ops.clean_volume).parameters) == ["mask_volume"]
    assert "label number" in ops.clean_volume.__doc__.lower()
    # the model: attribute, conf key and init_volumes' keyword, off by default
    assert GenS.filter_keep_largest is False
    assert "filter_keep_largest" in inspect.signature(GenS.init_volumes).parameters
    conf = gens_model_conf(volume_dims=(16, 8, 4))
    assert GenS(conf).filter_keep_largest is False and "filter_keep_largest" not in vars(GenS(conf))
    assert GenS(Conf({**conf, "filter_keep_largest": True})).filter_keep_largest is True
