"""K23 (ray-cast mesh cleaning) without a GPU: the new entry points check their arguments before any launch, the ctypes table covers them,
and the float64 restatement's `values[1:]` logic (utils/clean_mesh.py:79-92) on hand-built hit lists."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_clean_reference as R  # noqa: E402

NEW = ("gens_mesh_grid_count", "gens_mesh_grid_fill", "gens_ray_first_hit", "gens_view_rays_hit_faces", "gens_face_cc_hook",
       "gens_face_cc_compress")


@pytest.fixture(scope="module")
def lib():
    from gens_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("libgens_hip.so is not built")
    return L.load()


def _grid(L, null=False, **kw):
    fake = None if null else C.c_void_p(0x7E0000000000)
    g = L.MeshGridArgs(fake, fake, fake, fake, 100, 0.0, 0.0, 0.0, 0.5, 4, 4, 4)
    for k, v in kw.items():
        setattr(g, k, v)
    return C.byref(g)


def test_new_names_are_in_the_ctypes_table():
    from gens_amd import lib as L
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gens_hip.h")).read()
    for name in NEW:
        assert name + "(" in header and name in L.SIGNATURES


def test_mesh_cull_entry_points_reject_bad_arguments_without_a_gpu(lib):
    from gens_amd import lib as L
    p = C.c_void_p(0x7E0000001000)
    assert lib.gens_mesh_grid_count(None, p, None) == -1
    assert lib.gens_mesh_grid_count(_grid(L, null=True), p, None) == -1
    assert lib.gens_mesh_grid_count(_grid(L), None, None) == -1
    for bad in (dict(nx=0), dict(ny=513), dict(nz=-1), dict(n_faces=-1), dict(n_faces=(1 << 31) + 5), dict(cell=0.0), dict(cell=float("nan")),
                dict(lo_x=float("inf"))):
        assert lib.gens_mesh_grid_fill(_grid(L, **bad), p, None) == -2, bad
    assert lib.gens_mesh_grid_fill(_grid(L, cell_faces=None), p, None) == -1
    assert lib.gens_ray_first_hit(_grid(L), None, p, 10, p, p, None) == -1
    assert lib.gens_ray_first_hit(_grid(L), p, p, -1, p, p, None) == -2
    assert lib.gens_ray_first_hit(_grid(L), p, p, (1 << 31) + 5, p, p, None) == -2
    assert lib.gens_ray_first_hit(_grid(L), p, p, 0, p, p, None) == 0                  # nothing to do: no launch
    assert lib.gens_view_rays_hit_faces(_grid(L), p, None, 3, 48, 64, 96, 128, 0.5, p, p, None) == -1
    for nv, h, w, hu, wu, s in ((0, 48, 64, 96, 128, 0.5), (3, 0, 64, 96, 128, 0.5), (3, 48, 64, 1 << 20, 1 << 20, 0.5), (3, 48, 64, 96, 128, 0.0),
                                (3, 48, 64, 96, -1, 0.5), (3, 48, 64, 96, 128, float("nan"))):
        assert lib.gens_view_rays_hit_faces(_grid(L), p, p, nv, h, w, hu, wu, s, p, p, None) == -2
    assert lib.gens_face_cc_hook(None, 10, p, 10, None) == -1
    assert lib.gens_face_cc_hook(p, -1, p, 10, None) == -2
    assert lib.gens_face_cc_hook(p, 10, p, (1 << 31) + 5, None) == -2
    assert lib.gens_face_cc_compress(p, 10, None, None) == -1
    assert lib.gens_face_cc_compress(p, -1, p, None) == -2
    assert b"gens_face_cc_compress" in lib.gens_last_error()


def test_values_quirk_drops_the_first_sorted_entry():
    # some masked ray missed: -1 heads the sorted list and is the entry dropped; every hit face stays
    assert R.values_after_quirk([np.array([-1, 7, 3]), np.array([3, 2])]).tolist() == [2, 3, 7]
    # no masked ray missed: the smallest face index hit is dropped
    assert R.values_after_quirk([np.array([7, 3]), np.array([3, 2])]).tolist() == [3, 7]
    assert R.values_after_quirk([np.array([5])]).tolist() == []
    # no hits at all: nothing, with or without misses
    assert R.values_after_quirk([np.array([], dtype=np.int64), np.array([-1])]).tolist() == []
    assert R.values_after_quirk([np.array([], dtype=np.int64)]).tolist() == []


def test_restatement_adjacency_is_exactly_two_faces():
    # faces 0-1 share edge (1,2); faces 2, 3, 4 share edge (2,4): three faces, no adjacency there; face 1-2 share edge (2,3)
    tri = np.array([[0, 1, 2], [1, 3, 2], [2, 3, 4], [2, 4, 5], [2, 4, 6]])
    assert sorted(map(tuple, R.face_adjacency(tri).tolist())) == [(0, 1), (1, 2)]
    keep = R.large_components_keep(R.face_adjacency(tri), len(tri), 1)
    assert keep.tolist() == [True, True, True, False, False]                # faces without a neighbour are in no component
    # a face with a repeated vertex uses its edge (0, 1) twice: no pair of the face with itself (trimesh drops it)
    assert R.face_adjacency(np.array([[0, 0, 1], [2, 3, 4], [3, 2, 5]])).tolist() == [[1, 2]]


def test_frustum_step_without_the_mask_step_is_rejected(tmp_path):
    from gens_amd import io
    with pytest.raises(ValueError):
        io.save_validation_outputs(str(tmp_path), {}, {}, "epoch0", clean=False, clean_frustum=True)
    assert list(tmp_path.iterdir()) == []
