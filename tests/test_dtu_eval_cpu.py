"""The float64 restatement of evaluation/dtu_eval.py (tests/dtu_eval_reference.py) against golden g20 -- the reference's own script run
on the 15 synthetic scans -- and against sklearn; K24's argument checks.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dtu_eval_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = ("n_sampled", "n_down", "n_in", "n_in_obs", "n_stl_above")


def ulps(a, b):
    """|a - b| in units of the last place of b (float64)."""
    return np.abs(a - b) / np.spacing(np.abs(b))


@pytest.fixture(scope="module")
def g20():
    return np.load(os.path.join(ROOT, "tests", "golden", "g20_dtu_eval.npz"))


@pytest.fixture(scope="module")
def restated():
    """The restatement on all 15 scans (its conditions -- no l / thr within 1e-9 of an integer, no |d^2 - r^2| <= 1e-9 r^2 -- are asserted
    inside, for every scan)."""
    return [R.dtu_chamfer(R.make_scan(k), rng=np.random.default_rng(R.SHUFFLE_SEED + k)) for k in range(15)]


def test_golden_parameters_are_the_restatements(g20):
    assert tuple(g20["scan_ids"]) == R.SCAN_IDS and int(g20["shuffle_seed"]) == R.SHUFFLE_SEED
    assert (float(g20["density"]), float(g20["patch"]), float(g20["max_dist"])) == (R.DENSITY, R.PATCH, R.MAX_DIST)


def test_restatement_reproduces_the_scripts_counts_and_triples(g20, restated):
    for k, r in enumerate(restated):
        print(R.SCAN_IDS[k], [r[c] for c in COUNTS], r["d2s"], r["s2d"], r["overall"])
        assert [r[c] for c in COUNTS] == g20["counts"][k].tolist()
        got = np.array([r["d2s"], r["s2d"], r["overall"]])
        # float64 means of <= 3e4 terms in another summation order: n 2^-53 ~ 3e-12, plus margin
        assert (np.abs(got - g20["triples"][k]) <= 1e-10 * np.abs(g20["triples"][k])).all(), (k, got, g20["triples"][k])
    means = np.array([[r["d2s"], r["s2d"], r["overall"]] for r in restated]).mean(0)
    assert (np.abs(means - g20["final"]) <= 1e-10 * np.abs(g20["final"])).all()


def test_restatement_reproduces_the_last_scans_intermediates(g20, restated):
    r = restated[-1]
    assert np.array_equal(r["data_down"], g20["last_data_down"])                     # bit for bit, in order
    assert np.array_equal(r["inbound"], g20["last_inbound"]) and np.array_equal(r["in_obs"], g20["last_in_obs"])
    assert np.array_equal(r["above"], g20["last_above"])
    for name in ("dist_d2s", "dist_s2d"):
        worst = ulps(r[name], g20["last_" + name]).max()
        print(name, "worst ulp", worst)
        assert worst <= 4


def test_the_special_scans_exercise_what_they_claim(restated):
    s3 = R.make_scan(3)
    tv = s3["vertices"][s3["triangles"][-2:].astype(np.int64)]
    assert (np.linalg.norm(np.cross(tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0]), axis=-1) == 0).all()          # zero area, distinct vertices / a repeated index
    s5 = R.make_scan(5)
    assert len(np.unique(s5["vertices"], axis=0)) <= len(s5["vertices"]) - 40                                # duplicate vertices
    r7 = restated[7]
    assert r7["n_in"] < r7["n_down"]                                                                          # part of the mesh fails `inbound`
    s7 = R.make_scan(7)
    grid = np.around((r7["data_in"] - s7["BB"].astype(np.float32)[:1]) / s7["Res"])
    assert (grid >= R.OBS_N).any()                                                                            # ... and part lies outside the ObsMask array
    r9 = restated[9]
    assert (r9["dist_s2d"] >= R.MAX_DIST).any() and (r9["dist_d2s"] >= R.MAX_DIST).any()                      # beyond the cap, both ways


def test_sampling_restatement_on_the_equality_lattice():
    """n1 = n2 = 2: the lattice sums 0.25 + 0.25, 0.25 + 0.75 (= 1, excluded), 0.75 + 0.25 (= 1, excluded): one point."""
    v = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.0, 0.5, 0.0]])
    pts = R.sample_mesh_points(v, np.array([[0, 1, 2]]), 0.2)
    assert len(pts) == 3 + 1 and np.array_equal(pts[3], [0.125, 0.125, 0.0])


def test_restatement_agrees_with_sklearn():
    skln = pytest.importorskip("sklearn.neighbors")
    rng = np.random.default_rng(5)
    scan = R.make_scan(2)
    pts = R.sample_mesh_points(scan["vertices"], scan["triangles"], R.DENSITY)
    rng.shuffle(pts, axis=0)
    nn = skln.NearestNeighbors(n_neighbors=1, radius=R.DENSITY, algorithm="kd_tree")
    nn.fit(pts)
    mask = np.ones(len(pts), dtype=np.bool_)
    for curr, idxs in enumerate(nn.radius_neighbors(pts, radius=R.DENSITY, return_distance=False)):      # dtu_eval.py:96-101
        if mask[curr]:
            mask[idxs] = 0
            mask[curr] = 1
    assert np.array_equal(R.greedy_downsample(pts, R.DENSITY), mask)
    order = rng.permutation(len(pts))
    mask_o = np.ones(len(pts), dtype=np.bool_)
    nbrs = nn.radius_neighbors(pts, radius=R.DENSITY, return_distance=False)
    for curr in order:
        if mask_o[curr]:
            mask_o[nbrs[curr]] = 0
            mask_o[curr] = 1
    assert np.array_equal(R.greedy_downsample(pts, R.DENSITY, order=order), mask_o)
    nn.fit(scan["stl"])
    dist, idx = nn.kneighbors(pts[mask], n_neighbors=1, return_distance=True)
    d, i, uniq = R.nearest(pts[mask], scan["stl"])
    assert ulps(d, dist[:, 0]).max() <= 4
    assert np.array_equal(i[uniq], idx[uniq, 0])


def test_read_ply_reads_point_clouds_with_extra_properties(tmp_path):
    from gens_amd import io
    rng = np.random.default_rng(0)
    rows = np.zeros(50, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("red", "u1"),
                               ("green", "u1"), ("blue", "u1")])
    xyz = rng.standard_normal((50, 3)).astype(np.float32)
    rows["x"], rows["y"], rows["z"], rows["red"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], 7
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex 50\nproperty float x\nproperty float y\nproperty float z\n"
              "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    path = str(tmp_path / "cloud.ply")
    with open(path, "wb") as f:
        f.write(header.encode("ascii") + rows.tobytes())
    v, t = io.read_ply(path)
    assert v.dtype == np.float32 and np.array_equal(v, xyz) and t.shape == (0, 3)
    tri = np.array([[0, 1, 2], [2, 1, 3]], dtype=np.int32)                        # meshes read as before
    io.write_ply(str(tmp_path / "mesh.ply"), xyz, tri)
    v, t = io.read_ply(str(tmp_path / "mesh.ply"))
    assert v.dtype == np.float32 and t.dtype == np.int32 and np.array_equal(v, xyz) and np.array_equal(t, tri)


def test_k24_entries_validate_their_arguments_without_a_gpu():
    import ctypes as C
    from gens_amd import lib as L
    lib = L.load()
    assert lib.gens_abi_version() == 12
    assert lib.gens_mesh_sample_count(None, 3, None, 1, 0.2, None, None) == -1 and b"null" in lib.gens_last_error()
    one = C.c_void_p(8)                                       # a non-null pointer that is never dereferenced: every call below fails its checks
    assert lib.gens_mesh_sample_count(one, -1, one, 1, 0.2, one, None) == -1
    assert lib.gens_mesh_sample_count(one, 3, one, 1, 0.0, one, None) == -1 and b"density" in lib.gens_last_error()
    assert lib.gens_mesh_sample_emit(one, 3, one, 1, float("nan"), one, 1, one, None) == -1
    assert lib.gens_mesh_sample_emit(one, 3, one, 1, 0.2, None, 1, one, None) == -1
    assert lib.gens_mesh_sample_emit(one, 3, one, 1, 0.2, one, -1, one, None) == -1

    def grid(n=4, cell=1.0, dims=(2, 2, 2), points=8, filled=8):
        return L.PointGridArgs(points, filled, filled, filled, n, 0.0, 0.0, 0.0, cell, *dims)
    assert lib.gens_point_grid_count(None, one, None) == -1
    assert lib.gens_point_grid_count(C.byref(grid(points=None)), one, None) == -1 and b"null" in lib.gens_last_error()
    assert lib.gens_point_grid_count(C.byref(grid(n=-1)), one, None) == -1
    assert lib.gens_point_grid_count(C.byref(grid(cell=0.0)), one, None) == -1
    assert lib.gens_point_grid_count(C.byref(grid(dims=(2048, 2048, 2048))), one, None) == -2
    assert lib.gens_point_grid_fill(C.byref(grid(filled=None)), one, None) == -1
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.gens_radius_downsample_round(C.byref(grid()), one, bad, one, C.c_void_p(16), one, None) == -1 and b"radius" in lib.gens_last_error()
    assert lib.gens_radius_downsample_round(C.byref(grid()), None, 0.5, one, C.c_void_p(16), one, None) == -1
    assert lib.gens_radius_downsample_round(C.byref(grid()), one, 0.5, one, one, one, None) == -1              # one buffer for both states
    assert lib.gens_radius_downsample_round(C.byref(grid()), one, 1.5, one, C.c_void_p(16), one, None) == -2    # radius > cell
    assert lib.gens_nearest_point(C.byref(grid()), one, -1, 1.0, one, one, None) == -1
    assert lib.gens_nearest_point(C.byref(grid()), one, 1, 0.0, one, one, None) == -1 and b"max_dist" in lib.gens_last_error()
    assert lib.gens_nearest_point(C.byref(grid()), None, 1, 1.0, one, one, None) == -1


def test_operators_refuse_cpu_tensors():
    import torch
    from gens_amd import ops
    with pytest.raises(RuntimeError):
        ops.sample_mesh_points(torch.zeros(3, 3, dtype=torch.float64), torch.zeros(1, 3, dtype=torch.int32), 0.2)
    with pytest.raises(RuntimeError):
        ops.radius_downsample(torch.zeros(3, 3, dtype=torch.float64), 0.2)
    with pytest.raises(RuntimeError):
        ops.nearest_distance(torch.zeros(3, 3, dtype=torch.float64), torch.zeros(3, 3, dtype=torch.float64), 1.0)
