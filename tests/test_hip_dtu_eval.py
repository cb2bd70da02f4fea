"""K24 on the MI355X: mesh sampling, radius down-sampling and capped nearest neighbours against the float64 restatement of
evaluation/dtu_eval.py (tests/dtu_eval_reference.py), and gens_amd.evaluation.dtu_chamfer end to end against golden g20 (the reference's
own script on the 15 synthetic scans).  The restatement asserts the conditions that make exact comparisons meaningful."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dtu_eval_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
COUNTS = ("n_sampled", "n_down", "n_in", "n_in_obs", "n_stl_above")


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV).to(dtype)


def ulps(a, b):
    return np.abs(a - b) / np.spacing(np.abs(b))


@pytest.fixture(scope="module")
def g20():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "g20_dtu_eval.npz"))


# ------------------------------------------------------------------------------------------------------------------ sampling
def _sample_check(v, t, density=R.DENSITY, check=True):
    from gens_amd import ops
    want = R.sample_mesh_points(v, t, density, check=check)
    got = ops.sample_mesh_points(dev(v), dev(t, torch.int32), density).cpu().numpy()
    print("sampled", len(want), "got", len(got))
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.int64), want.view(np.int64))                  # bit-equal, in order
    return want


@pytest.mark.parametrize("k", [0, 3, 5, 7, 14])
def test_sampling_is_bit_equal_on_the_g20_scans(k):
    s = R.make_scan(k)
    _sample_check(s["vertices"], s["triangles"])


def test_sampling_special_triangles():
    rng = np.random.default_rng(11)
    v = [[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.0, 0.5, 0.0],                 # n1 = n2 = 2: 0.75 + 0.25 == 1 exactly, excluded
         [10.0, 0.0, 0.0], [10.05, 0.0, 0.0], [10.0, 0.07, 0.0],            # smaller than the lattice: n1 = n2 = 0
         [20.0, 0.0, 0.0], [23.03, 0.0, 0.0], [20.0, 0.011, 0.0],            # slivers: one edge long, the other below the threshold
         [30.0, 0.0, 0.0], [30.0, 0.013, 0.0], [34.0, 0.0, 1.0],
         [40.0, 0.0, 0.0], [43.0, 0.001, 0.0], [46.0, 0.003, 0.0],          # a needle: both edges long, the area tiny
         [50.0, 1.0, 2.0], [50.0, 1.0, 2.0], [51.0, 1.0, 2.0],              # zero area: coincident vertices
         [60.0, 0.0, 0.0], [61.0, 1.0, 1.0], [62.0, 2.0, 2.0]]              # zero area: collinear
    v = np.array(v)
    t = np.arange(len(v)).reshape(-1, 3)
    pts = _sample_check(v, t)
    assert len(pts) > len(v)
    only_first = _sample_check(v[:3], t[:1])
    assert len(only_first) == 3 + 1                                          # (0.25, 0.25) alone survives `< 1`
    # the equality lattice at other scales and orientations, and generic triangles of many sizes
    vs, ts = [], []
    for i in range(200):
        a = rng.standard_normal(3) * 50
        e1, e2 = rng.standard_normal(3), rng.standard_normal(3)
        size = 10.0 ** rng.uniform(-1.5, 0.8)
        vs += [a, a + size * e1, a + size * e2]
        ts.append([3 * i, 3 * i + 1, 3 * i + 2])
    _sample_check(np.array(vs), np.array(ts))
    for scale in (0.25, 1.0, 3.0):                                           # isosceles right triangles: l1 == l2, so n1 == n2 and the sums hit 1
        _sample_check(v[:3] * scale, t[:1])
        _sample_check(v[:3] * scale, t[:1], density=0.2 * scale)


def test_sampling_empty_and_refused():
    from gens_amd import ops
    v = dev(np.zeros((4, 3)))
    out = ops.sample_mesh_points(v, torch.zeros(0, 3, device=DEV, dtype=torch.int32), 0.2)
    assert out.shape == (4, 3)
    assert ops.sample_mesh_points(v[:0], torch.zeros(0, 3, device=DEV, dtype=torch.int32), 0.2).shape == (0, 3)
    with pytest.raises(ValueError):
        ops.sample_mesh_points(v, torch.tensor([[0, 1, 4]], device=DEV, dtype=torch.int32), 0.2)
    big = dev(np.array([[0.0, 0.0, 0.0], [1e9, 0.0, 0.0], [0.0, 1e9, 0.0]]))
    with pytest.raises(RuntimeError):
        ops.sample_mesh_points(big, torch.tensor([[0, 1, 2]], device=DEV, dtype=torch.int32), 0.2)


# ------------------------------------------------------------------------------------------------------------------ down-sampling
def _downsample_check(points, radius, order=None):
    from gens_amd import ops
    want = R.greedy_downsample(points, radius, order=order, device=DEV)
    o = None if order is None else torch.as_tensor(order, device=DEV)
    got = ops.radius_downsample(dev(points), radius, o)
    again = ops.radius_downsample(dev(points), radius, o)
    print("points", len(points), "kept", int(want.sum()), "rounds", ops.points.last_downsample_rounds)
    assert got.dtype == torch.bool and torch.equal(got, again)                       # two calls: identical
    assert np.array_equal(got.cpu().numpy(), want), int((got.cpu().numpy() != want).sum())
    return want


@pytest.mark.parametrize("k", range(15))
def test_downsampling_equals_the_sequential_greedy_on_the_g20_scans(k):
    s = R.make_scan(k)
    pts = R.sample_mesh_points(s["vertices"], s["triangles"], R.DENSITY)
    np.random.default_rng(R.SHUFFLE_SEED + k).shuffle(pts, axis=0)
    _downsample_check(pts, R.DENSITY)


def test_downsampling_with_an_explicit_order():
    s = R.make_scan(1)
    pts = R.sample_mesh_points(s["vertices"], s["triangles"], R.DENSITY)
    order = np.random.default_rng(3).permutation(len(pts))
    mask = _downsample_check(pts, R.DENSITY, order)
    assert np.array_equal(mask[order], R.greedy_downsample(pts[order], R.DENSITY, device=DEV))


def test_downsampling_worst_case_chain():
    """A line visited in spatial order: every decision waits for the one before it (as many rounds as points)."""
    x = 300.0 + 0.07 * np.arange(1500) + 0.003 * np.random.default_rng(2).standard_normal(1500)
    pts = np.stack([x, np.full_like(x, -120.5), np.full_like(x, 640.25)], -1)
    mask = _downsample_check(pts, 0.2)
    assert 400 < mask.sum() < 600


def test_downsampling_duplicates_boundaries_negative_and_far_clouds():
    rng = np.random.default_rng(4)
    base = rng.uniform(-1.0, 1.0, (3000, 3))
    dup = np.concatenate([base, base[:500], base[:100]], 0)                         # duplicates at distance 0
    mask = _downsample_check(dup, 0.11, rng.permutation(len(dup)))
    assert mask.sum() < len(base)
    # points on cell boundaries (multiples of the radius, a dyadic one so that they are exact) at negative coordinates
    r = 0.125
    ij = np.stack(np.meshgrid(np.arange(-12, 12), np.arange(-12, 12), np.arange(-2, 2), indexing="ij"), -1).reshape(-1, 3)
    lattice = ij * (r * 0.75) + np.array([-3.0, -7.0, -1.0])
    _downsample_check(np.concatenate([lattice, lattice + rng.uniform(-0.02, 0.02, lattice.shape)], 0), r, rng.permutation(2 * len(lattice)))
    # DTU coordinates are hundreds of mm: a cloud far from the origin (float32 would not resolve the radius test there)
    far = R.f32(base * 3.0) + np.array([412.0, -388.0, 655.0])
    _downsample_check(far, 0.2, rng.permutation(len(far)))
    _downsample_check(far + 5e4, 0.2)


def test_downsampling_empty_single_and_bad_arguments():
    from gens_amd import ops
    assert ops.radius_downsample(torch.zeros(0, 3, device=DEV, dtype=torch.float64), 0.2).shape == (0,)
    assert ops.radius_downsample(torch.zeros(1, 3, device=DEV, dtype=torch.float64), 0.2).tolist() == [True]
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            ops.radius_downsample(torch.zeros(2, 3, device=DEV, dtype=torch.float64), bad)
    with pytest.raises(ValueError):
        ops.radius_downsample(torch.zeros(3, 3, device=DEV, dtype=torch.float64), 0.2, torch.tensor([0, 0, 1], device=DEV))


# ------------------------------------------------------------------------------------------------------------------ nearest neighbour
def _nearest_check(q, t, max_dist=float("inf")):
    from gens_amd import ops
    want_d, want_i, uniq = R.nearest(q, t, max_dist, device=DEV)
    d, i = ops.nearest_distance(dev(q), dev(t), max_dist)
    d, i = d.cpu().numpy(), i.cpu().numpy()
    far = np.isinf(want_d)
    assert np.array_equal(np.isinf(d), far) and (i[far] == -1).all()
    worst = ulps(d[~far], want_d[~far]).max() if (~far).any() else 0.0
    print("queries", len(q), "targets", len(t), "beyond the cap", int(far.sum()), "worst ulp", worst, "unique", int(uniq.sum()))
    assert worst <= 4
    assert np.array_equal(i[uniq], want_i[uniq])
    return d, i


def test_nearest_on_a_g20_scan_both_ways():
    s = R.make_scan(9)
    pts = R.sample_mesh_points(s["vertices"], s["triangles"], R.DENSITY)
    d, _ = _nearest_check(pts, s["stl"], R.MAX_DIST)
    assert np.isinf(d).any()                                                        # the back of the sphere has no scan points within the cap
    d, _ = _nearest_check(s["stl"], pts, R.MAX_DIST)
    assert np.isinf(d).any()                                                        # the far cluster
    _nearest_check(pts[::7], s["stl"])                                              # no cap: every query finds its target


def test_nearest_ties_single_target_and_outside_queries():
    rng = np.random.default_rng(6)
    t = rng.uniform(-2.0, 2.0, (4000, 3)) + np.array([300.0, -200.0, 600.0])
    t = np.concatenate([t, t[:300]], 0)                                             # equal distances: the smaller index must win
    q = np.concatenate([t[:600] + rng.uniform(-0.05, 0.05, (600, 3)), t[100:200]], 0)
    want_d, want_i, uniq = R.nearest(q, t, device=DEV)
    from gens_amd import ops
    d, i = ops.nearest_distance(dev(q), dev(t))
    assert np.array_equal(i.cpu().numpy(), want_i)                                  # ties included: R.nearest reports the first index
    assert ulps(d.cpu().numpy()[want_d > 0], want_d[want_d > 0]).max() <= 4 and (d.cpu().numpy()[want_d == 0] == 0).all()
    assert not uniq.all()
    one = np.array([[1.5, -2.5, 3.5]])
    _nearest_check(rng.uniform(-5, 5, (500, 3)), one)
    _nearest_check(rng.uniform(-5, 5, (500, 3)), one, 4.0)
    outside = np.concatenate([t[:50] + np.array([30.0, 0.0, 0.0]), t[:50] - np.array([0.0, 8.0, 9.0]), t[:50] * 3.0], 0)
    _nearest_check(outside, t)
    _nearest_check(outside, t, 12.0)
    _nearest_check(outside, t, 0.5)


def test_nearest_empty_inputs():
    from gens_amd import ops
    z = torch.zeros(0, 3, device=DEV, dtype=torch.float64)
    p = torch.zeros(5, 3, device=DEV, dtype=torch.float64)
    d, i = ops.nearest_distance(z, p, 1.0)
    assert d.shape == (0,) and i.shape == (0,)
    d, i = ops.nearest_distance(p, z, 1.0)
    assert torch.isinf(d).all() and (i == -1).all()
    with pytest.raises(ValueError):
        ops.nearest_distance(p, p, 0.0)


# ------------------------------------------------------------------------------------------------------------------ end to end
def _chamfer(scan, k, **kw):
    from gens_amd import evaluation
    return evaluation.dtu_chamfer(dev(scan["vertices"]), dev(scan["triangles"], torch.int64), dev(scan["stl"]), scan["ObsMask"], scan["BB"],
                                  scan["Res"], scan["P"], density=R.DENSITY, patch=R.PATCH, max_dist=R.MAX_DIST,
                                  rng=np.random.default_rng(R.SHUFFLE_SEED + k), **kw)


def _close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return bool((np.abs(got - want) <= 1e-10 * np.abs(want)).all())


@pytest.mark.parametrize("k", range(15))
def test_dtu_chamfer_matches_the_script_on_every_scan(g20, k):
    r = _chamfer(R.make_scan(k), k)
    print(R.SCAN_IDS[k], [r[c] for c in COUNTS], r["d2s"], r["s2d"], r["overall"], "golden", g20["triples"][k].tolist())
    assert [r[c] for c in COUNTS] == g20["counts"][k].tolist()
    assert _close([r["d2s"], r["s2d"], r["overall"]], g20["triples"][k])


def test_dtu_chamfer_pcd_mode_is_the_mesh_mode_on_its_samples(g20):
    from gens_amd import evaluation
    k = 4
    s = R.make_scan(k)
    pts = R.sample_mesh_points(s["vertices"], s["triangles"], R.DENSITY)
    r = evaluation.dtu_chamfer(None, None, dev(s["stl"]), s["ObsMask"], s["BB"], s["Res"], s["P"], points=dev(pts), density=R.DENSITY,
                               patch=R.PATCH, max_dist=R.MAX_DIST, rng=np.random.default_rng(R.SHUFFLE_SEED + k))
    assert r == _chamfer(s, k)
    assert _close([r["d2s"], r["s2d"], r["overall"]], g20["triples"][k])


def test_dtu_chamfer_empty_selection_is_nan():
    s = dict(R.make_scan(0))
    s["ObsMask"] = np.zeros_like(s["ObsMask"])
    r = _chamfer(s, 0)
    assert r["n_in_obs"] == 0 and np.isnan(r["d2s"]) and np.isnan(r["overall"]) and np.isfinite(r["s2d"])


def test_command_line_prints_the_scripts_lines(g20, tmp_path, capsys):
    scipy_io = pytest.importorskip("scipy.io")
    from gens_amd import evaluation, io

    class SeededOnce:
        """evaluate_dtu's rng for all scans in turn: scan k is shuffled by default_rng(SHUFFLE_SEED + k), as in the generator."""
        k = -1

        def permutation(self, n):
            self.k += 1
            return np.random.default_rng(R.SHUFFLE_SEED + self.k).permutation(n)

    out, data = tmp_path / "out", tmp_path / "data"
    os.makedirs(out / "meshes" / "final")
    os.makedirs(data / "ObsMask")
    os.makedirs(data / "Points" / "stl")
    for k, n in enumerate(R.SCAN_IDS):
        s = R.make_scan(k)
        io.write_ply(str(out / "meshes" / "final" / f"scan{n}.ply"), s["vertices"], s["triangles"])
        io.write_ply(str(data / "Points" / "stl" / f"stl{n:03}_total.ply"), s["stl"], np.zeros((0, 3), dtype=np.int32))
        scipy_io.savemat(str(data / "ObsMask" / f"ObsMask{n}_10.mat"), {"ObsMask": s["ObsMask"], "BB": s["BB"], "Res": s["Res"]})
        scipy_io.savemat(str(data / "ObsMask" / f"Plane{n}.mat"), {"P": s["P"]})
    res = evaluation.evaluate_dtu(str(out), str(data), density=R.DENSITY, patch=R.PATCH, max_dist=R.MAX_DIST, rng=SeededOnce())
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 17 and lines[15] == "final result"
    for k, n in enumerate(R.SCAN_IDS):
        words = lines[k].split()
        assert int(words[0]) == n and _close([float(w) for w in words[1:]], g20["triples"][k])
    assert _close([float(w) for w in lines[16].split()], g20["final"]) and _close([res["d2s"], res["s2d"], res["overall"]], g20["final"])
    # the argument names of the script, through the module's entry point (a fresh generator shuffles: the counts move, the format does not)
    evaluation.main(["--out_dir", str(out), "--dataset_dir", str(data), "--downsample_density", str(R.DENSITY), "--patch_size", str(R.PATCH),
                     "--max_dist", str(R.MAX_DIST), "--mode", "mesh"])
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 17 and lines[15] == "final result" and [int(line.split()[0]) for line in lines[:15]] == list(R.SCAN_IDS)
    assert all(len(line.split()) == 4 for line in lines[:15]) and len(lines[16].split()) == 3
