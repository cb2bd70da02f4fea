"""K25 on the MI355X: the dilation bit for bit, the vertex votes, the per-view ray flags against the float64 brute force, both functions and
finalize_dtu_meshes against golden g21 (the reference's own script at 1200 x 1600) and against the restatement of
tests/dtu_clean_reference.py on small seeded scans, the chain into the scorer, and a full-size run (1200 x 1600, three views, a 512^3 marching-cubes mesh)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dtu_clean_reference as R  # noqa: E402
import mesh_clean_reference as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CAP = 0.005             # the share of a population that may be left out of an exact comparison


def _dilate_check(img, k, channels=None):
    from gens_amd import ops
    got = ops.dilate_u8(torch.from_numpy(img).to(DEV), ops.opencv_ellipse(k, k), k, channels=channels).cpu().numpy()
    fp = R.ellipse_footprint(k, k)
    want = np.stack([R.dilate(m, fp) for m in img])
    if channels is not None:
        want = want[..., :channels]
    assert got.shape == want.shape and np.array_equal(got, want), (img.shape, k, int((got != want).sum()))


@pytest.mark.parametrize("k", [3, 5, 11, 31])
def test_dilate_u8_is_bit_equal_to_the_definition(k):
    rng = np.random.default_rng(k)
    _dilate_check(rng.integers(0, 256, (2, 37, 53, 1), dtype=np.uint8), k)
    _dilate_check(rng.integers(0, 256, (1, 37, 53), dtype=np.uint8), k)
    _dilate_check(rng.integers(0, 256, (3, 1, 1, 1), dtype=np.uint8), k)
    _dilate_check(rng.integers(0, 256, (1, 70, 131, 3), dtype=np.uint8), k)
    _dilate_check(rng.integers(0, 256, (1, 70, 131, 3), dtype=np.uint8), k, channels=1)
    _dilate_check(np.zeros((1, 40, 70, 3), dtype=np.uint8), k)
    _dilate_check(np.full((1, 40, 70, 3), 255, dtype=np.uint8), k)
    corners = np.zeros((4, 33, 65, 1), dtype=np.uint8)                  # a single set pixel in each corner: the border rule
    for n, (y, x) in enumerate([(0, 0), (0, 64), (32, 0), (32, 64)]):
        corners[n, y, x, 0] = 200 + n
    _dilate_check(corners, k)


@pytest.mark.parametrize("k", [11, 31])
def test_dilate_u8_full_size(k):
    rng = np.random.default_rng(100 + k)
    img = rng.integers(0, 256, (1, 1200, 1600, 3), dtype=np.uint8)
    img[rng.random((1, 1200, 1600, 3)) < 0.9] = 0                        # sparse maxima: every tap matters somewhere
    _dilate_check(img, k)


def _random_cameras(rng, n=3, W=1600, H=1200):
    E = np.stack([R.look_at(c) for c in rng.uniform(-1, 1, (n, 3)) * 100 + np.array([650.0, 0, 0])])
    K4 = np.float32(np.diag([1, 1, 1, 1]))
    K4[:3, :3] = np.array([[2900.0, 0, W / 2], [0, 2900.0, H / 2], [0, 0, 1]], dtype=np.float32)
    return np.stack([K4 @ e.astype(np.float32) for e in E])


def test_vertex_mask_votes_match_the_restatement_on_a_million_points():
    from gens_amd import ops
    rng = np.random.default_rng(7)
    H, W = 1200, 1600
    P = _random_cameras(rng)
    pts = rng.uniform(-160, 160, (1_000_000, 3))
    pts[:50_000] += np.array([1300.0, 0, 0])                            # behind the cameras: no test for that in the script
    pts[50_000:60_000] *= 10                                            # far outside the images
    masks = (rng.random((3, H, W)) < 0.5).astype(np.uint8) * 255
    masks[:, :3] = 255
    masks[:, :, :3] = 0
    want, near = R.vertex_votes(pts, P, masks)
    got = ops.vertex_mask_votes(torch.from_numpy(pts).to(DEV), torch.from_numpy(P).to(DEV), torch.from_numpy(masks).to(DEV)).cpu().numpy()
    assert near.mean() <= CAP
    assert np.array_equal(got[~near], want[~near]), int((got[~near] != want[~near]).sum())
    assert (want == 0).mean() > 0.05 and (want == 3).mean() > 0.01 and (want[:50_000] > 0).any()


def test_vertex_mask_votes_frame_and_degenerate_points():
    from gens_amd import ops
    H, W = 12, 16
    P = np.zeros((1, 4, 4), dtype=np.float32)
    P[0, 0, 0] = P[0, 1, 1] = P[0, 2, 3] = P[0, 3, 3] = 1.0
    mask = np.zeros((1, H, W), dtype=np.uint8)
    mask[0, 3, 5] = 255
    mask[0, 3, W - 1] = 129
    mask[0, 4, W - 1] = 128
    pts = np.array([[5, 3, 0], [4, 2, 0], [-1, 7, 0], [7, -1, 0], [-2, 7, 0], [W - 1, 3, 0], [W - 1, 4, 0], [W, 3, 0], [1e300, 3, 0], [np.nan, 3, 0],
                    [-3e9, 2, 0]], dtype=np.float64)
    run = lambda P_: ops.vertex_mask_votes(torch.from_numpy(pts).to(DEV), torch.from_numpy(P_).to(DEV), torch.from_numpy(mask).to(DEV)).cpu().tolist()  # noqa: E731
    assert run(P) == [1, 0, 1, 1, 0, 1, 0, 0, 0, 0, 0]
    assert run(P)[:8] == R.vertex_votes(pts[:8], P, mask)[0].tolist()
    Pz = P.copy()
    Pz[0, 2, 3] = 0.0
    assert run(Pz) == [0] * len(pts)                                    # q[2] == 0: not inside


def _small(seed, misses):
    H, W = 120, 160
    sc = R.make_scene(seed, H=H, W=W, misses=misses)
    masks = np.stack([R.disk_mask(d, H, W) for d in sc["disks"]])
    return sc, R.scene_P(sc), masks, H, W


def _flags(sc, P, dil, dep_min=425):
    from gens_amd import ops
    from gens_amd.datasets.camera import load_K_Rt_from_P
    v = torch.from_numpy(sc["vertices"].astype(np.float64)).to(DEV)
    grid = ops.build_mesh_grid(v, torch.from_numpy(sc["triangles"]).to(DEV))
    cams = [load_K_Rt_from_P(None, p[:3, :]) for p in P]
    intrs, c2ws = torch.from_numpy(np.stack([c[0] for c in cams])), torch.from_numpy(np.stack([c[1] for c in cams]))
    return grid, ops.view_rays_hit_counts(grid, torch.from_numpy(dil).to(DEV), intrs, c2ws, dep_min)


@pytest.mark.parametrize("seed,misses", [(1, True), (2, False)])
def test_view_rays_hit_counts_match_the_brute_force_and_the_torch_built_rays(seed, misses):
    from gens_amd import ops
    sc, P, masks, H, W = _small(seed, misses)
    dil = np.stack([R.dilate(m, R.ellipse_footprint(11, 11)) for m in masks])
    grid, (counts, flags, any_miss) = _flags(sc, P, dil)
    flags, any_miss = flags.cpu().numpy().astype(bool), any_miss.cpu().numpy()
    assert np.array_equal(counts.cpu().numpy(), flags.sum(0))
    F = len(sc["triangles"])
    n_amb = 0
    for i in range(3):
        ro, rd, _ = R.view_rays(P[i], dil[i], H, W)
        # the rays the kernel generates are the torch-built ones bit for bit (the 425 advance included): the kernel's general first-hit
        # entry on the restated rays marks exactly the same faces
        f_dev, _ = ops.ray_mesh_first_hit(ro.to(DEV), rd.to(DEV), grid)
        f_dev = f_dev.cpu().numpy()
        mark = np.zeros(F, dtype=bool)
        mark[f_dev[f_dev >= 0]] = True
        assert np.array_equal(flags[i], mark)
        assert bool(any_miss[i]) == bool((f_dev < 0).any())
        # ... and agree with the float64 brute force outside its ambiguous rays
        face, _, amb = M.first_hits(sc["vertices"].astype(np.float64), sc["triangles"], ro, rd, device=DEV)
        face, amb = face.numpy(), amb.numpy()
        n_amb += int(amb.sum())
        assert np.array_equal(f_dev[~amb], face[~amb])
        sure = np.zeros(F, dtype=bool)
        sure[face[(face >= 0) & ~amb]] = True
        shaky = ~sure & R._near_ambiguous(sc["vertices"].astype(np.float64), sc["triangles"], ro[amb], rd[amb], None)
        assert np.array_equal(flags[i][~shaky], sure[~shaky]) and shaky.mean() <= CAP
        if ((face < 0) & ~amb).any() or not (face < 0).any():
            assert bool(any_miss[i]) == bool((face < 0).any())
    assert n_amb <= CAP * 3 * int((dil > 128).sum())
    assert (sum(any_miss) >= 2) == misses


def test_the_advance_skips_geometry_nearer_than_dep_min():
    sc, P, masks, H, W = _small(1, True)
    dil = np.stack([R.dilate(m, R.ellipse_footprint(11, 11)) for m in masks])
    near = np.arange(len(sc["triangles"]) - 2 * 7 * 12, len(sc["triangles"]))         # the last part of make_scene: 300 mm from camera 0
    _, (_, flags425, _) = _flags(sc, P, dil, 425)
    _, (_, flags0, _) = _flags(sc, P, dil, 0)
    assert not flags425[0, near].any() and flags0[0, near].any()


@pytest.mark.parametrize("seed,misses", [(1, True), (2, False)])
def test_both_functions_match_the_restatement(seed, misses):
    from gens_amd import clean_meshes as cm
    sc, P, masks, H, W = _small(seed, misses)
    v64 = sc["vertices"].astype(np.float64)
    dil = np.stack([R.dilate(m, R.ellipse_footprint(11, 11)) for m in masks])
    _, near = R.vertex_votes(v64, P, dil)
    assert not near.any()
    for minimal_vis in (0, 1):
        v1, t1 = cm.clean_mesh_faces_by_mask(sc["vertices"], sc["triangles"], P, masks, minimal_vis=minimal_vis)
        rv, rt, keep = R.clean_mesh_faces_by_mask(v64, sc["triangles"], P, masks, minimal_vis=minimal_vis)
        assert v1.dtype == np.float32 and np.array_equal(v1, sc["vertices"][keep]) and np.array_equal(t1, rt)
        assert keep.sum() > 0 and (minimal_vis == 0 or keep.sum() < len(keep))        # the two-view rule removes something in these scenes
    # step two on the unfiltered mesh (for misses=False fewer than two views have a miss: values[1:] drops a face) and on step one's
    for v_in, t_in in ((sc["vertices"], sc["triangles"]), (v1, t1)):
        lists, shaky = R.hit_lists(v_in.astype(np.float64), t_in, P, dil, H, W, device=DEV)
        assert sum(int(s.sum()) for s in shaky) == 0, "the scene has faces whose status rests on ambiguous rays: compare outside them"
        st, rst = {}, {}
        v2, t2 = cm.clean_mesh_faces_outside_frustum(v_in, t_in, P, masks, H=H, W=W, min_faces=100, stats=st)
        rv2, rt2 = R.clean_mesh_faces_outside_frustum(v_in, t_in, P, masks, H=H, W=W, min_faces=100, device=DEV, stats=rst)
        assert st == rst and np.array_equal(v2, rv2) and np.array_equal(t2, rt2) and len(t2) > 100
    values = R.values_of(R.hit_lists(sc["vertices"].astype(np.float64), sc["triangles"], P, dil, H, W, device=DEV)[0])
    assert (values[0] == -1) == misses


@pytest.fixture(scope="module")
def g21():
    return R.load_g21()


def _view_flags(v, t, P, dil, dep_min=425):
    from gens_amd import ops
    from gens_amd.datasets.camera import load_K_Rt_from_P
    grid = ops.build_mesh_grid(torch.from_numpy(np.asarray(v, dtype=np.float64)).to(DEV), torch.from_numpy(np.asarray(t, dtype=np.int64)).to(DEV))
    cams = [load_K_Rt_from_P(None, p[:3, :]) for p in P]
    intrs, c2ws = torch.from_numpy(np.stack([c[0] for c in cams])), torch.from_numpy(np.stack([c[1] for c in cams]))
    return ops.view_rays_hit_counts(grid, dil, intrs, c2ws, dep_min)


@pytest.mark.parametrize("scan,name", [(24, "chain"), (37, "chain"), (37, "raw")])
def test_both_functions_match_the_references_own_run(g21, scan, name):
    """Golden g21: the reference's evaluation/clean_meshes.py itself, at 1200 x 1600.  Kept vertices and faces after each stage, the
    per-view hit sets and miss flags and the printed counts, equal outside the flagged sets (which g21 caps at 0.5 %)."""
    from gens_amd import clean_meshes as cm
    d, run = g21[scan], g21[scan]["runs"][name]
    sc = d["scene"]
    assert not d["near_half"].any()
    v1, t1 = cm.clean_mesh_faces_by_mask(sc["vertices"], sc["triangles"], d["P"], d["masks"], minimal_vis=1)
    assert v1.dtype == np.float32 and np.array_equal(v1, d["clean_vertices"]) and np.array_equal(t1, d["clean_faces"])
    v_in, t_in = (v1, t1) if name == "chain" else (sc["vertices"], sc["triangles"])
    counts, flags, any_miss = _view_flags(v_in, t_in, d["P"], cm.dilated_masks(d["masks"]))
    flags = flags.cpu().numpy().astype(bool)
    assert np.array_equal(flags[~run["shaky"]], run["listed"][~run["shaky"]]), int((flags != run["listed"]).sum())
    assert any_miss.cpu().numpy().astype(bool).tolist() == run["miss"].tolist()
    st = {}
    v2, t2 = cm.clean_mesh_faces_outside_frustum(v_in, t_in, d["P"], d["masks"], stats=st)
    assert [st["n_faces"], st["n_values"]] == run["printed"]
    assert np.array_equal(v2, run["final_vertices"]) and np.array_equal(t2, run["final_faces"])


def test_restatement_in_full_matches_the_references_own_run(g21):
    """The whole restated ray step (every cast ray through the float64 brute force, on the device) against g21's scan 24."""
    d, run = g21[24], g21[24]["runs"]["chain"]
    st = {}
    v, t = R.clean_mesh_faces_outside_frustum(run["vertices"], run["triangles"], d["P"], d["masks"], device=DEV, stats=st)
    assert [st["n_faces"], st["n_values"]] == run["printed"]
    assert np.array_equal(np.asarray(v, dtype=np.float32), run["final_vertices"]) and np.array_equal(t, run["final_faces"])


def test_finalize_then_score_on_the_g21_tree(g21, tmp_path, capsys):
    """python -m gens_amd.clean_meshes on g21's tree (colour PNGs, cam.txt files, *_epoch0.ply), then python -m gens_amd.evaluation on the
    files it wrote: the printed lines and both written PLYs of each scan equal the reference's, and the scorer gives for the written
    scan{n}.ply exactly what dtu_chamfer gives for g21's final mesh."""
    scipy_io = pytest.importorskip("scipy.io")
    from gens_amd import clean_meshes as cm, evaluation, io
    scans = tuple(g21)
    root, exp, data = str(tmp_path / "DTU_TEST"), str(tmp_path / "exp"), tmp_path / "dtu_points"
    out = os.path.join(exp, "meshes")
    R.write_tree(root, out, {n: g21[n]["scene"] for n in scans}, cm.VIEW_LISTS[0][:3], colour=True)
    written = cm.finalize_dtu_meshes(root, out, n_view=3, set=0, scans=scans)
    lines = capsys.readouterr().out.splitlines()
    want = []
    for n in scans:
        run = g21[n]["runs"]["chain"]
        final = os.path.join(out, "final", "scan%d.ply" % n)
        want += ["processing scan%d" % n, "Surfaces/Kept: %d/%d" % tuple(run["printed"]), "save to " + final, "finishing removing triangles",
                 "finish processing scan%d" % n]
        cv, ct = io.read_ply(os.path.join(out, "final", "clean_%03d.ply" % n))
        assert np.array_equal(cv, g21[n]["clean_vertices"]) and np.array_equal(ct, g21[n]["clean_faces"])
        fv, ft = io.read_ply(final)
        assert np.array_equal(fv, run["final_vertices"]) and np.array_equal(ft, run["final_faces"])
    assert lines == want and written == [os.path.join(out, "final", "scan%d.ply" % n) for n in scans]
    # the scorer's inputs around the 100 mm object: everything observed, the plane below it, scan points on the big sphere
    (data / "ObsMask").mkdir(parents=True)
    (data / "Points" / "stl").mkdir(parents=True)
    rng = np.random.default_rng(5)
    pts = rng.standard_normal((4000, 3))
    stl = (50.0 * pts / np.linalg.norm(pts, axis=1, keepdims=True)).astype(np.float32)
    obs = dict(ObsMask=np.ones((40, 40, 40), dtype=np.uint8), BB=np.array([[-60.0] * 3, [60.0] * 3], dtype=np.float32), Res=np.array([[3.0]]))
    plane = np.array([0.0, 0.0, 1.0, 100.0]).reshape(4, 1)
    for n in scans:
        io.write_ply(str(data / "Points" / "stl" / f"stl{n:03}_total.ply"), stl, np.zeros((0, 3), dtype=np.int32))
        scipy_io.savemat(str(data / "ObsMask" / f"ObsMask{n}_10.mat"), obs)
        scipy_io.savemat(str(data / "ObsMask" / f"Plane{n}.mat"), {"P": plane})
    kw = dict(density=1.0, patch=60, max_dist=20)
    res = evaluation.evaluate_dtu(exp, str(data), scans=scans, rng=np.random.default_rng(3), **kw)
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == len(scans) + 2 and lines[-2] == "final result"
    rng = np.random.default_rng(3)
    for n in scans:
        run = g21[n]["runs"]["chain"]
        r = evaluation.dtu_chamfer(torch.from_numpy(run["final_vertices"].astype(np.float64)).to(DEV), torch.from_numpy(run["final_faces"]).to(DEV),
                                   torch.from_numpy(stl.astype(np.float64)).to(DEV), obs["ObsMask"], obs["BB"], obs["Res"], plane, rng=rng, **kw)
        got = res["scans"][n]
        assert got["n_in_obs"] > 1000 and [got[c] for c in ("d2s", "s2d", "overall")] == [r[c] for c in ("d2s", "s2d", "overall")]
        assert got["d2s"] < 3.0         # the kept faces lie on the big sphere, whose 4000 scan points are about 2.8 mm apart (the shell is 25 mm away)


def test_full_size_run_is_repeatable_and_every_kept_face_is_seen_by_two_views():
    """A K12 mesh of a 512^3 sphere-with-floaters lattice scaled to DTU units, three views at 1200 x 1600, run twice."""
    from gens_amd import clean_meshes as cm, ops
    from gens_amd.datasets.camera import load_K_Rt_from_P
    n = 512
    lin = torch.linspace(-1, 1, n, device=DEV)
    x, y, z = torch.meshgrid(lin, lin, lin, indexing="ij")
    sdf = torch.sqrt(x * x + y * y + z * z) - 0.72
    for c in ((0.8, 0.1, 0.0), (0.75, -0.3, 0.2), (0.7, 0.2, -0.4)):
        sdf = torch.minimum(sdf, torch.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - 0.012)      # floaters: ~350 faces each, below 500
    v, t = ops.marching_cubes(sdf, 0.0)
    del sdf, x, y, z
    v = ((v / (n - 1) * 2 - 1) * (49.6 / 0.72)).cpu().numpy().astype(np.float32)    # a 99 mm sphere
    t = t.cpu().numpy()
    assert len(t) > 1_000_000
    H, W = 1200, 1600
    sc = R.make_scene(1, H=H, W=W, misses=True)
    P, masks = R.scene_P(sc), np.stack([R.disk_mask(d, H, W) for d in sc["disks"]])
    st1, st2 = {}, {}
    v1, t1 = cm.clean_mesh_faces_outside_frustum(v, t, P, masks, stats=st1)
    v2, t2 = cm.clean_mesh_faces_outside_frustum(v, t, P, masks, stats=st2)
    assert st1 == st2 and np.array_equal(v1, v2) and np.array_equal(t1, t2)
    # not vacuous: a result that is not empty holds a component of at least min_faces = 500 faces; and a ray hits one face, so no more
    # faces can be kept than rays are cast.  (A face of this mesh, 0.024 mm^2, is smaller than a pixel's footprint at 650 mm, 0.05 mm^2:
    # each view marks fewer faces than it sees, two views agree on few of them, and most of those fall to the component rule.)
    assert 500 <= len(t1) <= 3 * int((cm.dilated_masks(masks) > 128).sum())
    assert (np.abs(np.linalg.norm(v1.astype(np.float64), axis=1) - 49.6) < 0.5).all()          # the floaters are gone
    # every kept face is first-hit from at least two views, re-checked with the general first-hit entry on the torch-built rays
    dil = cm.dilated_masks(masks).cpu().numpy()
    grid = ops.build_mesh_grid(torch.from_numpy(v.astype(np.float64)).to(DEV), torch.from_numpy(t.astype(np.int64)).to(DEV))
    seen = torch.zeros(len(t), dtype=torch.int32, device=DEV)
    for i in range(3):
        ro, rd, _ = R.view_rays(P[i], dil[i], H, W)
        f, _ = ops.ray_mesh_first_hit(ro.to(DEV), rd.to(DEV), grid)
        mark = torch.zeros(len(t), dtype=torch.int32, device=DEV)
        mark[f[f >= 0].long()] = 1
        seen += mark
    # the kept faces as rows of the input: match by their (float32) vertex coordinates
    key = lambda vv, tt: np.ascontiguousarray(vv[tt].reshape(len(tt), 9)).view([("", vv.dtype)] * 9).reshape(-1)  # noqa: E731
    idx = np.nonzero(np.isin(key(v, t), key(v1, t1)))[0]
    assert len(idx) == len(t1) and bool((seen[torch.from_numpy(idx).to(DEV)] >= 2).all())
