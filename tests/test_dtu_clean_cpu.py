"""The DTU mesh finalising step (gens_amd.clean_meshes, K25) without a GPU: the structuring element, the dilation restatement against
scipy, both branches of the `values[1:]` rule, and the file layout / camera parsing / CLI of finalize_dtu_meshes with the device calls
replaced by the float64 restatement of tests/dtu_clean_reference.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dtu_clean_reference as R  # noqa: E402


def test_opencv_ellipse_tables():
    from gens_amd import ops
    assert [2 * d + 1 for d in ops.opencv_ellipse(11, 11)] == [1, 7, 9, 11, 11, 11, 11, 11, 9, 7, 1]
    assert [2 * d + 1 for d in ops.opencv_ellipse(5, 5)] == [1, 5, 5, 5, 1]
    assert ops.opencv_ellipse(1, 1) == [0] and ops.opencv_ellipse(3, 3) == [0, 1, 0]
    for k in (3, 5, 7, 11, 21, 31):
        assert np.array_equal(ops.ellipse_footprint(k, k), R.ellipse_footprint(k, k))
    assert np.array_equal(ops.ellipse_footprint(7, 3), R.ellipse_footprint(7, 3))


@pytest.mark.parametrize("shape,k", [((37, 53), 11), ((37, 53, 3), 5), ((1, 1), 3), ((9, 4, 3), 31), ((40, 41), 3)])
def test_dilation_restatement_equals_scipy_grey_dilation(shape, k):
    from scipy import ndimage
    rng = np.random.default_rng(k + len(shape))
    img = rng.integers(0, 256, shape, dtype=np.uint8)
    fp = R.ellipse_footprint(k, k)
    foot = fp if img.ndim == 2 else fp[:, :, None]
    want = ndimage.grey_dilation(img, footprint=foot, mode="constant", cval=0)
    assert np.array_equal(R.dilate(img, fp), want)


def test_values_rule_both_branches():
    from gens_amd.clean_meshes import kept_after_quirk
    counts = torch.tensor([0, 2, 1, 3, 2, 0], dtype=torch.int32)
    # at least two views had a miss: -1 is values[0], every face with count >= 2 stays, len(values) counts the -1
    keep, n = kept_after_quirk(counts, torch.tensor([1, 0, 1], dtype=torch.int32))
    assert keep.tolist() == [False, True, False, True, True, False] and n == 4
    # one view with a miss: its -1 has count 1 and is not in values; the smallest hit face goes instead
    keep, n = kept_after_quirk(counts, torch.tensor([0, 1, 0], dtype=torch.int32))
    assert keep.tolist() == [False, False, False, True, True, False] and n == 3
    keep, n = kept_after_quirk(counts, torch.zeros(3, dtype=torch.int32))
    assert keep.tolist() == [False, False, False, True, True, False] and n == 3
    keep, n = kept_after_quirk(torch.zeros(4, dtype=torch.int32), torch.zeros(3, dtype=torch.int32))
    assert not keep.any() and n == 0
    # the restatement's Counter agrees
    lists = [np.array([-1, 1, 3]), np.array([1, 3, 4]), np.array([-1, 2, 3, 4])]
    assert R.values_of(lists) == [-1, 1, 3, 4]
    assert R.values_of([np.array([1, 3]), np.array([-1, 1, 3, 4]), np.array([2, 3, 4])]) == [1, 3, 4]


def test_vertex_votes_restatement_keeps_the_frame_quirks():
    H, W = 12, 16
    P = np.zeros((1, 4, 4), dtype=np.float32)
    P[0, 0, 0] = P[0, 1, 1] = P[0, 2, 3] = 1.0                 # (u, v) = (x, y), q[2] = 1; z free
    P[0, 3, 3] = 1.0
    mask = np.zeros((1, H, W), dtype=np.uint8)
    mask[0, 3, 5] = 255
    pts = np.array([[5, 3, 0], [4, 2, 0], [-1, 7, 0], [7, -1, 0], [-2, 7, 0], [W - 1, 3, 0], [W, 3, 0], [5.5, 3, -9], [4.5, 3, 0]], dtype=np.float64)
    votes, near = R.vertex_votes(pts, P, mask)
    # (5,3) is the set pixel; (-1, y) and (x, -1) round onto the frame of ones: inside; (-2, y): outside; u = W (x = W - 1): mask column
    # W - 1; x = W: u = W + 1 fails; 5.5 rounds to 6 (half to even), 4.5 to 4: both off the set pixel, and both flagged near-half
    assert votes.tolist() == [1, 0, 1, 1, 0, 0, 0, 0, 0]
    assert near.tolist() == [False] * 7 + [True, True]
    Pz = P.copy()
    Pz[0, 2, 3] = 0.0                                           # q[2] == 0: not inside
    assert R.vertex_votes(pts[:1], Pz, mask)[0].tolist() == [0]


def test_module_imports_no_cpu_geometry_package():
    import gens_amd.clean_meshes as cm
    src = open(cm.__file__).read() + open(os.path.join(os.path.dirname(cm.__file__), "ops", "finalize.py")).read()
    for name in ("cv2", "trimesh", "open3d", "pyembree", "tqdm"):
        assert f"import {name}" not in src and f"from {name}" not in src


def test_read_cam_file_is_the_float32_product(tmp_path):
    from gens_amd import clean_meshes as cm
    sc = R.make_scene(1, H=120, W=160)
    R.write_tree(str(tmp_path / "data"), str(tmp_path / "out"), {24: sc}, [23, 24, 33])
    P = np.stack([cm.read_cam_file(str(tmp_path / "data" / "cameras" / f"{vid:0>8}_cam.txt")) for vid in (23, 24, 33)])
    assert P.dtype == np.float32 and np.array_equal(P, R.scene_P(sc))


@pytest.mark.parametrize("colour", [False, True])
def test_finalize_file_layout_and_printed_lines(tmp_path, monkeypatch, capsys, colour):
    """finalize_dtu_meshes over the script's layout, the two device functions replaced by the restatement: which files are read and
    written, in which order the steps see them (the second through the float32 PLY of the first), and the printed lines."""
    from gens_amd import clean_meshes as cm, io
    H, W = 120, 160
    scenes = {24: R.make_scene(1, H=H, W=W), 37: R.make_scene(2, H=H, W=W, misses=False)}
    root, out = str(tmp_path / "DTU_TEST"), str(tmp_path / "outputs" / "mesh")
    R.write_tree(root, out, scenes, cm.VIEW_LISTS[0][:3], colour=colour)
    seen = []

    def by_mask(vertices, triangles, P, masks, minimal_vis=0, mask_dilated_size=11, device=None):
        seen.append(("mask", np.asarray(masks).copy(), minimal_vis, mask_dilated_size))
        _, t, keep = R.clean_mesh_faces_by_mask(np.asarray(vertices, dtype=np.float64), triangles, P, masks, minimal_vis, mask_dilated_size)
        return np.asarray(vertices)[keep], t

    def outside(vertices, triangles, P, masks, H=1200, W=1600, mask_dilated_size=11, device=None, stats=None, **kw):
        seen.append(("frustum", np.asarray(vertices).dtype, H, W))
        return R.clean_mesh_faces_outside_frustum(vertices, triangles, P, masks, H=H, W=W, mask_dilated_size=mask_dilated_size, min_faces=100,
                                                  stats=stats)

    monkeypatch.setattr(cm, "clean_mesh_faces_by_mask", by_mask)
    monkeypatch.setattr(cm, "clean_mesh_faces_outside_frustum", outside)
    written = cm.finalize_dtu_meshes(root, out, n_view=3, set=0, scans=(24, 37))
    assert written == [os.path.join(out, "final", "scan24.ply"), os.path.join(out, "final", "scan37.ply")]
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == "processing scan24" and lines[4] == "finish processing scan24" and lines[5] == "processing scan37"
    assert lines[2] == "save to " + written[0] and lines[3] == "finishing removing triangles"
    for k, scan in enumerate((24, 37)):
        sc = scenes[scan]
        P = R.scene_P(sc)
        masks = np.stack([R.disk_mask(d, H, W) for d in sc["disks"]])
        kind, m, minimal_vis, size = seen[2 * k]
        assert kind == "mask" and minimal_vis == 1 and size == 11 and np.array_equal(m, masks)          # blue channel of a colour PNG
        assert seen[2 * k + 1] == ("frustum", np.dtype("<f4"), H, W)
        v1, t1, _ = R.clean_mesh_faces_by_mask(sc["vertices"].astype(np.float64), sc["triangles"], P, masks, minimal_vis=1)
        cv, ct = io.read_ply(os.path.join(out, "final", "clean_%03d.ply" % scan))
        assert np.array_equal(cv, v1.astype(np.float32)) and np.array_equal(ct, t1)
        st = {}
        v2, t2 = R.clean_mesh_faces_outside_frustum(cv, ct, P, masks, H=H, W=W, min_faces=100, stats=st)
        fv, ft = io.read_ply(written[k])
        assert np.array_equal(fv, np.asarray(v2, dtype=np.float32)) and np.array_equal(ft, t2) and len(ft) > 100
        assert lines[5 * k + 1] == f"Surfaces/Kept: {len(ct)}/{st['n_values']}"


def test_cli_takes_the_scripts_arguments(monkeypatch):
    from gens_amd import clean_meshes as cm
    got = []
    monkeypatch.setattr(cm, "finalize_dtu_meshes", lambda *a, **k: got.append((a, k)))
    cm.main([])
    cm.main(["--root_dir", "a", "--out_dir", "b", "--n_view", "5", "--set", "1"])
    assert got == [(("./DTU_TEST", "./outputs/mesh"), dict(n_view=3, set=0)), (("a", "b"), dict(n_view=5, set=1))]
    assert cm.VIEW_LISTS[1][:3] == [43, 33, 44] and cm.VIEW_LISTS[0][:3] == [23, 24, 33] and cm.VIEW_LISTS == R.VIEW_LISTS


def test_step_two_alone_has_a_scene_for_each_branch():
    """The scenes the GPU test uses for the two branches of `values[1:]`: on the unfiltered mesh with masks (almost) inside the silhouette
    fewer than two views have a cast ray that misses, so values[0] is a face; with masks past the silhouette it is the -1."""
    H, W = 120, 160
    sc = R.make_scene(2, H=H, W=W, misses=False)
    masks = np.stack([R.disk_mask(d, H, W) for d in sc["disks"]])
    dil = np.stack([R.dilate(m, R.ellipse_footprint(11, 11)) for m in masks])
    lists, _ = R.hit_lists(sc["vertices"].astype(np.float64), sc["triangles"], R.scene_P(sc), dil, H, W)
    assert sum(l[0] < 0 for l in lists) < 2 and R.values_of(lists)[0] >= 0
    sc = R.make_scene(1, H=H, W=W, misses=True)
    masks = np.stack([R.disk_mask(d, H, W) for d in sc["disks"]])
    dil = np.stack([R.dilate(m, R.ellipse_footprint(11, 11)) for m in masks])
    lists, _ = R.hit_lists(sc["vertices"].astype(np.float64), sc["triangles"], R.scene_P(sc), dil, H, W)
    assert sum(l[0] < 0 for l in lists) >= 2 and R.values_of(lists)[0] == -1


# ------------------------------------------------------------------------------------------------------------------ golden g21
CAP = 0.005


@pytest.fixture(scope="module")
def g21():
    return R.load_g21()


def test_g21_holds_the_conditions_and_both_branches(g21):
    """The sets left out of exact comparisons are capped at 0.5 % in the reference's own run, and both branches of `values[1:]` occur."""
    branches = set()
    for d in g21.values():
        assert d["near_half"].mean() <= CAP
        for run in d["runs"].values():
            assert (run["shaky"].mean(1) <= CAP).all()
            low, high = (run["listed"] & ~run["shaky"]).sum(0), (run["listed"] | run["shaky"]).sum(0)
            assert not ((low < 2) & (high >= 2)).any()              # no face's place in `values` rests on ambiguous rays
            branches.add(int(run["miss"].sum()) >= 2)
    assert branches == {True, False}


@pytest.mark.parametrize("scan", list(R.G21_SCANS))
def test_restatement_reproduces_g21_mask_step(g21, scan):
    d = g21[scan]
    sc = d["scene"]
    v, t, keep = R.clean_mesh_faces_by_mask(sc["vertices"].astype(np.float64), sc["triangles"], d["P"], d["masks"], minimal_vis=1)
    ok = ~d["near_half"]
    assert np.array_equal(keep[ok], d["keep_vertices"][ok])
    assert not d["near_half"].any() and np.array_equal(t, d["clean_faces"]) and np.array_equal(v.astype(np.float32), d["clean_vertices"])


@pytest.mark.parametrize("scan,name", [(24, "chain"), (37, "chain"), (37, "raw")])
def test_restatement_reproduces_g21_ray_step_stage_by_stage(g21, scan, name):
    """The ray stage on every 16th cast ray of each view (64th on the unfiltered mesh: the float64 brute force is the cost), the stages
    after it in full: Counter >= 2 and sort, `values[1:]`, the printed counts, the components, the unreferenced vertices."""
    d, run = g21[scan], g21[scan]["runs"][name]
    H, W = d["scene"]["H"], d["scene"]["W"]
    dil = np.stack([R.dilate(m, R.ellipse_footprint(11, 11)) for m in d["masks"]])
    stride = 1 if name == "chain" else 4
    for i in range(3):
        ro, rd, _ = R.view_rays(d["P"][i], dil[i], H, W)
        assert len(ro) == run["n_cast"][i]                          # the cast rule on the dilated blue channel
        sub = slice(0, None, R.G21_SUBSAMPLE * stride)
        face, _, amb = R.M.first_hits(run["vertices"].astype(np.float64), run["triangles"], ro[sub], rd[sub])
        sure = ~(amb.numpy() | run["sub_amb"][i][::stride])
        assert sure.mean() >= 1 - CAP and np.array_equal(face.numpy()[sure], run["sub_face"][i][::stride][sure])
    values = R.values_of(run["hits"])
    assert (values[0] == -1) == (int(run["miss"].sum()) >= 2)
    assert run["printed"] == [len(run["triangles"]), len(values)]
    keep = np.zeros(len(run["triangles"]), dtype=bool)
    keep[np.asarray(values[1:], dtype=np.int64)] = True
    assert np.array_equal(keep, run["keep_values"])
    tri = run["triangles"][keep]
    comp = R.M.large_components_keep(R.M.face_adjacency(tri), len(tri), 500)
    assert np.array_equal(comp, run["keep_components"])
    v, t = R.M.remove_unreferenced(run["vertices"], tri[comp])
    assert np.array_equal(np.asarray(v, dtype=np.float32), run["final_vertices"]) and np.array_equal(t, run["final_faces"])
