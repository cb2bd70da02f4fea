"""GPU tests of the depth-map fusion (K32): both kernels against the numpy restatement (tests/depth_fusion_reference.py), bit for bit, at
shapes that cover one pixel, a tile smaller than a wave and ragged edges of the 8 x 8 tiling on both axes; the planted pixels of the CPU file;
the empty cases; ImplicitSurface.fuse_surface on the g23 model against the restatement applied to per-view render_surface maps; validate and
the writer; the refusals."""
import os

import numpy as np
import pytest
import torch

from . import depth_fusion_reference as FR

gpu = pytest.mark.gpu
K32 = {"gens_fuse_depth_maps", "gens_fused_points"}
SHAPES = ((2, 1, 1), (3, 5, 7), (4, 33, 65), (6, 48, 64))


def _same(a, b):
    """Equal dtype, shape and bits (no NaN is ever written: a kept pixel's sums are finite)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == bool or b.dtype == bool:
        a, b = a.astype(np.uint8), b.astype(np.uint8)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _device_cloud(depth, cams, normal=None, img=None, dedupe_radius=None, **kw):
    """ops.fuse_depth_maps + ops.fused_points on uploaded host arrays -> the dict FR.cloud returns, as host arrays."""
    from gens_amd import ops
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    d_normal = up(normal)
    votes, keep, fused = ops.fuse_depth_maps(up(depth), cams, normal=d_normal if kw.get("normal_cos") is not None else None, **kw)
    points, normals, colors, pixel = ops.fused_points(fused, cams, keep, d_normal, up(img), dedupe_radius)
    out = {"votes": votes.cpu().numpy(), "keep": keep.cpu().numpy(), "fused": fused.cpu().numpy(), "pixel": pixel.cpu().numpy(),
           "points": points.cpu().numpy()}
    if normal is not None:
        out["normals"] = normals.cpu().numpy()
    if img is not None:
        out["colors"] = colors.cpu().numpy()
    return out


def _assert_cloud(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert _same(got[k], want[k]), (what, k)


def _shape_scene(nv, h, w):
    """The analytic sphere at this shape (focal length scaled with the width, so that the views still overlap), seeded colours, and -- where
    the image has room -- the non-finite and non-positive depths of the CPU file planted in every view."""
    depth, normal, intrs, c2ws = FR.sphere_scene(nv, h, w, f=60.0 * w / 64.0)
    img = np.random.default_rng(nv * h * w).integers(0, 256, (nv, h, w, 3)).astype(np.uint8)
    if h * w > 1000:
        for v in range(nv):
            flat = depth[v].reshape(-1)
            idx = np.nonzero(FR.usable(flat))[0]
            for j, bad in enumerate((0.0, -1.5, np.nan, np.inf, -np.inf)):
                if len(idx) > 5:
                    flat[idx[(j + 1) * len(idx) // 7]] = bad
        turned = normal[0].reshape(-1, 3)                      # every third normal of view 0 with its components rotated: still unit, elsewhere
        turned[::3] = turned[::3][:, [1, 2, 0]]
    return depth, normal, img, FR.cams_table(intrs, c2ws)


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_both_kernels_equal_the_restatement(shape):
    nv, h, w = shape
    depth, normal, img, cams = _shape_scene(nv, h, w)
    every = FR.default_pairs(nv)
    options = [
        ("every other view", dict(pairs=None, min_views=min(2, nv - 1))),
        ("k = 1 with padding", dict(pairs=np.array([[(r + 1) % nv, -1] for r in range(nv)], np.int32), min_views=1)),
        ("k = nv - 1 with padding", dict(pairs=np.concatenate([np.full((nv, 1), -1, np.int32), every[:, ::-1], np.full((nv, 2), -1, np.int32)], axis=1),
                                        min_views=1, pix_tol=0.75, rel_tol=0.004)),
        ("normals", dict(pairs=None, min_views=1, normal_cos=0.97)),
    ]
    voted = False
    for name, kw in options:
        want = FR.cloud(depth, cams, normal=normal, img=img, **kw)
        got = _device_cloud(depth, cams, normal=normal, img=img, **kw)
        _assert_cloud(got, want, f"{shape} {name}")
        assert want["keep"].dtype == bool and got["keep"].dtype == np.uint8 and got["fused"].dtype == np.float64
        voted = voted or bool(want["votes"].any())
        print(f"{shape} {name}: usable {int(FR.usable(depth).sum())}, kept {int(want['keep'].sum())}, votes {np.bincount(want['votes'].reshape(-1)).tolist()}")
    assert voted == (h * w > 1)                                # (one pixel has no 2 x 2 taps to read: nothing can vote)
    if h * w > 1000:                                           # the normal test really decided something, and the strict thresholds too
        assert FR.fuse(depth, cams, min_views=1, normal=normal, normal_cos=0.97)[0].sum() < FR.fuse(depth, cams, min_views=1)[0].sum()
    # points without attribute maps, and with one of them
    bare = _device_cloud(depth, cams, min_views=1)
    _assert_cloud(bare, FR.cloud(depth, cams, min_views=1), f"{shape} bare")
    _assert_cloud(_device_cloud(depth, cams, img=img, min_views=1), FR.cloud(depth, cams, img=img, min_views=1), f"{shape} colours only")


@gpu
def test_planted_pixels_take_every_branch_on_the_device():
    from .test_depth_fusion_cpu import PAIRS01
    depth, normal, cams, cases = FR.planted_scene()
    for kw in ({}, {"pix_tol": 0.0}, {"rel_tol": 0.0}, {"pix_tol": 1e-100, "rel_tol": 1e-300}, {"normal_cos": 0.5}, {"normal_cos": float(np.nextafter(0.5, 1.0))},
               {"min_views": 2}, {"pairs": np.array([[-1, 1, -1, 2], [0, -1, -1, 2], [-1, 0, 1, -1]], np.int32)}, {"pairs": np.full((3, 2), -1, np.int32)}):
        kw = {"pairs": PAIRS01, "min_views": 1, **kw}
        want = FR.cloud(depth, cams, normal=normal, **kw)
        _assert_cloud(_device_cloud(depth, cams, normal=normal, **kw), want, str(kw))
    base = FR.fuse(depth, cams, pairs=PAIRS01, min_views=1)[0]
    assert base[cases["x0 + 1 == W - 1"]] == 1 and base[cases["x0 + 1 == W"]] == 0 and base[cases["one unusable tap"]] == 0
    depth, cams = FR.back_facing_scene()
    pairs = np.array([[1], [-1]], np.int32)
    _assert_cloud(_device_cloud(depth, cams, pairs=pairs, min_views=1), FR.cloud(depth, cams, pairs=pairs, min_views=1), "q'_z <= 0")
    depth[1] = 2.0
    want = FR.cloud(depth, cams, pairs=pairs, min_views=1)
    assert want["keep"].any()
    _assert_cloud(_device_cloud(depth, cams, pairs=pairs, min_views=1), want, "q'_z > 0")


@gpu
def test_votes_saturate_at_255_and_the_count_goes_on():
    """300 listed sources (the same view again and again): votes reads 255, keep and fused still use all 300."""
    depth, cams = FR.back_facing_scene()
    depth[1] = 2.0
    pairs = np.array([[1] * 300, [-1] * 300], np.int32)
    want = FR.cloud(depth, cams, pairs=pairs, min_views=300)
    assert want["votes"].max() == 255 and want["keep"].any()
    _assert_cloud(_device_cloud(depth, cams, pairs=pairs, min_views=300), want, "300 sources")
    assert not _device_cloud(depth, cams, pairs=pairs, min_views=301)["keep"].any()


@gpu
def test_empty_cases_launch_nothing():
    from gens_amd import lib as L, ops
    depth, normal, img, cams = _shape_scene(3, 5, 7)
    L.profile_begin(only={"gens_fused_points", "gens_compact_valid"})
    got = _device_cloud(depth, cams, normal=normal, img=img, min_views=2, pairs=np.full((3, 1), -1, np.int32))      # nothing is kept
    assert not L.profile_end(raw=True)
    assert not got["votes"].any() and not got["keep"].any() and not got["fused"].any()
    assert got["points"].shape == (0, 3) and got["points"].dtype == np.float64 and got["pixel"].shape == (0,) and got["pixel"].dtype == np.int64
    assert got["normals"].shape == (0, 3) and got["normals"].dtype == np.float32 and got["colors"].shape == (0, 3) and got["colors"].dtype == np.uint8
    # no views, and views without pixels
    for shape in ((0, 5, 7), (2, 0, 7)):
        nv = shape[0]
        votes, keep, fused = ops.fuse_depth_maps(torch.zeros(shape, device="cuda"), np.zeros((nv, 24)))
        assert votes.shape == keep.shape == fused.shape == shape
        assert ops.fused_points(fused, np.zeros((nv, 24)), keep)[0].shape == (0, 3)
    # N = 0 at the entry point itself: no launch, no error, whatever the pointers
    assert L.load().gens_fused_points(None, None, None, 0, 3, 5, 7, None, None, None, None, None, None) == 0
    # a list entry outside the maps gives a zero row and reads nothing
    fused = torch.ones(3, 5, 7, device="cuda", dtype=torch.float64)
    lst = torch.tensor([-1, 3 * 5 * 7, 4], device="cuda")
    pts = torch.full((3, 3), 7.0, device="cuda", dtype=torch.float64)
    L.call("gens_fused_points", L.ptr(fused, torch.float64), L.ptr(torch.from_numpy(cams).cuda(), torch.float64), L.ptr(lst, torch.int64), 3, 3, 5, 7,
           None, None, L.ptr(pts, torch.float64), None, None, L.stream())
    assert not pts[:2].any() and _same(pts[2:].cpu().numpy(), FR.points(np.ones((3, 5, 7)), cams, [4]))


# ------------------------------------------------------------------------------------------------------------------------------------
# the model: the g23 surface and the synthetic 48 x 64 views of tests/test_hip_vertex_attrs.py
# ------------------------------------------------------------------------------------------------------------------------------------
RES = 128
FUSE = {"min_views": 2, "resolution": RES, "near": 0.0, "far": 5.0}
_FUSED = {}


def _model_cloud(precision):
    """fuse_surface of the g23 model and, per view, render_surface on the same rays; with as many views as it takes for the restatement to
    keep something; once per precision -> (surf, vols, scene, views, nv, fuse_surface's dict, its stats, the per-view maps, the restated cloud)."""
    from gens_amd import ops
    from .test_hip_vertex_attrs import _bounds, _scene, _surface
    surf, vols = _surface(precision)                           # (one model for both precisions: this sets the one asked for, cached or not)
    if precision not in _FUSED:
        lo, hi = _bounds()
        for nv in (3, 5, 7):
            sc, views = _scene(surf, nv)
            got = surf.fuse_surface(vols, sc["intrs"], sc["c2ws"], (48, 64), lo, hi, views=views, **FUSE)
            stats = surf.last_fusion_stats
            maps = []
            near, far = torch.full((1,), FUSE["near"], device="cuda"), torch.full((1,), FUSE["far"], device="cuda")
            for v in range(nv):
                o, d = surf.view_rays(sc["intrs"], sc["c2ws"], v, (48, 64))
                maps.append(surf.render_surface(o, d, near, far, vols, lo, hi, sc["c2ws"][[v]], views=views, resolution=RES, hw=(48, 64)))
            stacked = {k: np.stack([m[k] for m in maps]) for k in ("depth", "normal", "img", "seen", "hit")}
            want = FR.cloud(stacked["depth"], ops.fusion_cams(sc["intrs"], sc["c2ws"]), normal=stacked["normal"], img=stacked["img"], min_views=2)
            if want["keep"].any():
                break
        _FUSED[precision] = (surf, vols, sc, views, nv, got, stats, stacked, want)
    return _FUSED[precision]


@gpu
@pytest.mark.parametrize("precision", ["f32", "f16x2"])
def test_fuse_surface_is_the_restatement_on_the_render_surface_maps(precision):
    from gens_amd import synthetic
    surf, vols, sc, views, nv, got, stats, maps, want = _model_cloud(precision)
    n = len(want["pixel"])
    print(f"{precision}: {nv} views, usable {int(FR.usable(maps['depth']).sum())}, kept {n}, votes {np.bincount(want['votes'].reshape(-1)).tolist()}")
    assert n > 0
    assert sorted(got) == ["colors", "normals", "pixel", "points", "seen", "view"]
    assert _same(got["points"], want["points"]) and _same(got["pixel"], want["pixel"])
    assert got["view"].dtype == np.int32 and np.array_equal(got["view"], want["pixel"] // (48 * 64))
    # every point's normal, colour and seen are render_surface's maps at (view, pixel)
    assert _same(got["normals"], maps["normal"].reshape(-1, 3)[got["pixel"]])
    assert _same(got["colors"], maps["img"].reshape(-1, 3)[got["pixel"]])
    assert got["seen"].dtype == bool and np.array_equal(got["seen"], maps["seen"].reshape(-1)[got["pixel"]])
    assert maps["hit"].reshape(-1)[got["pixel"]].all() and np.array_equal(maps["hit"], FR.usable(maps["depth"]))
    # the stats
    assert stats["points"] == n and len(stats["views"]) == nv
    for v in range(nv):
        s = stats["views"][v]
        assert s["usable"] == int(maps["hit"][v].sum()) == s["trace"]["hit"] and s["kept"] == int(want["keep"][v].sum())
        assert s["votes"] == np.bincount(want["votes"][v].reshape(-1), minlength=nv).tolist()
    # the device rays are make_rays' (view 0: the ones validate is given), to float32 rounding of the two small products
    o, d = surf.view_rays(sc["intrs"], sc["c2ws"], 0, (48, 64))
    ro, rd = synthetic.make_rays(sc["intrs"].cpu(), sc["c2ws"].cpu(), 48, 64)
    assert torch.equal(o.cpu(), ro) and float((d.cpu() - rd).abs().max()) < 1e-6


@gpu
def test_dedupe_radius_returns_the_subset_radius_downsample_names():
    from gens_amd import ops
    from .test_hip_vertex_attrs import _bounds
    surf, vols, sc, views, nv, full, _, _, _ = _model_cloud("f32")
    lo, hi = _bounds()
    radius = 0.03
    thin = surf.fuse_surface(vols, sc["intrs"], sc["c2ws"], (48, 64), lo, hi, views=views, dedupe_radius=radius, **FUSE)
    mask = ops.radius_downsample(torch.from_numpy(full["points"]).cuda(), radius).cpu().numpy()
    assert 0 < mask.sum() < len(mask)
    for k in full:
        assert _same(thin[k], full[k][mask]), k
    assert surf.last_fusion_stats["points"] == int(mask.sum())
    only = surf.fuse_surface(vols, sc["intrs"], sc["c2ws"], (48, 64), lo, hi, attributes=(), **FUSE)          # depth alone needs no views
    assert sorted(only) == ["pixel", "points", "view"] and _same(only["points"], full["points"])


def _validate_args(surf, vols, nv):
    """validate's positional arguments for the whole 48 x 64 image of view 0 of the seeded scene."""
    from gens_amd import synthetic
    from .test_hip_vertex_attrs import _bounds, _scene
    sc, _ = _scene(surf, nv)
    rays_o, rays_d = synthetic.make_rays(sc["intrs"].cpu(), sc["c2ws"].cpu(), 48, 64)
    masks = [torch.ones(1, 1, *v.shape[2:], device="cuda") for v in vols]
    lo, hi = _bounds()
    return (rays_o.cuda(), rays_d.cuda(), sc["near"], sc["far"], vols, masks, sc["imgs"], sc["features"], sc["features"], sc["intrs"], sc["c2ws"], lo, hi,
            (48, 64))


@gpu
def test_nothing_changes_when_the_option_is_unset_and_validate_adds_four_keys_when_set(tmp_path):
    from gens_amd import io as gio, lib as L
    from gens_amd.config import Conf, gens_model_conf
    from gens_amd.models.gens import GenS
    from gens_amd.models.modules.implicit_surface import ImplicitSurface
    from .test_hip_vertex_attrs import TODAYS_KEYS, _bounds
    assert ImplicitSurface.surface_fusion is None
    surf, vols, sc, views, nv, cloud, _, _, _ = _model_cloud("f32")
    assert "surface_fusion" not in vars(surf)
    args = _validate_args(surf, vols, nv)
    L.profile_begin(only=K32)
    torch.manual_seed(3)
    ref = surf.validate(*args, extract_geometry=True, mesh_resolution=33)
    torch.manual_seed(3)
    off = surf.validate(*args, extract_geometry=True, mesh_resolution=33, surface_fusion=False)
    assert not L.profile_end(raw=True)
    assert set(ref) == set(off) == TODAYS_KEYS
    L.profile_begin(only=K32)
    torch.manual_seed(3)
    option = {k: v for k, v in FUSE.items() if k not in ("near", "far")}
    out = surf.validate(*args, extract_geometry=True, mesh_resolution=33, surface_fusion={**option, "near": FUSE["near"], "far": FUSE["far"]})
    assert {k for k, *_ in L.profile_end(raw=True)} == K32
    new = {"fused_points", "fused_normals", "fused_colors", "fused_seen"}
    assert set(out) == TODAYS_KEYS | new
    for k in TODAYS_KEYS:
        assert torch.equal(torch.as_tensor(out[k]), torch.as_tensor(ref[k])) and torch.equal(torch.as_tensor(off[k]), torch.as_tensor(ref[k])), k
    assert _same(out["fused_points"], cloud["points"]) and _same(out["fused_normals"], cloud["normals"])
    assert _same(out["fused_colors"], cloud["colors"]) and _same(out["fused_seen"], cloud["seen"]) and len(cloud["points"]) > 0
    # the attribute does what the keyword does (True: the defaults, at the mesh's resolution)
    surf.surface_fusion = True
    try:
        torch.manual_seed(3)
        assert new <= set(surf.validate(*args, extract_geometry=False, mesh_resolution=64))
        assert surf.last_fusion_stats["views"][0]["trace"]["rays"] == 48 * 64
        with pytest.raises(ValueError, match="not sharded"):
            surf.validate(*args, extract_geometry=False, shard=object())
    finally:
        del surf.surface_fusion
    # the writer: pcd/ only when the keys are there; world coordinates through scale_mat; unseen colours mid-grey
    scale = torch.eye(4)
    scale[:3, :3] = torch.diag(torch.tensor([1.5, 1.0, 0.75]))                  # not a uniform scale: the normals need the inverse transpose
    scale[:3, 3] = torch.tensor([0.5, -1.0, 2.0])
    inputs = {"scene": "scan1", "file_name": "scan1_view0", "scale_mat": scale}
    plain = gio.save_validation_outputs(str(tmp_path / "plain"), ref, inputs, "epoch0")
    assert "pcd" not in plain and not (tmp_path / "plain" / "pcd").exists()
    assert sorted(os.listdir(tmp_path / "plain")) == ["meshes", "val_img", "val_normal", "val_render_depth", "val_sdf_depth"]
    seen = out["fused_seen"].copy()
    seen[::7] = False                                                           # (force a few, so that the grey rule is exercised either way)
    out["fused_seen"] = seen
    paths = gio.save_validation_outputs(str(tmp_path / "set"), out, inputs, "epoch0")
    assert paths["pcd"] == str(tmp_path / "set" / "pcd" / "scan1_epoch0.ply")
    v, t, attrs = gio.read_ply(paths["pcd"], attributes=True)
    assert t.shape == (0, 3) and np.array_equal(v, gio.transform_vertices(out["fused_points"], scale.numpy()).astype(np.float32))
    assert np.array_equal(attrs["normals"], gio.transform_normals(out["fused_normals"], scale.numpy()).astype(np.float32))
    assert np.array_equal(attrs["colors"], np.where(seen[:, None], out["fused_colors"], np.uint8(128))) and (~seen).any()
    # the conf key reaches the attribute (and its absence leaves the class default)
    conf = gens_model_conf(volume_dims=(16, 8, 4), has_vol=True)
    assert "surface_fusion" not in vars(GenS(conf).implicit_surface)
    assert GenS(Conf({**conf, "surface_fusion": True})).implicit_surface.surface_fusion is True
    assert GenS(Conf({**conf, "surface_fusion": {"min_views": 2}})).implicit_surface.surface_fusion == {"min_views": 2}


@gpu
def test_refusals_come_before_any_launch():
    from gens_amd import lib as L, ops
    from .test_hip_surface_trace import K31
    from .test_hip_vertex_attrs import NETWORK, _bounds, _scene, _surface
    surf, vols = _surface("f32")
    sc, views = _scene(surf, 3)
    lo, hi = _bounds()
    six = ops.VolumeSet.packed([torch.zeros(1, 4, 4, 4, 4, device="cuda") for _ in range(6)])
    base = (sc["intrs"], sc["c2ws"], (48, 64), lo, hi)
    depth = torch.ones(3, 5, 7, device="cuda")
    cams = ops.fusion_cams(sc["intrs"], sc["c2ws"])
    normal = torch.zeros(3, 5, 7, 3, device="cuda")
    keep = torch.ones(3, 5, 7, device="cuda", dtype=torch.uint8)
    fused = torch.ones(3, 5, 7, device="cuda", dtype=torch.float64)
    L.profile_begin(only=K32 | K31 | NETWORK | {"gens_compact_valid"})
    with pytest.raises(ValueError, match="1 to 5 packed volume levels, not 6"):
        surf.fuse_surface(six, *base, views=views)
    with pytest.raises(ValueError, match="needs the scene's views"):
        surf.fuse_surface(vols, *base)
    with pytest.raises(ValueError, match="the known ones are"):
        surf.fuse_surface(vols, *base, views=views, attributes=("normals", "albedo"))
    with pytest.raises(ValueError, match="min_step"):
        surf.fuse_surface(vols, *base, views=views, min_step=0.0)
    with pytest.raises(ValueError, match="max_steps"):
        surf.fuse_surface(vols, *base, views=views, max_steps=0)
    with pytest.raises(TypeError, match="unknown keywords"):
        surf.fuse_surface(vols, *base, views=views, outputs=("depth",))
    for kw in ({"pairs": [[0], [0], [0]]}, {"pairs": [[1], [2], [3]]}, {"pairs": [[1], [2]]}, {"min_views": 0}, {"pix_tol": -1.0}, {"rel_tol": float("nan")},
               {"normal_cos": 2.0}, {"normal_cos": 0.5, "attributes": ("colors",)}, {"dedupe_radius": 0.0}):
        with pytest.raises(ValueError):
            surf.fuse_surface(vols, *base, views=views, **kw)
    with pytest.raises(ValueError, match="fusion_cams"):
        surf.fuse_surface(vols, sc["intrs"][:2], sc["c2ws"], (48, 64), lo, hi, views=views)
    with pytest.raises(ValueError, match="hw"):
        surf.fuse_surface(vols, sc["intrs"], sc["c2ws"], (0, 64), lo, hi, views=views)
    for args, kw in (((depth.double(), cams), {}), ((depth[0], cams[:1]), {}), ((depth, cams[:2]), {}), ((depth, cams.astype(np.float32)), {}),
                     ((depth, cams), {"pairs": [[0], [0], [0]]}), ((depth, cams), {"min_views": 0}), ((depth, cams), {"pix_tol": float("inf")}),
                     ((depth, cams), {"normal": normal[:, :4], "normal_cos": 0.5}), ((depth, cams), {"normal": normal.cpu(), "normal_cos": 0.5}),
                     ((depth, cams), {"normal_cos": 0.5})):
        with pytest.raises(ValueError):
            ops.fuse_depth_maps(*args, **kw)
    for args, kw in (((fused.float(), cams, keep), {}), ((fused, cams, keep[:2]), {}), ((fused, cams, keep.float()), {}), ((fused, cams[:2], keep), {}),
                     ((fused, cams, keep), {"normal": normal[..., :2]}), ((fused, cams, keep), {"img": normal}), ((fused, cams, keep), {"dedupe_radius": -1.0}),
                     ((fused, cams, keep), {"dedupe_radius": float("inf")})):
        with pytest.raises(ValueError):
            ops.fused_points(*args, **kw)
    assert not L.profile_end(raw=True)
