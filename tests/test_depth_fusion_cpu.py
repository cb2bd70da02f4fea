"""CPU tests of the depth-map fusion (K32): the numpy restatement (tests/depth_fusion_reference.py) pinned on an analytic sphere and on
planted pixels for every branch of the rule; the argument checks of the two entry points through ctypes and of the ops functions (these need
the built library, not a GPU); the point-cloud writer."""
import ctypes as C

import numpy as np
import pytest
import torch

from . import depth_fusion_reference as FR

RADIUS, REL_TOL = 0.5, 0.01
_SPHERE = {}


def _sphere():
    """The six-view sphere scene and its fusion with every other view voting, min_views = 2; computed once, never modified."""
    if not _SPHERE:
        depth, normal, intrs, c2ws = FR.sphere_scene()
        cams = FR.cams_table(intrs, c2ws)
        _SPHERE.update(depth=depth, normal=normal, cams=cams, out=FR.cloud(depth, cams, min_views=2, rel_tol=REL_TOL))
    return _SPHERE


def test_the_restatement_keeps_a_consistent_sphere():
    s = _sphere()
    depth, out = s["depth"], s["out"]
    keep, fused, votes = out["keep"], out["fused"], out["votes"]
    usable = FR.usable(depth)
    print(f"usable {int(usable.sum())}, kept {int(keep.sum())}, votes histogram {np.bincount(votes.reshape(-1)).tolist()}")
    assert keep.sum() > 0 and not keep[~usable].any() and not votes[~usable].any()
    assert np.array_equal(keep, votes >= 2) and not fused[~keep].any()
    d = depth.astype(np.float64)[keep]
    # every vote's q'_z is strictly within rel_tol d of d, so is the mean of d and the votes; 4 ulps for the sum's roundings and the division
    assert (np.abs(fused[keep] - d) <= REL_TOL * d + 4 * np.spacing(d)).all()
    p = out["points"]
    off = np.abs(np.sqrt((p * p).sum(axis=1)) - RADIUS)
    print(f"kept points off the sphere: max {off.max():.3e}, median {np.median(off):.3e}; rel_tol d >= {REL_TOL * d.min():.3e}")
    # the point moves along its own pixel's ray by at most |fused - d| < rel_tol d times the ray's length per unit depth
    assert (off <= REL_TOL * d).all()
    assert len(out["pixel"]) == keep.sum() and (np.diff(out["pixel"]) > 0).all()


def test_a_planted_outlier_block_gets_no_vote_and_no_other_view_changes():
    s = _sphere()
    depth = s["depth"].copy()
    block = (2, slice(20, 28), slice(28, 36))
    assert FR.usable(depth[block]).all() and s["out"]["keep"][block].any()
    depth[block] = (depth[block] * np.float32(0.93)).astype(np.float32)
    votes, keep, _ = FR.fuse(depth, s["cams"], min_views=2, rel_tol=REL_TOL)
    assert not votes[block].any() and not keep[block].any()
    for v in range(depth.shape[0]):
        if v != 2:
            assert np.array_equal(keep[v], s["out"]["keep"][v]), v
    outside = np.ones(depth.shape[1:], bool)
    outside[block[1:]] = False
    assert np.array_equal(keep[2][outside], s["out"]["keep"][2][outside])


PAIRS01 = np.array([[1, 2], [0, 2], [0, 1]], np.int32)


def _votes(case, depth, cams, cases, **kw):
    return int(FR.fuse(depth, cams, pairs=kw.pop("pairs", PAIRS01), min_views=kw.pop("min_views", 1), **kw)[0][cases[case]])


def test_planted_pixels_take_every_branch():
    depth, normal, cams, cases = FR.planted_scene()
    v = lambda case, **kw: _votes(case, depth, cams, cases, **kw)  # noqa: E731
    for name in ("zero", "negative", "nan", "inf"):
        assert v("unusable " + name) == 0
    votes, keep, fused = FR.fuse(depth, cams, pairs=PAIRS01, min_views=1)
    assert not keep[0, 0, :4].any() and not fused[0, 0, :4].any()
    assert not votes[2].any()                                   # behind the source, and nothing of views 0 / 1 is in front of view 2
    assert v("behind the source") == 0
    assert v("x0 < 0") == 0
    assert v("x0 + 1 == W") == 0 and v("x0 + 1 == W - 1") == 1
    assert v("one unusable tap") == 0 and v("all taps usable") == 1
    # thresholds hit with equality: the planes agree exactly, the errors are 0, and 0 < 0 is false
    assert v("all taps usable", pix_tol=0.0) == 0 and v("all taps usable", rel_tol=0.0) == 0
    assert v("all taps usable", pix_tol=1e-100, rel_tol=1e-300) == 1
    # the normal test on either side of cos = 0.5 (the planted dot product is exactly 0.5)
    assert v("normal tilted", normal=normal, normal_cos=0.5) == 1
    assert v("normal tilted", normal=normal, normal_cos=np.nextafter(0.5, 1.0)) == 0
    assert v("all taps usable", normal=normal, normal_cos=1.0) == 1
    assert v("normal tilted", normal=normal, normal_cos=None) == 1
    # -1 pads a row: the same votes with padding anywhere, none with padding only
    padded = np.array([[-1, 1, -1, 2], [0, -1, -1, 2], [-1, 0, 1, -1]], np.int32)
    assert np.array_equal(FR.fuse(depth, cams, pairs=padded, min_views=1)[0], votes)
    assert not FR.fuse(depth, cams, pairs=np.full((3, 2), -1, np.int32), min_views=1)[0].any()
    with pytest.raises(ValueError):
        FR.fuse(depth, cams, pairs=np.array([[0], [0], [0]]))
    with pytest.raises(ValueError):
        FR.fuse(depth, cams, pairs=np.array([[3], [0], [0]]))
    # fused: the mean of the pixel's depth and its voters' (all 2 here)
    assert fused[cases["all taps usable"]] == 2.0


def test_min_views_of_one_and_of_k():
    """Three parallel cameras in a row see one plane: the middle view's inner pixels get 2 votes, one from each side."""
    h, w = 6, 8
    intrs = np.stack([FR.intrinsics(h, w, 4.0)] * 3)
    c2ws = np.stack([np.eye(4)] * 3)
    c2ws[0, 0, 3], c2ws[2, 0, 3] = -0.5, 0.5
    cams = FR.cams_table(intrs, c2ws)
    depth = np.full((3, h, w), 2.0, np.float32)
    votes, keep1, _ = FR.fuse(depth, cams, min_views=1)
    assert votes[1, 2, 3] == 2 and votes[1, 2, 0] == 1 and votes[1, 5, 3] == 0 and votes.max() == 2
    keep2 = FR.fuse(depth, cams, min_views=2)[1]
    assert np.array_equal(keep1, votes >= 1) and np.array_equal(keep2, votes >= 2) and keep2.sum() < keep1.sum() and keep2.any()
    assert not FR.fuse(depth, cams, min_views=3)[1].any()


def test_a_source_point_behind_the_reference_does_not_vote():
    depth, cams = FR.back_facing_scene()
    pairs = np.array([[1], [-1]], np.int32)
    assert not FR.fuse(depth, cams, pairs=pairs, min_views=1)[0].any()          # q'_z = -26
    depth[1] = 2.0
    assert FR.fuse(depth, cams, pairs=pairs, min_views=1)[0][0, 1:, :7].all()


# ------------------------------------------------------------------------------------------------------------------------------------
# the library's argument checks (no GPU: nothing here gets as far as a launch)
# ------------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_report_bad_arguments_without_a_gpu():
    from gens_amd import lib as L
    lib = L.load()
    p = lambda k: C.c_void_p(0x7e0000000000 + 4096 * k)  # noqa: E731  (made-up addresses: never dereferenced by the host code)

    def refused(rc, *words, code=-1):
        msg = lib.gens_last_error().decode()
        assert rc == code and all(w in msg for w in words), (rc, msg)

    def fuse(depth=p(0), cams=p(1), pairs=p(2), normal=None, nv=3, h=5, w=7, k=2, pix=1.0, rel=0.01, mv=3, cos=0.0, votes=p(3), keep=p(4), fused=p(5)):
        return lib.gens_fuse_depth_maps(depth, cams, pairs, normal, nv, h, w, k, pix, rel, mv, cos, votes, keep, fused, None)

    for name in ("depth", "cams", "pairs", "votes", "keep", "fused"):
        refused(fuse(**{name: None}), "gens_fuse_depth_maps", "null")
    refused(fuse(nv=-1), "gens_fuse_depth_maps", "-1 maps")
    refused(fuse(h=-5), "gens_fuse_depth_maps", "-5 x 7")
    refused(fuse(k=-1), "gens_fuse_depth_maps", "-1 source views")
    refused(fuse(pix=-1.0), "gens_fuse_depth_maps", "pix_tol")
    refused(fuse(pix=float("nan")), "gens_fuse_depth_maps", "pix_tol")
    refused(fuse(rel=float("inf")), "gens_fuse_depth_maps", "rel_tol")
    refused(fuse(mv=0), "gens_fuse_depth_maps", "min_views = 0")
    refused(fuse(normal=p(6), cos=float("nan")), "gens_fuse_depth_maps", "normal_cos")
    refused(fuse(nv=1 << 10, h=1 << 11, w=1 << 10), "gens_fuse_depth_maps", "below 2^31", code=-2)
    refused(fuse(nv=1, h=1 << 16, w=1 << 16), "gens_fuse_depth_maps", "below 2^31", code=-2)
    assert fuse(nv=0, depth=None, cams=None, pairs=None, votes=None, keep=None, fused=None) == 0
    assert fuse(w=0, depth=None, cams=None, pairs=None, votes=None, keep=None, fused=None) == 0

    def points(fused=p(0), cams=p(1), lst=p(2), n=9, nv=3, h=5, w=7, normal=None, img=None, out=p(3), normals=None, colors=None):
        return lib.gens_fused_points(fused, cams, lst, n, nv, h, w, normal, img, out, normals, colors, None)

    for name in ("fused", "cams", "lst", "out"):
        refused(points(**{name: None}), "gens_fused_points", "null")
    refused(points(normal=p(4)), "gens_fused_points", "null")
    refused(points(colors=p(4)), "gens_fused_points", "null")
    refused(points(n=-2), "gens_fused_points", "-2 pixels")
    refused(points(n=(1 << 31) + 5), "gens_fused_points", "below 2^31", code=-2)
    refused(points(nv=-1), "gens_fused_points", "-1 maps")
    refused(points(nv=0), "gens_fused_points", "empty maps")
    assert points(n=0, fused=None, cams=None, lst=None, out=None) == 0
    assert lib.gens_abi_version() == 12
    assert L.SIGNATURES["gens_fuse_depth_maps"][8] is C.c_double and len(L.SIGNATURES["gens_fused_points"]) == 13


def test_ops_refuse_bad_arguments_before_any_launch():
    from gens_amd import ops
    depth, normal, intrs, c2ws = FR.sphere_scene(nv=3, h=5, w=7)
    cams = ops.fusion_cams(intrs, c2ws)
    assert cams.shape == (3, 24) and cams.dtype == np.float64
    assert np.allclose(cams, FR.cams_table(intrs, c2ws), rtol=1e-12, atol=1e-12)
    assert np.array_equal(ops.fusion_cams(torch.from_numpy(intrs).float()[:, :3, :3], torch.from_numpy(c2ws).float())[:, 21:],
                          c2ws[:, :3, 3].astype(np.float32).astype(np.float64))
    with pytest.raises(ValueError, match="fusion_cams"):
        ops.fusion_cams(intrs[:2], c2ws)
    with pytest.raises(ValueError, match="fusion_cams"):
        ops.fusion_cams(intrs, c2ws[:, :3])
    with pytest.raises(ValueError, match="singular"):
        ops.fusion_cams(intrs, np.zeros_like(c2ws))
    with pytest.raises(ValueError, match="not finite"):
        ops.fusion_cams(intrs * np.nan, c2ws)
    # host tensors: there is no CPU path
    with pytest.raises(ValueError, match="no CPU path"):
        ops.fuse_depth_maps(torch.from_numpy(depth), cams)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.fuse_depth_maps(depth, cams)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.fused_points(torch.zeros(3, 5, 7, dtype=torch.float64), cams, torch.zeros(3, 5, 7, dtype=torch.uint8))
    # pairs and thresholds (the helper both fuse_depth_maps and fuse_surface call first)
    ok = ops.fusion_request("t", 3, None, 1.0, 0.01, 3, False, None)
    assert np.array_equal(ok[0], FR.default_pairs(3)) and ok[0].dtype == np.int32 and ok[1:] == (1.0, 0.01, 3, None)
    assert np.array_equal(ops.fusion_request("t", 3, [[1, -1], [2, 0], [-1, -1]], 0, 0, 1, True, 0.5)[0], [[1, -1], [2, 0], [-1, -1]])
    for pairs in ([[0], [0], [0]], [[1], [3], [0]], [[1], [-2], [0]], [[1], [0]], [1, 0, 0], [[1.0], [0.0], [0.0]]):
        with pytest.raises(ValueError, match="pairs"):
            ops.fusion_request("t", 3, pairs, 1.0, 0.01, 3, False, None)
    for kw in ({"pix_tol": -1.0}, {"pix_tol": float("nan")}, {"rel_tol": float("inf")}, {"rel_tol": -0.01}, {"min_views": 0}, {"min_views": 1.5},
               {"normal_cos": 0.5}, {"normal_cos": 1.5, "has_normal": True}, {"normal_cos": float("nan"), "has_normal": True}):
        args = {"pix_tol": 1.0, "rel_tol": 0.01, "min_views": 3, "has_normal": False, "normal_cos": None, **kw}
        with pytest.raises(ValueError):
            ops.fusion_request("t", 3, None, args["pix_tol"], args["rel_tol"], args["min_views"], args["has_normal"], args["normal_cos"])


def test_point_clouds_round_trip_through_the_ply_writer(tmp_path):
    from gens_amd import io as gio
    rng = np.random.default_rng(0)
    pts = rng.normal(size=(37, 3))
    nrm = rng.normal(size=(37, 3)).astype(np.float32)
    col = rng.integers(0, 256, (37, 3)).astype(np.uint8)
    path = str(tmp_path / "cloud.ply")
    gio.write_point_cloud(path, pts)
    v, t, attrs = gio.read_ply(path, attributes=True)
    assert np.array_equal(v, pts.astype(np.float32)) and t.shape == (0, 3) and attrs == {}
    gio.write_point_cloud(path, pts, normals=nrm, colors=col)
    v, t, attrs = gio.read_ply(path, attributes=True)
    assert np.array_equal(v, pts.astype(np.float32)) and t.shape == (0, 3)
    assert np.array_equal(attrs["normals"], nrm) and np.array_equal(attrs["colors"], col) and attrs["colors"].dtype == np.uint8
    gio.write_point_cloud(path, pts, colors=col)
    assert sorted(gio.read_ply(path, attributes=True)[2]) == ["colors"]
    gio.write_point_cloud(path, np.zeros((0, 3)), normals=np.zeros((0, 3), np.float32), colors=np.zeros((0, 3), np.uint8))
    v, t, attrs = gio.read_ply(path, attributes=True)
    assert v.shape == (0, 3) and t.shape == (0, 3) and attrs["normals"].shape == (0, 3) and attrs["colors"].shape == (0, 3)
    gio.write_point_cloud(path, np.zeros((0, 3)))
    assert gio.read_ply(path)[0].shape == (0, 3)
    with pytest.raises(ValueError):
        gio.write_point_cloud(path, pts, normals=nrm[:5])
