"""K34 without a GPU: what the texture-atlas rule guarantees, proved on its numpy restatement (tests/mesh_texture_reference.py): texel
ownership, no bleeding under bilinear filtering, affine reproduction, exact corners, the snap's skip rules; the host-side layout and its
refusals, the OBJ writer, and the argument checks of the C entry points through ctypes with made-up pointers."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from . import mesh_texture_reference as TR

F = np.float32
SIZES = [(s, t) for s in (3, 4, 5, 8, 64) for t in (1, 2, 3, 7)]


def _mesh(t, seed=0):
    """t triangles on 3 t random vertices (no vertex shared, so every face has its own plane)."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((3 * t, 3)).astype(F), np.arange(3 * t, dtype=np.int32).reshape(t, 3)


def _barycentric(n):
    """A dense grid of barycentric weights (m, 3), edges and corners included."""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    keep = i + j <= n
    a, b = i[keep] / n, j[keep] / n
    return np.stack([1.0 - a - b, a, b], axis=-1)


def _owner(s, t):
    """(H, W) int64: the sample that owns each pixel, -1 for none; asserts that no pixel has two owners."""
    h, w, _, _, p = TR.layout(t, s)
    face, ip, jp = TR.sample_faces(s, 0, t * p)
    x, y = TR.pixel(t, s, face, ip, jp)
    assert x.min() >= 0 and x.max() < w and y.min() >= 0 and y.max() < h
    owner = np.full((h, w), -1, dtype=np.int64)
    flat = y * w + x
    assert len(np.unique(flat)) == len(flat), "two samples share a pixel"
    owner[y, x] = np.arange(t * p)
    return owner


@pytest.mark.parametrize("s,t", SIZES)
def test_every_pixel_has_at_most_one_owner_and_owned_pixels_are_t_p(s, t):
    h, w, cols, rows, p = TR.layout(t, s)
    assert p == s * (s + 1) // 2 and h == rows * s and w == cols * (s + 1)
    assert (cols - 1) ** 2 < (t + 1) // 2 <= cols ** 2 and (rows - 1) * cols < (t + 1) // 2 <= rows * cols
    owner = _owner(s, t)
    assert (owner >= 0).sum() == t * p
    # the enumeration: j' outer, i' inner, i' + j' <= S - 1
    ip, jp = TR.local_texels(s)
    assert len(ip) == p and (ip + jp <= s - 1).all() and np.array_equal(np.lexsort((ip, jp)), np.arange(p))


@pytest.mark.parametrize("s,t", SIZES)
def test_bilinear_taps_inside_a_face_are_that_faces_texels(s, t):
    """For a dense grid of barycentric points of every face's uv triangle, edges and corners included, every bilinear tap THAT CARRIES
    WEIGHT is a texel of that face.  A tap's weight is compared with `slack`, the rounding of the float64 arithmetic that forms the
    sampling position from barycentric weights (a few ulps of the texel coordinate, which is below W): on an edge of the uv triangle the
    position is an integer in exact arithmetic and the neighbouring tap has weight 0; rounding can leave it a weight of that order, which
    colours nothing."""
    h, w, _, _, p = TR.layout(t, s)
    owner = _owner(s, t)
    uv = TR.texture_uv(t, s, dtype=np.float64)
    bary = _barycentric(2 * (s - 2) + 3)
    slack = 16 * max(h, w) * np.finfo(np.float64).eps
    for f in range(t):
        at = bary @ uv[f]
        (x0, y0), (fx, fy) = TR.bilinear_taps(at, h, w)
        for dx, dy, wt in ((0, 0, (1 - fx) * (1 - fy)), (1, 0, fx * (1 - fy)), (0, 1, (1 - fx) * fy), (1, 1, fx * fy)):
            live = wt > slack
            xx, yy = x0[live] + dx, y0[live] + dy
            assert (xx >= 0).all() and (xx < w).all() and (yy >= 0).all() and (yy < h).all(), (f, dx, dy)
            assert (owner[yy, xx] // p == f).all(), (f, dx, dy)


@pytest.mark.parametrize("s,t", SIZES)
def test_bilinear_sampling_reproduces_an_affine_function_of_the_texel_points(s, t):
    """Texel colours set to an affine function of the texel's point (float64, no quantisation): sampling at the uv of a barycentric point
    returns the function at that point.  A half-texel error in the points or in the uv would show as an error of the order of the function's
    change over a texel (>= 1e-2 here); the bound is the rounding of the float32 texel points (2^-24 relative, the values are below 8)
    through the function's coefficients (below 4 in sum)."""
    pts, tri = _mesh(t, seed=s)
    h, w, _, _, p = TR.layout(t, s)
    coef, offset = np.array([0.7, -1.3, 1.9]), 0.25
    samples = TR.texture_points(pts, tri, s).astype(np.float64)
    face, ip, jp = TR.sample_faces(s, 0, t * p)
    x, y = TR.pixel(t, s, face, ip, jp)
    image = np.zeros((h, w, 1))
    image[y, x, 0] = samples @ coef + offset
    uv = TR.texture_uv(t, s, dtype=np.float64)
    bary = _barycentric(2 * (s - 2) + 3)
    for f in range(t):
        got = TR.bilinear_sample(image, bary @ uv[f])[:, 0]
        want = (bary @ pts[tri[f]].astype(np.float64)) @ coef + offset
        assert np.abs(got - want).max() <= 4 * 8 * 2.0 ** -24 * 4, f
    # the float32 coordinates the kernels write are those coordinates rounded once
    assert np.array_equal(TR.texture_uv(t, s), uv.astype(F))


@pytest.mark.parametrize("s", (3, 4, 5, 8, 64))
def test_corner_texels_are_the_corners_bit_for_bit(s):
    big = F(2.0 ** 30)
    pts = np.array([[0.1, -0.7, 0.3], [1.3, 0.9, -2.1], [-0.4, 2.2, 0.8],
                    [1.0 + 2.0 ** -23, -3.0, 5e-3], [big * F(1.0 + 2.0 ** -23), big, -big], [-big, 1.0 - 2.0 ** -24, big * F(1.5)]], dtype=F)
    tri = np.array([[0, 1, 2], [3, 4, 5], [2, 2, 1]], dtype=np.int32)
    p = TR.layout(3, s)[4]
    out = TR.texture_points(pts, tri, s)
    ip, jp = TR.local_texels(s)
    corner = [int(np.flatnonzero((ip == a) & (jp == b))[0]) for a, b in ((0, 0), (s - 2, 0), (0, s - 2))]
    for f in range(3):
        for c in range(3):
            assert out[f * p + corner[c]].tobytes() == pts[tri[f, c]].tobytes(), (f, c)
    # texels with i' + j' = S - 1 lie on the plane, outside the triangle
    n = np.cross((pts[1] - pts[0]).astype(np.float64), (pts[2] - pts[0]).astype(np.float64))
    outer = np.flatnonzero(ip + jp == s - 1)
    assert np.abs((out[outer].astype(np.float64) - pts[0]) @ n).max() < 1e-5 * np.linalg.norm(n)
    # a bad index gives NaN points and reads nothing
    bad = TR.texture_points(pts, np.array([[0, 1, 6], [0, -1, 2], [0, 1, 2]], np.int32), s, with_edge=True)
    assert np.isnan(bad[0][:2 * p]).all() and np.isnan(bad[1][:2 * p]).all() and np.isfinite(bad[0][2 * p:]).all()
    assert bad[1][2 * p] == F(np.sqrt(max(((pts[a].astype(np.float64) - pts[b]) ** 2).sum() for a, b in ((0, 1), (1, 2), (2, 0)))))


def test_snap_reduces_g_on_a_sphere_and_skips_what_it_should():
    """g = |p| - 1, grad = p / |p|: the chord points of an inscribed triangle lie inside the sphere; one round puts them on it."""
    rng = np.random.default_rng(5)
    verts = rng.standard_normal((3, 3))
    verts = (verts / np.linalg.norm(verts, axis=1, keepdims=True) * np.array([[1.0], [1.0], [1.0]])).astype(F)
    pts, edge = TR.texture_points(verts, np.array([[0, 1, 2]], np.int32), 8, with_edge=True)
    field = lambda q: (np.linalg.norm(q.astype(np.float64), axis=1) - 1.0).astype(F)  # noqa: E731
    grad = lambda q: (q.astype(np.float64) / np.linalg.norm(q.astype(np.float64), axis=1, keepdims=True)).astype(F)  # noqa: E731
    moved, taken = TR.texture_snap(pts, field(pts), grad(pts), limit=edge)
    assert taken.all()
    before, after = np.abs(field(pts)), np.abs(field(moved))
    assert (after <= before).all() and after.max() < 1e-6 and before.max() > 1e-2
    # a threshold moves the level set: g = sdf + threshold
    moved_t, _ = TR.texture_snap(pts, field(pts), grad(pts), threshold=0.05, limit=edge)
    assert np.abs(field(moved_t) + F(0.05)).max() < 1e-6
    # planted: g not finite, gradient not finite, zero gradient, a step longer than the limit (per sample and one for all), a NaN limit
    p5 = np.tile(np.array([[0.5, 0.0, 0.0]], F), (8, 1))
    value = np.array([np.nan, np.inf, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5], F)
    g5 = np.tile(np.array([[1.0, 0.0, 0.0]], F), (8, 1))
    g5[2] = (np.nan, 0, 0)
    g5[3] = (np.inf, 0, 0)
    g5[4] = 0
    limit = np.array([1, 1, 1, 1, 1, 0.49, 0.5, np.nan], F)
    moved, taken = TR.texture_snap(p5, value, g5, limit=limit)
    assert taken.tolist() == [False] * 6 + [True, False]
    assert np.array_equal(moved[~taken], p5[~taken]) and np.array_equal(moved[6], np.array([0.0, 0.0, 0.0], F))
    assert TR.texture_snap(p5, value, g5, max_move=0.49)[1].sum() == 0 and TR.texture_snap(p5, value, g5, max_move=0.5)[1].tolist() == [False] * 5 + [True] * 3


def test_the_guard_turns_back_steps_that_do_not_lower_g():
    """texture_keep_better on planted values: back where |g| rose or is not a number, kept where it fell or stayed; and a guarded round on
    the sphere turns nothing back."""
    p1, p0 = np.full((6, 3), 1.0, F), np.full((6, 3), 2.0, F)
    g1, g0 = np.full((6, 3), 3.0, F), np.full((6, 3), 4.0, F)
    v1 = np.array([0.2, -0.2, 0.1, np.nan, 0.3, -0.05], F)
    v0 = np.array([0.1, 0.2, -0.2, 0.1, np.nan, 0.05], F)
    pts, val, grad, back = TR.texture_keep_better(p1, v1, g1, p0, v0, g0)
    assert back.tolist() == [True, False, False, True, True, False]
    assert np.array_equal(pts[:, 0], np.where(back, 2.0, 1.0)) and np.array_equal(grad[:, 0], np.where(back, 4.0, 3.0))
    assert np.array_equal(val[~back], v1[~back]) and np.array_equal(val[back][:2], v0[back][:2]) and np.isnan(val[4])
    # the threshold enters both sides: g = sdf + threshold
    assert TR.texture_keep_better(p1, v1, g1, p0, v0, g0, threshold=-0.2)[3].tolist() == [False, True, False, True, True, True]
    verts = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], F)
    chord = TR.texture_points(verts, np.array([[0, 1, 2]], np.int32), 8)
    field = lambda q: (np.linalg.norm(q.astype(np.float64), axis=1) - 1.0).astype(F)  # noqa: E731
    grad_of = lambda q: (q.astype(np.float64) / np.linalg.norm(q.astype(np.float64), axis=1, keepdims=True)).astype(F)  # noqa: E731
    moved, taken = TR.texture_snap(chord, field(chord), grad_of(chord), max_move=2.0)
    assert taken.all() and not TR.texture_keep_better(moved, field(moved), grad_of(moved), chord, field(chord), grad_of(chord))[3].any()


def test_layout_and_its_refusals():
    from gens_amd import ops
    for s, t in SIZES + [(8, 0), (16, 51921), (8, 930404)]:
        assert ops.texture_layout(t, s) == TR.layout(t, s)
    assert ops.texture_layout(0, 8) == (0, 0, 0, 0, 36)
    for bad in (2, 65, 0, -3, 8.0, "8", None, True):
        with pytest.raises(ValueError, match="texels"):
            ops.texture_layout(4, bad)
    with pytest.raises(ValueError, match="faces"):
        ops.texture_layout(-1, 8)
    # the largest tile edge that fits a 16 384-pixel atlas: it fits, the next one does not
    for t in (51921, 930404, 5_000_000):
        s = ops.texture_fit(t)
        assert max(ops.texture_layout(t, s)[:2]) <= ops.TEXTURE_MAX_EDGE
        assert s == ops.TEXTURE_MAX_TEXELS or max(ops.texture_layout(t, s + 1)[:2]) > ops.TEXTURE_MAX_EDGE
    assert ops.texture_fit(200_000_000) is None


class _NoLaunch:
    """Stands for volumes and views in checks that must fail before either is looked at closely."""


def test_texture_request_refuses_before_any_launch():
    """The refusals of ImplicitSurface._texture_request that need no device: they come before the networks or views are touched."""
    from gens_amd import ops
    from gens_amd.config import gens_model_conf
    from gens_amd.models.modules.implicit_surface import ImplicitSurface
    surf = ImplicitSurface(gens_model_conf(volume_dims=(16, 8, 4))["implicit_surface"])
    vols, views = [torch.zeros(1, 4, 4, 4, 4)], _NoLaunch()
    tri = np.zeros((4, 3), np.int32)
    for kw, word in (({"texels": 2}, "texels"), ({"texels": 65}, "texels"), ({"texels": 7.5}, "texels"), ({"snap": -1}, "snap"), ({"snap": 1.5}, "snap"),
                     ({"max_move": 0.0}, "max_move"), ({"max_move": -1.0}, "max_move"), ({"max_move": float("nan")}, "max_move")):
        with pytest.raises(ValueError, match=word):
            surf.texture_mesh(np.zeros((3, 3), F), tri, vols, views, **kw)
    with pytest.raises(ValueError, match="views"):
        surf.texture_mesh(np.zeros((3, 3), F), tri, vols, None)
    with pytest.raises(ValueError, match="SceneViews"):
        surf.texture_mesh(np.zeros((3, 3), F), tri, vols, views)
    # the atlas limit: the message names the face count and a tile edge that really fits, and points at simplify
    n = 5_000_000
    surf._attribute_request = lambda *a, **k: ("colors",)          # (this check is about the atlas; the network limits are K30's)
    with pytest.raises(ValueError) as err:
        surf._texture_request(n, vols, views, texels=32)
    fit = ops.texture_fit(n)
    assert str(n) in str(err.value) and f"fits is {fit}" in str(err.value) and "simplify" in str(err.value)
    assert surf._texture_request(n, vols, views, texels=fit) == (fit, 0, None)
    with pytest.raises(ValueError, match="no tile edge fits"):
        surf._texture_request(200_000_000, vols, views, texels=3)
    # the option of extract_geometry / validate / the conf key
    assert surf._texture_option(None) is None and surf._texture_option(False) is None and surf._texture_option(0) is None
    assert surf._texture_option(8) == {"texels": 8} and surf._texture_option({"texels": 16, "snap": 2}) == {"texels": 16, "snap": 2}
    for bad in (True, 8.5, "8", {"texel": 8}):
        with pytest.raises(ValueError, match="texture"):
            surf._texture_option(bad)
    surf.mesh_texture = 12
    assert surf._texture_option(None) == {"texels": 12} and surf._texture_option(0) is None


def _textured(t=5, s=4, seed=3):
    pts, tri = _mesh(t, seed)
    h, w, _, _, p = TR.layout(t, s)
    rng = np.random.default_rng(seed)
    color = rng.random((t * p, 3)).astype(F)
    vis = (rng.random((t * p, 3)) < 0.4).astype(np.uint8)
    atlas, seen = TR.texture_pack(color, vis, t, s)
    return pts, tri, TR.texture_uv(t, s), atlas, seen.astype(bool)


def test_write_obj_read_obj_round_trip(tmp_path):
    from gens_amd import io
    pts, tri, uv, atlas, seen = _textured()
    normals = np.random.default_rng(1).standard_normal(pts.shape).astype(F)
    for name, nrm, sn in (("plain", None, None), ("full.obj", normals, seen)):
        paths = io.write_obj(str(tmp_path / name), pts, tri, uv, atlas, normals=nrm, seen=sn)
        stem = str(tmp_path / name.replace(".obj", ""))
        assert paths == (stem + ".obj", stem + ".mtl", stem + ".png") and all(os.path.exists(p) for p in paths)
        back = io.read_obj(paths[0])
        assert back["vertices"].tobytes() == pts.tobytes() and np.array_equal(back["triangles"], tri) and back["triangles"].dtype == np.int32
        assert back["uv"].tobytes() == uv.tobytes()
        assert (back["normals"] is None) if nrm is None else back["normals"].tobytes() == nrm.tobytes()
        want = atlas if sn is None else np.where(sn[:, :, None], atlas, np.uint8(128))
        assert np.array_equal(back["texture"], want)
        text = open(paths[0]).read()
        assert text.count("\nvt ") == 3 * len(tri) and f"mtllib {os.path.basename(stem)}.mtl" in text
        assert f"map_Kd {os.path.basename(stem)}.png" in open(paths[1]).read()
    assert (~seen).any() and (np.where(seen[:, :, None], atlas, np.uint8(128)) != atlas).any()       # (the grey rule was exercised)
    with pytest.raises(ValueError, match="corner coordinates"):
        io.write_obj(str(tmp_path / "bad"), pts, tri, uv[:-1], atlas)
    with pytest.raises(ValueError, match="out of range"):
        io.write_obj(str(tmp_path / "bad"), pts[:3], tri, uv, atlas)
    assert not os.path.exists(str(tmp_path / "bad.obj"))


def test_save_validation_outputs_writes_the_obj_and_refuses_cleaning(tmp_path):
    from gens_amd import io
    pts, tri, uv, atlas, seen = _textured()
    depth = np.zeros((12, 16), F)
    outputs = {"vertices": pts.astype(np.float64), "triangles": tri, "img_fine": np.zeros((12, 16, 3)), "normal_img": np.zeros((12, 16, 3)),
               "sdf_depth": depth, "render_depth": depth}
    scale = torch.eye(4)
    scale[:3, 3] = torch.tensor([1.0, 2.0, 3.0])
    inputs = {"scene": "scan24", "file_name": "scan24_view3", "scale_mat": scale}
    plain = io.save_validation_outputs(str(tmp_path / "plain"), outputs, inputs, "epoch7")
    assert sorted(os.listdir(tmp_path / "plain" / "meshes")) == ["scan24_epoch7.ply"] and "obj" not in plain
    textured = {**outputs, "texture": atlas, "texture_seen": seen, "texture_uv": uv}
    paths = io.save_validation_outputs(str(tmp_path / "set"), textured, inputs, "epoch7")
    assert sorted(os.listdir(tmp_path / "set" / "meshes")) == ["scan24_epoch7." + e for e in ("mtl", "obj", "ply", "png")]
    assert {k: v for k, v in paths.items() if k not in ("obj", "mtl", "texture")}.keys() == plain.keys()
    back = io.read_obj(paths["obj"])
    assert np.array_equal(back["vertices"], (pts.astype(np.float64) + np.array([1.0, 2.0, 3.0])).astype(F))       # world coordinates
    assert np.array_equal(back["triangles"], tri) and back["uv"].tobytes() == uv.tobytes()
    assert np.array_equal(back["texture"], np.where(seen[:, :, None], atlas, np.uint8(128)))
    assert np.array_equal(io.read_ply(paths["mesh"])[1], tri)
    with pytest.raises(ValueError, match="texture_mesh"):
        io.save_validation_outputs(str(tmp_path / "clean"), textured, inputs, "epoch7", clean=True)
    assert not os.path.exists(tmp_path / "clean")


def test_entry_points_report_bad_arguments_without_a_gpu():
    """Arguments are checked before any launch: -1 with a message for null pointers, negative counts and bad parameters, -2 for the size
    limits; empty ranges succeed whatever the pointers."""
    from gens_amd import lib as L
    lib = L.load()
    p = lambda k: 0x7e0000000000 + 4096 * k  # noqa: E731  (made-up addresses: never dereferenced by the host code)

    def refused(rc, *words):
        msg = lib.gens_last_error().decode()
        assert rc == -1 and all(w in msg for w in words), (rc, msg)

    points = lambda v=9, t=4, s=8, s0=0, s1=144, pts=p(1), tri=p(2), out=p(3), edge=None: lib.gens_texture_points(  # noqa: E731
        pts, v, tri, t, s, s0, s1, out, edge, None)
    for s in (2, 65, 0, -1):
        refused(points(s=s), "gens_texture_points", "texels")
    refused(points(t=-1), "gens_texture_points", "-1 triangles")
    refused(points(v=-2), "gens_texture_points", "-2 vertices")
    refused(points(s0=-1), "gens_texture_points", "samples")
    refused(points(s0=5, s1=4), "gens_texture_points", "samples")
    refused(points(s1=145), "gens_texture_points", "samples")
    refused(points(tri=None), "gens_texture_points", "null")
    refused(points(out=None), "gens_texture_points", "null")
    refused(points(pts=None), "gens_texture_points", "null")
    assert points(t=1 << 31) == -2 and points(v=1 << 31) == -2
    assert points(t=(1 << 31) - 1, s=64, s1=(1 << 31) + 7) == -2           # one launch takes fewer than 2^31 samples ...
    assert points(s0=77, s1=77, pts=None, tri=None, out=None) == 0 and points(t=0, s1=0, pts=None, tri=None, out=None) == 0
    assert points(t=(1 << 31) - 1, s=64, s0=1 << 40, s1=1 << 40, tri=None, out=None) == 0       # ... at any 64-bit offset

    snap = lambda n=5, pts=p(1), val=p(2), grad=p(3), limit=p(4), mm=0.0, thr=0.0, taken=p(5): lib.gens_texture_snap(  # noqa: E731
        pts, val, grad, limit, mm, thr, n, taken, None)
    refused(snap(n=-1), "gens_texture_snap", "-1 samples")
    refused(snap(limit=None), "gens_texture_snap", "max_move")
    refused(snap(limit=None, mm=-1.0), "gens_texture_snap", "max_move")
    refused(snap(limit=None, mm=float("nan")), "gens_texture_snap", "max_move")
    refused(snap(thr=float("inf")), "gens_texture_snap", "threshold")
    for null in ("pts", "val", "grad", "taken"):
        refused(snap(**{null: None}), "gens_texture_snap", "null")
    assert snap(n=1 << 31) == -2
    assert snap(n=0, pts=None, val=None, grad=None, taken=None) == 0

    keep = lambda n=5, thr=0.0, **null: lib.gens_texture_keep_better(  # noqa: E731
        *[None if k in null else p(i) for i, k in enumerate(("pts", "val", "grad", "ppts", "pval", "pgrad"))], thr, n, None if "rev" in null else p(9), None)
    refused(keep(n=-1), "gens_texture_keep_better", "-1 samples")
    refused(keep(thr=float("nan")), "gens_texture_keep_better", "threshold")
    for null in ("pts", "val", "grad", "ppts", "pval", "pgrad", "rev"):
        refused(keep(**{null: 1}), "gens_texture_keep_better", "null")
    assert keep(n=1 << 31) == -2
    assert keep(n=0, pts=1, val=1, grad=1, ppts=1, pval=1, pgrad=1, rev=1) == 0

    pack = lambda t=4, s=8, s0=0, s1=144, n_src=3, color=p(1), vis=p(2), atlas=p(3), seen=p(4): lib.gens_texture_pack(  # noqa: E731
        color, vis, n_src, t, s, s0, s1, atlas, seen, None)
    for s in (2, 65):
        refused(pack(s=s), "gens_texture_pack", "texels")
    refused(pack(t=-1), "gens_texture_pack", "-1 triangles")
    for n_src in (0, 256, -1):
        refused(pack(n_src=n_src), "gens_texture_pack", "source views")
    refused(pack(s1=145), "gens_texture_pack", "samples")
    refused(pack(s0=-1), "gens_texture_pack", "samples")
    for null in ("color", "vis", "atlas", "seen"):
        refused(pack(**{null: None}), "gens_texture_pack", "null")
    assert pack(t=1 << 31) == -2
    assert pack(s0=9, s1=9, color=None, vis=None, atlas=None, seen=None) == 0

    for s in (2, 65):
        refused(lib.gens_texture_uv(4, s, p(1), None), "gens_texture_uv", "texels")
    refused(lib.gens_texture_uv(-1, 8, p(1), None), "gens_texture_uv", "-1 triangles")
    refused(lib.gens_texture_uv(4, 8, None, None), "gens_texture_uv", "null")
    assert lib.gens_texture_uv(1 << 31, 8, p(1), None) == -2
    assert lib.gens_texture_uv(0, 8, None, None) == 0
