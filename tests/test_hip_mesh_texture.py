"""GPU tests of the texture atlases (K34): the five kernels against the numpy restatement (tests/mesh_texture_reference.py), bit for bit, with
chunks that split triangles and planted inputs; out-of-range indices; empty cases launch nothing; ImplicitSurface.texture_mesh on the g23
model's cell-2 simplified R = 64 mesh against the restatement driven by the device's blend_views, against vertex_attributes at the corners,
for every chunking and with a snap; extract_geometry(texture=) on the three routes; validate, the conf key and the written OBJ; nothing
changes when the option is unset; the refusals."""
import warnings

import numpy as np
import pytest
import torch

from . import mesh_texture_reference as TR

gpu = pytest.mark.gpu
F = np.float32
SNAP = {"gens_texture_snap", "gens_texture_keep_better"}
K34 = {"gens_texture_points", "gens_texture_pack", "gens_texture_uv"} | SNAP


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _same_floats(a, b):
    """Equal bits wherever either is a number (signed zeros and subnormals included) and NaN in the same places: which NaN an operation
    returns (its sign and payload) is not fixed by IEEE 754, and the host and the device choose differently."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    nan = np.isnan(a)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and a[~nan].tobytes() == b[~nan].tobytes()


def _planted_mesh(t, seed):
    """t triangles on t + 2 random vertices (neighbours share edges), with a degenerate triangle, one with a repeated vertex, signed zeros,
    the smallest positive floats and a NaN vertex planted where the mesh is large enough to hold them."""
    rng = np.random.default_rng(seed)
    pts = rng.standard_normal((t + 2, 3)).astype(F)
    tri = (np.arange(t, dtype=np.int32)[:, None] + np.arange(3, dtype=np.int32)[None]).astype(np.int32)
    if t >= 3:
        pts[0] = (0.0, -0.0, np.finfo(F).smallest_subnormal)
        pts[1] = (-0.0, np.finfo(F).tiny, -np.finfo(F).smallest_subnormal)
        tri[1] = (2, 2, 2)                                          # degenerate
        tri[2] = (3, 1, 3)                                          # a repeated vertex
    if t >= 65:
        pts[40] = (np.nan, 0.5, -0.5)                               # the triangles 38, 39, 40 touch it
        tri[64] = tri[7]                                            # a repeated triangle
    return pts, tri


def _chunks(n, t):
    return [c for c in dict.fromkeys((1, 7, 64, n)) if c >= 1] if t else [1]


@gpu
@pytest.mark.parametrize("s", [3, 4, 8])
@pytest.mark.parametrize("t", [0, 1, 2, 3, 65, 257])
def test_points_pack_and_uv_equal_the_restatement(t, s):
    from gens_amd import ops
    pts, tri = _planted_mesh(t, seed=100 * t + s)
    h, w, _, _, p = TR.layout(t, s)
    n = t * p
    want_pts, want_edge = TR.texture_points(pts, tri, s, with_edge=True)
    rng = np.random.default_rng(t + s)
    n_src = 1 + (t + s) % 3
    color = (rng.random((n, 3)) * 1.5 - 0.25).astype(F)
    if n > 8:
        color[:8, 0] = (np.nan, np.inf, -np.inf, 1.0, 0.99999994, -0.0, 0.00390625, 1e-45)
    vis = (rng.random((n, n_src)) < 0.3).astype(np.uint8) * rng.integers(1, 256, (n, n_src)).astype(np.uint8)
    want_atlas, want_seen = TR.texture_pack(color, vis, t, s)
    d_pts, d_tri = torch.from_numpy(pts).cuda(), torch.from_numpy(tri).cuda()
    d_color, d_vis = torch.from_numpy(color).cuda(), torch.from_numpy(vis).cuda()
    assert ops.texture_layout(t, s) == (h, w, *TR.layout(t, s)[2:])
    for chunk in _chunks(n, t):
        got_pts, got_edge = [], []
        atlas = torch.zeros(h, w, 3, device="cuda", dtype=torch.uint8)
        seen = torch.zeros(h, w, device="cuda", dtype=torch.uint8)
        for s0 in range(0, n, chunk):
            s1 = min(s0 + chunk, n)
            a, b = ops.texture_points(d_pts, d_tri, s, s0, s1, with_edge=True)
            got_pts.append(a)
            got_edge.append(b)
            if s0 % (3 * chunk) == 0:                               # (without the edge: the same points)
                assert torch.equal(ops.texture_points(d_pts, d_tri, s, s0, s1).view(torch.int32), a.view(torch.int32))
            ops.texture_pack(d_color[s0:s1], d_vis[s0:s1], t, s, s0, s1, atlas=atlas, seen=seen)
        got_pts = torch.cat(got_pts).cpu().numpy() if got_pts else np.zeros((0, 3), F)
        got_edge = torch.cat(got_edge).cpu().numpy() if got_edge else np.zeros(0, F)
        assert _same_floats(got_pts, want_pts) and _same_floats(got_edge, want_edge), chunk
        assert _same(atlas.cpu().numpy(), want_atlas) and _same(seen.cpu().numpy(), want_seen), chunk
    whole = ops.texture_pack(d_color, d_vis, t, s)                  # new arrays: zeroed where no triangle owns the texel
    assert _same(whole[0].cpu().numpy(), want_atlas) and _same(whole[1].cpu().numpy(), want_seen)
    assert _same(ops.texture_uv(t, s, "cuda").cpu().numpy(), TR.texture_uv(t, s))
    if t >= 65:
        assert np.isnan(want_pts[38 * p:41 * p]).any() and np.isfinite(want_pts[41 * p:]).all()
        assert _same(want_pts[64 * p:65 * p], want_pts[7 * p:8 * p])


@gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_snap_equals_the_restatement(n):
    from gens_amd import ops
    rng = np.random.default_rng(n)
    pts = rng.standard_normal((n, 3)).astype(F)
    value = (rng.standard_normal(n) * 0.1).astype(F)
    grad = rng.standard_normal((n, 3)).astype(F)
    limit = np.abs(rng.standard_normal(n) * 0.1).astype(F)
    if n >= 63:
        value[:4] = (np.nan, np.inf, -np.inf, 0.0)
        grad[4], grad[5], grad[6], grad[7] = (np.nan, 1, 1), (np.inf, 0, 0), (0, 0, 0), (-0.0, 0.0, -0.0)
        grad[8], value[8] = (1e-30, 0, 0), 1e-30                    # |grad|^2 underflows nowhere in float64
        grad[9], value[9] = (3e38, 3e38, 3e38), 1.0
        limit[10:13] = (np.nan, np.inf, 0.0)
        pts[13] = (np.nan, 0.0, -0.0)
    for threshold in (0.0, 0.05, -0.3):
        for kw in ({"limit": limit}, {"max_move": 0.08}, {"max_move": float("inf")}):
            want, want_taken = TR.texture_snap(pts, value, grad, threshold, **kw)
            d = torch.from_numpy(pts).cuda()
            taken = ops.texture_snap(d, torch.from_numpy(value).cuda(), torch.from_numpy(grad).cuda(), threshold,
                                     **{k: torch.from_numpy(v).cuda() if k == "limit" else v for k, v in kw.items()})
            assert _same_floats(d.cpu().numpy(), want) and _same(taken.cpu().numpy().astype(bool), want_taken), (threshold, list(kw))
            assert n < 63 or (0 < want_taken.sum() < n)


@gpu
@pytest.mark.parametrize("n", [1, 64, 65, 1000])
def test_keep_better_equals_the_restatement(n):
    from gens_amd import ops
    rng = np.random.default_rng(n)
    cur = [rng.standard_normal((n, 3)).astype(F), (rng.standard_normal(n) * 0.1).astype(F), rng.standard_normal((n, 3)).astype(F)]
    prev = [rng.standard_normal((n, 3)).astype(F), (rng.standard_normal(n) * 0.1).astype(F), rng.standard_normal((n, 3)).astype(F)]
    if n >= 64:
        cur[1][:8] = (np.nan, 0.5, np.nan, 0.25, -0.25, 0.0, -0.0, np.inf)
        prev[1][:8] = (0.5, np.nan, np.nan, 0.25, 0.25, -0.0, 1e-45, np.inf)
    for threshold in (0.0, 0.05, -0.3):
        want = TR.texture_keep_better(*cur, *prev, threshold)
        d = [torch.from_numpy(a.copy()).cuda() for a in cur]
        back = ops.texture_keep_better(*d, *[torch.from_numpy(a).cuda() for a in prev], threshold)
        assert all(_same_floats(a.cpu().numpy(), b) for a, b in zip(d, want[:3])) and _same(back.cpu().numpy().astype(bool), want[3]), threshold
        assert n < 64 or (0 < want[3].sum() < n)
    if n >= 64:                                                     # (NaN now, NaN before, NaN both: back; equal |g|: kept)
        assert TR.texture_keep_better(*cur, *prev)[3][:8].tolist() == [True, True, True, False, False, False, False, False]


@gpu
def test_out_of_range_indices_give_nan_points_and_are_not_read_through():
    from gens_amd import ops
    pts = torch.from_numpy(np.random.default_rng(0).standard_normal((5, 3)).astype(F)).cuda()
    i32 = np.iinfo(np.int32)
    tri = np.array([[0, 1, 2], [0, 1, 5], [-1, 1, 2], [0, i32.max, 2], [i32.min, 1, 2], [4, 3, 2], [1 << 30, 1 << 30, 1 << 30]], np.int32)
    got, edge = ops.texture_points(pts, torch.from_numpy(tri).cuda(), 4, with_edge=True)
    want, want_edge = TR.texture_points(pts.cpu().numpy(), tri, 4, with_edge=True)
    assert _same_floats(got.cpu().numpy(), want) and _same_floats(edge.cpu().numpy(), want_edge)
    bad = np.repeat(np.array([False, True, True, True, True, False, True]), 10)
    assert np.isnan(want[bad]).all() and np.isfinite(want[~bad]).all() and np.isnan(want_edge[bad]).all()
    # no vertices at all: every index is out of range
    none = ops.texture_points(torch.zeros(0, 3, device="cuda"), torch.from_numpy(tri).cuda(), 4)
    assert torch.isnan(none).all()


@gpu
def test_empty_cases_launch_nothing():
    from gens_amd import lib as L, ops
    from .test_hip_vertex_attrs import NETWORK, _scene, _surface
    surf, vols = _surface("f32")
    _, views = _scene(surf, 3)
    pts = torch.zeros(4, 3, device="cuda")
    none, one = torch.zeros(0, 3, device="cuda", dtype=torch.int32), torch.tensor([[0, 1, 2]], device="cuda", dtype=torch.int32)
    L.profile_begin(only=K34 | NETWORK)
    assert ops.texture_points(pts, none, 8).shape == (0, 3)
    got = ops.texture_points(pts, one, 8, 17, 17, with_edge=True)
    assert got[0].shape == (0, 3) and got[1].shape == (0,)
    assert ops.texture_snap(torch.zeros(0, 3, device="cuda"), torch.zeros(0, device="cuda"), torch.zeros(0, 3, device="cuda"), max_move=1.0).shape == (0,)
    z3, z1 = torch.zeros(0, 3, device="cuda"), torch.zeros(0, device="cuda")
    assert ops.texture_keep_better(z3, z1, z3.clone(), z3.clone(), z1.clone(), z3.clone()).shape == (0,)
    atlas, seen = ops.texture_pack(torch.zeros(0, 3, device="cuda"), torch.zeros(0, 2, device="cuda", dtype=torch.uint8), 0, 8)
    assert atlas.shape == (0, 0, 3) and seen.shape == (0, 0)
    atlas, seen = ops.texture_pack(torch.zeros(0, 3, device="cuda"), torch.zeros(0, 2, device="cuda", dtype=torch.uint8), 1, 8, 5, 5)
    assert atlas.shape == (8, 9, 3) and not atlas.any() and not seen.any()
    assert ops.texture_uv(0, 8, "cuda").shape == (0, 3, 2)
    out = surf.texture_mesh(np.zeros((4, 3)), np.zeros((0, 3), np.int32), vols, views, texels=8, snap=2)
    assert out["texture"].shape == (0, 0, 3) and out["texture_seen"].shape == (0, 0) and out["texture_uv"].shape == (0, 3, 2)
    assert out["texture"].dtype == np.uint8 and out["texture_seen"].dtype == bool and out["texture_uv"].dtype == F
    assert surf.last_texture_stats == {"H": 0, "W": 0, "samples": 0, "unseen": 0.0, "snap": 2, "snap_skipped": 0, "snap_reverted": 0}
    assert not L.profile_end(raw=True)
    lib = L.load()
    assert lib.gens_texture_points(None, 0, None, 0, 8, 0, 0, None, None, None) == 0
    assert lib.gens_texture_snap(None, None, None, None, 1.0, 0.0, 0, None, None) == 0
    assert lib.gens_texture_keep_better(None, None, None, None, None, None, 0.0, 0, None, None) == 0
    assert lib.gens_texture_pack(None, None, 1, 0, 8, 0, 0, None, None, None) == 0
    assert lib.gens_texture_uv(0, 8, None, None) == 0


# ------------------------------------------------------------------------------------------------------------------------------------
# the model: the g23 surface and the synthetic views of tests/test_hip_vertex_attrs.py, R = 64, the cell-2 simplified mesh
# ------------------------------------------------------------------------------------------------------------------------------------
R = 64
ROUTES = (("dense", {}), ("lattice", {"sparse": 4}), ("mesh", {"sparse": 4, "sparse_mesh": True}))
_MODEL = {}


def _model(precision):
    """The surface at this precision (set on every call: the model is shared), and once per precision its R = 64 mesh simplified at cell 2
    on the device, as float32 points in the model's frame, with a Lipschitz bound that holds by construction."""
    from gens_amd import ops
    from .test_hip_sparse_lattice import _l_obs
    from .test_hip_vertex_attrs import _bounds, _scene, _surface
    surf, vols = _surface(precision)
    if precision not in _MODEL:
        _, views = _scene(surf, 3)
        lo, hi = _bounds()
        u = surf.sdf_grid(vols, lo, hi, R)
        dv, dt = ops.marching_cubes(u, 0.0)
        sv, st, _, _ = ops.simplify_mesh(dv, dt, 2.0, origin=(-0.5, -0.5, -0.5))
        span = (hi.cpu().numpy() - lo.cpu().numpy()).astype(np.float64).tolist()
        points = ops.vertex_points(sv, R, span, lo.cpu().numpy().astype(np.float64).tolist())
        _MODEL[precision] = dict(vols=vols, views=views, lo=lo, hi=hi, lipschitz=3 ** 0.5 * _l_obs(u, R) * (1 + 1e-3), points=points, tri=st,
                                 points_np=points.cpu().numpy(), tri_np=st.cpu().numpy())
    return {"surf": surf, **_MODEL[precision]}


def _same_dict(a, b):
    return sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)


@gpu
@pytest.mark.parametrize("precision", ["f32", "f16x2"])
def test_texture_mesh_equals_the_restatement_and_vertex_attributes_at_the_corners(precision):
    from gens_amd import lib as L, ops
    m = _model(precision)
    surf, vols, views, pts, tri = m["surf"], m["vols"], m["views"], m["points_np"], m["tri_np"]
    t = len(tri)
    assert t > 500
    for s in (8, 5):
        h, w, _, _, p = TR.layout(t, s)
        L.profile_begin(only=K34)
        out = surf.texture_mesh(m["points"], m["tri"], vols, views, texels=s)
        assert {k for k, *_ in L.profile_end(raw=True)} == K34 - SNAP
        assert sorted(out) == ["texture", "texture_seen", "texture_uv"]
        assert out["texture"].shape == (h, w, 3) and out["texture"].dtype == np.uint8 and out["texture_seen"].dtype == bool
        # the restatement, driven by the device's blend_views on the restatement's points
        samples = TR.texture_points(pts, tri, s)
        with torch.no_grad():
            rgb, vis = ops.blend_views(surf._fused_blend_plan(views), views, torch.from_numpy(samples).cuda())
        atlas, seen = TR.texture_pack(rgb.cpu().numpy(), vis.cpu().numpy(), t, s)
        assert _same(out["texture"], atlas) and _same(out["texture_seen"], seen.astype(bool)) and _same(out["texture_uv"], TR.texture_uv(t, s))
        stats = surf.last_texture_stats
        assert stats == {"H": h, "W": w, "samples": t * p, "unseen": 1.0 - float(seen.sum()) / (t * p), "snap": 0, "snap_skipped": 0,
                         "snap_reverted": 0}
        print(f"{precision} texels {s}: {t} faces, atlas {h} x {w}, unseen {stats['unseen']:.4f}")
        # the three corner texels of every face: vertex_attributes' colours and seen at that face's vertices
        attrs = surf.vertex_attributes(m["points"], vols, views, ("colors",))
        face = np.arange(t)[:, None]
        x, y = TR.pixel(t, s, face, np.array([[0, s - 2, 0]]), np.array([[0, 0, s - 2]]))
        assert _same(out["texture"][y, x], attrs["colors"][tri]) and _same(out["texture_seen"][y, x], attrs["seen"][tri])
        # numpy inputs (float64 points, int64 triangles) give the same atlas
        assert _same_dict(surf.texture_mesh(pts.astype(np.float64), tri.astype(np.int64), vols, views, texels=s), out)


@gpu
@pytest.mark.parametrize("precision", ["f32", "f16x2"])
def test_texture_mesh_does_not_depend_on_the_chunk(precision):
    m = _model(precision)
    surf, vols, views = m["surf"], m["vols"], m["views"]
    for kw in ({"texels": 4}, {"texels": 4, "snap": 1}):
        whole = surf.texture_mesh(m["points"], m["tri"], vols, views, **kw)
        stats = surf.last_texture_stats
        for chunk in (64, 1000):
            assert _same_dict(surf.texture_mesh(m["points"], m["tri"], vols, views, chunk=chunk, **kw), whole), (kw, chunk)
            assert surf.last_texture_stats == stats


@gpu
@pytest.mark.parametrize("precision", ["f32", "f16x2"])
def test_snap_does_not_raise_g_where_the_step_was_taken(precision):
    """With snap = 2, |g| at the snapped interior texel points is no larger than before on every texel whose step was taken; the skipped
    and turned-back counts are reported.  No bound on |g| itself is asserted: none can be derived (Newton's method promises nothing from a
    chord point).  g is the snap's own evaluator's.  The guard (ops.texture_keep_better) is what makes this hold at the evaluator's
    resolution: without it, at f16x2, 2 of 58 604 moved texels went from |g| = 6.0e-8 = 2^-24 to 1.2e-7 (measured on an MI355X)."""
    from gens_amd import lib as L, ops
    m = _model(precision)
    surf, views, pts, tri = m["surf"], m["views"], m["points"], m["tri"]
    vols = ops.VolumeSet.packed(m["vols"])
    s, t = 8, len(m["tri_np"])
    p = TR.layout(t, s)[4]
    before, skipped0, reverted0 = surf._texture_samples(pts, tri, vols, s, 0, None, 0.0, 1 << 21)
    L.profile_begin(only=K34)
    after, skipped, reverted = surf._texture_samples(pts, tri, vols, s, 2, None, 0.0, 1 << 21)
    assert {k for k, *_ in L.profile_end(raw=True)} == {"gens_texture_points"} | SNAP
    assert skipped0 == 0 and reverted0 == 0 and 0 <= skipped <= 2 * t * p and 0 <= reverted <= 2 * t * p
    assert _same(before.cpu().numpy(), TR.texture_points(m["points_np"], m["tri_np"], s))

    def g(q):                                                       # the snap's own evaluator: the lattice's value + gradient launch
        with torch.no_grad():
            plan = surf._fused_plan(vols)
            sdf = ops.sdf_mlp(plan, vols, q, want_grad=True, precision=surf._precision(plan, True))[0]
        return sdf.reshape(-1).double().abs().cpu().numpy()

    g0, g2 = g(before), g(after)
    ip, jp = TR.local_texels(s)
    interior = np.tile(ip + jp <= s - 2, t)
    moved = (before != after).any(dim=1).cpu().numpy()
    worse = moved & interior & ~(g2 <= g0)
    print(f"{precision}: {t * p} samples, {int(moved.sum())} moved, {skipped} of {2 * t * p} steps skipped, {reverted} turned back; interior |g| median {np.median(g0[interior]):.3e} -> "
          f"{np.median(g2[interior]):.3e}, max {g0[interior].max():.3e} -> {g2[interior].max():.3e}; {int(worse.sum())} moved interior texels with a larger |g|"
          + (f" (largest |g| after among them {g2[worse].max():.3e}, before {g0[worse].max():.3e})" if worse.any() else ""))
    assert moved.any() and not worse.any()
    # texture_mesh reports the count and colours the snapped points
    out = surf.texture_mesh(pts, tri, m["vols"], views, texels=s, snap=2)
    assert surf.last_texture_stats["snap"] == 2 and surf.last_texture_stats["snap_skipped"] == skipped
    assert surf.last_texture_stats["snap_reverted"] == reverted
    with torch.no_grad():
        rgb, vis = ops.blend_views(surf._fused_blend_plan(views), views, after)
    atlas, seen = TR.texture_pack(rgb.cpu().numpy(), vis.cpu().numpy(), t, s)
    assert _same(out["texture"], atlas) and _same(out["texture_seen"], seen.astype(bool))
    # one max_move for all: a tiny one skips every step but those of length 0 (g = 0 exactly) and leaves the plain atlas
    tiny = surf.texture_mesh(pts, tri, m["vols"], views, texels=s, snap=2, max_move=1e-30)
    zero_steps = 2 * t * p - surf.last_texture_stats["snap_skipped"]
    print(f"{precision}: max_move = 1e-30 leaves {zero_steps} steps of length 0")
    assert 0 <= zero_steps <= 2 * int((g0 == 0).sum()) and _same_dict(tiny, surf.texture_mesh(pts, tri, m["vols"], views, texels=s))


@gpu
def test_extract_geometry_returns_the_texture_of_the_returned_mesh_on_every_route():
    from gens_amd import lib as L
    from .test_hip_vertex_attrs import _same as same_attrs
    m = _model("f32")
    surf, vols, views, lo, hi = m["surf"], m["vols"], m["views"], m["lo"], m["hi"]
    surf.lattice_lipschitz = m["lipschitz"]
    try:
        for simplify in (None, 2):
            first = None
            plain = surf.extract_geometry(vols, lo, hi, R, 0.0, simplify=simplify)
            for route, kw in ROUTES:
                with warnings.catch_warnings():
                    warnings.simplefilter("error")
                    L.profile_begin(only=K34)
                    got = surf.extract_geometry(vols, lo, hi, R, 0.0, views=views, simplify=simplify, texture=8, **kw)
                    assert {k for k, *_ in L.profile_end(raw=True)} == K34 - SNAP, route
                assert route == "dense" or not surf.last_lattice_stats["fell_back"]
                assert len(got) == 4 and got[2] is None and _same(got[0], plain[0]) and _same(got[1], plain[1]), (route, simplify)
                stats = surf.last_texture_stats
                # the same dict as texture_mesh of the returned mesh (whose float32 rounding is what was textured)
                assert _same_dict(got[3], surf.texture_mesh(got[0], got[1], vols, views, texels=8)), (route, simplify)
                assert surf.last_texture_stats == stats and stats["samples"] == 36 * len(got[1])
                first = first or got[3]
                assert _same_dict(got[3], first), (route, simplify)
        # with attributes: the attribute dict keeps its place; a dict of keywords; the attribute does what the keyword does
        v, t, attrs, tex = surf.extract_geometry(vols, lo, hi, R, 0.0, views=views, simplify=2, attributes=("normals", "colors"), texture={"texels": 5, "snap": 1})
        assert same_attrs(attrs, surf.vertex_attributes(v, vols, views))
        assert _same_dict(tex, surf.texture_mesh(v, t, vols, views, texels=5, snap=1))
        three = surf.extract_geometry(vols, lo, hi, R, 0.0, views=views, simplify=2, attributes=("normals", "colors"))
        assert len(three) == 3 and _same(three[0], v) and _same(three[1], t) and same_attrs(three[2], attrs)
        surf.mesh_texture = {"texels": 5, "snap": 1}
        try:
            again = surf.extract_geometry(vols, lo, hi, R, 0.0, views=views, simplify=2)
            assert len(again) == 4 and again[2] is None and _same_dict(again[3], tex)
            assert len(surf.extract_geometry(vols, lo, hi, R, 0.0, views=views, simplify=2, texture=0)) == 2
        finally:
            del surf.mesh_texture
        # this call's threshold is the snap's level set
        v, t, _, tex = surf.extract_geometry(vols, lo, hi, R, 0.01, views=views, simplify=2, texture={"texels": 4, "snap": 1})
        assert _same_dict(tex, surf.texture_mesh(v, t, vols, views, texels=4, snap=1, threshold=0.01))
        assert not _same_dict(tex, surf.texture_mesh(v, t, vols, views, texels=4, snap=1))
    finally:
        surf.lattice_lipschitz = 2.0


@gpu
def test_validate_the_conf_key_and_the_written_obj(tmp_path):
    from gens_amd import io as gio
    from gens_amd.config import Conf, gens_model_conf
    from gens_amd.models.gens import GenS
    from .test_hip_vertex_attrs import TODAYS_KEYS, _validate_args
    m = _model("f32")
    surf, vols, views = m["surf"], m["vols"], m["views"]
    args = _validate_args(surf, vols)
    torch.manual_seed(3)
    ref = surf.validate(*args, extract_geometry=True, mesh_resolution=R, mesh_simplify=2)
    torch.manual_seed(3)
    out = surf.validate(*args, extract_geometry=True, mesh_resolution=R, mesh_simplify=2, mesh_texture=8)
    assert set(out) == TODAYS_KEYS | {"texture", "texture_seen", "texture_uv"}
    for k in TODAYS_KEYS:
        assert torch.equal(torch.as_tensor(out[k]), torch.as_tensor(ref[k])), k
    want = surf.texture_mesh(out["vertices"], out["triangles"], vols, views, texels=8)
    assert _same_dict({k: out[k] for k in want}, want)
    torch.manual_seed(3)
    both = surf.validate(*args, extract_geometry=True, mesh_resolution=R, mesh_simplify=2, mesh_texture={"texels": 8}, mesh_attributes=("normals",))
    assert set(both) == set(out) | {"vertex_normals"} and _same_dict({k: both[k] for k in want}, want)
    surf.mesh_texture = 8
    try:
        torch.manual_seed(3)
        again = surf.validate(*args, extract_geometry=True, mesh_resolution=R, mesh_simplify=2)
        assert _same_dict({k: again[k] for k in want}, want)
    finally:
        del surf.mesh_texture
    # the conf key reaches the attribute (and its absence leaves the class default)
    conf = gens_model_conf(volume_dims=(16, 8, 4), has_vol=True)
    assert "mesh_texture" not in vars(GenS(conf).implicit_surface)
    assert GenS(Conf({**conf, "mesh_texture": 16})).implicit_surface.mesh_texture == 16
    assert GenS(Conf({**conf, "mesh_texture": {"texels": 16, "snap": 2}})).implicit_surface.mesh_texture == {"texels": 16, "snap": 2}
    # the writer: an OBJ beside the PLY, in world coordinates, unseen texels mid-grey
    scale = torch.eye(4)
    scale[:3, :3] = torch.diag(torch.tensor([1.5, 1.0, 0.75]))
    scale[:3, 3] = torch.tensor([0.5, -1.0, 2.0])
    inputs = {"scene": "scan1", "file_name": "scan1_view0", "scale_mat": scale}
    paths = gio.save_validation_outputs(str(tmp_path), both, inputs, "epoch0")
    assert paths["obj"].endswith("meshes/scan1_epoch0.obj") and paths["texture"].endswith("meshes/scan1_epoch0.png")
    back = gio.read_obj(paths["obj"])
    assert _same(back["vertices"], gio.transform_vertices(both["vertices"], scale.numpy()).astype(F)) and _same(back["triangles"], both["triangles"])
    assert _same(back["uv"], both["texture_uv"])
    assert _same(back["normals"], gio.transform_normals(both["vertex_normals"], scale.numpy()).astype(F))
    assert _same(back["texture"], np.where(both["texture_seen"][:, :, None], both["texture"], np.uint8(128)))
    assert _same(gio.read_ply(paths["mesh"])[1], both["triangles"])
    with pytest.raises(ValueError, match="texture_mesh"):
        gio.save_validation_outputs(str(tmp_path / "clean"), both, {**inputs, "masks": None}, "epoch0", clean=True)
    assert not (tmp_path / "clean").exists()


@gpu
def test_nothing_changes_when_the_option_is_unset():
    from gens_amd import lib as L
    from gens_amd.models.modules.implicit_surface import ImplicitSurface
    from .test_hip_vertex_attrs import TODAYS_KEYS, _same as same_attrs, _validate_args
    assert ImplicitSurface.mesh_texture is None and ImplicitSurface.last_texture_stats is None
    m = _model("f32")
    surf, vols, views, lo, hi = m["surf"], m["vols"], m["views"], m["lo"], m["hi"]
    assert "mesh_texture" not in vars(surf)
    surf.lattice_lipschitz = m["lipschitz"]
    L.profile_begin(only=K34)
    try:
        for route, kw in ROUTES:
            plain = surf.extract_geometry(vols, lo, hi, R, 0.0, attributes=("normals", "colors"), views=views, simplify=2, **kw)
            for off in ({"texture": None}, {"texture": False}, {"texture": 0}):
                got = surf.extract_geometry(vols, lo, hi, R, 0.0, attributes=("normals", "colors"), views=views, simplify=2, **kw, **off)
                assert len(got) == 3 and _same(got[0], plain[0]) and _same(got[1], plain[1]) and same_attrs(got[2], plain[2]), (route, off)
            bare = surf.extract_geometry(vols, lo, hi, R, 0.0, **kw, texture=0)
            assert len(bare) == 2 and _same(bare[0], surf.extract_geometry(vols, lo, hi, R, 0.0, **kw)[0])
    finally:
        surf.lattice_lipschitz = 2.0
    args = _validate_args(surf, vols)
    torch.manual_seed(3)
    ref = surf.validate(*args, extract_geometry=True, mesh_resolution=33)
    torch.manual_seed(3)
    off = surf.validate(*args, extract_geometry=True, mesh_resolution=33, mesh_texture=0)
    assert not L.profile_end(raw=True)
    assert set(ref) == set(off) == TODAYS_KEYS
    for k in TODAYS_KEYS:
        assert torch.equal(torch.as_tensor(off[k]), torch.as_tensor(ref[k])), k


@gpu
def test_refusals_come_before_any_launch():
    from gens_amd import lib as L, ops
    from .test_hip_brick_mcubes import K29
    from .test_hip_sparse_lattice import K28
    from .test_hip_vertex_attrs import NETWORK, _validate_args
    m = _model("f32")
    surf, vols, views, lo, hi, pts, tri = m["surf"], m["vols"], m["views"], m["lo"], m["hi"], m["points"], m["tri"]
    L.profile_begin(only=K34 | K28 | K29 | NETWORK | {"gens_compact_valid", "gens_mc_classify", "gens_mc_emit", "gens_lattice_points", "gens_vertex_points"})
    for kw in ({"texels": 2}, {"texels": 65}, {"texels": 8.0}, {"texels": True}, {"snap": -1}, {"snap": 0.5}, {"max_move": 0}, {"max_move": -1.0},
               {"max_move": float("nan")}):
        with pytest.raises(ValueError):
            surf.texture_mesh(pts, tri, vols, views, **kw)
        with pytest.raises(ValueError):
            surf.extract_geometry(vols, lo, hi, 33, 0.0, views=views, texture=kw)
        with pytest.raises(ValueError):
            surf.validate(*_validate_args(surf, vols), extract_geometry=True, mesh_resolution=33, mesh_texture=kw)
    for bad in (True, 2, 65, 8.5, "8", {"texel": 8}):
        with pytest.raises(ValueError):
            surf.extract_geometry(vols, lo, hi, 33, 0.0, views=views, texture=bad)
    with pytest.raises(ValueError, match="needs the scene's views"):
        surf.texture_mesh(pts, tri, vols, None)
    with pytest.raises(ValueError, match="needs the scene's views"):
        surf.extract_geometry(vols, lo, hi, 33, 0.0, texture=8)
    with pytest.raises(ValueError, match="SceneViews"):
        surf.texture_mesh(pts, tri, vols, object())
    with pytest.raises(ValueError, match="threshold"):
        surf.texture_mesh(pts, tri, vols, views, threshold=float("nan"))
    with pytest.raises(ValueError, match="expected \\(T, 3\\)"):
        surf.texture_mesh(pts, tri.reshape(-1), vols, views)
    six = ops.VolumeSet.packed([torch.zeros(1, 4, 4, 4, 4, device="cuda") for _ in range(6)])
    with pytest.raises(ValueError, match="1 to 5 packed volume levels, not 6"):
        surf.texture_mesh(pts, tri, six, views, snap=1)              # (the snap needs the gradient kernels; colours alone do not)
    surf.fused_blend = False
    try:
        with pytest.raises(ValueError, match="fused blending kernel"):
            surf.texture_mesh(pts, tri, vols, views)
    finally:
        surf.fused_blend = True
    # the atlas limit, from the face count alone: 5 M faces (whose vertices need not exist) at 32 texels
    many = torch.zeros(5_000_000, 3, device="cuda", dtype=torch.int32)
    with pytest.raises(ValueError, match="5000000 faces.*fits is %d.*simplify" % ops.texture_fit(5_000_000)):
        surf.texture_mesh(pts, many, vols, views, texels=32)
    for kw in ({"texels": 2}, {"s0": -1}, {"s0": 5, "s1": 4}, {"s1": 10 ** 9}):
        with pytest.raises(ValueError):
            ops.texture_points(pts, tri, **{"texels": 8, **kw})
    for p_, t_ in ((pts.double(), tri), (pts, tri.long()), (pts[:, :2], tri), (pts.cpu(), tri), (pts, tri.cpu())):
        with pytest.raises(ValueError):
            ops.texture_points(p_, t_, 8)
    with pytest.raises(ValueError, match="max_move"):
        ops.texture_snap(pts.clone(), pts[:, 0], pts)
    with pytest.raises(ValueError, match="in place"):
        ops.texture_snap(pts.double(), pts[:, 0], pts, max_move=1.0)
    with pytest.raises(ValueError, match="gradients"):
        ops.texture_snap(pts.clone(), pts[:, 0], pts[:-1], max_move=1.0)
    with pytest.raises(ValueError, match="samples"):
        ops.texture_pack(torch.zeros(5, 3, device="cuda"), torch.zeros(5, 2, device="cuda", dtype=torch.uint8), 1, 8, 0, 6)
    with pytest.raises(ValueError, match="atlas"):
        ops.texture_pack(torch.zeros(5, 3, device="cuda"), torch.zeros(5, 2, device="cuda", dtype=torch.uint8), 1, 8, 0, 5,
                         atlas=torch.zeros(8, 8, 3, device="cuda", dtype=torch.uint8), seen=torch.zeros(8, 9, device="cuda", dtype=torch.uint8))
    assert not L.profile_end(raw=True)
