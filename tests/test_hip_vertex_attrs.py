"""GPU tests of the per-vertex mesh attributes (K30): the two kernels against their restatement (tests/vertex_attrs_reference.py);
ImplicitSurface.vertex_attributes against the chain written out by hand, bit for bit; the three extraction routes; the defaults; the
refusals; what the normals mean on a real mesh; validate and save_validation_outputs end to end.  The argument checks need no device."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from . import vertex_attrs_reference as VR

gpu = pytest.mark.gpu

K30 = {"gens_vertex_points", "gens_vertex_pack"}
NETWORK = {"gens_sdf_mlp", "gens_sdf_grad", "gens_sdf_grad_f16", "gens_sdf_grad_bf16x3", "gens_blend_views", "gens_blend_views_bf16x3", "gens_blend_views_t",
           "gens_lattice_points", "gens_mc_classify"}
BOX_LO, BOX_HI = (-1.0, -0.5, -0.25), (1.0, 0.75, 0.5)           # a non-cubic box: every axis has its own span and corner
TAG = ("c", "g23c_filter_volume")      # the CPU oracle's gradient norm at this mesh's vertices: 0.60 .. 1.43 at R = 33 and R = 64 (all three g23 tags alike)


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. gens_vertex_points
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("r", [2, 33, 2049])
def test_vertex_points_are_the_float32_rounding_of_the_host_expression(r):
    """Bit-equal to numpy.float32 of extract_geometry's host expression, float32 bound difference included: the definition is un-fused
    IEEE double arithmetic with one rounding, so equality is the bar."""
    from gens_amd import ops
    lo, hi = np.array(BOX_LO, dtype=np.float32), np.array(BOX_HI, dtype=np.float32)
    span = (hi - lo).astype(np.float64).tolist()                 # as extract_geometry hands it over: the float32 difference, widened
    rng = np.random.default_rng(r)
    for n in (0, 1, 63, 64, 65, 257):
        v = rng.integers(0, r - 1, (n, 3)).astype(np.float64) + rng.uniform(0.0, 1.0, (n, 3))       # integer plus fraction, up to R - 1
        v[: n // 4] = np.floor(v[: n // 4])
        if n > 2:
            v[-1], v[-2] = r - 1.0, 0.0
        assert v.size == 0 or (v.min() >= 0 and v.max() <= r - 1)
        got = ops.vertex_points(torch.from_numpy(v).cuda(), r, span, lo.astype(np.float64).tolist())
        want = VR.points(v, r, lo, hi)
        assert got.dtype == torch.float32 and got.shape == (n, 3)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), (r, n)


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. gens_vertex_pack
# ------------------------------------------------------------------------------------------------------------------------------------
def _pack_inputs(s):
    """The CPU edge rows (every flag row of S views beside them) followed by 1 000 seeded random rows -> grad, color, vis."""
    eg, ec = VR.edge_rows()
    fl = VR.flag_rows(s)
    rg, rc, rv = VR.random_rows(1000, s, seed=100 + s)
    return (np.concatenate([eg, rg]), np.concatenate([ec, rc]), np.concatenate([fl[np.arange(len(eg)) % len(fl)], rv]))


@gpu
@pytest.mark.parametrize("s", [1, 2, 4])
def test_vertex_pack_equals_the_restatement(s):
    """Colours and seen exact; normals within one float32 unit in the last place of the float64 restatement (<= 2^-23 absolute, |n| <= 1:
    one rounding of a correctly rounded double quotient), zero rows exactly zero."""
    from gens_amd import ops
    grad, color, vis = _pack_inputs(s)
    for n in (1, 31, 32, 33, 64, 65, 257, len(grad)):
        g, c, f = (torch.from_numpy(a[:n].copy()).cuda() for a in (grad, color, vis))
        normals, colors, seen = ops.vertex_pack(g, c, f)
        assert normals.dtype == torch.float32 and colors.dtype == torch.uint8 and seen.dtype == torch.uint8
        want64 = VR.normals64(grad[:n])
        got = normals.cpu().numpy()
        err = np.abs(got.astype(np.float64) - want64)
        print(f"S={s} n={n}: largest normal error {err.max():.3e} (bound {2.0 ** -23:.3e})")
        assert err.max() <= 2.0 ** -23
        zero = ~want64.any(axis=1)
        assert zero.any() or n < 2
        assert np.array_equal(got[zero].view(np.uint32), np.zeros_like(got[zero]).view(np.uint32))
        assert np.array_equal(colors.cpu().numpy(), VR.colors(color[:n]))
        assert np.array_equal(seen.cpu().numpy().astype(bool), VR.seen(vis[:n]))


@gpu
def test_vertex_pack_with_one_input_writes_only_its_outputs():
    from gens_amd import lib as L, ops
    grad, color, vis = _pack_inputs(2)
    n = 257
    g, c, f = (torch.from_numpy(a[:n].copy()).cuda() for a in (grad, color, vis))
    both = ops.vertex_pack(g, c, f)
    u8 = torch.uint8
    normals = torch.full((n, 3), -7.0, device="cuda")
    colors, seen = torch.full((n, 3), 201, device="cuda", dtype=u8), torch.full((n,), 201, device="cuda", dtype=u8)
    L.call("gens_vertex_pack", L.ptr(g), None, None, 0, n, L.ptr(normals), L.ptr(colors, u8), L.ptr(seen, u8), L.stream())        # normals alone
    assert torch.equal(normals, both[0]) and bool((colors == 201).all()) and bool((seen == 201).all())
    normals.fill_(-7.0)
    L.call("gens_vertex_pack", None, L.ptr(c), L.ptr(f, u8), 2, n, L.ptr(normals), L.ptr(colors, u8), L.ptr(seen, u8), L.stream())  # colours alone
    assert bool((normals == -7.0).all()) and torch.equal(colors, both[1]) and torch.equal(seen, both[2])
    # the operator's forms
    only_n = ops.vertex_pack(grad=g)
    assert torch.equal(only_n[0], both[0]) and only_n[1] is None and only_n[2] is None
    only_c = ops.vertex_pack(color=c, vis=f.bool())
    assert only_c[0] is None and torch.equal(only_c[1], both[1]) and torch.equal(only_c[2], both[2])
    empty = ops.vertex_pack(g[:0], c[:0], f[:0])
    assert [tuple(t.shape) for t in empty] == [(0, 3), (0, 3), (0,)]
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.vertex_pack(g.cpu(), c, f)
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.vertex_points(torch.zeros(4, 3, dtype=torch.float64), 33, [2.0] * 3, [-1.0] * 3)
    with pytest.raises(ValueError):
        ops.vertex_pack()
    with pytest.raises(ValueError):
        ops.vertex_pack(color=c)


def test_entry_points_report_bad_arguments_without_a_gpu():
    """Arguments are checked before any launch: -1 with a message for null pointers, a negative n, resolution < 2; n == 0 succeeds."""
    from gens_amd import lib as L
    lib = L.load()
    p = lambda k: C.c_void_p(0x7e0000000000 + 4096 * k)  # noqa: E731  (made-up addresses: never dereferenced by the host code)
    box = (2.0, 2.0, 2.0, -1.0, -1.0, -1.0)

    def refused(rc, *words):
        msg = lib.gens_last_error().decode()
        assert rc == -1 and all(w in msg for w in words), (rc, msg)

    refused(lib.gens_vertex_points(None, 5, 33, *box, p(1), None), "gens_vertex_points", "null")
    refused(lib.gens_vertex_points(p(0), 5, 33, *box, None, None), "gens_vertex_points", "null")
    refused(lib.gens_vertex_points(p(0), -1, 33, *box, p(1), None), "gens_vertex_points", "-1 vertices")
    refused(lib.gens_vertex_points(p(0), 5, 1, *box, p(1), None), "gens_vertex_points", "resolution 1")
    assert lib.gens_vertex_points(None, 0, 33, *box, None, None) == 0
    assert lib.gens_vertex_points(p(0), (1 << 31) + 5, 33, *box, p(1), None) == -2
    refused(lib.gens_vertex_pack(None, None, None, 2, 5, p(3), p(4), p(5), None), "gens_vertex_pack", "null")
    refused(lib.gens_vertex_pack(p(0), None, None, 0, 5, None, p(4), p(5), None), "gens_vertex_pack", "null")
    refused(lib.gens_vertex_pack(None, p(1), None, 2, 5, None, p(4), p(5), None), "gens_vertex_pack", "null")
    refused(lib.gens_vertex_pack(None, p(1), p(2), 2, 5, None, None, p(5), None), "gens_vertex_pack", "null")
    refused(lib.gens_vertex_pack(None, p(1), p(2), 2, 5, None, p(4), None, None), "gens_vertex_pack", "null")
    refused(lib.gens_vertex_pack(p(0), p(1), p(2), 0, 5, p(3), p(4), p(5), None), "gens_vertex_pack", "0 source views")
    refused(lib.gens_vertex_pack(p(0), p(1), p(2), 2, -3, p(3), p(4), p(5), None), "gens_vertex_pack", "-3 vertices")
    assert lib.gens_vertex_pack(None, None, None, 0, 0, None, None, None, None) == 0
    assert lib.gens_vertex_pack(p(0), p(1), p(2), 2, (1 << 31) + 5, p(3), p(4), p(5), None) == -2
    assert lib.gens_abi_version() == 12


# ------------------------------------------------------------------------------------------------------------------------------------
# the model: the g23 surface of tests/test_hip_sparse_lattice.py with synthetic views
# ------------------------------------------------------------------------------------------------------------------------------------
_VIEWS = {}


def _surface(precision="f32"):
    from .test_hip_sparse_lattice import _surface as g23_surface
    return g23_surface(*TAG, precision)


def _scene(surf, nv):
    """The seeded scene of `nv` views at 48 x 64 with as many feature levels as the colour network takes -> (dict of device tensors,
    ops.SceneViews); once per view count."""
    from gens_amd import ops, synthetic
    if nv not in _VIEWS:
        n_levels = (surf.color_network.ray_dir_fc[2].weight.shape[0] - 3) // 4
        sc = synthetic.make_scene(nv, h=48, w=64, n_levels=n_levels, seed=11)
        dev = {k: ([f.cuda() for f in v] if isinstance(v, list) else v.cuda()) for k, v in sc.items() if k != "hw"}
        _VIEWS[nv] = (dev, ops.SceneViews(dev["imgs"], dev["intrs"], dev["c2ws"], dev["features"]))
    return _VIEWS[nv]


def _bounds():
    return torch.tensor([-1.0] * 3).cuda(), torch.tensor([1.0] * 3).cuda()


def _by_hand(surf, vols, views, points, chunk):
    """The chain vertex_attributes stands for, written out: float32 points -> ops.sdf_mlp(want_grad=True) -> ops.blend_views -> ops.vertex_pack."""
    from gens_amd import ops
    packed = ops.VolumeSet.packed(vols)
    pts = torch.from_numpy(np.asarray(points)).to(torch.float32).cuda()
    out = [[], [], []]
    with torch.no_grad():
        plan, bplan = surf._fused_plan(packed), surf._fused_blend_plan(views)
        assert plan is not None and bplan is not None
        for s in range(0, len(pts), chunk):
            _, grad = ops.sdf_mlp(plan, packed, pts[s:s + chunk], want_grad=True, precision=surf._precision(plan, True))
            rgb, vis = ops.blend_views(bplan, views, pts[s:s + chunk])
            for acc, part in zip(out, ops.vertex_pack(grad, rgb, vis)):
                acc.append(part)
    assert not surf._split_half_overflowed()                 # (else vertex_attributes would have repeated the pass in float32)
    normals, colors, seen = (torch.cat(a).cpu().numpy() for a in out)
    return {"normals": normals, "colors": colors, "seen": seen.astype(bool)}


def _same(a, b):
    return sorted(a) == sorted(b) and all(a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]) for k in a)


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. plumbing, bit for bit
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("precision", ["f32", "f16x2"])
@pytest.mark.parametrize("nv", [2, 3, 5])
def test_vertex_attributes_are_the_chain_written_out_by_hand(nv, precision):
    """vertex_attributes on an extracted R = 33 mesh equals sdf_mlp -> blend_views -> vertex_pack on the float32 vertices with the same
    chunking, at S = 1 (the general blend kernel), 2 and 4 source views and both precisions -- unchunked and with chunk = 64.
    Chunked against unchunked: the gradient kernel's independence from its batch is measured here (printed).  On an MI355X the largest
    normal difference is 0.000e+00 and the largest colour difference 0 in all six cases (V = 1072), so equality is asserted."""
    surf, vols = _surface(precision)
    _, views = _scene(surf, nv)
    lo, hi = _bounds()
    vertices, triangles = surf.extract_geometry(vols, lo, hi, 33, 0.0)
    v = len(vertices)
    assert v > 128 and v % 64 != 0 and len(triangles) > 0
    whole = surf.vertex_attributes(vertices, vols, views)
    assert whole["normals"].shape == (v, 3) and whole["normals"].dtype == np.float32
    assert whole["colors"].shape == (v, 3) and whole["colors"].dtype == np.uint8
    assert whole["seen"].shape == (v,) and whole["seen"].dtype == bool
    assert _same(whole, _by_hand(surf, vols, views, vertices, 1 << 21))
    parts = surf.vertex_attributes(vertices, vols, views, chunk=64)
    assert _same(parts, _by_hand(surf, vols, views, vertices, 64))
    d_n = float(np.abs(parts["normals"].astype(np.float64) - whole["normals"]).max())
    d_c = int(np.abs(parts["colors"].astype(np.int32) - whole["colors"]).max())
    print(f"nv={nv} {precision}: V={v}, chunk 64 against one chunk: largest normal difference {d_n:.3e}, largest colour difference {d_c}, "
          f"seen {int(whole['seen'].sum())} of {v}")
    assert np.array_equal(parts["seen"], whole["seen"])
    assert d_n == 0.0 and d_c == 0
    # the other input forms: a float32 tensor on the device, one attribute, no vertex
    again = surf.vertex_attributes(torch.from_numpy(vertices).float().cuda(), vols, views, attributes=("colors", "normals"))
    assert _same(again, whole)
    only = surf.vertex_attributes(vertices, vols, attributes="normals")
    assert sorted(only) == ["normals"] and np.array_equal(only["normals"], whole["normals"])
    none = surf.vertex_attributes(np.zeros((0, 3)), vols, views)
    assert none["normals"].shape == (0, 3) and none["normals"].dtype == np.float32 and none["colors"].shape == (0, 3)
    assert none["colors"].dtype == np.uint8 and none["seen"].shape == (0,) and none["seen"].dtype == bool


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. routes
# ------------------------------------------------------------------------------------------------------------------------------------
_ROUTES = {}


def _r64():
    """The R = 64 mesh with attributes on the three routes, extracted once: {"dense" | "lattice" | "mesh": (v, t, attrs, launched)}."""
    if not _ROUTES:
        from gens_amd import lib as L
        from .test_hip_sparse_lattice import _l_obs
        surf, vols = _surface("f32")
        _, views = _scene(surf, 3)
        lo, hi = _bounds()
        r = 64
        surf.lattice_lipschitz = 3 ** 0.5 * _l_obs(surf.sdf_grid(vols, lo, hi, r), r) * (1 + 1e-3)      # holds by construction: no leak
        try:
            for route, kw in (("dense", {}), ("lattice", {"sparse": 4}), ("mesh", {"sparse": 4, "sparse_mesh": True})):
                L.profile_begin(only=K30)
                with warnings.catch_warnings():
                    warnings.simplefilter("error")
                    out = surf.extract_geometry(vols, lo, hi, r, 0.0, attributes=("normals", "colors"), views=views, **kw)
                launched = {k for k, *_ in L.profile_end(raw=True)}
                assert route == "dense" or not surf.last_lattice_stats["fell_back"]
                _ROUTES[route] = (*out, launched)
        finally:
            surf.lattice_lipschitz = 2.0
    return _ROUTES


@gpu
def test_the_three_routes_return_the_same_mesh_and_attributes():
    routes = _r64()
    v0, t0, a0, _ = routes["dense"]
    surf, vols = _surface("f32")
    plain = surf.extract_geometry(vols, *_bounds(), 64, 0.0)
    assert len(plain) == 2 and np.array_equal(plain[0], v0) and np.array_equal(plain[1], t0)      # the mesh itself is today's
    assert len(t0) > 0 and sorted(a0) == ["colors", "normals", "seen"] and len(a0["normals"]) == len(v0)
    for route in ("dense", "lattice", "mesh"):
        v, t, a, launched = routes[route]
        assert launched == K30, route
        assert np.array_equal(v, v0) and np.array_equal(t, t0) and _same(a, a0), route
    # ... and they are vertex_attributes of the returned vertices
    _, views = _scene(surf, 3)
    assert _same(a0, surf.vertex_attributes(v0, vols, views))


@gpu
def test_the_leak_fallback_of_the_brick_route_returns_the_dense_meshs_attributes():
    """lattice_lipschitz = 1e-6 at R = 100, B = 8 (the planted failure of K28's and K29's tests): where the count is positive the call
    warns, takes the dense lattice and returns its mesh with its attributes."""
    from .test_hip_sparse_lattice import GOLDENS, _surface as g23_surface
    lo, hi = _bounds()
    r, b = 100, 8
    fell = 0
    for tag, name in GOLDENS:
        surf, vols = g23_surface(tag, name, "f32")
        _, views = _scene(surf, 3)
        v0, t0, a0 = surf.extract_geometry(vols, lo, hi, r, 0.0, attributes=("normals", "colors"), views=views)
        surf.lattice_lipschitz = 1e-6
        try:
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                v1, t1, a1 = surf.extract_geometry(vols, lo, hi, r, 0.0, sparse=b, sparse_mesh=True, attributes=("normals", "colors"), views=views)
        finally:
            surf.lattice_lipschitz = 2.0
        if surf.last_lattice_stats["fell_back"]:
            fell += 1
            assert [w for w in caught if issubclass(w.category, RuntimeWarning) and "lattice edges" in str(w.message)]
            assert np.array_equal(v0, v1) and np.array_equal(t0, t1) and _same(a0, a1) and len(a1["normals"]) == len(v1)
            break
    assert fell > 0


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. nothing changes when unset    6. refusals    8. validate
# ------------------------------------------------------------------------------------------------------------------------------------
def _validate_args(surf, vols, nv=3):
    """validate's positional arguments for a 24 x 32 image of the seeded scene (every second pixel of its 48 x 64 views)."""
    from gens_amd import synthetic
    sc, _ = _scene(surf, nv)
    rays_o, rays_d = synthetic.make_rays(sc["intrs"].cpu(), sc["c2ws"].cpu(), 48, 64, step=2)
    masks = [torch.ones(1, 1, *v.shape[2:], device="cuda") for v in vols]
    lo, hi = _bounds()
    return (rays_o.cuda(), rays_d.cuda(), sc["near"], sc["far"], vols, masks, sc["imgs"], sc["features"], sc["features"], sc["intrs"], sc["c2ws"], lo, hi,
            (24, 32))


TODAYS_KEYS = {"vertices", "triangles", "color_fine", "img_fine", "normal_img", "sdf_depth", "render_depth"}


@gpu
def test_nothing_changes_when_the_option_is_unset():
    from gens_amd import lib as L
    from gens_amd.config import Conf, gens_model_conf
    from gens_amd.models.gens import GenS
    from gens_amd.models.modules.implicit_surface import ImplicitSurface
    assert ImplicitSurface.mesh_attributes is None
    surf, vols = _surface("f32")
    assert "mesh_attributes" not in vars(surf)
    _, views = _scene(surf, 3)
    lo, hi = _bounds()
    L.profile_begin(only=K30)
    plain = surf.extract_geometry(vols, lo, hi, 33, 0.0)
    assert len(plain) == 2
    for off in (None, ()):
        got = surf.extract_geometry(vols, lo, hi, 33, 0.0, attributes=off, views=views)
        assert len(got) == 2 and np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
    torch.manual_seed(3)
    out = surf.validate(*_validate_args(surf, vols), extract_geometry=True, mesh_resolution=33)
    assert not L.profile_end(raw=True)
    assert set(out) == TODAYS_KEYS and np.array_equal(out["vertices"], plain[0]) and np.array_equal(out["triangles"], plain[1])
    # the attribute selects what the keyword selects, and () switches it off again
    surf.mesh_attributes = ("normals",)
    try:
        L.profile_begin(only=K30)
        v, t, attrs = surf.extract_geometry(vols, lo, hi, 33, 0.0)
        assert {k for k, *_ in L.profile_end(raw=True)} == K30
        assert sorted(attrs) == ["normals"] and np.array_equal(v, plain[0]) and np.array_equal(t, plain[1])
        assert len(surf.extract_geometry(vols, lo, hi, 33, 0.0, attributes=())) == 2
    finally:
        del surf.mesh_attributes
    # the conf key reaches the attribute (and its absence leaves the class default)
    conf = gens_model_conf(volume_dims=(16, 8, 4), has_vol=True)
    assert "mesh_attributes" not in vars(GenS(conf).implicit_surface)
    tuned = GenS(Conf({**conf, "mesh_attributes": ["normals", "colors"]}))
    assert tuned.implicit_surface.mesh_attributes == ("normals", "colors")
    assert GenS(Conf({**conf, "mesh_attributes": "normals"})).implicit_surface.mesh_attributes == ("normals",)


@gpu
def test_refusals_come_before_any_launch():
    from gens_amd import lib as L, ops
    surf, vols = _surface("f32")
    _, views = _scene(surf, 3)
    lo, hi = _bounds()
    pts = np.zeros((5, 3))
    six = ops.VolumeSet.packed([torch.zeros(1, 4, 4, 4, 4, device="cuda") for _ in range(6)])
    L.profile_begin(only=K30 | NETWORK)
    with pytest.raises(ValueError, match="needs the scene's views"):
        surf.vertex_attributes(pts, vols)
    with pytest.raises(ValueError, match="needs the scene's views"):
        surf.extract_geometry(vols, lo, hi, 33, 0.0, attributes=("normals", "colors"))
    with pytest.raises(ValueError, match="the known ones are"):
        surf.vertex_attributes(pts, vols, views, attributes=("normals", "tangents"))
    with pytest.raises(ValueError, match="the known ones are"):
        surf.extract_geometry(vols, lo, hi, 33, 0.0, attributes="uv", views=views)
    with pytest.raises(ValueError, match="1 to 5 packed volume levels, not 6"):
        surf.vertex_attributes(pts, six, views)
    with pytest.raises(ValueError, match="1 to 5 packed volume levels, not 6"):
        surf.extract_geometry(six, lo, hi, 33, 0.0, attributes="normals")
    surf.fused_blend = False
    try:
        with pytest.raises(ValueError, match="fused blending kernel"):
            surf.vertex_attributes(pts, vols, views)
    finally:
        surf.fused_blend = True
    assert not L.profile_end(raw=True)


@gpu
def test_validate_and_the_writer_end_to_end(tmp_path):
    """validate(mesh_attributes=...) -> the three vertex_* outputs beside the mesh; save_validation_outputs(clean, clean_frustum) writes
    them through the cleaning's vertex index, the normals through transform_normals, unseen colours mid-grey."""
    from gens_amd import io as gio
    surf, vols = _surface("f32")
    args = _validate_args(surf, vols)
    torch.manual_seed(3)
    ref = surf.validate(*args, extract_geometry=True, mesh_resolution=33)
    torch.manual_seed(3)
    out = surf.validate(*args, extract_geometry=True, mesh_resolution=33, mesh_attributes=("normals", "colors"))
    assert set(out) == TODAYS_KEYS | {"vertex_normals", "vertex_colors", "vertex_seen"}
    for k in TODAYS_KEYS:
        assert torch.equal(torch.as_tensor(out[k]), torch.as_tensor(ref[k])), k
    n_v = len(out["vertices"])
    assert n_v > 0 and len(out["vertex_normals"]) == n_v and len(out["vertex_colors"]) == n_v and len(out["vertex_seen"]) == n_v
    sc, views = _scene(surf, 3)
    assert _same({k[7:]: out[k] for k in out if k.startswith("vertex_")}, surf.vertex_attributes(out["vertices"], vols, views))
    # unseen vertices exist only if a view's frustum misses part of the box; force a few, so that the grey rule is exercised either way
    seen = out["vertex_seen"].copy()
    seen[::7] = False
    out["vertex_seen"] = seen
    scale = torch.eye(4)
    scale[:3, :3] = torch.diag(torch.tensor([1.5, 1.0, 0.75]))                  # not a uniform scale: the normals need the inverse transpose
    scale[:3, 3] = torch.tensor([0.5, -1.0, 2.0])
    masks = torch.ones(3, 48, 64)
    inputs = {"scene": "scan1", "file_name": "scan1_view0", "scale_mat": scale, "masks": masks, "intrs": sc["intrs"].cpu(), "c2ws": sc["c2ws"].cpu()}
    paths = gio.save_validation_outputs(str(tmp_path), out, inputs, "epoch0", clean=True, clean_frustum=True)
    cv, ct, index = gio.clean_mesh(out["vertices"], out["triangles"], masks, inputs["intrs"], inputs["c2ws"], return_index=True)
    assert 0 < len(index) < n_v and np.array_equal(out["vertices"][index], cv)
    v, t, attrs = gio.read_ply(paths["mesh"], attributes=True)
    assert np.array_equal(v, gio.transform_vertices(cv, scale.numpy()).astype(np.float32)) and np.array_equal(t, ct)
    want_c = np.where(seen[index][:, None], out["vertex_colors"][index], np.uint8(128))
    assert attrs["colors"].dtype == np.uint8 and np.array_equal(attrs["colors"], want_c) and (~seen[index]).any()
    want_n = gio.transform_normals(out["vertex_normals"][index], scale.numpy()).astype(np.float32)
    assert attrs["normals"].dtype == np.float32 and np.array_equal(attrs["normals"], want_n)
    plain = gio.read_ply(paths["mesh"])
    assert len(plain) == 2 and np.array_equal(plain[0], v) and np.array_equal(plain[1], t)


# ------------------------------------------------------------------------------------------------------------------------------------
# 7. meaning
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_normals_are_unit_and_agree_with_the_winding_one_way_or_the_other():
    """On the R = 64 mesh: non-zero normals have unit length to 2^-22; the share of faces whose winding normal (v1 - v0) x (v2 - v0) has a
    positive dot product with the mean of their three vertex normals is >= 0.99 or <= 0.01 -- anything between means the pass reads the
    wrong points.  Faces of area 0 are left out (at most 1 % of them)."""
    v, t, attrs, _ = _r64()["dense"]
    n = attrs["normals"].astype(np.float64)
    length = np.linalg.norm(n, axis=1)
    live = length > 0
    print(f"V={len(v)}: {int((~live).sum())} zero normals, |n| - 1 within {np.abs(length[live] - 1).max():.3e}")
    assert live.mean() > 0.99 and np.abs(length[live] - 1.0).max() <= 2.0 ** -22
    a, b, c = (v[t[:, k]] for k in range(3))
    face = np.cross(b - a, c - a)
    flat = np.linalg.norm(face, axis=1) == 0
    assert flat.mean() <= 0.01
    dots = (face * n[t].mean(axis=1)).sum(axis=1)[~flat]
    share = float((dots > 0).mean())
    print(f"{int(flat.sum())} of {len(t)} faces have no area; +grad sdf agrees with the winding normal on {share:.4f} of the others "
          f"-> {'the same side' if share >= 0.99 else 'opposite sides' if share <= 0.01 else 'NEITHER'}")
    assert share >= 0.99 or share <= 0.01
