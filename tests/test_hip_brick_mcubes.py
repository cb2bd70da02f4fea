"""GPU tests of the brick-sparse marching cubes (K29, ops.brick_marching_cubes): the point launches against gens_lattice_points bit for bit;
the mesh against ops.marching_cubes on the lattice the two-level method builds (tests/sparse_lattice_reference.py's `filled`), exactly, with
the leak count; a lattice whose flat indices pass 2^32 against a dense window of it; the option through ImplicitSurface / GenS / validate on
the frozen volumes of the filter_volume goldens.  The argument checks of the entry points need no device."""
import warnings

import numpy as np
import pytest
import torch

from . import brick_mcubes_reference as BR
from . import sparse_lattice_reference as SR

gpu = pytest.mark.gpu

LO, HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
K29 = {"gens_brick_coarse_points", "gens_brick_points", "gens_brick_active", "gens_brick_emit_flags", "gens_brick_mc_classify", "gens_brick_mc_emit"}


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. coordinates
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("r,b", [(r, b) for r in (9, 10, 33, 100) for b in (4, 8)])
def test_coarse_and_brick_points_are_the_lattice_points_bit_for_bit(r, b):
    from .test_hip_sparse_lattice import check_points_are_the_lattice_points_bit_for_bit
    check_points_are_the_lattice_points_bit_for_bit("brick", r, b)


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. the exact mesh
# ------------------------------------------------------------------------------------------------------------------------------------
_DENSE = {}


def _dense(name, field, r):
    """The dense lattice of a field on the device and on the host, evaluated once per session."""
    from gens_amd import ops
    if (name, r) not in _DENSE:
        d = ops.dense_lattice(field, LO, HI, r, device="cuda")
        _DENSE[name, r] = (d, d.cpu())
    return _DENSE[name, r]


def _check(name, field, r, b, t, lipschitz, chunk=1 << 21):
    """ops.brick_marching_cubes against ops.marching_cubes on the restatement's filled lattice: vertices (bit for bit: a non-finite value
    makes NaN coordinates), triangles, the leak count and the other stats -> (dense lattice, vertices, triangles, stats)."""
    from gens_amd import ops
    dense, host = _dense(name, field, r)
    us, act, _ = SR.filled(host, r, b, t, SR.margin(LO, HI, r, b, lipschitz))
    v0, t0 = ops.marching_cubes(us.cuda(), t)
    v1, t1, stats = ops.brick_marching_cubes(field, LO, HI, r, t, b, lipschitz, chunk=chunk, device="cuda")
    assert v1.dtype == torch.float64 and t1.dtype == torch.int32 and v1.shape == v0.shape and t1.shape == t0.shape, (v1.shape, v0.shape, t1.shape, t0.shape)
    assert torch.equal(_bits(v1), _bits(v0)) and torch.equal(t1, t0)
    c, nb, _ = SR.dims(r, b)
    assert stats["leaks"] == SR.leaks(us, act, r, b, t) and stats["fell_back"] is False
    assert stats["coarse_points"] == c ** 3 and stats["bricks"] == nb ** 3 and stats["active_bricks"] == int(act.sum())
    assert stats["emitting_bricks"] == int(BR.emitting(act).sum())
    assert stats["evaluated_points"] == c ** 3 + (int(SR.point_brick_flags(act, r, b).sum()) * b ** 3 if stats["emitting_bricks"] else 0)
    return dense, v1, t1, stats


SMOOTH = [("sphere", SR.sphere(0.5), 0.0), ("two_spheres", SR.two_spheres, 0.0), ("two_spheres", SR.two_spheres, 0.05), ("plane", SR.plane, 0.0)]
MESH_SIZES = [(r, b) for r in (9, 10, 33, 65, 100) for b in (4, 8)] + [(33, 2), (33, 3), (33, 5)]


@gpu
@pytest.mark.parametrize("r,b", MESH_SIZES)
def test_smooth_fields_give_the_mesh_of_the_filled_lattice(r, b):
    """Under lipschitz = 1 the filled lattice's mesh is the dense lattice's as well (K28's claim), which is checked here too; a small chunk at
    R = 100 makes the bricks span several evaluation calls."""
    from gens_amd import ops
    for name, field, t in SMOOTH:
        dense, v, tri, stats = _check(name, field, r, b, t, 1.0, chunk=30000 if r == 100 else 1 << 21)
        assert tri.shape[0] > 0 and stats["leaks"] == 0
        vd, td = ops.marching_cubes(dense, t)
        assert torch.equal(vd, v) and torch.equal(td, tri)
        if r == 100:
            assert stats["active_bricks"] <= stats["emitting_bricks"] < stats["bricks"]


@gpu
def test_a_failed_bound_is_counted_and_the_mesh_is_still_the_filled_lattices():
    """The sphere at R = 100, B = 8 under lipschitz = 1e-6 (leaks, as K28's test of that case establishes), and lattice noise under 0.05."""
    _, _, _, stats = _check("sphere", SR.sphere(0.5), 100, 8, 0.0, 1e-6)
    assert stats["leaks"] > 0
    noise = BR.noise_lattice(33, 33)
    for b in (4, 8):
        _, _, tri, stats = _check("noise", BR.lookup_field(noise), 33, b, 0.0, 0.05, chunk=30000)
        print(f"noise at R = 33, B = {b}: {stats['leaks']} leaks, {stats['active_bricks']} of {stats['bricks']} bricks active, {tri.shape[0]} triangles")
        # (the issue quotes 85 leaks at B = 4 for its own noise tensor, which it does not give; this seeded one has 77 and 281 -- _check holds
        # the device count to the restatement's either way)
        assert tri.shape[0] > 0 and stats["leaks"] == {4: 77, 8: 281}[b]


@gpu
def test_every_brick_active_gives_the_dense_mesh():
    from gens_amd import ops
    noise = BR.noise_lattice(33, 33)
    for b in (4, 8):
        dense, v, tri, stats = _check("noise", BR.lookup_field(noise), 33, b, 0.0, 100.0)
        assert stats["active_bricks"] == stats["bricks"] == stats["emitting_bricks"] and stats["leaks"] == 0
        vd, td = ops.marching_cubes(dense, 0.0)
        assert torch.equal(vd, v) and torch.equal(td, tri) and tri.shape[0] > 0


@gpu
@pytest.mark.parametrize("b", [4, 8])
def test_non_finite_values_at_corners_and_inside_active_bricks(b):
    r = 33
    vals = SR.sphere(0.5)(SR.lattice(r)).reshape(r, r, r).clone()
    corners = [((8, 8, 8), float("nan")), ((8, 16, 16), float("inf")), ((24, 16, 16), float("-inf")), ((16, 24, 16), float("nan")), ((0, 0, 0), float("inf")),
               ((32, 32, 32), float("-inf"))]
    inside = [((9, 17, 18), float("nan")), ((25, 17, 17), float("inf")), ((17, 25, 15), float("-inf")), ((15, 17, 9), float("nan")), ((17, 7, 17), float("inf"))]
    for at, v in corners + inside:
        vals[at] = v
    assert all(i % b == 0 for at, _ in corners for i in at) and all(any(i % 8 for i in at) for at, _ in inside)
    name = f"nonfinite{b}"
    _, v, tri, stats = _check(name, BR.lookup_field(vals), r, b, 0.0, 1.0)
    _, act, _ = SR.filled(_dense(name, None, r)[1], r, b, 0.0, SR.margin(LO, HI, r, b, 1.0))
    owner = SR.per_point(act, r, b)
    assert all(bool(owner[at]) for at, _ in inside)                        # the planted interior points are evaluated ones
    assert tri.shape[0] > 0 and bool(torch.isnan(v).any())                 # and they reach the mesh


@gpu
def test_no_surface_in_the_box_gives_an_empty_mesh():
    for b in (4, 8):
        _, v, tri, stats = _check("inside", SR.sphere(5.0), 33, b, 0.0, 1.0)
        assert v.shape == (0, 3) and tri.shape == (0, 3) and stats["active_bricks"] == 0 and stats["emitting_bricks"] == 0


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. beyond 2^31 lattice points
# ------------------------------------------------------------------------------------------------------------------------------------
def _small_sphere(p):
    """The sphere of radius 0.05 around (0.6, 0.5, 0.4), column by column: a row's value cannot depend on its batch."""
    dx, dy, dz = p[:, 0] - 0.6, p[:, 1] - 0.5, p[:, 2] - 0.4
    return (dx * dx + dy * dy + dz * dz).sqrt().sub(0.05).reshape(-1, 1)


@gpu
def test_a_lattice_beyond_two_to_the_31_equals_a_dense_window_of_it():
    """R = 2049, B = 8: 8.6e9 lattice points, flat indices past 2^32.  The sphere spans 103 cells; the dense 160^3 window of the same lattice
    coordinates around it gives the mesh to compare with.  Vertices: index + t against (window index + t) + origin, two float64 roundings at
    magnitudes below 4096 (2^-41 each): 1e-12.  The dense lattice alone would be 34 GB; the call must stay below 2 GiB."""
    from gens_amd import ops
    r, b, w = 2049, 8, 160
    xs = torch.linspace(-1.0, 1.0, r)
    origin = [int(round((c + 1.0) * 0.5 * (r - 1))) - w // 2 for c in (0.6, 0.5, 0.4)]
    axes = [xs[o:o + w].cuda() for o in origin]
    pts = torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    assert torch.equal(_bits(pts[:: w * w + w + 1]), _bits(torch.cat([ops.lattice_points(LO, HI, r, ((origin[0] + i) * r + origin[1] + i) * r + origin[2] + i, 1,
                                                                                          "cuda") for i in range(w)])))
    window = (-_small_sphere(pts)).reshape(w, w, w)
    v0, t0 = ops.marching_cubes(window, 0.0)
    assert v0.shape[0] - t0.shape[0] // 2 == 2 and t0.shape[0] % 2 == 0 and t0.shape[0] > 10000         # a closed surface of genus 0, on the window first
    inner = (v0.min() > 8) and (v0.max() < w - 9)                                                    # (the sphere is well inside the window)
    assert bool(inner)
    del pts
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    v1, t1, stats = ops.brick_marching_cubes(_small_sphere, LO, HI, r, 0.0, b, 1.0, device="cuda")
    peak = torch.cuda.max_memory_allocated()
    print(f"R = 2049, B = 8: V = {v1.shape[0]}, T = {t1.shape[0]}, {stats['emitting_bricks']} emitting of {stats['bricks']} bricks, "
          f"evaluated share {stats['evaluated_points'] / r ** 3:.2e}, peak allocated {peak / 2 ** 30:.3f} GiB")
    assert torch.equal(t1, t0)
    shift = torch.tensor(origin, dtype=torch.float64, device="cuda")
    assert v1.shape == v0.shape and float((v1 - (v0 + shift)).abs().max()) <= 1e-12
    assert v1.shape[0] - t1.shape[0] // 2 == 2
    assert stats["leaks"] == 0 and stats["coarse_points"] == 257 ** 3 and stats["fell_back"] is False
    assert peak < 2 * 2 ** 30


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. the model
# ------------------------------------------------------------------------------------------------------------------------------------
PRECISIONS = {"f32": ("f32", "transposed"), "f16x2": ("f16x2", "bf16x3"), "bf16x3": ("f32", "bf16x3")}       # sdf_precision, kernels.sdf_value


@gpu
@pytest.mark.parametrize("precision", sorted(PRECISIONS))
def test_extract_geometry_on_the_bricks_equals_the_sparse_lattice_route(precision, monkeypatch):
    from gens_amd import lib as L, ops
    from .test_hip_sparse_lattice import GOLDENS, _bounds, _l_obs, _surface
    prec, generation = PRECISIONS[precision]
    monkeypatch.setattr(ops.kernels, "sdf_value", generation)
    lo, hi = _bounds()
    r = 64
    for tag, name in GOLDENS:
        surf, vols = _surface(tag, name, prec)
        u = surf.sdf_grid(vols, lo, hi, r)
        surf.lattice_lipschitz = 3 ** 0.5 * _l_obs(u, r) * (1 + 1e-3)           # the bound holds by construction: no leak (K28's end-to-end test)
        try:
            v0, t0 = surf.extract_geometry(vols, lo, hi, r, 0.0, sparse=4)
            s0 = dict(surf.last_lattice_stats)
            L.profile_begin(only=K29 | {"gens_mc_classify", "gens_sparse_fill"})
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                v1, t1 = surf.extract_geometry(vols, lo, hi, r, 0.0, sparse=4, sparse_mesh=True)
            launched = {k for k, *_ in L.profile_end(raw=True)}
        finally:
            surf.lattice_lipschitz = 2.0
        s1 = surf.last_lattice_stats
        assert launched == K29                                                    # no lattice was filled, K12 did not run
        assert len(t0) > 0 and isinstance(v1, np.ndarray) and v1.dtype == np.float64 and t1.dtype == np.int32
        assert np.array_equal(v0, v1) and np.array_equal(t0, t1)
        assert s1["leaks"] == 0 and s1["fell_back"] is False and s1["emitting_bricks"] >= s1["active_bricks"] > 0
        assert {k: s1[k] for k in s0} == s0


@gpu
def test_the_option_its_defaults_and_its_refusals():
    from gens_amd import lib as L, ops
    from gens_amd.config import Conf, gens_model_conf
    from gens_amd.distributed import Shard
    from gens_amd.models.gens import GenS
    from gens_amd.models.modules.implicit_surface import ImplicitSurface
    from .test_hip_sparse_lattice import _bounds, _surface
    assert ImplicitSurface.sparse_mesh is None
    surf, vols = _surface("a", "g23_filter_volume", "f32")
    assert "sparse_mesh" not in vars(surf)
    lo, hi = _bounds()
    r = 33
    # with nothing set, and with the sparse lattice alone, no K29 kernel runs
    L.profile_begin(only=K29)
    v0, t0 = surf.extract_geometry(vols, lo, hi, r, 0.0)
    surf.extract_geometry(vols, lo, hi, r, 0.0, sparse=4)
    assert not L.profile_end(raw=True)
    # the refusals, before any launch
    L.profile_begin(only=K29 | {"gens_sparse_coarse_points", "gens_lattice_points"})
    with pytest.raises(ValueError, match="sparse_mesh needs the sparse lattice"):
        surf.extract_geometry(vols, lo, hi, r, 0.0, sparse_mesh=True)
    with pytest.raises(ValueError, match="2 to 8"):
        surf.extract_geometry(vols, lo, hi, r, 0.0, sparse=16, sparse_mesh=True)
    with pytest.raises(ValueError, match="2 to 8"):
        surf.extract_geometry(vols, lo, hi, r, 0.0, sparse=1, sparse_mesh=True)
    assert not L.profile_end(raw=True)
    # the attributes select the route as the keywords do
    surf.sparse_lattice, surf.sparse_mesh, surf.lattice_lipschitz = 4, True, 50.0
    try:
        L.profile_begin(only=K29)
        v1, t1 = surf.extract_geometry(vols, lo, hi, r, 0.0)
        assert {k for k, *_ in L.profile_end(raw=True)} == K29 and surf.last_lattice_stats["emitting_bricks"] > 0
        assert np.array_equal(v0, v1) and np.array_equal(t0, t1)
        L.profile_begin(only=K29)
        surf.extract_geometry(vols, lo, hi, r, 0.0, sparse_mesh=False)
        assert not L.profile_end(raw=True)
        # a shard: one warning, today's sharded route, the same mesh
        sink, got = {}, None
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            L.profile_begin(only=K29)
            for brick in (4, 16):                                                     # (with a shard the brick limit is not in effect either)
                for rank in range(2):
                    got = surf.extract_geometry(vols, lo, hi, r, 0.0, shard=Shard.single(rank, 2, sink), sparse=brick)
            assert not L.profile_end(raw=True)
        assert len([w for w in caught if issubclass(w.category, RuntimeWarning) and "sparse_mesh is not sharded" in str(w.message)]) == 1
        assert np.array_equal(got[0], v0) and np.array_equal(got[1], t0)
    finally:
        surf.sparse_lattice, surf.lattice_lipschitz = None, 2.0
        del surf.sparse_mesh
        for once in ("_warned_sparse_shard", "_warned_sparse_mesh_shard"):     # the surface is shared with other tests: they meet it as new
            vars(surf).pop(once, None)
    # the conf key reaches the attribute (and its absence leaves the class default)
    conf = gens_model_conf(volume_dims=(16, 8, 4), has_vol=True)
    assert "sparse_mesh" not in vars(GenS(conf).implicit_surface)
    tuned = GenS(Conf({**conf, "sparse_lattice": 4, "sparse_mesh": True}))
    assert tuned.implicit_surface.sparse_mesh is True and tuned.implicit_surface.sparse_lattice == 4
    assert GenS(Conf({**conf, "sparse_mesh": False})).implicit_surface.sparse_mesh is False
    assert ops.BRICK_MC_MAX == 8


@gpu
def test_a_bound_that_fails_on_a_real_network_warns_and_returns_the_dense_route_mesh(monkeypatch):
    """lattice_lipschitz = 1e-6 at R = 100, B = 8 on the golden scenes (K28's test of that name): the count equals the restatement's on the
    lattice the method builds; where it is positive the call warns once, naming the count and the bound, and returns the dense mesh.  Beyond
    2^31 lattice points there is no dense lattice: the same count raises."""
    from gens_amd import ops
    from .test_hip_sparse_lattice import GOLDENS, _bounds, _surface
    r, b = 100, 8
    lo, hi = _bounds()
    counted = 0
    for tag, name in GOLDENS:
        surf, vols = _surface(tag, name, "f32")
        u = surf.sdf_grid(vols, lo, hi, r)
        v0, t0 = surf.extract_geometry(vols, lo, hi, r, 0.0)
        us, act, _ = SR.filled(u.cpu(), r, b, 0.0, SR.margin(LO, HI, r, b, 1e-6))
        visible = SR.leaks(us, act, r, b, 0.0)
        surf.lattice_lipschitz = 1e-6
        try:
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                v1, t1 = surf.extract_geometry(vols, lo, hi, r, 0.0, sparse=b, sparse_mesh=True)
        finally:
            surf.lattice_lipschitz = 2.0
        stats = surf.last_lattice_stats
        warned = [w for w in caught if issubclass(w.category, RuntimeWarning) and "lattice edges" in str(w.message)]
        assert stats["leaks"] == visible and stats["emitting_bricks"] == int(BR.emitting(act).sum())
        if visible:
            counted += 1
            assert len(warned) == 1 and str(visible) in str(warned[0].message) and "1e-06" in str(warned[0].message)
            assert stats["fell_back"] is True and np.array_equal(v0, v1) and np.array_equal(t0, t1)
        else:
            assert not warned and stats["fell_back"] is False
    assert counted > 0
    # no dense lattice to fall back to: the leak count must not pass quietly
    empty = (torch.empty(0, 3, dtype=torch.float64, device="cuda"), torch.empty(0, 3, dtype=torch.int32, device="cuda"))
    monkeypatch.setattr(ops, "brick_marching_cubes", lambda *a, **k: (*empty, {"leaks": 3, "evaluated_points": 0, "fell_back": False}))
    with pytest.warns(RuntimeWarning, match="3 lattice edges"):
        with pytest.raises(RuntimeError, match="2\\^31"):
            surf.extract_geometry(vols, lo, hi, 1300, 0.0, sparse=b, sparse_mesh=True)


@gpu
def test_validate_passes_the_option_through(golden):
    from gens_amd import lib as L
    from .test_hip_render import build_surface, scene_inputs
    from .test_hip_sparse_lattice import _l_obs
    g = golden("g9a_render")
    surf = build_surface(g)
    feats, vols, masks, match, _ = scene_inputs(g)
    c = lambda t: t.cuda()  # noqa: E731
    bmin, bmax = torch.tensor([-1.0, -1, -1]), torch.tensor([1.0, 1, 1])
    args = (c(g["rays_o"]), c(g["rays_d"]), c(g["near"]), c(g["far"]), vols, masks, c(g["imgs"]), feats, match, c(g["intrs"]), c(g["c2ws"]), bmin, bmax,
            (4, 6))
    u = surf.sdf_grid(vols, bmin, bmax, 33)
    surf.lattice_lipschitz = 3 ** 0.5 * _l_obs(u, 33) * (1 + 1e-3)
    torch.manual_seed(3)
    L.profile_begin(only=K29)
    ref = surf.validate(*args, extract_geometry=True, mesh_resolution=33, sparse=4)
    assert not L.profile_end(raw=True)
    torch.manual_seed(3)
    L.profile_begin(only=K29)
    out = surf.validate(*args, extract_geometry=True, mesh_resolution=33, sparse=4, sparse_mesh=True)
    assert {k for k, *_ in L.profile_end(raw=True)} == K29
    assert surf.last_lattice_stats["emitting_bricks"] > 0 and not surf.last_lattice_stats["fell_back"]
    for k in ("vertices", "triangles", "color_fine", "sdf_depth"):
        assert torch.equal(torch.as_tensor(out[k]), torch.as_tensor(ref[k])), k


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. argument checks: before any launch, so they run without a device
# ------------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_report_bad_arguments_without_a_gpu():
    import ctypes as C
    from gens_amd import lib as L
    from .test_hip_sparse_lattice import check_shared_refusals
    lib = L.load()
    lo, hi = (C.c_float * 3)(-1, -1, -1), (C.c_float * 3)(1, 1, 1)
    one = C.c_void_p(16)                                                  # a non-null, aligned pointer: every call below is refused before it is used
    calls = {
        "gens_brick_coarse_points": lambda r, b: lib.gens_brick_coarse_points(lo, hi, r, b, 0, 1, one, None),
        "gens_brick_points": lambda r, b: lib.gens_brick_points(lo, hi, r, b, one, 1, 0, 1, one, None),
        "gens_brick_active": lambda r, b: lib.gens_brick_active(one, r, b, 0.0, 0.1, one, None),
        "gens_brick_emit_flags": lambda r, b: lib.gens_brick_emit_flags(one, r, b, one, None),
        "gens_brick_mc_classify": lambda r, b: lib.gens_brick_mc_classify(one, one, one, one, r, b, one, 1, 0.0, one, one, one, one, one, None),
        "gens_brick_mc_emit": lambda r, b: lib.gens_brick_mc_emit(one, one, one, one, r, b, one, 1, 0.0, one, 18, one, one, one, one, one, one, one, one,
                                                                    one, one, None),
    }
    assert set(calls) == {n for n in L.SIGNATURES if n.startswith("gens_brick_")}
    for name, call in calls.items():
        assert call(1, 4) == -1 and b"res = 1" in lib.gens_last_error() and name.encode() in lib.gens_last_error()
        for b in (0, 1, 9, 16):
            assert call(64, b) == -1 and b"brick = %d" % b in lib.gens_last_error()
        assert call(10400, 8) == -2 and b"2^31" in lib.gens_last_error()               # C = 1301: 1301^3 >= 2^31 > 1290^3
        assert call(5161, 4) == -2                                                      # C = 1291 at the other brick
    check_shared_refusals(lib, "gens_brick_coarse_points", "gens_brick_active", "gens_brick_points")
    assert lib.gens_brick_points(lo, hi, 4096, 8, one, 1 << 24, 0, 1 << 24, one, None) == -2 and b"rows" in lib.gens_last_error()   # 2^24 * 512 rows
    assert lib.gens_brick_emit_flags(None, 16, 4, one, None) == -1 and b"null" in lib.gens_last_error()
    assert lib.gens_brick_emit_flags(one, 16, 4, None, None) == -1
    assert lib.gens_brick_mc_classify(one, one, one, one, 16, 4, one, -1, 0.0, one, one, one, one, one, None) == -1
    assert lib.gens_brick_mc_classify(one, one, one, one, 16, 4, one, 1 << 31, 0.0, one, one, one, one, one, None) == -2
    assert lib.gens_brick_mc_classify(one, None, one, one, 16, 4, one, 1, 0.0, one, one, one, one, one, None) == -1 and b"null" in lib.gens_last_error()
    assert lib.gens_brick_mc_classify(one, one, one, one, 16, 4, None, 1, 0.0, one, one, one, one, one, None) == -1 and b"null" in lib.gens_last_error()
    assert lib.gens_brick_mc_classify(one, one, one, one, 16, 4, one, 1, 0.0, one, one, one, C.c_void_p(17), one, None) == -1 and b"misaligned" in lib.gens_last_error()
    assert lib.gens_brick_mc_classify(None, None, None, None, 16, 4, None, 0, 0.0, None, None, None, None, None, None) == 0     # an empty list
    emit = lambda **k: lib.gens_brick_mc_emit(*[k.get(n, one) for n in ("uc", "store", "pslot", "eslot")], 16, 4, k.get("list", one), k.get("n", 1), 0.0,  # noqa: E731
                                              one, k.get("stride", 18), one, one, one, one, k.get("voff", one), one, one, one, one, one, None)
    assert emit(stride=14) == -1 and b"stride" in lib.gens_last_error()
    assert emit(eslot=None) == -1 and b"null" in lib.gens_last_error()
    assert emit(list=None) == -1 and b"null" in lib.gens_last_error()
    assert emit(voff=C.c_void_p(20)) == -1 and b"misaligned" in lib.gens_last_error()
    assert emit(n=-1) == -1 and emit(n=1 << 31) == -2
