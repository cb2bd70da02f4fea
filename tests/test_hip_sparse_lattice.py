"""GPU tests of the two-level SDF lattice (K28): each kernel against the torch restatement (tests/sparse_lattice_reference.py), exactly;
ops.sparse_lattice on analytic fields; ImplicitSurface.sdf_grid / extract_geometry(sparse=B) on the frozen volumes of the filter_volume
goldens, where the sparse mesh must EQUAL the dense one; the fallback; the defaults.  The argument checks need no device."""
import warnings

import numpy as np
import pytest
import torch

from . import sparse_lattice_reference as SR

gpu = pytest.mark.gpu

LO, HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
BOX_LO, BOX_HI = (-1.0, -0.9, -1.1), (1.0, 1.05, 0.95)          # an uneven box for the point kernels: every axis has its own spacing
SIZES = [(9, 4), (9, 8), (10, 4), (10, 8), (33, 4), (33, 8), (100, 4), (100, 8)]
# the operators both families of entry points have (K28's gens_sparse_*, K29's gens_brick_*): dims, coarse points, brick points, classify
FAMILIES = {"sparse": ("sparse_lattice_dims", "sparse_coarse_points", "sparse_brick_points", "sparse_classify"),
            "brick": ("brick_mc_dims", "brick_coarse_points", "brick_points", "brick_active")}
K28 = {"gens_sparse_coarse_points", "gens_sparse_classify", "gens_sparse_brick_points", "gens_sparse_fill", "gens_sparse_scatter",
       "gens_sparse_leaks"}


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------------------------------
# the kernels, one by one
# ------------------------------------------------------------------------------------------------------------------------------------
def check_points_are_the_lattice_points_bit_for_bit(family, r, b):
    """A family's coarse and brick points against gens_lattice_points (tests/test_hip_brick_mcubes.py runs it for K29's)."""
    from gens_amd import ops
    dims, coarse_points, brick_points = (getattr(ops, n) for n in FAMILIES[family][:3])
    dev = torch.device("cuda")
    full = ops.lattice_points(BOX_LO, BOX_HI, r, 0, r ** 3, dev).cpu().reshape(r, r, r, 3)
    c, _, p = SR.dims(r, b)
    assert dims(r, b) == (c, p)
    ci = SR.coarse_index(r, b)
    want = full[ci][:, ci][:, :, ci].reshape(-1, 3)
    got = coarse_points(BOX_LO, BOX_HI, r, b, 0, c ** 3, dev).cpu()
    assert torch.equal(_bits(got), _bits(want))
    first, count = c ** 3 // 3, c ** 3 - c ** 3 // 3 - 1                                   # a range that starts and ends inside a row
    assert torch.equal(_bits(coarse_points(BOX_LO, BOX_HI, r, b, first, count, dev)), _bits(want[first:first + count]))
    g = torch.Generator().manual_seed(r * 16 + b)
    entries = torch.randperm(p ** 3, generator=g)
    rows = SR.brick_rows(r, b, entries).clamp(max=r - 1)
    want = full[rows[:, 0], rows[:, 1], rows[:, 2]]
    got = brick_points(BOX_LO, BOX_HI, r, b, entries.cuda(), 0, len(entries))
    assert got.shape == (len(entries) * b ** 3, 3) and torch.equal(_bits(got), _bits(want))
    first, count = len(entries) // 2, len(entries) - len(entries) // 2
    got = brick_points(BOX_LO, BOX_HI, r, b, entries.cuda(), first, count)
    assert torch.equal(_bits(got), _bits(want[first * b ** 3:]))


@gpu
@pytest.mark.parametrize("r,b", SIZES)
def test_coarse_and_brick_points_are_the_lattice_points_bit_for_bit(r, b):
    check_points_are_the_lattice_points_bit_for_bit("sparse", r, b)


def _planted_corners(c, t, mrg, seed):
    """(C, C, C) coarse values: two half-spaces far from the threshold on either side (so that most bricks are inactive and the bricks at
    the interface disagree), with corners planted at NaN, +-inf, exactly t, and t +- margin to the last bit."""
    g = torch.Generator().manual_seed(seed)
    uc = torch.where(torch.arange(c)[:, None, None] * 2 < c, 2.0, -2.0).expand(c, c, c).clone() + 0.1 * torch.randn(c, c, c, generator=g)
    t32, m32 = torch.tensor(t, dtype=torch.float32), torch.tensor(mrg, dtype=torch.float32)
    up, down = torch.tensor(float("inf")), torch.tensor(float("-inf"))
    hi, lo = t32 + m32, t32 - m32
    special = [float("nan"), float("inf"), float("-inf"), float(t32), float(hi), float(lo), float(torch.nextafter(hi, up)), float(torch.nextafter(hi, down)),
               float(torch.nextafter(lo, up)), float(torch.nextafter(lo, down)), float(torch.nextafter(t32, up)), float(torch.nextafter(t32, down))]
    where = torch.randperm(c ** 3, generator=g)[:min(len(special), max(1, c ** 3 // 4))]
    uc.view(-1)[where] = torch.tensor(special, dtype=torch.float32)[:len(where)]
    return uc


@gpu
@pytest.mark.parametrize("r,b", SIZES)
def test_classify_equals_the_active_rule(r, b):
    """Both families' classify: SIZES has 2 <= B <= 8 throughout, K29's limit, with the plane brick (R = 9: P == C) and the ragged last brick
    (R = 10)."""
    from gens_amd import ops
    c, nb, _ = SR.dims(r, b)
    seen = set()
    for t in (0.0, 0.05):
        for mrg in (0.0, 0.3):
            for seed in range(3 if c <= 4 else 1):            # (few corners: more draws, so that every planted value is met somewhere)
                uc = _planted_corners(c, t, mrg, 7 * r + b + seed)
                want = SR.active(uc, t, mrg)
                for family in sorted(FAMILIES):
                    got = getattr(ops, FAMILIES[family][3])(uc.cuda(), r, b, t, mrg).cpu().reshape(nb, nb, nb)
                    assert torch.equal(got.bool(), want), (family, t, mrg)
                    assert set(got.unique().tolist()) <= {0, 1}
                seen |= set(want.reshape(-1).tolist())
    if nb > 2:
        assert seen == {False, True}                                   # both answers occur: the comparison above is not vacuous


@gpu
@pytest.mark.parametrize("r,b", SIZES)
def test_fill_scatter_and_leaks_equal_the_restatement(r, b):
    from gens_amd import ops
    c, nb, p = SR.dims(r, b)
    g = torch.Generator().manual_seed(100 * r + b)
    uc = torch.randn(c, c, c, generator=g)
    u = ops.sparse_fill(uc.cuda(), r, b)
    assert u.shape == (r ** 3,) and torch.equal(u.cpu().reshape(r, r, r), SR.fill(uc, r, b))
    # scatter: a random half of the point bricks in random order, in two calls; the rows past R - 1 are dropped, the rest negated
    entries = torch.randperm(p ** 3, generator=g)[:max(1, p ** 3 // 2)]
    rows = SR.brick_rows(r, b, entries)
    sdf = torch.randn(len(rows), generator=g)
    want = u.cpu().clone().reshape(r, r, r)
    own = (rows < r).all(1)
    want[rows[own, 0], rows[own, 1], rows[own, 2]] = -sdf[own]
    half = len(entries) // 2
    e_dev = entries.cuda()
    ops.sparse_scatter(sdf[:half * b ** 3].cuda(), u, r, b, e_dev, 0, half)
    ops.sparse_scatter(sdf[half * b ** 3:].cuda(), u, r, b, e_dev, half, len(entries) - half)
    assert torch.equal(u.cpu().reshape(r, r, r), want)
    # leaks: noise crosses the threshold everywhere, random flags make about three edges in four count
    noise = torch.randn(r, r, r, generator=g)
    noise.view(-1)[torch.randperm(r ** 3, generator=g)[:5]] = torch.tensor([float("nan"), float("inf"), float("-inf"), 0.0, 0.05])
    flags = torch.rand(nb, nb, nb, generator=g) < 0.5
    flags[0, 0, 0] = False                                    # (a single brick must not be the active one)
    for t in (0.0, 0.05):
        got = int(ops.sparse_leaks(noise.cuda(), flags.to(torch.uint8).cuda(), r, b, t))
        assert got == SR.leaks(noise, flags, r, b, t) and got > 0
    assert int(ops.sparse_leaks(noise.cuda(), torch.ones(nb ** 3, dtype=torch.uint8).cuda(), r, b, 0.0)) == 0


# ------------------------------------------------------------------------------------------------------------------------------------
# ops.sparse_lattice on analytic fields
# ------------------------------------------------------------------------------------------------------------------------------------
def _check_against_dense(evaluate, r, b, t, lipschitz, chunk=1 << 21):
    from gens_amd import ops
    dense = ops.dense_lattice(evaluate, LO, HI, r, device="cuda")
    u, stats = ops.sparse_lattice(evaluate, LO, HI, r, t, b, lipschitz, chunk=chunk, device="cuda")
    c, nb, p = SR.dims(r, b)
    d = dense.cpu()
    us, act, _ = SR.filled(d, r, b, t, SR.margin(LO, HI, r, b, lipschitz))
    assert stats["coarse_points"] == c ** 3 and stats["bricks"] == nb ** 3 and stats["active_bricks"] == int(act.sum())
    assert stats["evaluated_points"] == c ** 3 + int(SR.point_brick_flags(act, r, b).sum()) * b ** 3
    assert stats["leaks"] == SR.leaks(us, act, r, b, t)
    return dense, u, stats, us, act


FIELDS = {"sphere": SR.sphere(0.5), "two_spheres": SR.two_spheres}


@gpu
@pytest.mark.parametrize("r,b", [(33, 4), (33, 8), (65, 8), (100, 8), (128, 4)])
@pytest.mark.parametrize("name", sorted(FIELDS))
def test_sparse_lattice_on_analytic_fields_gives_the_dense_mesh(name, r, b):
    from gens_amd import ops
    for t in (0.0, 0.05):
        dense, u, stats, us, act = _check_against_dense(FIELDS[name], r, b, t, 1.0, chunk=1 << 21 if r != 100 else 30000)
        assert stats["leaks"] == 0 and stats["fell_back"] is False
        assert 0 < stats["active_bricks"] and (r < 100 or stats["active_bricks"] < stats["bricks"])
        assert torch.equal(u.cpu(), us)                       # dense on the points active bricks own, the brick's lowest corner elsewhere
        v0, t0 = ops.marching_cubes(dense, t)
        v1, t1 = ops.marching_cubes(u, t)
        assert t0.shape[0] > 0 and torch.equal(v0, v1) and torch.equal(t0, t1)
    if (name, r, b) == ("sphere", 128, 4):
        share = stats["evaluated_points"] / r ** 3
        print(f"evaluated share at 128^3, B = 4: {share:.4f}")
        assert share < 0.25                                   # a cap: the test cannot pass by evaluating everything (the restatement: 0.147 owned points)


@gpu
def test_a_visible_violation_falls_back_to_the_dense_lattice():
    """lipschitz = 1e-6 leaves only the bricks whose corners disagree: the sphere's caps poke through faces of bricks whose corners are all
    outside, next to active bricks -- crossing edges with one endpoint in an inactive brick, which the count must see."""
    from gens_amd import ops
    r, b = 100, 8
    field = FIELDS["sphere"]
    dense = ops.dense_lattice(field, LO, HI, r, device="cuda")
    us, act, _ = SR.filled(dense.cpu(), r, b, 0.0, SR.margin(LO, HI, r, b, 1e-6))
    want = SR.leaks(us, act, r, b, 0.0)
    assert want > 0
    with pytest.warns(RuntimeWarning, match=f"{want} lattice edges.*1e-06"):
        u, stats = ops.sparse_lattice(field, LO, HI, r, 0.0, b, 1e-6, device="cuda")
    assert stats["leaks"] == want and stats["fell_back"] is True and torch.equal(u, dense)
    assert stats["evaluated_points"] > r ** 3


@gpu
def test_a_violation_hidden_inside_one_brick_is_what_the_count_cannot_see():
    """The planted small sphere (radius 0.6 h around one lattice point in the middle of a brick far from the surface, lipschitz = 1): the
    restatement counts its six edges on the DENSE lattice, but no evaluated point is next to it -- the two-level lattice never looks there,
    so the device count, taken on the lattice it built, equals the restatement's count on that same lattice: zero.  (What the count does see:
    test_a_visible_violation_falls_back_to_the_dense_lattice.)"""
    from gens_amd import ops
    r, b = 65, 4
    field, i = SR.planted(r, b)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        dense, u, stats, us, act = _check_against_dense(field, r, b, 0.0, 1.0)
    assert SR.leaks(dense.cpu(), act, r, b, 0.0) == 6 and stats["leaks"] == 0 and not stats["fell_back"]
    assert torch.equal(u.cpu(), us) and float(dense[i, i, i]) > 0.0 > float(u[i, i, i])


# ------------------------------------------------------------------------------------------------------------------------------------
# a real network: the frozen volumes of the filter_volume goldens
# ------------------------------------------------------------------------------------------------------------------------------------
GOLDENS = [("a", "g23_filter_volume"), ("b", "g23_filter_volume"), ("c", "g23c_filter_volume")]
_SCENES = {}


def _scene(tag, name):
    """(model, volumes) of a golden, loaded as tests/test_hip_filter_volume.py loads them; once per session."""
    if tag not in _SCENES:
        from .test_hip_filter_volume import _golden, _golden_model
        g, main = _golden(name), _golden("g23_filter_volume")
        dims = tuple(int(d) for d in g[tag + ".dims"])
        model = _golden_model(dims, int(main["seed"]), {k[3:]: torch.from_numpy(v) for k, v in main.items() if k.startswith("sd.")})
        vols = [torch.from_numpy(g[f"{tag}.volume{i}"]).cuda() for i in range(len(dims))]
        _SCENES[tag] = (model, vols)
    return _SCENES[tag]


def _bounds():
    return torch.tensor([-1.0] * 3).cuda(), torch.tensor([1.0] * 3).cuda()


def _surface(tag, name, precision):
    model, vols = _scene(tag, name)
    surf = model.implicit_surface
    surf.sdf_precision = precision
    surf.sparse_lattice, surf.lattice_lipschitz = None, 2.0
    return surf, vols


@gpu
@pytest.mark.parametrize("precision", ["f32", "f16x2"])
def test_lattice_values_do_not_depend_on_the_batch(precision):
    """The precondition of the end-to-end test: a dense 64^3 lattice through sdf_grid, and the same points evaluated in a seeded random
    permutation (other chunk boundaries, other neighbours in every wave), give the same bits.  Measured on an MI355X: the largest
    difference is 0 at both precisions, so the end-to-end test compares vertices and triangles exactly."""
    from gens_amd import ops
    surf, vols = _surface("c", "g23c_filter_volume", precision)
    lo, hi = _bounds()
    r = 64
    u = surf.sdf_grid(vols, lo, hi, r).reshape(-1)
    packed = ops.VolumeSet.packed(vols)
    pts = ops.lattice_points(LO, HI, r, 0, r ** 3, u.device)
    perm = torch.randperm(r ** 3, generator=torch.Generator().manual_seed(5)).cuda()
    with torch.no_grad():
        plan = surf._fused_plan(packed)
        assert plan is not None
        got = torch.empty(r ** 3, device=u.device)
        for s in range(0, r ** 3, 100003):                   # a chunk that is no multiple of anything
            idx = perm[s:s + 100003]
            got[idx] = -ops.sdf_mlp(plan, packed, pts[idx].contiguous(), precision=surf._precision(plan))[:, 0]
    assert not surf._split_half_overflowed()
    print(f"{precision}: largest difference between the two orders {float((got - u).abs().max()):.3e}")
    assert torch.equal(got, u)


def _l_obs(u, r):
    """The largest |du| / h over all axis-neighbour pairs of finite values (bounds -1 .. 1: one spacing for the three axes)."""
    h = 2.0 / (r - 1)
    worst = 0.0
    for ax in range(3):
        a, b = u.narrow(ax, 0, r - 1).double(), u.narrow(ax, 1, r - 1).double()
        d = (a - b).abs()
        d = d[torch.isfinite(d)]
        worst = max(worst, float(d.max()) / h)
    return worst


@gpu
@pytest.mark.parametrize("precision", ["f32", "f16x2"])
@pytest.mark.parametrize("tag,name", GOLDENS)
def test_extract_geometry_with_the_sparse_lattice_equals_the_dense_mesh(tag, name, precision):
    """sqrt(3) * L_obs bounds |u(p) - u(q)| / |p - q| between ANY two lattice points (an axis path between them is at most sqrt(3) times
    their distance), so with it the method's hypothesis holds by construction: no leak, no fallback, the same vertices and triangles.
    Exact equality rests on test_lattice_values_do_not_depend_on_the_batch."""
    surf, vols = _surface(tag, name, precision)
    lo, hi = _bounds()
    for r in (100, 128):
        u = surf.sdf_grid(vols, lo, hi, r)
        assert surf.last_lattice_stats is None
        v0, t0 = surf.extract_geometry(vols, lo, hi, r, 0.0)
        assert len(t0) > 0
        surf.lattice_lipschitz = 3 ** 0.5 * _l_obs(u, r) * (1 + 1e-3)
        for b in (4, 8):
            us = surf.sdf_grid(vols, lo, hi, r, sparse=b)
            stats = surf.last_lattice_stats
            print(f"{tag} {precision} R={r} B={b}: L_obs-based bound {surf.lattice_lipschitz:.3f}, evaluated share {stats['evaluated_points'] / r ** 3:.3f}")
            assert stats["leaks"] == 0 and stats["fell_back"] is False and stats["bricks"] == SR.dims(r, b)[1] ** 3
            ref, act, _ = SR.filled(u.cpu(), r, b, 0.0, SR.margin(LO, HI, r, b, surf.lattice_lipschitz))
            assert stats["active_bricks"] == int(act.sum()) and torch.equal(us.cpu(), ref)
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                v1, t1 = surf.extract_geometry(vols, lo, hi, r, 0.0, sparse=b)
            assert not surf.last_lattice_stats["fell_back"]
            assert np.array_equal(v0, v1) and np.array_equal(t0, t1)
        surf.lattice_lipschitz = 2.0


@gpu
def test_a_bound_that_fails_on_a_real_network_falls_back():
    """lattice_lipschitz = 1e-6 on the golden scenes: wherever the restatement counts leaks on the dense lattice the call warns, reports the
    fallback and returns the dense mesh; the device count itself equals the restatement's on the lattice the method builds."""
    r, b = 100, 8
    lo, hi = _bounds()
    counted = 0
    for tag, name in GOLDENS:
        surf, vols = _surface(tag, name, "f32")
        u = surf.sdf_grid(vols, lo, hi, r)
        v0, t0 = surf.extract_geometry(vols, lo, hi, r, 0.0)
        us, act, _ = SR.filled(u.cpu(), r, b, 0.0, SR.margin(LO, HI, r, b, 1e-6))
        on_dense, visible = SR.leaks(u.cpu(), act, r, b, 0.0), SR.leaks(us, act, r, b, 0.0)
        print(f"{tag}: restatement counts {on_dense} leaks on the dense lattice, {visible} on the two-level one")
        surf.lattice_lipschitz = 1e-6
        try:
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                v1, t1 = surf.extract_geometry(vols, lo, hi, r, 0.0, sparse=b)
        finally:
            surf.lattice_lipschitz = 2.0
        stats = surf.last_lattice_stats
        warned = [w for w in caught if issubclass(w.category, RuntimeWarning) and "lattice edges" in str(w.message)]
        assert stats["leaks"] == visible
        if on_dense > 0:
            counted += 1
            assert len(warned) == 1 and str(stats["leaks"]) in str(warned[0].message) and "1e-06" in str(warned[0].message)
            assert stats["fell_back"] is True
            assert np.array_equal(v0, v1) and np.array_equal(t0, t1)
        else:
            assert not warned and stats["fell_back"] is False
    assert counted > 0         # (an analytic field with the same property: test_a_visible_violation_falls_back_to_the_dense_lattice)


@gpu
def test_defaults_run_the_dense_lattice_and_no_k28_kernel():
    from gens_amd import lib as L, ops
    from gens_amd.config import Conf, gens_model_conf
    from gens_amd.distributed import Shard
    from gens_amd.models.gens import GenS
    from gens_amd.models.modules.implicit_surface import ImplicitSurface
    assert ImplicitSurface.sparse_lattice is None and ImplicitSurface.lattice_lipschitz == 2.0 and ImplicitSurface.last_lattice_stats is None
    surf, vols = _surface("a", "g23_filter_volume", "f32")
    assert "sparse_lattice" not in vars(surf) or surf.sparse_lattice is None
    lo, hi = _bounds()
    r, chunk = 33, 5000
    # what the dense path has always computed: K11's points chunk by chunk through the fused network
    packed = ops.VolumeSet.packed(vols)
    want = torch.empty(r ** 3, device="cuda")
    with torch.no_grad():
        plan = surf._fused_plan(packed)
        for first in range(0, r ** 3, chunk):
            count = min(chunk, r ** 3 - first)
            want[first:first + count] = -ops.sdf_mlp(plan, packed, ops.lattice_points(LO, HI, r, first, count, want.device), precision="f32")[:, 0]
    L.profile_begin(only=K28)
    u = surf.sdf_grid(vols, lo, hi, r, chunk=chunk)
    v0, t0 = surf.extract_geometry(vols, lo, hi, r, 0.0)
    assert not L.profile_end(raw=True) and surf.last_lattice_stats is None
    assert torch.equal(u.reshape(-1), want)
    vm, tm = ops.marching_cubes(want.reshape(r, r, r), 0.0)
    assert np.array_equal(v0, vm.cpu().numpy() / (r - 1.0) * 2.0 - 1.0) and np.array_equal(t0, tm.cpu().numpy())
    # the same through the option, which launches them
    L.profile_begin(only=K28)
    v1, t1 = surf.extract_geometry(vols, lo, hi, r, 0.0, sparse=4)
    assert {k for k, *_ in L.profile_end(raw=True)} == K28 and surf.last_lattice_stats["bricks"] == 8 ** 3
    surf.sparse_lattice = True                                # the attribute, and what True means
    surf.sdf_grid(vols, lo, hi, r)
    assert surf.last_lattice_stats["bricks"] == SR.dims(r, ImplicitSurface.SPARSE_BRICK)[1] ** 3
    surf.sdf_grid(vols, lo, hi, r, sparse=False)
    assert surf.last_lattice_stats is None
    # a shard: the option is ignored with one warning, the sharded lattice is the dense one
    surf.sparse_lattice = 4
    sink, got = {}, None
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        L.profile_begin(only=K28)
        for rank in range(2):
            got = surf.sdf_grid(vols, lo, hi, r, chunk=chunk, shard=Shard.single(rank, 2, sink))
        assert not L.profile_end(raw=True)
    assert len([w for w in caught if issubclass(w.category, RuntimeWarning) and "shard" in str(w.message)]) == 1
    assert torch.equal(got, u)
    surf.sparse_lattice = None
    # the conf keys reach the attributes (and their absence leaves the class defaults)
    conf = gens_model_conf(volume_dims=(16, 8, 4), has_vol=True)
    plain = GenS(conf)
    assert "sparse_lattice" not in vars(plain.implicit_surface) and "lattice_lipschitz" not in vars(plain.implicit_surface)
    tuned = GenS(Conf({**conf, "sparse_lattice": 16, "lattice_lipschitz": 3.5}))
    assert tuned.implicit_surface.sparse_lattice == 16 and tuned.implicit_surface.lattice_lipschitz == 3.5
    assert GenS(Conf({**conf, "sparse_lattice": True})).implicit_surface.sparse_lattice is True


@gpu
def test_validate_passes_the_option_through(golden):
    """validate(sparse=B) returns the mesh of validate() and the same image; without the keyword no K28 kernel runs."""
    from gens_amd import lib as L
    from .test_hip_render import build_surface, scene_inputs
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
    L.profile_begin(only=K28)
    ref = surf.validate(*args, extract_geometry=True, mesh_resolution=33)
    assert not L.profile_end(raw=True)
    torch.manual_seed(3)
    out = surf.validate(*args, extract_geometry=True, mesh_resolution=33, sparse=4)
    assert surf.last_lattice_stats is not None and not surf.last_lattice_stats["fell_back"]
    for k in ("vertices", "triangles", "color_fine", "sdf_depth"):
        assert torch.equal(torch.as_tensor(out[k]), torch.as_tensor(ref[k])), k


# ------------------------------------------------------------------------------------------------------------------------------------
# argument checks: before any launch, so they run without a device
# ------------------------------------------------------------------------------------------------------------------------------------
def check_shared_refusals(lib, coarse_points, classify, brick_points):
    """What the coarse-point, classify and brick-point entry points of either family refuse alike (tests/test_hip_brick_mcubes.py runs it
    for K29's)."""
    import ctypes as C
    coarse_points, classify, brick_points = (getattr(lib, n) for n in (coarse_points, classify, brick_points))
    lo, hi = (C.c_float * 3)(-1, -1, -1), (C.c_float * 3)(1, 1, 1)
    one = C.c_void_p(16)
    assert coarse_points(None, hi, 16, 4, 0, 1, one, None) == -1 and b"null" in lib.gens_last_error()
    assert coarse_points(lo, hi, 16, 4, 0, 1, None, None) == -1 and b"null" in lib.gens_last_error()
    assert coarse_points(lo, hi, 16, 4, 100, 26, one, None) == -1 and b"beyond" in lib.gens_last_error()      # C = 5: 125 points
    assert coarse_points(lo, hi, 16, 4, -1, 1, one, None) == -1
    assert coarse_points(lo, hi, 16, 4, 125, 0, None, None) == 0                                             # an empty range asks for nothing
    assert classify(None, 16, 4, 0.0, 0.1, one, None) == -1 and b"null" in lib.gens_last_error()
    assert classify(one, 16, 4, 0.0, -0.1, one, None) == -1 and b"margin" in lib.gens_last_error()
    assert classify(one, 16, 4, 0.0, float("nan"), one, None) == -1
    assert brick_points(lo, hi, 16, 4, one, 3, 2, 2, one, None) == -1 and b"beyond the list" in lib.gens_last_error()
    assert brick_points(lo, hi, 16, 4, None, 3, 0, 3, one, None) == -1 and b"null" in lib.gens_last_error()
    assert brick_points(lo, hi, 16, 4, one, 3, 0, 3, None, None) == -1 and b"null" in lib.gens_last_error()
    assert brick_points(lo, hi, 16, 4, None, 0, 0, 0, None, None) == 0


def test_entry_points_report_bad_arguments_without_a_gpu():
    import ctypes as C
    from gens_amd import lib as L
    from gens_amd import ops
    lib = L.load()
    lo, hi = (C.c_float * 3)(-1, -1, -1), (C.c_float * 3)(1, 1, 1)
    one = C.c_void_p(16)                                      # a non-null, aligned pointer: every call below is refused before it is used
    calls = {
        "gens_sparse_coarse_points": lambda r, b: lib.gens_sparse_coarse_points(lo, hi, r, b, 0, 1, one, None),
        "gens_sparse_classify": lambda r, b: lib.gens_sparse_classify(one, r, b, 0.0, 0.1, one, None),
        "gens_sparse_brick_points": lambda r, b: lib.gens_sparse_brick_points(lo, hi, r, b, one, 1, 0, 1, one, None),
        "gens_sparse_fill": lambda r, b: lib.gens_sparse_fill(one, r, b, one, None),
        "gens_sparse_scatter": lambda r, b: lib.gens_sparse_scatter(one, r, b, one, 1, 0, 1, one, None),
        "gens_sparse_leaks": lambda r, b: lib.gens_sparse_leaks(one, r, b, one, 0.0, one, None),
    }
    assert set(calls) == K28
    for name, call in calls.items():
        assert call(1, 4) == -1 and b"res = 1" in lib.gens_last_error() and name.encode() in lib.gens_last_error()
        assert call(16, 0) == -1 and b"brick = 0" in lib.gens_last_error()
        assert call(1291, 4) == -2 and b"2^31" in lib.gens_last_error()               # 1291^3 >= 2^31 > 1290^3
    check_shared_refusals(lib, "gens_sparse_coarse_points", "gens_sparse_classify", "gens_sparse_brick_points")
    assert lib.gens_sparse_brick_points(lo, hi, 1200, 1025, one, 3, 0, 1, one, None) == -2
    assert lib.gens_sparse_brick_points(lo, hi, 1024, 512, one, 8, 0, 8, one, None) == -2 and b"rows" in lib.gens_last_error()   # 8 * 512^3 rows
    assert lib.gens_sparse_fill(one, 16, 4, C.c_void_p(20), None) == -1 and b"misaligned" in lib.gens_last_error()
    assert lib.gens_sparse_fill(None, 16, 4, one, None) == -1
    assert lib.gens_sparse_scatter(one, 16, 4, one, 3, 0, 4, one, None) == -1 and b"beyond the list" in lib.gens_last_error()
    assert lib.gens_sparse_scatter(None, 16, 4, one, 3, 0, 3, one, None) == -1 and b"null" in lib.gens_last_error()
    assert lib.gens_sparse_leaks(one, 16, 4, None, 0.0, one, None) == -1 and b"null" in lib.gens_last_error()
    assert lib.gens_sparse_leaks(one, 16, 4, one, 0.0, C.c_void_p(12), None) == -1 and b"misaligned" in lib.gens_last_error()
    # the operator refuses the same things in its own words, before it needs a device
    for bad in [dict(resolution=1, brick=4), dict(resolution=16, brick=0), dict(resolution=1291, brick=4)]:
        with pytest.raises(ValueError):
            ops.sparse_lattice_dims(**bad)
    with pytest.raises(ValueError, match="lipschitz"):
        ops.sparse_lattice(lambda p: p[:, :1], LO, HI, 16, 0.0, 4, 0.0, device="cpu")
    assert ops.sparse_lattice_dims(128, 4) == (33, 32) and ops.sparse_lattice_dims(9, 8) == (2, 2) and ops.sparse_lattice_dims(10, 8) == (3, 2)
    assert ops.sparse_lattice_margin(LO, HI, 128, 4, 1.0) == SR.margin(LO, HI, 128, 4, 1.0)
