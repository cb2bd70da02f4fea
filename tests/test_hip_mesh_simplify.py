"""GPU tests of the mesh simplification (K33): the three kernels and ops.simplify_mesh against the numpy restatement
(tests/mesh_simplify_reference.py), bit for bit, on the empty mesh, one triangle, a 300-triangle fan (one long entry segment), meshes with
63, 64, 65 and 257 clusters, the white-noise 7 x 19 x 66 marching-cubes mesh of the K12 tests, the planted inputs and the analytic meshes of
the CPU file; determinism; io.simplify_mesh and the command line; extract_geometry(simplify=) on the g23 model's three routes, its attributes,
validate and the writer; nothing changes when the option is unset; the refusals."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from . import mesh_simplify_reference as SR

gpu = pytest.mark.gpu
K33 = {"gens_cluster_keys", "gens_cluster_triangles", "gens_cluster_solve"}
COMPARED = ("input_vertices", "input_triangles", "output_vertices", "output_triangles", "collapsed_triangles", "duplicate_triangles", "fell_back")


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _noise_mesh():
    """The ragged white-noise lattice of tests/test_marching_cubes.py at its threshold."""
    from gens_amd import mc_tables
    from oracle import mc_oracle
    u = np.random.default_rng(2).standard_normal((7, 19, 66)).astype(np.float32)
    v, t = mc_oracle.marching_cubes(u, 0.25, mc_tables.TRI_TABLE, mc_tables.TRI_COUNT)
    return v, t.astype(np.int32)


def _cases():
    """name -> (vertices, triangles, cell, origin or None, reg)."""
    half = np.full(3, -0.5)
    out = {"one triangle": (np.array([[0.5, 0.5, 0.5], [1.5, 0.6, 0.4], [0.4, 1.5, 0.7]]), np.array([[0, 1, 2]], np.int32), 1.0, np.zeros(3), SR.REG),
           "one triangle in one cell": (np.array([[0.5, 0.5, 0.5], [0.6, 0.6, 0.4], [0.4, 0.7, 0.7]]), np.array([[0, 1, 2]], np.int32), 1.0, None, SR.REG),
           "fan": (*SR.fan_mesh(), SR.FAN_CELL, np.zeros(3), SR.REG),
           "fan, coarse": (*SR.fan_mesh(), 1.0, None, SR.REG),
           "planted": (*SR.planted_mesh(), SR.REG),
           "planted, default origin": (*SR.planted_mesh()[:3], None, 1e-2)}
    for n in (63, 64, 65, 257):
        out[f"{n} clusters"] = (*SR.clusters_mesh(n), SR.REG)
    nv, nt = _noise_mesh()
    for cell in (1.0, 2.5):
        out[f"noise, cell {cell}"] = (nv, nt, cell, half, SR.REG)
    out["noise, cell 0.3"] = (nv, nt, 0.3, None, 1e-4)
    for name, field in (("sphere", SR.sphere_field), ("box", SR.box_field)):
        v, t = SR.lattice_mesh(field)
        out[f"{name}, cell 2"] = (v, t, 2.0, half, SR.REG)
    out["sphere, cell 3.7, world grid"] = (SR.lattice_mesh(SR.sphere_field)[0] * 0.01 - 3.0, SR.lattice_mesh(SR.sphere_field)[1], 0.037, None, SR.REG)
    return out


_CASES = {}


def _case(name):
    if not _CASES:
        _CASES.update(_cases())
    return _CASES[name]


CASE_NAMES = ["one triangle", "one triangle in one cell", "fan", "fan, coarse", "planted", "planted, default origin", "63 clusters", "64 clusters",
              "65 clusters", "257 clusters", "noise, cell 1.0", "noise, cell 2.5", "noise, cell 0.3", "sphere, cell 2", "box, cell 2",
              "sphere, cell 3.7, world grid"]


def _device(v, t, cell, origin, reg):
    from gens_amd import ops
    ov, ot, src, stats = ops.simplify_mesh(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).cuda(),
                                           torch.from_numpy(np.ascontiguousarray(t, dtype=np.int32)).cuda(), cell, origin=origin, reg=reg)
    assert ov.is_cuda and ot.is_cuda and src.is_cuda
    return ov.cpu().numpy(), ot.cpu().numpy(), src.cpu().numpy(), stats


@gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_simplify_mesh_equals_the_restatement(name):
    v, t, cell, origin, reg = _case(name)
    want = SR.simplify(v, t, cell, origin, reg=reg)
    ov, ot, src, stats = _device(v, t, cell, origin, reg)
    print(f"{name}: {want['stats']}, {len(want['cluster_keys'])} clusters")
    assert _same(ov, want["vertices"]) and _same(ot, want["triangles"]) and _same(src, want["source"])
    assert {k: stats[k] for k in COMPARED} == want["stats"] and stats["clusters"] == len(want["cluster_keys"])
    assert stats["origin"] == want["origin"].tolist() and stats["cell"] == cell and stats["reg"] == reg
    # twice: equal bits
    again = _device(v, t, cell, origin, reg)
    assert _same(again[0], ov) and _same(again[1], ot) and _same(again[2], src) and again[3] == stats


def _segments(want, t):
    """The kernel's segment inputs, built with numpy from the restatement's ranks: entries 3 t + k sorted stably by cluster, members sorted
    stably by key, and both segment tables."""
    n_c = len(want["cluster_keys"])
    flat = want["ranks"].reshape(-1)
    entries = np.argsort(flat, kind="stable").astype(np.int32)
    entry_start = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=n_c))]).astype(np.int32)
    members = np.argsort(want["keys"], kind="stable").astype(np.int32)
    member_start = np.concatenate([[0], np.cumsum(np.bincount(want["vertex_cluster"], minlength=n_c))]).astype(np.int32)
    return entries, entry_start, members, member_start


@gpu
@pytest.mark.parametrize("name", ["fan", "planted", "65 clusters", "noise, cell 2.5", "sphere, cell 2"])
def test_the_three_kernels_equal_the_restatement_one_by_one(name):
    from gens_amd import lib as L
    v, t, cell, origin, reg = _case(name)
    want = SR.simplify(v, t, cell, origin, reg=reg)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    f64, i32, i64, u8 = torch.float64, torch.int32, torch.int64, torch.uint8
    n_v, n_t, n_c, n_o = len(v), len(t), len(want["cluster_keys"]), len(want["out_clusters"])
    dv, dt = up(np.asarray(v, dtype=np.float64)), up(np.asarray(t, dtype=np.int32))
    keys = torch.full((n_v + 1,), -7, device="cuda", dtype=i64)                       # (one slot past the end: it stays)
    L.call("gens_cluster_keys", L.ptr(dv, f64), n_v, *[float(o) for o in origin], float(cell), L.ptr(keys, i64), L.stream())
    assert _same(keys[:n_v].cpu().numpy(), want["keys"]) and int(keys[n_v]) == -7
    ranks = torch.full((n_t + 1, 3), -7, device="cuda", dtype=i32)
    survive = torch.full((n_t + 1,), 7, device="cuda", dtype=u8)
    triple = torch.full((n_t + 1, 3), -7, device="cuda", dtype=i32)
    L.call("gens_cluster_triangles", L.ptr(dt, i32), n_t, L.ptr(up(want["vertex_cluster"]), i32), n_v, L.ptr(ranks, i32), L.ptr(survive, u8),
           L.ptr(triple, i32), L.stream())
    assert _same(ranks[:n_t].cpu().numpy(), want["ranks"]) and _same(triple[:n_t].cpu().numpy(), want["triple"])
    assert np.array_equal(survive[:n_t].cpu().numpy().astype(bool), want["survive"])
    assert (ranks[n_t] == -7).all() and int(survive[n_t]) == 7 and (triple[n_t] == -7).all()
    entries, entry_start, members, member_start = _segments(want, t)
    out_v = torch.full((n_o + 1, 3), -7.0, device="cuda", dtype=f64)
    source = torch.full((n_o + 1,), -7, device="cuda", dtype=i32)
    fell = torch.full((n_o + 1,), 7, device="cuda", dtype=u8)
    held = [up(want["survive"].astype(np.uint8)), up(want["cluster_keys"]), up(entries), up(entry_start), up(members), up(member_start),
            up(want["out_clusters"])]
    args = L.ClusterSolveArgs(L.ptr(dv, f64), L.ptr(dt, i32), L.ptr(held[0], u8), L.ptr(held[1], i64), L.ptr(held[2], i32), L.ptr(held[3], i32),
                              L.ptr(held[4], i32), L.ptr(held[5], i32), L.ptr(held[6], i32), n_v, n_t, n_c, n_o, (C.c_double * 3)(*[float(o) for o in origin]),
                              float(cell), float(reg), L.ptr(out_v, f64), L.ptr(source, i32), L.ptr(fell, u8))
    L.call("gens_cluster_solve", C.byref(args), L.stream())
    assert _same(out_v[:n_o].cpu().numpy(), want["vertices"]) and np.array_equal(source[:n_o].cpu().numpy(), want["source"])
    assert np.array_equal(fell[:n_o].cpu().numpy().astype(bool), want["fell_back"])
    assert (out_v[n_o] == -7.0).all() and int(source[n_o]) == -7 and int(fell[n_o]) == 7


@gpu
def test_out_of_range_input_is_skipped_by_the_kernels_not_read_through():
    """What ops.simplify_mesh refuses beforehand, given to the entry points directly: a vertex outside the key range gets key -1, a
    triangle with an index outside the vertices does not survive, and the solve kernel skips entries, members and indices outside their
    ranges and writes a zero row for a cluster rank outside the clusters."""
    from gens_amd import lib as L
    f64, i32, i64, u8 = torch.float64, torch.int32, torch.int64, torch.uint8
    v = torch.tensor([[0.5, 0.5, 0.5], [-0.5, 0.5, 0.5], [float("nan"), 0.5, 0.5], [0.5, 3e6, 0.5], [1.5, 2.5, 3.5]], device="cuda", dtype=f64)
    keys = torch.empty(5, device="cuda", dtype=i64)
    L.call("gens_cluster_keys", L.ptr(v, f64), 5, 0.0, 0.0, 0.0, 1.0, L.ptr(keys, i64), L.stream())
    assert keys.tolist() == [0, -1, -1, -1, (3 << 42) + (2 << 21) + 1]
    t = torch.tensor([[0, 1, 2], [0, 1, 5], [-1, 1, 2], [2, 2, 1]], device="cuda", dtype=i32)
    vc = torch.tensor([4, 2, 0, 1, 3], device="cuda", dtype=i32)
    ranks, survive, triple = torch.empty(4, 3, device="cuda", dtype=i32), torch.empty(4, device="cuda", dtype=u8), torch.empty(4, 3, device="cuda", dtype=i32)
    L.call("gens_cluster_triangles", L.ptr(t, i32), 4, L.ptr(vc, i32), 5, L.ptr(ranks, i32), L.ptr(survive, u8), L.ptr(triple, i32), L.stream())
    assert ranks.tolist() == [[4, 2, 0], [4, 2, -1], [-1, 2, 0], [0, 0, 2]] and survive.tolist() == [1, 0, 0, 0]
    assert triple.tolist() == [[0, 2, 4], [-1, 2, 4], [-1, 0, 2], [0, 0, 2]]
    # the solve kernel with poisoned lists around the one-triangle case
    pv, pt, cell, origin, reg = _case("one triangle")
    want = SR.simplify(pv, pt, cell, origin, reg=reg)
    up = lambda a, dt: torch.tensor(a, device="cuda", dtype=dt)  # noqa: E731
    dv, dt_ = up(pv.tolist(), f64), up([[0, 1, 2], [0, 9, 1]], i32)
    survive = up([1, 1], u8)
    ck = up(want["cluster_keys"].tolist(), i64)
    order = np.argsort(want["ranks"].reshape(-1), kind="stable")
    # every segment holds one good entry among bad ones: -1 and 77 are outside 0 .. 3 T - 1 = 14; entry 3 is triangle 1, whose index 9 is
    # outside the 9 vertices; entry 6 is triangle 2, all of whose indices are; members -5 and 1000 are outside the vertices
    entries = [[-1, 77, int(e), 3, 6] for e in order]
    members = [[-5, int(m), 1000] for m in np.argsort(want["keys"], kind="stable")]
    outc = up([2, 7, 0, -1], i32)                                  # ranks 7 and -1 are outside the 4 clusters: zero rows
    out_v, source, fell = torch.empty(4, 3, device="cuda", dtype=f64), torch.empty(4, device="cuda", dtype=i32), torch.empty(4, device="cuda", dtype=u8)
    ck4 = torch.cat([ck, up([1 << 50], i64)])                      # (a fourth cluster that nothing references, so that n_out = 4 is allowed)
    held = [up(sum(entries, []), i32), up([0, 5, 10, 15, 15], i32), up(sum(members, []), i32), up([0, 3, 6, 9, 9], i32)]
    # sizes that hold the lists: 3 T = 15 entries, V = 9 members; the triangles and vertices beyond the real ones are never reached
    dv9 = torch.cat([dv, torch.zeros(6, 3, device="cuda", dtype=f64)])
    dt5 = torch.cat([dt_, torch.full((3, 3), 100, device="cuda", dtype=i32)])
    sv5 = torch.cat([survive, torch.ones(3, device="cuda", dtype=u8)])
    args = L.ClusterSolveArgs(L.ptr(dv9, f64), L.ptr(dt5, i32), L.ptr(sv5, u8), L.ptr(ck4, i64), L.ptr(held[0], i32), L.ptr(held[1], i32), L.ptr(held[2], i32),
                              L.ptr(held[3], i32), L.ptr(outc, i32), 9, 5, 4, 4, (C.c_double * 3)(*origin.tolist()), cell, reg, L.ptr(out_v, f64),
                              L.ptr(source, i32), L.ptr(fell, u8))
    L.call("gens_cluster_solve", C.byref(args), L.stream())
    got_v, got_s = out_v.cpu().numpy(), source.tolist()
    assert _same(got_v[[2, 0]], want["vertices"][[0, 2]]) and [got_s[2], got_s[0]] == want["source"][[0, 2]].tolist()
    assert not got_v[[1, 3]].any() and [got_s[1], got_s[3]] == [-1, -1] and [fell.tolist()[1], fell.tolist()[3]] == [1, 1]


@gpu
def test_empty_cases_launch_nothing():
    from gens_amd import lib as L, ops
    f64, i32 = torch.float64, torch.int32
    v, t, cell, origin, reg = _case("one triangle in one cell")
    L.profile_begin(only=K33 | {"gens_compact_valid"})
    for vv, tt in ((np.zeros((0, 3)), np.zeros((0, 3), np.int32)), (v, np.zeros((0, 3), np.int32))):
        ov, ot, src, stats = _device(vv, tt, 1.0, None, SR.REG)
        assert ov.shape == (0, 3) and ov.dtype == np.float64 and ot.shape == (0, 3) and ot.dtype == np.int32 and src.shape == (0,) and src.dtype == np.int64
        assert stats["output_vertices"] == 0 and stats["output_triangles"] == 0 and stats["input_vertices"] == len(vv)
    assert not L.profile_end(raw=True)
    # every triangle collapses: the first two kernels run, the solve does not
    L.profile_begin(only=K33 | {"gens_compact_valid"})
    ov, ot, src, stats = _device(v, t, cell, origin, reg)
    assert {k for k, *_ in L.profile_end(raw=True)} == {"gens_cluster_keys", "gens_cluster_triangles"}
    assert ov.shape == (0, 3) and ot.shape == (0, 3) and stats["collapsed_triangles"] == 1 and stats["clusters"] == 1
    big = SR.lattice_mesh(SR.sphere_field)
    assert _device(*big, 64.0, np.full(3, -0.5), SR.REG)[3]["collapsed_triangles"] == len(big[1])
    # n = 0 at the entry points themselves: no launch, no error, whatever the pointers
    lib = L.load()
    assert lib.gens_cluster_keys(None, 0, 0.0, 0.0, 0.0, 1.0, None, None) == 0
    assert lib.gens_cluster_triangles(None, 0, None, 0, None, None, None, None) == 0
    assert ops.simplify_mesh(torch.zeros(0, 3, device="cuda", dtype=f64), torch.zeros(0, 3, device="cuda", dtype=i32), 2.0)[3]["clusters"] == 0


@gpu
def test_io_simplify_mesh_and_the_command_line(tmp_path):
    from gens_amd import io as gio, simplify as cli
    v, t = SR.lattice_mesh(SR.sphere_field)
    rng = np.random.default_rng(5)
    normals = rng.normal(size=(len(v), 3)).astype(np.float32)
    colors = rng.integers(0, 256, (len(v), 3)).astype(np.uint8)
    seen = rng.random(len(v)) < 0.7
    want = SR.simplify(v, t, 2.0)                              # the default origin: multiples of the cell
    ov, ot, attrs = gio.simplify_mesh(v, t.astype(np.int64), 2.0, normals=normals, colors=colors, seen=seen)
    assert _same(ov, want["vertices"]) and ot.dtype == np.int64 and np.array_equal(ot, want["triangles"]) and _same(attrs["source"], want["source"])
    assert _same(attrs["normals"], normals[want["source"]]) and _same(attrs["colors"], colors[want["source"]]) and _same(attrs["seen"], seen[want["source"]])
    assert sorted(attrs) == ["colors", "normals", "seen", "source", "stats"] and attrs["stats"]["output_vertices"] == len(ov)
    bare = gio.simplify_mesh(torch.from_numpy(v), torch.from_numpy(t), 2.0, origin=[-0.5] * 3, device="cuda:0")
    assert sorted(bare[2]) == ["source", "stats"] and _same(bare[0], SR.simplify(v, t, 2.0, [-0.5] * 3)["vertices"]) and bare[1].dtype == np.int32
    # the command line: PLY in, PLY out, attributes carried by the source vertex; the file holds float32 vertices, so the rule runs on those
    src_path, dst_path = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    gio.write_ply(src_path, v, t, normals=normals, colors=colors)
    assert cli.main([src_path, dst_path, "--cell", "2", "--reg", "1e-2"]) == 0
    v32 = v.astype(np.float32)
    want = SR.simplify(v32, t, 2.0, reg=1e-2)
    fv, ft, fa = gio.read_ply(dst_path, attributes=True)
    assert _same(fv, want["vertices"].astype(np.float32)) and np.array_equal(ft, want["triangles"])
    assert _same(fa["normals"], normals[want["source"]]) and _same(fa["colors"], colors[want["source"]])
    assert 0 < len(fv) < len(v) and (tmp_path / "out.ply").stat().st_size < (tmp_path / "in.ply").stat().st_size
    assert cli.main([src_path, dst_path, "--cell", "0"]) == 2


# ------------------------------------------------------------------------------------------------------------------------------------
# the model: the g23 surface and the synthetic views of tests/test_hip_vertex_attrs.py, R = 64, f32
# ------------------------------------------------------------------------------------------------------------------------------------
R = 64
ROUTES = (("dense", {}), ("lattice", {"sparse": 4}), ("mesh", {"sparse": 4, "sparse_mesh": True}))
_MODEL = {}


def _model():
    """The unsimplified R = 64 mesh on the device (sdf_grid + marching_cubes: the dense route's own steps), ops.simplify_mesh of it at cell 2,
    and a Lipschitz bound that holds by construction (no leak on the sparse routes); once."""
    if not _MODEL:
        from gens_amd import ops
        from .test_hip_sparse_lattice import _l_obs
        from .test_hip_vertex_attrs import _bounds, _scene, _surface
        surf, vols = _surface("f32")
        _, views = _scene(surf, 3)
        lo, hi = _bounds()
        u = surf.sdf_grid(vols, lo, hi, R)
        dv, dt = ops.marching_cubes(u, 0.0)
        sv, st, src, stats = ops.simplify_mesh(dv, dt, 2.0, origin=(-0.5, -0.5, -0.5))
        _MODEL.update(surf=surf, vols=vols, views=views, lo=lo, hi=hi, lipschitz=3 ** 0.5 * _l_obs(u, R) * (1 + 1e-3), full=(dv.cpu().numpy(), dt.cpu().numpy()),
                      simple=(sv.cpu().numpy(), st.cpu().numpy(), src.cpu().numpy(), stats))
    return _MODEL


def _world(index_vertices, lo, hi):
    """extract_geometry's host expression (implicit_surface.py:424-425)."""
    b_max, b_min = hi.cpu().numpy(), lo.cpu().numpy()
    return index_vertices / (R - 1.0) * (b_max - b_min)[None, :] + b_min[None, :]


@gpu
def test_extract_geometry_simplifies_on_every_route_and_evaluates_attributes_at_the_new_vertices():
    from gens_amd import lib as L
    from .test_hip_vertex_attrs import _same as same_attrs
    m = _model()
    surf, vols, views, lo, hi = m["surf"], m["vols"], m["views"], m["lo"], m["hi"]
    sv, st, src, stats = m["simple"]
    want = SR.simplify(*m["full"], 2.0, [-0.5] * 3)
    assert _same(sv, want["vertices"]) and _same(st, want["triangles"]) and _same(src, want["source"])      # the model's mesh, against the restatement
    print(f"g23 R = {R}: {stats}")
    assert 0 < len(sv) < len(m["full"][0]) and 0 < len(st) < len(m["full"][1])
    surf.lattice_lipschitz = m["lipschitz"]
    try:
        first = None
        for route, kw in ROUTES:
            L.profile_begin(only=K33)
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                v, t, attrs = surf.extract_geometry(vols, lo, hi, R, 0.0, attributes=("normals", "colors"), views=views, simplify=2, **kw)
            assert {k for k, *_ in L.profile_end(raw=True)} == K33, route
            assert route == "dense" or not surf.last_lattice_stats["fell_back"]
            assert _same(v, _world(sv, lo, hi)) and _same(t, st), route
            assert surf.last_simplify_stats == stats, route
            # the attributes are evaluated at the new vertices, not carried from the old ones
            assert same_attrs(attrs, surf.vertex_attributes(v, vols, views)), route
            first = first or attrs
            assert same_attrs(attrs, first), route
        plain = surf.extract_geometry(vols, lo, hi, R, 0.0, simplify=2)
        assert len(plain) == 2 and _same(plain[0], v) and _same(plain[1], t)
        # another cell edge, a fractional one; and the attribute does what the keyword does
        v3, t3 = surf.extract_geometry(vols, lo, hi, R, 0.0, simplify=3.5)
        w3 = SR.simplify(*m["full"], 3.5, [-0.5] * 3)
        assert _same(v3, _world(w3["vertices"], lo, hi)) and _same(t3, w3["triangles"]) and len(t3) < len(t)
        surf.mesh_simplify = 2
        try:
            got = surf.extract_geometry(vols, lo, hi, R, 0.0)
            assert _same(got[0], v) and _same(got[1], t)
            off = surf.extract_geometry(vols, lo, hi, R, 0.0, simplify=0)
            assert _same(off[0], _world(m["full"][0], lo, hi)) and _same(off[1], m["full"][1]) and surf.last_simplify_stats is None
        finally:
            del surf.mesh_simplify
    finally:
        surf.lattice_lipschitz = 2.0


@gpu
def test_nothing_changes_when_the_option_is_unset():
    from gens_amd import lib as L
    from gens_amd.config import Conf, gens_model_conf
    from gens_amd.models.gens import GenS
    from gens_amd.models.modules.implicit_surface import ImplicitSurface
    from .test_hip_vertex_attrs import TODAYS_KEYS, _validate_args
    assert ImplicitSurface.mesh_simplify is None
    m = _model()
    surf, vols, views, lo, hi = m["surf"], m["vols"], m["views"], m["lo"], m["hi"]
    assert "mesh_simplify" not in vars(surf)
    L.profile_begin(only=K33)
    surf.lattice_lipschitz = m["lipschitz"]
    try:
        for route, kw in ROUTES:
            for off in ({}, {"simplify": None}, {"simplify": False}, {"simplify": 0}):
                got = surf.extract_geometry(vols, lo, hi, R, 0.0, **kw, **off)
                assert len(got) == 2 and _same(got[0], _world(m["full"][0], lo, hi)) and _same(got[1], m["full"][1]), (route, off)
                assert surf.last_simplify_stats is None
    finally:
        surf.lattice_lipschitz = 2.0
    args = _validate_args(surf, vols)
    torch.manual_seed(3)
    ref = surf.validate(*args, extract_geometry=True, mesh_resolution=33)
    torch.manual_seed(3)
    off = surf.validate(*args, extract_geometry=True, mesh_resolution=33, mesh_simplify=0)
    assert not L.profile_end(raw=True)
    assert set(ref) == set(off) == TODAYS_KEYS
    for k in TODAYS_KEYS:
        assert torch.equal(torch.as_tensor(off[k]), torch.as_tensor(ref[k])), k
    plain = surf.extract_geometry(vols, lo, hi, 33, 0.0)
    assert _same(ref["vertices"], plain[0]) and _same(ref["triangles"], plain[1])
    # the conf key reaches the attribute (and its absence leaves the class default)
    conf = gens_model_conf(volume_dims=(16, 8, 4), has_vol=True)
    assert "mesh_simplify" not in vars(GenS(conf).implicit_surface)
    assert GenS(Conf({**conf, "mesh_simplify": 2})).implicit_surface.mesh_simplify == 2.0


@gpu
def test_validate_and_the_writer_end_to_end(tmp_path):
    from gens_amd import io as gio, lib as L
    from .test_hip_vertex_attrs import TODAYS_KEYS, _same as same_attrs, _scene, _validate_args
    m = _model()
    surf, vols, views, lo, hi = m["surf"], m["vols"], m["views"], m["lo"], m["hi"]
    args = _validate_args(surf, vols)
    torch.manual_seed(3)
    ref = surf.validate(*args, extract_geometry=True, mesh_resolution=R)
    L.profile_begin(only=K33)
    torch.manual_seed(3)
    out = surf.validate(*args, extract_geometry=True, mesh_resolution=R, mesh_simplify=2, mesh_attributes=("normals", "colors"))
    assert {k for k, *_ in L.profile_end(raw=True)} == K33
    assert set(out) == TODAYS_KEYS | {"vertex_normals", "vertex_colors", "vertex_seen"}
    for k in TODAYS_KEYS - {"vertices", "triangles"}:
        assert torch.equal(torch.as_tensor(out[k]), torch.as_tensor(ref[k])), k
    assert _same(out["vertices"], _world(m["simple"][0], lo, hi)) and _same(out["triangles"], m["simple"][1])
    assert surf.last_simplify_stats == m["simple"][3] and len(out["vertices"]) < len(ref["vertices"])
    assert same_attrs({k[7:]: out[k] for k in out if k.startswith("vertex_")}, surf.vertex_attributes(out["vertices"], vols, views))
    # the attribute selects what the keyword selects
    surf.mesh_simplify = 2.0
    try:
        torch.manual_seed(3)
        again = surf.validate(*args, extract_geometry=True, mesh_resolution=R)
        assert _same(again["vertices"], out["vertices"]) and _same(again["triangles"], out["triangles"])
    finally:
        del surf.mesh_simplify
    # the writer needs no change: a PLY that read_ply returns unchanged
    scale = torch.eye(4)
    scale[:3, :3] = torch.diag(torch.tensor([1.5, 1.0, 0.75]))
    scale[:3, 3] = torch.tensor([0.5, -1.0, 2.0])
    inputs = {"scene": "scan1", "file_name": "scan1_view0", "scale_mat": scale}
    paths = gio.save_validation_outputs(str(tmp_path), out, inputs, "epoch0")
    v, t, attrs = gio.read_ply(paths["mesh"], attributes=True)
    assert _same(v, gio.transform_vertices(out["vertices"], scale.numpy()).astype(np.float32)) and np.array_equal(t, out["triangles"])
    assert _same(attrs["normals"], gio.transform_normals(out["vertex_normals"], scale.numpy()).astype(np.float32))
    assert _same(attrs["colors"], np.where(out["vertex_seen"][:, None], out["vertex_colors"], np.uint8(128)))
    again_path = str(tmp_path / "again.ply")
    gio.write_ply(again_path, v, t, normals=attrs["normals"], colors=attrs["colors"])
    assert open(again_path, "rb").read() == open(paths["mesh"], "rb").read()


@gpu
def test_refusals_come_before_any_launch():
    from gens_amd import lib as L, ops
    from .test_hip_brick_mcubes import K29
    from .test_hip_sparse_lattice import K28
    from .test_hip_vertex_attrs import NETWORK, _validate_args
    m = _model()
    surf, vols, lo, hi = m["surf"], m["vols"], m["lo"], m["hi"]
    f64, i32 = torch.float64, torch.int32
    v = torch.tensor([[0.5, 0.5, 0.5], [1.5, 0.6, 0.4], [0.4, 1.5, 0.7]], device="cuda", dtype=f64)
    t = torch.tensor([[0, 1, 2]], device="cuda", dtype=i32)
    nan, inf = float("nan"), float("inf")
    L.profile_begin(only=K33 | K28 | K29 | NETWORK | {"gens_compact_valid", "gens_mc_classify", "gens_mc_emit", "gens_lattice_points"})
    for bad in (True, -2, nan, inf, "coarse"):
        with pytest.raises(ValueError):
            surf.extract_geometry(vols, lo, hi, 33, 0.0, simplify=bad)
        with pytest.raises(ValueError):
            surf.validate(*_validate_args(surf, vols), extract_geometry=True, mesh_resolution=33, mesh_simplify=bad)
    with pytest.raises(ValueError, match="not finite"):
        ops.simplify_mesh(torch.where(v == 0.6, torch.full_like(v, nan), v), t, 1.0)
    with pytest.raises(ValueError, match="not finite"):
        ops.simplify_mesh(torch.where(v == 0.6, torch.full_like(v, inf), v), t, 1.0)
    for bad_t in ([[0, 1, 3]], [[-1, 1, 2]]):
        with pytest.raises(ValueError, match="outside the 3 vertices"):
            ops.simplify_mesh(v, torch.tensor(bad_t, device="cuda", dtype=i32), 1.0)
    for cell, reg in ((0.0, 1e-3), (-1.0, 1e-3), (nan, 1e-3), (inf, 1e-3), (1.0, 0.0), (1.0, -1.0), (1.0, nan), (1.0, inf)):
        with pytest.raises(ValueError):
            ops.simplify_mesh(v, t, cell, reg=reg)
    with pytest.raises(ValueError, match="below origin"):
        ops.simplify_mesh(v, t, 1.0, origin=(0.0, 0.55, 0.0))      # the lowest y is 0.5
    with pytest.raises(ValueError, match="2\\^21 cells"):
        ops.simplify_mesh(v, t, 1e-7, origin=(0.0, 0.0, 0.0))
    with pytest.raises(ValueError, match="2\\^21 cells"):
        ops.simplify_mesh(v * 1e9, t, 1.0)                         # the default origin is at the minimum: the extent decides
    with pytest.raises(ValueError, match="origin"):
        ops.simplify_mesh(v, t, 1.0, origin=(0.0, nan, 0.0))
    with pytest.raises(ValueError, match="origin"):
        ops.simplify_mesh(v, t, 1.0, origin=(0.0, 0.0))
    for vv, tt in ((v.float(), t), (v, t.long()), (v[:, :2], t), (v, t.reshape(-1)), (v.cpu(), t), (v, t.cpu())):
        with pytest.raises(ValueError):
            ops.simplify_mesh(vv, tt, 1.0)
    assert not L.profile_end(raw=True)
    assert ops.simplify_mesh(v, t, 1.0, origin=(0.4, 0.5, 0.4))[3]["output_triangles"] == 1      # at the minimum is not below
