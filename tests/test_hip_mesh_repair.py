"""GPU tests of the mesh repair (K38): every integer output, source map, flag and count of ops.repair_mesh equals the numpy restatement
(tests/mesh_repair_reference.py) exactly, kept vertices bit for bit, centroids to a derived bound; segment walks across wave boundaries (fans
at one vertex, faces on one edge, long rims, long strips, many components); ops.mesh_topology of the result; io.repair_mesh and the command
line; extract_geometry(repair=) on the g23 model on the three lattice routes; nothing changes when the option is unset; the refusals."""
import functools
import json

import numpy as np
import pytest
import torch

from . import mesh_repair_reference as RR
from . import mesh_topology_reference as TR

gpu = pytest.mark.gpu
K38 = {"gens_mesh_face_keys", "gens_mesh_split_corners", "gens_mesh_orient_pairs", "gens_mesh_apply_flips", "gens_mesh_loop_centroids",
       "gens_mesh_fill_emit"}
INTEGER_FIELDS = ("triangles", "vertex_source", "face_source", "face_flipped")
COUNTS = ("vertices", "vertices_referenced", "faces", "faces_invalid", "edges", "edges_boundary", "edges_manifold", "edges_flipped",
          "edges_nonmanifold", "vertices_pinched", "vertices_nonmanifold", "components", "largest_component_faces", "boundary_components", "euler",
          "closed", "oriented", "manifold", "watertight", "genus")
MODEL_REPAIR = {"min_component_faces": 2, "max_hole_edges": 8}


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _up(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


@functools.lru_cache(maxsize=None)
def _cases():
    out = dict(RR.hand_cases())
    for n in (63, 64, 65, 257):
        out[f"cones {n}"] = (*RR.cones(n), {"max_hole_edges": 8})
    out["book 65"] = (*TR.book(65), RR.DEFAULTS)
    for n in (63, 64, 65, 1000):
        out[f"disk {n}"] = (*RR.disk(n), {"max_hole_edges": n})
    out["disk 65 open"] = (*RR.disk(65), {"max_hole_edges": 64})
    out["strip 1000"] = (*RR.strip_alternating(1000), RR.DEFAULTS)
    out["islands 65"] = (*RR.islands(65), {"min_component_faces": 33})
    out["clustered sphere"] = (*RR.clustered_sphere(), RR.ALL_ON)
    for seed in (2, 6, 9, 10, 35):
        out[f"soup {seed}"] = (*RR.random_soup(seed), {"max_hole_edges": 6})
    return out


CASE_NAMES = tuple(RR.hand_cases()) + tuple(f"cones {n}" for n in (63, 64, 65, 257)) + ("book 65",) + tuple(
    f"disk {n}" for n in (63, 64, 65, 1000)) + ("disk 65 open", "strip 1000", "islands 65", "clustered sphere") + tuple(
    f"soup {s}" for s in (2, 6, 9, 10, 35))


@functools.lru_cache(maxsize=None)
def _want(name):
    v, t, kw = _cases()[name]
    out = RR.repair(v, t, **kw)
    return out, RR.report(out)


def _run(name):
    from gens_amd import ops
    v, t, kw = _cases()[name]
    got = ops.repair_mesh(_up(v, np.float64), _up(t, np.int32), **kw)
    return dict(zip(("vertices",) + INTEGER_FIELDS + ("stats",), got))


def _check_against(got, want, source_vertices, name):
    for field in INTEGER_FIELDS:
        assert _same(got[field].cpu().numpy(), want[field]), (name, field)
    assert got["stats"] == want["stats"] and tuple(got["stats"]) == RR.STAT_KEYS, (name, got["stats"], want["stats"])
    gv, src = got["vertices"].cpu().numpy(), want["vertex_source"]
    assert gv.shape == want["vertices"].shape and gv.dtype == np.float64
    kept = src >= 0
    assert _same(gv[kept], np.asarray(source_vertices, dtype=np.float64)[src[kept]]), name       # bit-identical to their sources
    # a centroid: an ordered sum of k <= 1 000 terms, each good to an ulp, then one division
    bound = 1e-12 * (1.0 + np.abs(want["vertices"]).max(initial=0.0))
    err = np.abs(gv[~kept] - want["vertices"][~kept]).max(initial=0.0)
    print(f"{name}: {int((~kept).sum())} centroids, max error {err:.3e} (bound {bound:.3e}); {got['stats']}")
    assert err <= bound, (name, err, bound)


def _check_report(got, want, name, moved=0, size=1.0):
    """Counts exactly.  Area and volume: 1e-12 relative, as K37's tests ask, plus what `moved` fill faces can add when their apex lies
    within 1e-12 x size of the restatement's: a face's area changes by at most half its opposite edge (<= size) times that, its signed
    volume by a sixth of |a x b| (<= size^2) times that."""
    assert set(got) == set(want), name
    for k in want:
        if k in ("area", "volume"):
            slack = moved * 1e-12 * size * (size if k == "area" else size * size)
            assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]) + slack, (name, k, got[k], want[k])
        else:
            assert got[k] == want[k] and type(got[k]) is type(want[k]), (name, k, got[k], want[k])


@gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_every_output_equals_the_restatement(name):
    from gens_amd import ops
    want, want_report = _want(name)
    got = _run(name)
    _check_against(got, want, _cases()[name][0], name)
    rep = ops.mesh_topology(got["vertices"], got["triangles"]).report()
    size = 1.0 + float(np.abs(want["vertices"]).max(initial=0.0))
    _check_report(rep, want_report, name, moved=want["stats"]["fill_faces"], size=size)
    assert rep["manifold"] and rep["faces_invalid"] == 0 and rep["vertices_referenced"] == rep["vertices"]
    if _cases()[name][2].get("split", True) and _cases()[name][2].get("orient", True) and not want["stats"]["components_nonorientable"]:
        assert rep["oriented"]


@gpu
def test_what_the_walk_shapes_are_there_for():
    for n in (63, 64, 65, 257):
        want = _want(f"cones {n}")[0]
        assert want["stats"]["vertices_split"] == n - 1 and (want["vertex_source"][:n] == 0).all() and (want["vertex_source"][n:] > 0).all()
        assert want["stats"]["loops_open"] == n and want["stats"]["loops_filled"] == 0            # lone triangles: their rims stay open
    book = _want("book 65")
    assert book[0]["stats"]["vertices_split"] == 2 * 64 and book[1]["components"] == 65 and book[1]["edges_nonmanifold"] == 0
    for n in (63, 64, 65, 1000):
        want, rep = _want(f"disk {n}")
        assert want["stats"]["fill_faces"] == n and want["stats"]["fill_vertices"] == 1 and rep["watertight"] and rep["genus"] == 0
    assert _want("disk 65 open")[0]["stats"] == {**dict.fromkeys(RR.STAT_KEYS, 0), "split_rounds": 1, "loops_open": 1}
    strip = _want("strip 1000")
    assert strip[0]["face_flipped"].sum() == 500 and strip[0]["face_flipped"][1::2].all() and strip[1]["oriented"] and strip[1]["edges_flipped"] == 0
    isl = _want("islands 65")
    assert isl[1]["components"] == 33 and isl[0]["stats"]["faces_small_component"] == 32 * 33 // 2 and len(isl[0]["triangles"]) == sum(range(33, 66))
    ball = _want("clustered sphere")
    assert ball[0]["stats"]["vertices_split"] > 0 and ball[0]["stats"]["loops_filled"] > 0
    assert len(isl[0]["vertices"]) > 256 * 6 and len(_want("disk 1000")[0]["triangles"]) > 256 * 7       # more than one workgroup of every item
    assert sum(_want(f"soup {s}")[0]["stats"]["loops_filled"] for s in (2, 6, 9, 10, 35)) > 0


@gpu
def test_the_same_bits_twice_and_a_second_pass_changes_nothing():
    from gens_amd import ops
    for name in ("clustered sphere", "soup 10", "disk 1000"):
        a, b = _run(name), _run(name)
        for field in ("vertices",) + INTEGER_FIELDS:
            assert torch.equal(a[field], b[field]), (name, field)
        again = ops.repair_mesh(a["vertices"], a["triangles"], **_cases()[name][2])
        assert torch.equal(again[0], a["vertices"]) and torch.equal(again[1], a["triangles"]) and not again[4].any(), name
        assert (again[2] == torch.arange(len(again[2]), device="cuda")).all() and (again[3] == torch.arange(len(again[3]), device="cuda")).all()


@gpu
def test_io_repair_mesh_and_the_command_line(tmp_path, capsys):
    from gens_amd import io as gio, repair_mesh as cli
    v, t = RR.cube_minus_square()
    want = _want("cube_hole_filled")[0]
    normals = v - 0.5
    colors = (np.arange(24).reshape(8, 3) * 10).astype(np.uint8)
    seen = np.arange(8) != 2
    out_v, out_t, attrs = gio.repair_mesh(v, t.astype(np.int64), normals=normals, colors=colors, seen=seen, max_hole_edges=4)
    assert _same(out_v, want["vertices"]) and _same(out_t, want["triangles"].astype(np.int64)) and attrs["stats"] == want["stats"]
    for field in ("vertex_source", "face_source", "face_flipped"):
        assert _same(attrs[field], want[field]), field
    carried = gio.carry_repair_attributes(want["triangles"], want["vertex_source"], want["face_source"], normals=normals, colors=colors, seen=seen)
    assert set(attrs) == {"normals", "colors", "seen", "vertex_source", "face_source", "face_flipped", "stats"}
    assert all(_same(attrs[k], carried[k]) for k in carried)
    assert attrs["normals"][8].tolist() == [-1.0, 0.0, 0.0] and attrs["colors"][8].tolist() == [45, 55, 65] and not attrs["seen"][8]
    tensors = gio.repair_mesh(torch.from_numpy(v), torch.from_numpy(t), max_hole_edges=4)
    assert _same(tensors[0], out_v) and _same(tensors[1], want["triangles"])
    fv, ft = RR.fin_octahedron()
    src, out = str(tmp_path / "fin.ply"), str(tmp_path / "out.ply")
    gio.write_ply(src, fv, ft, colors=(np.arange(21).reshape(7, 3) * 10).astype(np.uint8))
    assert cli.main([src, out, "--min-component", "2", "--fill", "8"]) == 0
    lines = capsys.readouterr().out.strip().split("\n")
    assert len(lines) == 3
    before, after, stats = (json.loads(x) for x in lines)
    assert before["edges_nonmanifold"] == 1 and not before["watertight"] and after["watertight"] and after["genus"] == 0 and after["faces"] == 8
    assert stats == {**dict.fromkeys(RR.STAT_KEYS, 0), "split_rounds": 1, "vertices_split": 2, "faces_small_component": 1}
    rv, rt, rattrs = gio.read_ply(out, attributes=True)
    assert np.array_equal(rt, TR.octahedron()[1]) and len(rv) == 6 and rattrs["colors"].tolist() == (np.arange(18).reshape(6, 3) * 10).tolist()
    assert cli.main([src, out, "--no-split", "--no-orient"]) == 0
    assert json.loads(capsys.readouterr().out.strip().split("\n")[1])["edges_nonmanifold"] == 1


# ------------------------------------------------------------------------------------------------------------------------------------
# the model: the g23 surface of tests/test_hip_mesh_simplify.py, R = 64, simplified at cell 4 (which leaves a fin on a non-manifold edge,
# pinched vertices and a small hole; at cell 2 the mesh is watertight as it is)
# ------------------------------------------------------------------------------------------------------------------------------------
R = 64
SIMPLIFY = 4


@functools.lru_cache(maxsize=None)
def _model_want():
    """The simplified mesh in index coordinates, ops.repair_mesh of it and the restatement of that."""
    from gens_amd import ops
    from .test_hip_mesh_simplify import _model
    m = _model()
    sv, st = ops.simplify_mesh(_up(m["full"][0], np.float64), _up(m["full"][1], np.int32), float(SIMPLIFY), origin=(-0.5, -0.5, -0.5))[:2]
    got = ops.repair_mesh(sv, st, **MODEL_REPAIR)
    sv, st = sv.cpu().numpy(), st.cpu().numpy()
    return (sv, st), got, RR.repair(sv, st, **MODEL_REPAIR)


@gpu
def test_extract_geometry_repairs_on_every_route():
    from gens_amd import lib as L, ops
    from .test_hip_mesh_simplify import ROUTES, _model, _world
    from .test_hip_mesh_texture import _same_dict
    from .test_hip_vertex_attrs import _same as same_attrs, _validate_args
    m = _model()
    surf, vols, views, lo, hi = m["surf"], m["vols"], m["views"], m["lo"], m["hi"]
    (sv, st), got, want = _model_want()
    _check_against(dict(zip(("vertices",) + INTEGER_FIELDS + ("stats",), got)), want, sv, "g23")
    rv, rt, stats = got[0].cpu().numpy(), got[1].cpu().numpy(), got[5]
    before = ops.mesh_topology(_up(sv, np.float64), _up(st, np.int32)).report()
    after = ops.mesh_topology(got[0], got[1]).report()
    print(f"g23 R = {R}, cell {SIMPLIFY}: before {json.dumps(before)}")
    print(f"g23 R = {R}, cell {SIMPLIFY}: after  {json.dumps(after)}; {json.dumps(stats)}")
    assert before["edges_nonmanifold"] > 0 and before["vertices_pinched"] > 0 and before["edges_boundary"] > 0        # there is something to repair
    assert after["manifold"] and after["oriented"] and after["edges_nonmanifold"] == 0 and after["vertices_pinched"] == 0
    assert stats["vertices_split"] > 0 and stats["faces_small_component"] > 0 and stats["fill_vertices"] > 0 and (got[2] == -1).sum() == stats["fill_vertices"]
    surf.lattice_lipschitz = m["lipschitz"]
    try:
        for route, kw in ROUTES:
            plain = surf.extract_geometry(vols, lo, hi, R, 0.0, simplify=SIMPLIFY, **kw)
            assert _same(plain[0], _world(sv, lo, hi)) and _same(plain[1], st) and surf.last_repair_stats is None
            L.profile_begin(only=K38)
            v, t, attrs, tex = surf.extract_geometry(vols, lo, hi, R, 0.0, simplify=SIMPLIFY, repair=MODEL_REPAIR, topology=True, views=views,
                                                     attributes=("normals", "colors"), texture=4, **kw)
            launched = {k for k, *_ in L.profile_end(raw=True)}
            assert {"gens_mesh_face_keys", "gens_mesh_split_corners", "gens_mesh_orient_pairs"} <= launched <= K38, route
            assert _same(v, _world(rv, lo, hi)) and _same(t, rt), route          # ops.repair_mesh of the un-repaired call's mesh
            assert surf.last_repair_stats == {**stats, "topology_before": before} and surf.last_mesh_topology == after, route
            assert surf.last_simplify_stats["output_triangles"] == len(st)
            # the attributes and the atlas are those of the repaired mesh
            assert same_attrs(attrs, surf.vertex_attributes(v, vols, views)) and len(attrs["normals"]) == len(rv), route
            assert _same_dict(tex, surf.texture_mesh(v, t, vols, views, texels=4)), route
        two = surf.extract_geometry(vols, lo, hi, R, 0.0, simplify=SIMPLIFY, repair=True)
        defaults = ops.repair_mesh(_up(sv, np.float64), _up(st, np.int32))
        assert len(two) == 2 and _same(two[1], defaults[1].cpu().numpy()) and surf.last_repair_stats == defaults[5] and surf.last_mesh_topology is None
        # the attribute and validate
        surf.mesh_repair = MODEL_REPAIR
        try:
            again = surf.extract_geometry(vols, lo, hi, R, 0.0, simplify=SIMPLIFY)
            assert _same(again[0], v) and _same(again[1], t) and surf.last_repair_stats == stats
            off = surf.extract_geometry(vols, lo, hi, R, 0.0, simplify=SIMPLIFY, repair=False)
            assert _same(off[1], st) and surf.last_repair_stats is None
        finally:
            del surf.mesh_repair
        torch.manual_seed(3)
        out = surf.validate(*_validate_args(surf, vols), extract_geometry=True, mesh_resolution=R, mesh_simplify=SIMPLIFY, mesh_repair=MODEL_REPAIR)
        assert _same(out["vertices"], v) and _same(out["triangles"], t) and surf.last_repair_stats == stats
    finally:
        surf.lattice_lipschitz = 2.0


@gpu
def test_nothing_changes_when_the_option_is_unset():
    from gens_amd import lib as L
    from gens_amd.models.modules.implicit_surface import ImplicitSurface
    from .test_hip_mesh_simplify import _model, _world
    from .test_hip_vertex_attrs import TODAYS_KEYS, _validate_args
    assert ImplicitSurface.mesh_repair is None and ImplicitSurface.last_repair_stats is None
    m = _model()
    surf, vols, lo, hi = m["surf"], m["vols"], m["lo"], m["hi"]
    assert "mesh_repair" not in vars(surf)
    L.profile_begin(only=K38)
    for off in ({}, {"repair": None}, {"repair": False}):
        got = surf.extract_geometry(vols, lo, hi, R, 0.0, simplify=2, topology=True, **off)
        assert len(got) == 2 and _same(got[0], _world(m["simple"][0], lo, hi)) and _same(got[1], m["simple"][1]), off
        assert surf.last_repair_stats is None and set(surf.last_simplify_stats) == set(m["simple"][3]) | {"topology_before"}
        plain = surf.extract_geometry(vols, lo, hi, R, 0.0, **off)
        assert _same(plain[0], _world(m["full"][0], lo, hi)) and _same(plain[1], m["full"][1]) and surf.last_repair_stats is None
    args = _validate_args(surf, vols)
    torch.manual_seed(3)
    ref = surf.validate(*args, extract_geometry=True, mesh_resolution=33, mesh_simplify=2)
    torch.manual_seed(3)
    off = surf.validate(*args, extract_geometry=True, mesh_resolution=33, mesh_simplify=2, mesh_repair=False)
    assert not L.profile_end(raw=True)                                           # not one K38 launch
    assert set(ref) == set(off) == TODAYS_KEYS
    for k in TODAYS_KEYS:
        assert torch.equal(torch.as_tensor(off[k]), torch.as_tensor(ref[k])), k


@gpu
def test_refusals_come_before_any_launch():
    from gens_amd import io as gio, lib as L, ops
    from .test_hip_mesh_simplify import K33, _model
    from .test_hip_mesh_topology import K37
    from .test_hip_vertex_attrs import NETWORK, _validate_args
    m = _model()
    surf, vols, lo, hi = m["surf"], m["vols"], m["lo"], m["hi"]
    v, t = TR.cube()
    dv, dt = _up(v, np.float64), _up(t, np.int32)
    L.profile_begin(only=K38 | K37 | K33 | NETWORK | {"gens_face_cc_hook", "gens_compact_valid", "gens_mc_classify", "gens_lattice_points"})
    for bad in (1, "yes", {"holes": 3}, {"split": 1}, {"max_hole_edges": 4, "orient": False}, {"min_component_faces": -1}, 2.0):
        with pytest.raises(ValueError):
            surf.extract_geometry(vols, lo, hi, 33, 0.0, repair=bad)
        with pytest.raises(ValueError):
            surf.validate(*_validate_args(surf, vols), extract_geometry=True, mesh_resolution=33, mesh_repair=bad)
    for bad_v, bad_t in ((dv.float(), dt), (dv, dt.long()), (dv[:, :2], dt), (dv, dt.reshape(-1)), (dv.cpu(), dt)):
        with pytest.raises(ValueError):
            ops.repair_mesh(bad_v, bad_t)
    for bad in ({"split": 1}, {"orient": None}, {"dedupe": "no"}, {"min_component_faces": 1.5}, {"max_hole_edges": -1},
                {"max_hole_edges": 3, "split": False}):
        with pytest.raises(ValueError):
            ops.repair_mesh(dv, dt, **bad)
        with pytest.raises(ValueError):
            gio.repair_mesh(v, t, **bad)
    with pytest.raises(ValueError, match="rows"):
        gio.repair_mesh(v, t, seen=np.ones(3, dtype=bool))
    assert not L.profile_end(raw=True)
