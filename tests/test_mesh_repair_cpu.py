"""CPU tests of the mesh repair (K38): the numpy restatement (tests/mesh_repair_reference.py) on shapes whose answers are known by hand,
its properties on seeded triangle soups and a vertex-clustered marching-cubes sphere, and every refusal of the new entry points and Python
layers, without a GPU."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from . import mesh_repair_reference as RR
from . import mesh_topology_reference as TR

CASES = RR.hand_cases()
N_SOUPS = 200


@functools.lru_cache(maxsize=None)
def _out(name):
    v, t, kw = CASES[name]
    return RR.repair(v, t, **kw)


def _stats(name, **expect):
    stats = _out(name)["stats"]
    assert tuple(stats) == RR.STAT_KEYS
    want = {**dict.fromkeys(RR.STAT_KEYS, 0), "split_rounds": 1, **expect}
    assert stats == want, (name, stats)


def test_two_tetrahedra_sharing_a_vertex_come_apart():
    out, rep = _out("tetrahedra_vertex"), RR.report(_out("tetrahedra_vertex"))
    assert len(out["vertices"]) == 8 and rep["components"] == 2 and rep["watertight"] and rep["genus"] == 0 and rep["vertices_pinched"] == 0
    assert out["vertex_source"].tolist() == [0, 0, 1, 2, 3, 4, 5, 6] and not out["face_flipped"].any()
    _stats("tetrahedra_vertex", vertices_split=1)


def test_two_tetrahedra_sharing_an_edge_come_apart():
    out, rep = _out("tetrahedra_edge"), RR.report(_out("tetrahedra_edge"))
    assert len(out["vertices"]) == 8 and rep["components"] == 2 and rep["watertight"] and rep["edges_nonmanifold"] == 0
    assert out["vertex_source"].tolist() == [0, 0, 1, 1, 2, 3, 4, 5]
    _stats("tetrahedra_edge", vertices_split=2)


def test_the_fin_on_an_octahedron():
    out, rep = _out("fin_dropped"), RR.report(_out("fin_dropped"))
    assert rep["watertight"] and rep["genus"] == 0 and out["face_source"].tolist() == list(range(8)) and len(out["vertices"]) == 6
    assert np.array_equal(out["triangles"], TR.octahedron()[1])
    _stats("fin_dropped", vertices_split=2, faces_small_component=1)
    out, rep = _out("fin_kept"), RR.report(_out("fin_kept"))
    assert rep["components"] == 2 and rep["boundary_components"] == 1 and rep["edges_boundary"] == 3 and rep["manifold"] and len(out["triangles"]) == 9
    assert rep["largest_component_faces"] == 8 and len(out["vertices"]) == 9


def test_one_reversed_face_of_a_cube_is_turned_back():
    out, rep = _out("cube_one_reversed"), RR.report(_out("cube_one_reversed"))
    assert rep["watertight"] and abs(rep["volume"] - 1.0) <= 1e-12 and out["face_flipped"].sum() == 1 and out["face_flipped"][5]
    assert np.array_equal(out["triangles"][5], np.roll(TR.cube()[1][5], 1)) and np.array_equal(np.delete(out["triangles"], 5, 0), np.delete(TR.cube()[1], 5, 0))
    _stats("cube_one_reversed", components_flipped=1)


def test_the_majority_wins():
    out, rep = _out("cube_all_but_one_reversed"), RR.report(_out("cube_all_but_one_reversed"))
    assert rep["watertight"] and abs(rep["volume"] + 1.0) <= 1e-12 and out["face_flipped"].sum() == 1 and out["face_flipped"][7]


def test_on_a_tie_the_smallest_faces_side_keeps_its_winding():
    out, rep = _out("two_face_tie"), RR.report(_out("two_face_tie"))
    assert out["triangles"].tolist() == [[0, 1, 2], [0, 3, 1]] and out["face_flipped"].tolist() == [False, True] and rep["oriented"]


def test_a_moebius_strip_is_left_alone():
    v, t, _ = CASES["moebius"]
    out = _out("moebius")
    assert np.array_equal(out["triangles"], t) and np.array_equal(out["vertices"], v) and not out["face_flipped"].any()
    _stats("moebius", components_nonorientable=1, loops_open=1)              # its one loop is not closed either
    assert not RR.report(out)["oriented"] and RR.report(out)["boundary_components"] == 1


def test_a_square_hole_gets_a_centroid_fan():
    out, rep = _out("cube_hole_filled"), RR.report(_out("cube_hole_filled"))
    assert rep["watertight"] and abs(rep["volume"] - 1.0) <= 1e-12 and len(out["triangles"]) == 14 and len(out["vertices"]) == 9
    assert out["vertices"][8].tolist() == [0.0, 0.5, 0.5] and out["vertex_source"][8] == -1 and (out["face_source"][10:] == -1).all()
    _stats("cube_hole_filled", loops_filled=1, fill_faces=4, fill_vertices=1)
    out, rep = _out("cube_hole_open"), RR.report(_out("cube_hole_open"))
    assert not rep["closed"] and len(out["triangles"]) == 10 and rep["boundary_components"] == 1
    _stats("cube_hole_open", loops_open=1)


def test_a_triangular_hole_gets_one_face():
    out, rep = _out("tetrahedron_hole"), RR.report(_out("tetrahedron_hole"))
    assert rep["watertight"] and abs(rep["volume"] - 1.0 / 6.0) <= 1e-12 and len(out["vertices"]) == 4 and out["face_source"].tolist() == [0, 1, 2, -1]
    _stats("tetrahedron_hole", loops_filled=1, fill_faces=1)


def test_duplicates_invalid_faces_unreferenced_vertices_and_empty_meshes():
    out = RR.repair(*RR.odd_soup())
    assert out["face_source"].tolist() == [0, 6] and out["vertex_source"].tolist() == [0, 1, 2, 3]       # vertices 4 and 5 are unreferenced
    assert out["stats"]["faces_invalid"] == 3 and out["stats"]["faces_duplicate"] == 3
    kept = _out("odd_soup_no_dedupe")
    assert kept["face_source"].tolist() == [0, 1, 2, 6, 7] and kept["stats"]["faces_duplicate"] == 0 and kept["stats"]["faces_invalid"] == 3
    assert RR.report(_out("odd_soup"))["watertight"]
    for name in ("empty", "no_faces"):
        out = _out(name)
        assert out["vertices"].shape == (0, 3) and out["triangles"].shape == (0, 3) and out["vertex_source"].shape == (0,)
        assert out["triangles"].dtype == np.int32 and out["face_flipped"].dtype == bool
    off = _out("cube_no_split_no_orient")
    assert np.array_equal(off["triangles"], CASES["cube_no_split_no_orient"][1]) and off["stats"]["split_rounds"] == 0
    with pytest.raises(ValueError):
        RR.repair(*TR.cube(), max_hole_edges=4, orient=False)


# ------------------------------------------------------------------------------------------------------------------------------------
# properties
# ------------------------------------------------------------------------------------------------------------------------------------
def _position_triples(vertices, triangles, valid_only=True):
    """The multiset of the faces' position triples up to winding."""
    out = {}
    nv = len(vertices)
    for tri in np.asarray(triangles).reshape(-1, 3):
        ids = [int(i) for i in tri]
        if valid_only and not (all(0 <= i < nv for i in ids) and len(set(ids)) == 3):
            continue
        key = tuple(sorted(tuple(vertices[i].tolist()) for i in ids))
        out[key] = out.get(key, 0) + 1
    return out


def _check_properties(v, t, kw):
    out = RR.repair(v, t, **kw)
    topo = TR.topology(out["vertices"], out["triangles"], normals=False)
    rep = topo["report"]
    # no class-4 edge and no pinch: no exceptions
    assert rep["edges_nonmanifold"] == 0 and rep["vertices_pinched"] == 0 and rep["manifold"] and rep["faces_invalid"] == 0
    assert rep["vertices_referenced"] == rep["vertices"]
    # no class-3 edge outside non-orientable components
    plain = RR.repair(out["vertices"], out["triangles"], dedupe=False)
    assert plain["stats"]["components_nonorientable"] == out["stats"]["components_nonorientable"]
    if out["stats"]["components_nonorientable"] == 0:
        assert rep["edges_flipped"] == 0
    else:
        nt = len(out["triangles"])
        sets = TR._Sets(2 * nt)
        for e in range(len(topo["edges"])):
            if topo["edge_class"][e] in (2, 3):
                fa, fb = (int(h) // 3 for h in topo["edge_halfedges"][e])
                cross = 1 if topo["edge_class"][e] == 3 else 0
                sets.join(2 * fa, 2 * fb + cross)
                sets.join(2 * fa + 1, 2 * fb + 1 - cross)
        label = sets.labels()
        for e in range(len(topo["edges"])):
            if topo["edge_class"][e] == 3:
                f = int(topo["edge_halfedges"][e, 0]) // 3
                assert label[2 * f] == label[2 * f + 1]
    # the kept faces are the deduped input's, position for position
    kept = out["face_source"] >= 0
    deduped = RR.repair(v, t, split=False, orient=False)
    if not kw.get("min_component_faces"):
        assert _position_triples(out["vertices"], out["triangles"][kept]) == _position_triples(deduped["vertices"], deduped["triangles"])
    # the source maps reproduce positions bit for bit
    old = out["vertex_source"] >= 0
    assert np.array_equal(out["vertices"][old], np.asarray(v, dtype=np.float64)[out["vertex_source"][old]])
    vv, tt = np.asarray(v, dtype=np.float64), np.asarray(t)
    for f in np.nonzero(kept)[0]:
        got = out["vertices"][out["triangles"][f]]
        a, b, c = vv[tt[out["face_source"][f]]]
        assert np.array_equal(got, np.array([a, c, b]) if out["face_flipped"][f] else np.array([a, b, c]))
    # idempotent
    again = RR.repair(out["vertices"], out["triangles"], **kw)
    assert np.array_equal(again["vertices"], out["vertices"]) and np.array_equal(again["triangles"], out["triangles"])
    assert not again["face_flipped"].any() and again["stats"]["vertices_split"] == 0
    return out


@pytest.mark.parametrize("block", range(4))
def test_the_properties_hold_on_random_triangle_soups(block):
    filled = 0
    for seed in range(block * N_SOUPS // 4, (block + 1) * N_SOUPS // 4):
        v, t = RR.random_soup(seed)
        kw = (RR.DEFAULTS, RR.ALL_ON, {"max_hole_edges": 5}, {"min_component_faces": 3})[seed % 4]
        filled += _check_properties(v, t, kw)["stats"]["loops_filled"]
    assert filled > 0


def test_the_properties_hold_on_a_clustered_marching_cubes_sphere():
    v, t = RR.clustered_sphere()
    before = TR.topology(v, t, normals=False)["report"]
    assert before["edges_nonmanifold"] + before["vertices_pinched"] > 0         # the simplification left something to repair
    for kw in (RR.DEFAULTS, RR.ALL_ON):
        _check_properties(v, t, kw)


# ------------------------------------------------------------------------------------------------------------------------------------
# the library's host side and the Python layers, without a GPU
# ------------------------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_report_bad_arguments_without_a_gpu():
    from gens_amd import lib as L
    lib = L.load()
    p = lambda k: C.c_void_p(0x1000 + 0x100 * k)  # noqa: E731  (never dereferenced: every call below is refused, or launches nothing)
    big = 1 << 31

    def refused(rc, *words, code=-1):
        msg = lib.gens_last_error().decode()
        assert rc == code and all(w in msg for w in words), (rc, msg)

    def nulls(fn, ok, which, who):
        for k in which:
            refused(fn(*[None if j == k else a for j, a in enumerate(ok)]), who, "null pointer")

    def edit(ok, **at):
        return [at.get(f"a{j}", a) for j, a in enumerate(ok)]

    who, fn = "gens_mesh_face_keys", lib.gens_mesh_face_keys
    ok = [p(0), 4, 4, p(1), p(2), None]
    nulls(fn, ok, (0, 3, 4), who)
    refused(fn(*edit(ok, a1=-1)), who, "-1 faces")
    refused(fn(*edit(ok, a2=-4)), who, "-4 vertices")
    refused(fn(*edit(ok, a2=big)), who, "below 2^31", code=-2)
    refused(fn(*edit(ok, a1=(big + 2) // 3)), who, "below 2^31", code=-2)
    assert fn(None, 0, 4, None, None, None) == 0

    who, fn = "gens_mesh_split_corners", lib.gens_mesh_split_corners
    ok = [p(0), p(1), p(2), p(3), 4, 9, 5, p(4), p(5), None]
    nulls(fn, ok, (0, 1, 2, 3, 7, 8), who)
    refused(fn(*edit(ok, a4=-1)), who, "-1 vertices")
    refused(fn(*edit(ok, a5=-3)), who, "-3 half-edges")
    refused(fn(*edit(ok, a6=-2)), who, "-2 new vertices")
    refused(fn(*edit(ok, a5=10)), who, "three per face")
    refused(fn(*edit(ok, a6=10)), who, "a fan has a corner")
    refused(fn(*edit(ok, a4=big)), who, "below 2^31", code=-2)
    refused(fn(*edit(ok, a5=big + 1)), who, "below 2^31", code=-2)
    assert fn(*[None] * 4, 4, 0, 0, None, None, None) == 0

    who, fn = "gens_mesh_orient_pairs", lib.gens_mesh_orient_pairs
    ok = [p(0), p(1), 5, 3, p(2), None]
    nulls(fn, ok, (0, 1, 4), who)
    refused(fn(*edit(ok, a2=-5)), who, "-5 edges")
    refused(fn(*edit(ok, a3=-3)), who, "-3 faces")
    refused(fn(*edit(ok, a2=10)), who, "an edge has a use")
    refused(fn(*edit(ok, a3=big)), who, "below 2^31", code=-2)
    assert fn(None, None, 0, 3, None, None) == 0

    who, fn = "gens_mesh_apply_flips", lib.gens_mesh_apply_flips
    ok = [p(0), p(1), 3, p(2), None]
    nulls(fn, ok, (0, 1, 3), who)
    refused(fn(*edit(ok, a2=-3)), who, "-3 faces")
    refused(fn(*edit(ok, a2=big)), who, "below 2^31", code=-2)
    assert fn(None, None, 0, None, None) == 0

    who, fn = "gens_mesh_loop_centroids", lib.gens_mesh_loop_centroids
    ok = [p(0), 9, p(1), p(2), 2, 8, p(3), 1, p(4), None]
    nulls(fn, ok, (0, 2, 3, 6, 8), who)
    refused(fn(*edit(ok, a1=-9)), who, "-9 vertices")
    refused(fn(*edit(ok, a4=-2)), who, "-2 loops")
    refused(fn(*edit(ok, a5=-8)), who, "-8 rim vertices")
    refused(fn(*edit(ok, a7=-1)), who, "-1 centroids")
    refused(fn(*edit(ok, a5=10)), who, "a loop has a vertex")
    refused(fn(*edit(ok, a4=9)), who, "a loop has a vertex")
    refused(fn(*edit(ok, a7=3)), who, "a loop has a vertex")
    refused(fn(*edit(ok, a1=big)), who, "below 2^31", code=-2)
    assert fn(None, 9, None, None, 0, 0, None, 0, None, None) == 0 and fn(None, 9, None, None, 2, 8, None, 0, None, None) == 0

    who, fn = "gens_mesh_fill_emit", lib.gens_mesh_fill_emit
    ok = [p(0), 6, 9, p(1), p(2), 8, p(3), p(4), p(5), p(6), 2, 7, p(7), None]
    nulls(fn, ok, (0, 3, 4, 6, 7, 8, 9, 12), who)
    refused(fn(*edit(ok, a1=-6)), who, "-6 faces")
    refused(fn(*edit(ok, a2=-9)), who, "-9 vertices")
    refused(fn(*edit(ok, a5=-8)), who, "-8 rim half-edges")
    refused(fn(*edit(ok, a10=-2)), who, "-2 loops")
    refused(fn(*edit(ok, a11=-7)), who, "-7 fill faces")
    refused(fn(*edit(ok, a5=19, a2=30)), who, "a rim vertex has a rim half-edge")
    refused(fn(*edit(ok, a2=7)), who, "a rim vertex has a rim half-edge")
    refused(fn(*edit(ok, a10=9)), who, "a rim vertex has a rim half-edge")
    refused(fn(*edit(ok, a11=9)), who, "a rim vertex has a rim half-edge")
    refused(fn(*edit(ok, a2=big)), who, "below 2^31", code=-2)
    refused(fn(*edit(ok, a1=big)), who, "below 2^31", code=-2)
    assert fn(None, 6, 9, None, None, 0, None, None, None, None, 0, 0, None, None) == 0
    assert fn(None, 6, 9, None, None, 8, None, None, None, None, 2, 0, None, None) == 0
    assert lib.gens_abi_version() == 12
    for name, n_args in (("gens_mesh_face_keys", 6), ("gens_mesh_split_corners", 10), ("gens_mesh_orient_pairs", 6), ("gens_mesh_apply_flips", 5),
                         ("gens_mesh_loop_centroids", 10), ("gens_mesh_fill_emit", 14)):
        assert len(L.SIGNATURES[name]) == n_args


def test_the_python_layers_refuse_bad_arguments_before_any_launch(tmp_path):
    from gens_amd import io as gio, ops, repair_mesh as cli
    from gens_amd.models.modules.implicit_surface import ImplicitSurface
    v, t = TR.cube()
    host_v, host_t = torch.from_numpy(v), torch.from_numpy(t)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.repair_mesh(host_v, host_t)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.repair_mesh(v, t)
    assert ops.repair_request("t") == {"split": True, "orient": True, "min_component_faces": 0, "max_hole_edges": 0, "dedupe": True}
    assert tuple(ops.repair_request("t")) == ops.REPAIR_KEYS and ops.REPAIR_STAT_KEYS == RR.STAT_KEYS
    bad_options = [{"split": 1}, {"orient": "yes"}, {"dedupe": None}, {"min_component_faces": -1}, {"min_component_faces": 2.0},
                   {"max_hole_edges": True}, {"max_hole_edges": 2 ** 31}, {"max_hole_edges": 4, "split": False},
                   {"max_hole_edges": 4, "orient": False}, {"holes": 4}]
    for bad in bad_options:
        with pytest.raises(ValueError, match=next(iter(bad)) if len(bad) == 1 else "max_hole_edges"):
            ops.repair_request("t", **bad)
        with pytest.raises(ValueError):
            gio.repair_mesh(v, t, **bad)                                         # (before the device is looked at)
    # extract_geometry's option: None and False are off, True the defaults, a dict the keywords
    surf = types.SimpleNamespace(mesh_repair=None)
    req = lambda x: ImplicitSurface._repair_request(surf, x)  # noqa: E731
    assert ImplicitSurface.mesh_repair is None and ImplicitSurface.last_repair_stats is None
    assert req(None) is None and req(False) is None and req(True) == ops.repair_request("t")
    assert req({"max_hole_edges": 8})["max_hole_edges"] == 8
    surf.mesh_repair = {"min_component_faces": 2}
    assert req(None)["min_component_faces"] == 2 and req(False) is None and req(True)["min_component_faces"] == 0
    for bad in (1, 0, "yes", 2.5, [], {1: 2}) + tuple(bad_options):
        with pytest.raises(ValueError):
            req(bad)
    # the host entry point
    with pytest.raises(ValueError, match="expected"):
        gio.repair_mesh(v[:, :2], t)
    with pytest.raises(ValueError, match="expected"):
        gio.repair_mesh(v, t.reshape(-1))
    with pytest.raises(ValueError, match="whole numbers"):
        gio.repair_mesh(v, t.astype(np.float64))
    with pytest.raises(ValueError, match="int32"):
        gio.repair_mesh(v, t.astype(np.int64) + 2 ** 31)
    with pytest.raises(ValueError, match="normals has 7 rows"):
        gio.repair_mesh(v, t, normals=np.zeros((7, 3)))
    path = str(tmp_path / "a.ply")
    gio.write_ply(path, v, t)
    out = str(tmp_path / "b.ply")
    assert cli.main([str(tmp_path / "missing.ply"), out]) == 2 and cli.main([str(tmp_path), out]) == 2
    assert cli.main([path, out, "--fill", "4", "--no-split"]) == 2 and cli.main([path, out, "--min-component", "-1"]) == 2


def test_extract_geometry_refuses_a_bad_repair_option_before_any_launch():
    from gens_amd.config import Conf, gens_model_conf
    from gens_amd.models.gens import GenS
    from gens_amd.models.modules.implicit_surface import ImplicitSurface
    surf = ImplicitSurface(gens_model_conf(volume_dims=(16, 8, 4))["implicit_surface"])
    lo, hi = torch.full((3,), -1.0), torch.full((3,), 1.0)
    for bad in (1, "yes", {"holes": 3}, {"max_hole_edges": 4, "orient": False}):
        with pytest.raises(ValueError, match="repair|max_hole_edges"):
            surf.extract_geometry([], lo, hi, 8, 0.0, repair=bad)
        with pytest.raises(ValueError, match="repair|max_hole_edges"):
            surf.validate(*[None] * 11, lo, hi, (4, 4), mesh_repair=bad)
    assert surf.last_repair_stats is None
    conf = gens_model_conf(volume_dims=(16, 8, 4), has_vol=True)
    assert "mesh_repair" not in vars(GenS(conf).implicit_surface)
    assert GenS(Conf({**conf, "mesh_repair": True})).implicit_surface.mesh_repair is True
    assert GenS(Conf({**conf, "mesh_repair": {"max_hole_edges": 8}})).implicit_surface.mesh_repair == {"max_hole_edges": 8}


def test_centroid_attributes_are_the_loops_means():
    from gens_amd import io as gio
    out = _out("cube_hole_filled")
    normals = np.tile(np.array([[0.0, 0.0, 2.0]]), (8, 1))
    normals[:4] = [[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 3.0, 0.0], [0.0, 1.0, 0.0]]               # the loop is the face x = 0: vertices 0 .. 3
    colors = (np.arange(24).reshape(8, 3) * 10).astype(np.uint8)
    seen = np.ones(8, dtype=bool)
    got = gio.carry_repair_attributes(out["triangles"], out["vertex_source"], out["face_source"], normals=normals, colors=colors, seen=seen)
    assert np.array_equal(got["normals"][:8], normals) and np.array_equal(got["colors"][:8], colors) and got["seen"].all()
    assert got["normals"][8].tolist() == [0.0, 1.0, 0.0] and got["colors"][8].tolist() == [45, 55, 65] and got["colors"].dtype == np.uint8
    seen[2] = False
    normals[:4] = [[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, -1.0, 0.0]]
    got = gio.carry_repair_attributes(out["triangles"], out["vertex_source"], out["face_source"], normals=normals, seen=seen)
    assert got["normals"][8].tolist() == [0.0, 0.0, 0.0] and not got["seen"][8] and got["seen"][[0, 1, 3]].all() and set(got) == {"normals", "seen"}
    three = _out("tetrahedron_hole")
    got = gio.carry_repair_attributes(three["triangles"], three["vertex_source"], three["face_source"], seen=np.ones(4, dtype=bool))
    assert got["seen"].shape == (4,) and got["seen"].all()
