"""CPU tests of the mesh topology (K37): the numpy restatement (tests/mesh_topology_reference.py) on shapes whose answers are known by hand,
its sign against the winding number, and every refusal of the new entry points and Python layers, without a GPU."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from . import mesh_distance_reference as DR
from . import mesh_topology_reference as TR

SHAPES = TR.hand_shapes()
SIGN_SEED = 5                       # chosen so that the precondition of the sign tests holds on every shape (asserted below)


def _report(name):
    return TR.topology(*SHAPES[name])["report"]


def _counts(rep):
    return tuple(rep[k] for k in ("edges_boundary", "edges_manifold", "edges_flipped", "edges_nonmanifold"))


def test_one_triangle():
    rep = _report("triangle")
    assert _counts(rep) == (3, 0, 0, 0) and rep["edges"] == 3 and rep["boundary_components"] == 1 and rep["euler"] == 1
    assert rep["components"] == 1 and not rep["closed"] and rep["oriented"] and rep["manifold"] and rep["genus"] is None
    assert rep["area"] == 0.5 and rep["faces_invalid"] == 0 and rep["vertices_referenced"] == 3


def test_two_triangles_on_an_edge():
    good, bad = TR.topology(*SHAPES["two_consistent"]), TR.topology(*SHAPES["two_flipped"])
    assert _counts(good["report"]) == (4, 1, 0, 0) and good["report"]["oriented"] and good["report"]["components"] == 1
    assert _counts(bad["report"]) == (4, 0, 1, 0) and not bad["report"]["oriented"] and bad["report"]["components"] == 1
    assert good["edges"][0].tolist() == [0, 1] and good["edge_forward"][0] == 1 and bad["edge_forward"][0] == 2
    assert good["edge_halfedges"][0].tolist() == [0, 3] and good["edge_class"][0] == 2 and bad["edge_class"][0] == 3
    assert (bad["vertex_flags"][:2] == (1 | 2 | 8)).all() and (good["vertex_flags"] == 3).all()
    assert good["report"]["boundary_components"] == 1 and good["report"]["euler"] == 1


def test_three_faces_on_one_edge():
    topo = TR.topology(*SHAPES["three_on_edge"])
    rep = topo["report"]
    assert _counts(rep) == (6, 0, 0, 1) and topo["edge_class"][0] == 4 and topo["edge_count"][0] == 3
    assert topo["edge_halfedges"][0].tolist() == [0, 3] and not rep["manifold"] and not rep["closed"]
    assert rep["components"] == 3 and rep["vertices_nonmanifold"] == 2 and topo["fans"][:2].tolist() == [3, 3]
    assert (topo["vertex_flags"][:2] & 4).all() and (topo["vertex_flags"][:2] & 16).all()


@pytest.mark.parametrize("name,volume,euler,genus", [("tetrahedron", 1.0 / 6.0, 2, 0), ("cube", 1.0, 2, 0), ("octahedron", 4.0 / 3.0, 2, 0),
                                                      ("cube_reversed", -1.0, 2, 0), ("l_prism", 4.0, 2, 0)])
def test_closed_solids(name, volume, euler, genus):
    topo = TR.topology(*SHAPES[name])
    rep = topo["report"]
    assert rep["watertight"] and rep["closed"] and rep["oriented"] and rep["manifold"] and rep["genus"] == genus and rep["euler"] == euler
    assert abs(rep["volume"] - volume) <= 1e-12 and rep["components"] == 1 and rep["boundary_components"] == 0
    assert rep["edges"] == rep["edges_manifold"] == 3 * rep["faces"] // 2 and (topo["fans"] == 1).all() and (topo["vertex_flags"] == 1).all()
    assert rep["largest_component_faces"] == rep["faces"]


def test_cube_figures():
    rep = _report("cube")
    assert rep["faces"] == 12 and rep["edges"] == 18 and rep["vertices"] == 8 and abs(rep["area"] - 6.0) <= 1e-12
    assert TR.topology(*SHAPES["cube"])["valence"].sum() == 36


def test_torus_has_genus_one():
    rep = _report("torus")
    assert rep["watertight"] and rep["genus"] == 1 and rep["euler"] == 0 and rep["faces"] == 96 and rep["edges"] == 144


def test_two_tetrahedra_sharing_a_vertex():
    topo = TR.topology(*SHAPES["tetrahedra_vertex"])
    rep = topo["report"]
    assert rep["closed"] and rep["oriented"] and not rep["manifold"] and not rep["watertight"] and rep["genus"] is None
    assert rep["edges_nonmanifold"] == 0 and rep["vertices_pinched"] == 1 and rep["vertices_nonmanifold"] == 1
    assert topo["fans"][0] == 2 and topo["valence"][0] == 6 and topo["vertex_flags"][0] == 17 and (topo["fans"][1:] == 1).all()
    assert rep["components"] == 2 and rep["largest_component_faces"] == 4 and rep["vertices"] == 7


def test_two_tetrahedra_sharing_an_edge():
    topo = TR.topology(*SHAPES["tetrahedra_edge"])
    rep = topo["report"]
    assert rep["edges_nonmanifold"] == 1 and topo["edges"][topo["edge_class"] == 4].tolist() == [[0, 1]] and topo["edge_count"][0] == 4
    assert not rep["closed"] and not rep["manifold"] and rep["edges_boundary"] == 0 and rep["vertices"] == 6


def test_cube_with_a_face_removed():
    rep = _report("cube_open")
    assert rep["boundary_components"] == 1 and rep["edges_boundary"] == 4 and not rep["closed"] and rep["manifold"] and rep["oriented"]
    assert rep["faces"] == 10 and rep["edges"] == 17 and rep["euler"] == 1


def test_invalid_faces_duplicates_and_unreferenced_vertices():
    topo = TR.topology(*SHAPES["odd_faces"])
    rep = topo["report"]
    assert rep["faces"] == 6 and rep["faces_invalid"] == 3 and topo["face_valid"].tolist() == [True, True, False, False, False, True]
    assert rep["vertices"] == 6 and rep["vertices_referenced"] == 4 and topo["vertex_flags"][4] == 0 and topo["vertex_flags"][5] == 0
    assert (topo["edge_of_halfedge"][6:15] == -1).all() and (topo["edge_of_halfedge"][:6] >= 0).all()
    # the duplicated face: its three edges have two uses in the same direction (flipped), (1, 2) a third from face 5
    assert topo["edges"].tolist() == [[0, 1], [0, 2], [1, 2], [1, 3], [2, 3]] and topo["edge_class"].tolist() == [3, 3, 4, 1, 1]
    assert topo["edge_count"].tolist() == [2, 2, 3, 1, 1] and topo["edge_halfedges"][2].tolist() == [1, 4]
    empty, bare = TR.topology(*SHAPES["empty"]), TR.topology(*SHAPES["no_faces"])
    for topo, nv in ((empty, 0), (bare, 4)):
        rep = topo["report"]
        assert rep["vertices"] == nv and rep["faces"] == rep["edges"] == rep["components"] == rep["euler"] == 0 and not rep["closed"]
        assert rep["oriented"] and rep["manifold"] and not rep["watertight"] and rep["genus"] is None and rep["area"] == rep["volume"] == 0.0
        assert len(topo["valence"]) == nv and not topo["vertex_flags"].any()


def test_marching_cubes_sphere_is_watertight():
    v, t = TR.mc_sphere(17)
    rep = TR.topology(v, t, normals=False)["report"]
    radius = 0.31 * 16
    assert rep["watertight"] and rep["genus"] == 0 and rep["components"] == 1 and rep["faces_invalid"] == 0 and rep["faces"] > 500
    assert abs(abs(rep["volume"]) / (4.0 / 3.0 * np.pi * radius ** 3) - 1.0) < 0.05 and abs(rep["area"] / (4.0 * np.pi * radius ** 2) - 1.0) < 0.05


# ------------------------------------------------------------------------------------------------------------------------------------
# the sign against the winding number
# ------------------------------------------------------------------------------------------------------------------------------------
def sign_case(name):
    """-> (v, t, topology, queries, K36's results, signed, dot, the chosen normals, the diagonal) of the restatement."""
    v, t = TR.mc_sphere(17) if name == "mc_sphere" else SHAPES[name]
    topo = TR.topology(v, t)
    q, diag = TR.sign_queries(v, t, SIGN_SEED, n=2000)
    near = DR.closest(v, t, q)
    signed, dot = TR.signed_distance(topo, t, q, near)
    return v, t, topo, q, near, signed, dot, TR.sign_normals(topo, t, near)[0], diag


@pytest.mark.parametrize("name", TR.WATERTIGHT + ("mc_sphere",))
def test_the_sign_equals_the_winding_number_side(name):
    v, t, topo, q, near, signed, dot, normals, diag = sign_case(name)
    assert topo["report"]["watertight"]
    assert TR.precondition(q, near, dot, normals, diag)                          # precondition
    assert not np.isnan(signed).any()                                            # no exceptions
    assert np.array_equal(np.abs(signed), np.sqrt(near["dist2"]))
    w = TR.winding_number(v, t, q)
    assert (np.abs(np.abs(w) - np.round(np.abs(w))) < 1e-6).all() and (np.abs(w) < 1.5).all()
    inside = np.abs(w) > 0.5
    outward = topo["report"]["volume"] > 0                                       # normals point outwards: inside is negative
    assert np.array_equal(signed < 0 if outward else signed > 0, inside)         # truth: zero exceptions
    assert inside.any() and (~inside).any()
    assert {0, 1, 4} <= set(int(r) if r == 0 else 1 if r <= 3 else 4 for r in near["region"]) or name in ("torus", "mc_sphere")


def test_the_closest_faces_normal_gives_wrong_signs_on_the_l_prism():
    """... which is why the sign takes pseudonormals: at a convex edge or vertex the smallest face index among the tied faces decides
    which face K36 names, and that face's plane can have the query on its inner side."""
    v, t, topo, q, near, signed, dot, normals, diag = sign_case("l_prism")
    u = q - near["point"]
    by_face = np.sign((u * topo["face_normal"][near["face"]]).sum(axis=1))
    assert (by_face != np.sign(signed)).sum() > 0
    assert (by_face[near["region"] == 0] == np.sign(signed)[near["region"] == 0]).all()


def test_the_open_cube_has_no_sign_at_its_rim():
    v, t = SHAPES["cube_open"]
    topo = TR.topology(v, t)
    q, diag = TR.sign_queries(v, t, SIGN_SEED, n=2000)
    near = DR.closest(v, t, q)
    signed, _ = TR.signed_distance(topo, t, q, near)
    rim_vertices = {0, 1, 2, 3}                                                 # the face x = 0 is the one removed
    rim = np.zeros(len(q), dtype=bool)
    for i in range(len(q)):
        f, r = int(near["face"][i]), int(near["region"][i])
        if 1 <= r <= 3:
            rim[i] = int(t[f, r - 1]) in rim_vertices
        elif r >= 4:
            rim[i] = {int(t[f, r - 4]), int(t[f, (r - 3) % 3])} <= rim_vertices
    assert rim.sum() > 20 and (~rim).sum() > 500
    assert np.isnan(signed[rim]).all() and not np.isnan(signed[~rim]).any()
    full_v, full_t = SHAPES["cube"]
    full_near = DR.closest(full_v, full_t, q)
    full_signed, _ = TR.signed_distance(TR.topology(full_v, full_t), full_t, q, full_near)
    same = ~rim & (full_near["dist2"] == near["dist2"]) & (full_near["point"] == near["point"]).all(axis=1)
    assert same.sum() > 500 and np.array_equal(full_signed[same], signed[same])


def test_on_the_mesh_the_distance_is_plus_zero():
    v, t = SHAPES["cube"]
    q = np.array([[0.5, 0.25, 0.0], [0.0, 0.0, 0.0], [1.0, 0.5, 1.0]])
    near = DR.closest(v, t, q)
    signed, _ = TR.signed_distance(TR.topology(v, t), t, q, near)
    assert (signed == 0.0).all() and not np.signbit(signed).any()


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

    who = "gens_mesh_edge_keys"
    refused(lib.gens_mesh_edge_keys(None, 4, 4, p(1), p(2), None), who, "null pointer")
    refused(lib.gens_mesh_edge_keys(p(0), 4, 4, None, p(2), None), who, "null pointer")
    refused(lib.gens_mesh_edge_keys(p(0), 4, 4, p(1), None, None), who, "null pointer")
    refused(lib.gens_mesh_edge_keys(p(0), -1, 4, p(1), p(2), None), who, "-1 faces")
    refused(lib.gens_mesh_edge_keys(p(0), 4, -4, p(1), p(2), None), who, "-4 vertices")
    refused(lib.gens_mesh_edge_keys(p(0), 4, big, p(1), p(2), None), who, "below 2^31", code=-2)
    refused(lib.gens_mesh_edge_keys(p(0), (big + 2) // 3, 4, p(1), p(2), None), who, "below 2^31", code=-2)
    assert lib.gens_mesh_edge_keys(None, 0, 4, None, None, None) == 0

    who = "gens_mesh_edge_classify"
    ok = [p(0), p(1), p(2), p(3), 5, 9, p(4), p(5), p(6), p(7), p(8), p(9), None]
    for k in (0, 1, 2, 3, 6, 7, 8, 9, 10, 11):
        refused(lib.gens_mesh_edge_classify(*[None if j == k else a for j, a in enumerate(ok)]), who, "null pointer")
    edit = lambda **kw: [kw.get({4: "e", 5: "h"}.get(j), a) for j, a in enumerate(ok)]  # noqa: E731
    refused(lib.gens_mesh_edge_classify(*edit(e=-1)), who, "-1 edges")
    refused(lib.gens_mesh_edge_classify(*edit(h=-3)), who, "-3 half-edges")
    refused(lib.gens_mesh_edge_classify(*edit(h=10)), who, "three per face")
    refused(lib.gens_mesh_edge_classify(*edit(e=10)), who, "an edge has a use")
    refused(lib.gens_mesh_edge_classify(*edit(h=big + 1)), who, "below 2^31", code=-2)
    assert lib.gens_mesh_edge_classify(*[None] * 4, 0, 0, *[None] * 7) == 0

    who = "gens_mesh_fan_pairs"
    ok = [p(0), 3, p(1), p(2), p(3), 5, p(4), None]
    for k in (0, 2, 3, 4, 6):
        refused(lib.gens_mesh_fan_pairs(*[None if j == k else a for j, a in enumerate(ok)]), who, "null pointer")
    refused(lib.gens_mesh_fan_pairs(p(0), -3, p(1), p(2), p(3), 5, p(4), None), who, "-3 faces")
    refused(lib.gens_mesh_fan_pairs(p(0), 3, p(1), p(2), p(3), -5, p(4), None), who, "-5 edges")
    refused(lib.gens_mesh_fan_pairs(p(0), 3, p(1), p(2), p(3), 10, p(4), None), who, "an edge has a use")
    refused(lib.gens_mesh_fan_pairs(p(0), big, p(1), p(2), p(3), 5, p(4), None), who, "below 2^31", code=-2)
    assert lib.gens_mesh_fan_pairs(None, 3, None, None, None, 0, None, None) == 0

    who = "gens_mesh_vertex_classify"
    ok = [p(0), p(1), p(2), p(3), p(4), 4, 9, 5, p(5), p(6), p(7), None]
    for k in (0, 1, 2, 3, 4, 8, 9, 10):
        refused(lib.gens_mesh_vertex_classify(*[None if j == k else a for j, a in enumerate(ok)]), who, "null pointer")
    edit = lambda **kw: [kw.get({5: "v", 6: "h", 7: "e"}.get(j), a) for j, a in enumerate(ok)]  # noqa: E731
    refused(lib.gens_mesh_vertex_classify(*edit(v=-1)), who, "-1 vertices")
    refused(lib.gens_mesh_vertex_classify(*edit(h=-3)), who, "-3 half-edges")
    refused(lib.gens_mesh_vertex_classify(*edit(e=-2)), who, "-2 edges")
    refused(lib.gens_mesh_vertex_classify(*edit(h=10)), who, "three per face")
    refused(lib.gens_mesh_vertex_classify(*edit(e=10)), who, "an edge has a use")
    refused(lib.gens_mesh_vertex_classify(*edit(v=big)), who, "below 2^31", code=-2)
    refused(lib.gens_mesh_vertex_classify(*edit(h=big + 1)), who, "below 2^31", code=-2)
    assert lib.gens_mesh_vertex_classify(*[None] * 5, 0, 9, 5, *[None] * 4) == 0

    who = "gens_mesh_pseudonormals"
    ok = [p(0), p(1), 4, 3, 5, p(2), p(3), p(4), p(5), p(6), p(7), p(8), None]
    for k in (0, 1, 5, 6, 7, 8, 9, 10, 11):
        refused(lib.gens_mesh_pseudonormals(*[None if j == k else a for j, a in enumerate(ok)]), who, "null pointer")
    edit = lambda **kw: [kw.get({2: "v", 3: "t", 4: "e"}.get(j), a) for j, a in enumerate(ok)]  # noqa: E731
    refused(lib.gens_mesh_pseudonormals(*edit(v=-1)), who, "-1 vertices")
    refused(lib.gens_mesh_pseudonormals(*edit(t=-1)), who, "-1 faces")
    refused(lib.gens_mesh_pseudonormals(*edit(e=-1)), who, "-1 edges")
    refused(lib.gens_mesh_pseudonormals(*edit(e=10)), who, "an edge has a use")
    refused(lib.gens_mesh_pseudonormals(*edit(v=big)), who, "below 2^31", code=-2)
    refused(lib.gens_mesh_pseudonormals(*edit(t=big)), who, "below 2^31", code=-2)
    assert lib.gens_mesh_pseudonormals(None, None, 0, 0, 0, *[None] * 8) == 0

    who = "gens_mesh_distance_sign"
    ok = [p(0), 7, p(1), p(2), p(3), p(4), p(5), 3, 4, 5, p(6), p(7), p(8), p(9), p(10), p(11), p(12), None]
    for k in (0, 2, 3, 4, 5, 6, 10, 11, 12, 13, 14, 15, 16):
        refused(lib.gens_mesh_distance_sign(*[None if j == k else a for j, a in enumerate(ok)]), who, "null pointer")
    edit = lambda **kw: [kw.get({1: "n", 7: "t", 8: "v", 9: "e"}.get(j), a) for j, a in enumerate(ok)]  # noqa: E731
    refused(lib.gens_mesh_distance_sign(*edit(n=-1)), who, "-1 queries")
    refused(lib.gens_mesh_distance_sign(*edit(t=-1)), who, "-1 faces")
    refused(lib.gens_mesh_distance_sign(*edit(v=-1)), who, "-1 vertices")
    refused(lib.gens_mesh_distance_sign(*edit(e=-1)), who, "-1 edges")
    refused(lib.gens_mesh_distance_sign(*edit(e=10)), who, "an edge has a use")
    refused(lib.gens_mesh_distance_sign(*edit(n=big)), who, "below 2^31", code=-2)
    refused(lib.gens_mesh_distance_sign(*edit(v=big)), who, "below 2^31", code=-2)
    assert lib.gens_mesh_distance_sign(None, 0, *[None] * 5, 3, 4, 5, *[None] * 8) == 0
    assert lib.gens_abi_version() == 12
    for name, n_args in (("gens_mesh_edge_keys", 6), ("gens_mesh_edge_classify", 13), ("gens_mesh_fan_pairs", 8), ("gens_mesh_vertex_classify", 12),
                         ("gens_mesh_pseudonormals", 13), ("gens_mesh_distance_sign", 18)):
        assert len(L.SIGNATURES[name]) == n_args


def test_the_python_layers_refuse_bad_arguments_before_any_launch(tmp_path):
    from gens_amd import compare_meshes as compare_cli, io as gio, mesh_report as cli, ops
    from gens_amd.models.modules.implicit_surface import ImplicitSurface
    v, t = SHAPES["cube"]
    host_v, host_t = torch.from_numpy(v), torch.from_numpy(t)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.mesh_topology(host_v, host_t)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.mesh_topology(v, t)
    grid = ops.MeshGrid(host_v, host_t, torch.zeros(2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), (0.0, 0.0, 0.0, 1.0), (1, 1, 1))
    topo = ops.MeshTopology(host_v, host_t)
    with pytest.raises(ValueError, match="MeshGrid"):
        ops.signed_distance_to_mesh(host_v, None, topo)
    with pytest.raises(ValueError, match="MeshTopology"):
        ops.signed_distance_to_mesh(host_v, grid, None)
    with pytest.raises(ValueError, match="without normals"):
        ops.signed_distance_to_mesh(host_v, grid, topo)
    topo.face_normal = topo.edge_normal = topo.vertex_normal = torch.zeros(1, 3, dtype=torch.float64)
    for other in (ops.MeshGrid(host_v[:7], host_t, None, None, (0.0, 0.0, 0.0, 1.0), (1, 1, 1)),
                  ops.MeshGrid(host_v, host_t[:11], None, None, (0.0, 0.0, 0.0, 1.0), (1, 1, 1))):
        with pytest.raises(ValueError, match="another mesh"):
            ops.signed_distance_to_mesh(host_v, other, topo)
    with pytest.raises(ValueError, match="no CPU path"):                      # ... and then what closest_point_on_mesh refuses
        ops.signed_distance_to_mesh(host_v, grid, topo)
    # mesh_distance's keyword
    assert "signed" in ops.MESH_DISTANCE_KEYS and ops.mesh_distance_request("t", signed=True) == (None, 1_000_000, float("inf"))
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="signed"):
            ops.mesh_distance_request("t", signed=bad)
        with pytest.raises(ValueError, match="signed"):
            gio.compare_meshes(v, t, v, t, signed=bad)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.mesh_distance(host_v, host_t, host_v, host_t, signed=True)
    # extract_geometry's options: None and False are off, True asks, anything else is refused
    surf = types.SimpleNamespace(mesh_topology=None, mesh_simplify_error=None)
    req = lambda x: ImplicitSurface._topology_request(surf, x)  # noqa: E731
    assert ImplicitSurface.mesh_topology is None and ImplicitSurface.last_mesh_topology is None
    assert req(None) is False and req(False) is False and req(True) is True
    surf.mesh_topology = True
    assert req(None) is True and req(False) is False
    for bad in (1, 0, "yes", {}, 2.5):
        with pytest.raises(ValueError, match="topology"):
            req(bad)
    assert ImplicitSurface._simplify_error_request(surf, {"signed": True, "samples": 100}, 2.0) == {"signed": True, "samples": 100}
    with pytest.raises(ValueError, match="signed"):
        ImplicitSurface._simplify_error_request(surf, {"signed": 1}, 2.0)
    # the host entry points
    with pytest.raises(ValueError, match="expected"):
        gio.mesh_report(v[:, :2], t)
    with pytest.raises(ValueError, match="expected"):
        gio.mesh_report(v, t.reshape(-1))
    with pytest.raises(ValueError, match="whole numbers"):
        gio.mesh_report(v, t.astype(np.float64))
    with pytest.raises(ValueError, match="int32"):
        gio.mesh_report(v, t.astype(np.int64) + 2 ** 31)
    path = str(tmp_path / "a.ply")
    gio.write_ply(path, v, t)
    assert cli.main([str(tmp_path / "missing.ply")]) == 2 and cli.main([str(tmp_path)]) == 2
    assert compare_cli.main([path, str(tmp_path / "missing.ply"), "--signed"]) == 2


def test_extract_geometry_refuses_a_bad_topology_option_before_any_launch():
    from gens_amd.config import gens_model_conf
    from gens_amd.models.modules.implicit_surface import ImplicitSurface
    surf = ImplicitSurface(gens_model_conf(volume_dims=(16, 8, 4))["implicit_surface"])
    lo, hi = torch.full((3,), -1.0), torch.full((3,), 1.0)
    for bad in (1, "yes", {"normals": True}):
        with pytest.raises(ValueError, match="topology"):
            surf.extract_geometry([], lo, hi, 8, 0.0, topology=bad)
        with pytest.raises(ValueError, match="topology"):
            surf.validate(*[None] * 11, lo, hi, (4, 4), mesh_topology=bad)
    with pytest.raises(ValueError, match="signed"):
        surf.extract_geometry([], lo, hi, 8, 0.0, simplify=2, simplify_error={"signed": "yes"})
    assert surf.last_mesh_topology is None
