"""K40 without a GPU: the numpy reference of tests/winding_reference.py on answers known by hand, its far-field traversal against its own
bound, and every refusal of the two entry points (through ctypes) and of the Python layers, all of which come before any launch."""
import ctypes as C
import math

import numpy as np
import pytest

from . import mesh_smooth_reference as SM
from . import mesh_topology_reference as TR
from . import winding_reference as WR


def _w(mesh, q):
    return np.asarray(WR.exact(mesh[0], mesh[1], np.asarray(q, dtype=np.float64).reshape(-1, 3))[0], dtype=np.float64)


def test_reference_on_hand_known_answers():
    cube = TR.cube()
    centre, outside = [0.5, 0.5, 0.5], [[1.7, 0.4, 0.3], [-3.0, -2.0, 5.0], [0.5, 0.5, 1.001]]
    assert abs(_w(cube, centre)[0] - 1.0) < 1e-15
    assert np.abs(_w(cube, outside)).max() < 1e-15
    assert abs(_w(TR.reversed_faces(cube), centre)[0] + 1.0) < 1e-15
    doubled = (cube[0], np.concatenate([cube[1], cube[1]]))
    assert abs(_w(doubled, centre)[0] - 2.0) < 1e-15
    for face in range(6):                                                   # the cube without one face: five sixths by symmetry
        open_cube = (cube[0], np.delete(cube[1], [2 * face, 2 * face + 1], axis=0))
        assert abs(_w(open_cube, centre)[0] - 5.0 / 6.0) < 1e-15
    # one triangle seen from directly above its centroid: a face of the regular tetrahedron from the tetrahedron's centre subtends pi (a
    # quarter of the sphere), the triangle (e_x, e_y, e_z) from the origin pi / 2 (an octant)
    s = 1.0
    tri = np.array([[0, 0, 0], [s, 0, 0], [0.5 * s, 0.5 * math.sqrt(3.0) * s, 0]])
    above = tri.mean(axis=0) + np.array([0, 0, s * math.sqrt(6.0) / 12.0])
    assert abs(_w((tri, np.array([[0, 1, 2]])), above)[0] * 4.0 * math.pi + math.pi) < 1e-15        # seen from the side the normal points to: negative
    assert abs(_w((tri, np.array([[0, 2, 1]])), above)[0] * 4.0 * math.pi - math.pi) < 1e-15
    octant = (np.eye(3), np.array([[0, 1, 2]]))
    assert abs(_w(octant, [0.0, 0.0, 0.0])[0] * 4.0 * math.pi - 0.5 * math.pi) < 1e-15
    # a face that is not valid adds nothing
    v, t = cube
    odd = (v, np.concatenate([t, [[0, 0, 1], [0, 1, 99], [-1, 2, 3], [5, 5, 5]]]).astype(np.int32))
    q = np.array([centre] + outside)
    omega = WR.omegas(*odd, q)[0]
    assert np.array_equal(omega[:, :12], WR.omegas(*cube, q)[0]) and (omega[:, 12:] == 0.0).all()
    assert np.abs(np.asarray(WR.exact(*odd, q)[0] - WR.exact(*cube, q)[0], dtype=np.float64)).max() < 1e-17
    assert np.isnan(_w(cube, [0.5, float("nan"), 0.5])[0]) and np.isnan(_w(cube, [float("inf"), 0.5, 0.5])[0])
    # the bracket: numpy's own float64 sum (the topology tests' truth) sits far inside it
    ico = SM.icosphere(2)
    qs = next(WR.query_stream(ico[0], 3))
    w, tol = WR.exact(*ico, qs)
    assert np.abs(TR.winding_number(*ico, qs) - np.asarray(w, dtype=np.float64)).max() < 1e-2 * np.median(tol)


def test_moments_of_a_leaf_by_hand():
    v, t = TR.cube()
    m = WR.moments(v, t, np.arange(12))
    assert m["leaf_count"].tolist() == [12] and m["node_count"].tolist() == [12]
    assert abs(m["leaf_area"][0] - 6.0) < 1e-14 and np.abs(m["leaf_normal"][0]).max() < 1e-15
    assert np.abs(m["leaf_centre"][0] - 0.5).max() < 1e-15 and abs(m["leaf_radius2"][0] - 0.75) < 1e-15
    assert abs(m["node_radius2"][0] - 0.75) < 1e-14 and abs(m["node_true_radius"][0] - math.sqrt(0.75)) < 1e-15
    none = WR.moments(v, np.array([[0, 0, 1]]), np.arange(1))
    assert none["leaf_count"].tolist() == [0] and none["node_count"].tolist() == [0]
    flat = WR.moments(np.array([[0.0, 0, 0], [1, 0, 0], [2, 0, 0]]), np.array([[0, 1, 2]]), np.arange(1))     # no area: the mean of the centroids
    assert flat["leaf_area"][0] == 0.0 and np.allclose(flat["leaf_centre"][0], [1, 0, 0]) and abs(flat["leaf_radius2"][0] - 1.0) < 1e-15


def test_traversal_reference_obeys_its_bound_and_degenerates_to_the_exact_sum():
    v, t = WR.without_cap(SM.icosphere(3))
    assert 64 < len(t) < 1280
    order = WR.morton_order(v, t)
    assert sorted(order.tolist()) == list(range(len(t)))
    m = WR.moments(v, t, order)
    q, omega, tol = WR.queries_with_bracket(v, t, 300, 11)
    w = omega.sum(axis=1) / WR.FOUR_PI
    fast = WR.traverse(omega, order, m, q, 2.0)
    assert (fast["far"] > 0).mean() > 0.5 and fast["bound"].max() > 0.0
    assert (np.abs(np.asarray(fast["w"] - w, dtype=np.float64)) <= fast["bound"] + tol).all()
    assert np.abs(np.asarray(fast["w"] - w, dtype=np.float64)).max() > 1e-6          # (the far field is really another sum)
    for beta in (1e9, 0.0):
        same = WR.traverse(omega, order, m, q, beta)
        assert (same["far"] == 0).all() and (same["bound"] == 0.0).all()
        assert np.abs(np.asarray(same["w"] - w, dtype=np.float64)).max() < 1e-17 * len(t)
    assert WR.inside([0.9, 0.1, 0.52, 0.5, float("nan")], [0.05, 0.05, 0.05, 0.0, 0.0]).tolist() == [1, 0, -1, 1, -1]


def _plan_args(n_faces=100, null=False, **over):
    from gens_amd import lib as L
    a = L.WindingPlanArgs()
    for name, typ in a._fields_:
        if typ is C.c_void_p:
            setattr(a, name, None if null else 0x7E0000000000)
    a.n_vertices, a.n_faces = 50, n_faces
    a.n_leaves = -(-n_faces // 64)
    a.n_nodes = -(-a.n_leaves // 64)
    for k, val in over.items():
        setattr(a, k, val)
    return a


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from gens_amd import lib as L
    lib = L.load()
    fake = C.c_void_p(0x7E0000100000)
    other = C.c_void_p(0x7E0000200000)

    def number(plan, queries=fake, n=10, beta=0.0, w=other, bound=None):
        return lib.gens_mesh_winding_number(None if plan is None else C.byref(plan), queries, n, beta, w, bound, None)

    def refused(rc, word):
        assert rc in (-1, -2), rc
        assert word.encode() in lib.gens_last_error(), lib.gens_last_error()
    refused(lib.gens_mesh_winding_moments(None, None), "null plan")
    refused(number(None), "null plan")
    for bad in (dict(n_faces=-1), dict(n_vertices=-1), dict(n_leaves=-1), dict(n_nodes=-1)):
        refused(lib.gens_mesh_winding_moments(C.byref(_plan_args(**bad)), None), "faces")
        refused(number(_plan_args(**bad)), "faces")
    for bad in (dict(n_leaves=1), dict(n_leaves=3), dict(n_nodes=2), dict(n_nodes=0)):
        refused(lib.gens_mesh_winding_moments(C.byref(_plan_args(**bad)), None), "64 faces a leaf")
        refused(number(_plan_args(**bad)), "64 faces a leaf")
    big = 2 ** 31
    assert lib.gens_mesh_winding_moments(C.byref(_plan_args(n_faces=big)), None) == -2
    assert number(_plan_args(n_vertices=big)) == -2
    refused(lib.gens_mesh_winding_moments(C.byref(_plan_args(null=True)), None), "null pointer")
    refused(lib.gens_mesh_winding_moments(C.byref(_plan_args(face_order=None)), None), "null pointer")
    refused(number(_plan_args(null=True)), "null pointer")
    refused(number(_plan_args(leaf_radius2=None)), "null pointer")
    refused(number(_plan_args(), n=-1), "queries")
    assert number(_plan_args(), n=big) == -2
    for beta in (1.0, 0.5, 1e-300, -2.0, float("nan"), float("inf"), -0.5):
        refused(number(_plan_args(), beta=beta), "beta")
    refused(number(_plan_args(), queries=None), "null pointer")
    refused(number(_plan_args(), w=None), "null pointer")
    refused(number(_plan_args(), w=fake), "share a buffer")
    refused(number(_plan_args(), bound=other), "share a buffer")
    # nothing to do is no error: no faces (moments), no queries
    assert lib.gens_mesh_winding_moments(C.byref(_plan_args(n_faces=0, null=True)), None) == 0
    assert number(_plan_args(), n=0, queries=None, w=None) == 0 and number(_plan_args(n_faces=0, null=True), n=0) == 0


def test_python_layers_refuse_before_any_launch(tmp_path):
    import torch
    from gens_amd import compare_meshes as cli, io as gio, ops
    v, t = TR.cube()
    hv, ht = torch.from_numpy(v), torch.from_numpy(t)
    for args in ((hv, ht), (v, t), (None, None)):
        with pytest.raises(ValueError, match="not a tensor on the device"):
            ops.build_winding_plan(*args)
    for who in (ops.winding_number, ops.mesh_inside):
        with pytest.raises(ValueError, match="WindingPlan"):
            who(hv, None)
        with pytest.raises(ValueError, match="WindingPlan"):
            who(hv, object(), beta=2.0)
    assert ops.winding_beta("t", None) == 0.0 and ops.winding_beta("t", 2) == 2.0 and ops.winding_beta("t", 1.5) == 1.5
    for bad in (1, 1.0, 0.0, 0.5, -3.0, float("nan"), float("inf"), True, "2", [2.0]):
        with pytest.raises(ValueError, match="beta"):
            ops.winding_beta("t", bad)
    # the sign keywords of mesh_distance, in a function of their own; mesh_distance_request keeps its three-tuple
    assert {"sign", "beta"} <= set(ops.MESH_DISTANCE_KEYS)
    assert ops.mesh_distance_request("t", signed=True) == (None, 1_000_000, float("inf"))
    assert ops.mesh_sign_request("t") == ("pseudonormal", None) and ops.mesh_sign_request("t", True) == ("pseudonormal", None)
    assert ops.mesh_sign_request("t", True, "winding") == ("winding", ops.MESH_DISTANCE_BETA)
    assert ops.mesh_sign_request("t", True, "winding", 3) == ("winding", 3.0) and ops.MESH_DISTANCE_BETA > 1.0
    for kw, word in ((dict(sign="normal"), "sign"), (dict(sign=None), "sign"), (dict(signed=True, sign=1), "sign"),
                     (dict(sign="winding"), "signed=True"), (dict(signed=False, sign="winding"), "signed=True"),
                     (dict(signed=True, beta=2.0), "beta"), (dict(beta=2.0), "beta"), (dict(signed=True, sign="winding", beta=1.0), "beta"),
                     (dict(signed=True, sign="winding", beta=float("nan")), "beta"), (dict(signed=True, sign="winding", beta=True), "beta")):
        with pytest.raises(ValueError, match=word):
            ops.mesh_sign_request("t", **kw)
        with pytest.raises(ValueError, match=word):
            ops.mesh_distance_keywords("t", kw)
        with pytest.raises(ValueError, match=word):
            gio.compare_meshes(v, t, v, t, **kw)
        with pytest.raises(ValueError):
            ops.mesh_distance(hv, ht, hv, ht, **kw)
    with pytest.raises(ValueError, match="unknown keyword"):
        gio.compare_meshes(v, t, v, t, winding=True)
    # signed_distance_to_mesh: the sign's name, and what goes with which
    for kw, word in ((dict(sign="exact"), "sign"), (dict(winding=object()), "go with"), (dict(beta=2.0), "go with"),
                     (dict(sign="winding"), "MeshGrid")):
        with pytest.raises(ValueError, match=word):
            ops.signed_distance_to_mesh(hv, None, None, **kw)
    # the command line: --sign without --signed, --beta without --sign winding
    a = str(tmp_path / "a.ply")
    gio.write_ply(a, v, t)
    for argv in ([a, a, "--sign", "winding"], [a, a, "--sign", "pseudonormal"], [a, a, "--signed", "--beta", "2"],
                 [a, a, "--signed", "--sign", "pseudonormal", "--beta", "2"], [a, a, "--signed", "--sign", "both"]):
        with pytest.raises(SystemExit) as stop:
            cli.main(argv)
        assert stop.value.code == 2
    assert cli.main([a, a, "--signed", "--sign", "winding", "--beta", "0.5", "--device", "cpu"]) == 2        # a bad beta: refused on the host
