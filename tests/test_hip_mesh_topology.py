"""GPU tests of the mesh topology (K37): every integer output, flag byte and count of ops.mesh_topology equals the numpy restatement
(tests/mesh_topology_reference.py) exactly, the pseudonormals to a derived bound, the sign of every query exactly; segment walks across
wave and launch boundaries; ops.mesh_distance(signed=True); extract_geometry(topology=) and simplify_error={"signed": True} on the g23 model;
nothing changes when the options are unset."""
import functools
import json

import numpy as np
import pytest
import torch

from . import mesh_distance_reference as DR
from . import mesh_topology_reference as TR

gpu = pytest.mark.gpu
K37 = {"gens_mesh_edge_keys", "gens_mesh_edge_classify", "gens_mesh_fan_pairs", "gens_mesh_vertex_classify", "gens_mesh_pseudonormals",
       "gens_mesh_distance_sign"}
INTEGER_FIELDS = ("edges", "edge_count", "edge_forward", "edge_halfedges", "edge_class", "edge_of_halfedge", "face_valid", "valence", "fans",
                  "vertex_flags", "corner_label", "face_component")
SIGN_SEED = 5                        # tests/test_mesh_topology_cpu.py's: the precondition of the sign tests holds there
SIGNED_KEYS = {"signed_mean", "inside", "no_sign"}
DIRECTION_KEYS = {"n", "unmatched", "mean", "rms", "max", "q50", "q90", "q99"}
TOP_KEYS = {"a_to_b", "b_to_a", "hausdorff", "chamfer", "density_a", "density_b"}


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _up(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


@functools.lru_cache(maxsize=None)
def _shapes():
    out = dict(TR.hand_shapes())
    out["mc_sphere"] = TR.mc_sphere(17)
    for n in (63, 64, 65, 257):
        out[f"bipyramid {n}"] = TR.bipyramid(n)
    for n in (1, 63, 64, 65, 1000):
        out[f"strip {n}"] = TR.strip(n)
    out["book 65"] = TR.book(65)
    return out


SHAPE_NAMES = tuple(TR.hand_shapes()) + ("mc_sphere",) + tuple(f"bipyramid {n}" for n in (63, 64, 65, 257)) + tuple(
    f"strip {n}" for n in (1, 63, 64, 65, 1000)) + ("book 65",)


@functools.lru_cache(maxsize=None)
def _want(name):
    return TR.topology(*_shapes()[name])


def _close(got, want, rel=1e-12):
    return abs(got - want) <= rel * abs(want)


def _check_report(got, want, name):
    assert set(got) == set(want), name
    for k in want:
        if k in ("area", "volume"):
            assert _close(got[k], want[k]), (name, k, got[k], want[k])
        else:
            assert got[k] == want[k] and type(got[k]) is type(want[k]), (name, k, got[k], want[k])


@gpu
@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_the_tables_and_the_report_equal_the_restatement(name):
    from gens_amd import ops
    v, t = _shapes()[name]
    want = _want(name)
    topo = ops.mesh_topology(_up(v, np.float64), _up(t, np.int32), normals=True)
    assert topo.n_edges == len(want["edges"]) and topo.n_vertices == len(v) and topo.n_faces == len(t)
    for field in INTEGER_FIELDS:
        assert _same(getattr(topo, field).cpu().numpy(), want[field]), (name, field)
    _check_report(topo.report(), want["report"], name)
    # the pseudonormals: |delta| <= 1e-12 x the sum of the weights (1 per use for an edge, the corner angles for a vertex); a face normal
    # is one term of weight 1
    assert np.abs(topo.face_normal.cpu().numpy() - want["face_normal"]).max(initial=0.0) <= 1e-12
    for got, ref, weight in ((topo.edge_normal, want["edge_normal"], want["edge_weight"]),
                             (topo.vertex_normal, want["vertex_normal"], want["vertex_weight"])):
        got = got.cpu().numpy()
        assert got.shape == ref.shape and (np.abs(got - ref) <= 1e-12 * weight[:, None]).all(), name
    plain = ops.mesh_topology(_up(v, np.float64), _up(t, np.int32))
    assert not plain.has_normals and plain.vertex_normal is None and plain.report() == topo.report()


@gpu
def test_what_the_walk_shapes_are_there_for():
    for n in (63, 64, 65, 257):
        want = _want(f"bipyramid {n}")
        assert want["valence"][n] == n and want["valence"][n + 1] == n and len(want["edges"]) == 3 * n and want["report"]["watertight"]
    assert _want("book 65")["edge_count"][0] == 65 and _want("book 65")["edge_class"][0] == 4 and _want("book 65")["fans"][0] == 65
    for n in (1, 63, 64, 65, 1000):
        rep = _want(f"strip {n}")["report"]
        assert rep["faces"] == n and rep["edges"] == 2 * n + 1 and rep["oriented"] and rep["boundary_components"] == 1 and rep["euler"] == 1
    assert 256 < len(_want("mc_sphere")["edges"]) and 3 * 1000 > 256 * 11           # more than one workgroup of edges and of half-edges


@gpu
def test_the_same_bits_twice():
    from gens_amd import ops
    v, t = _shapes()["mc_sphere"]
    dv, dt = _up(v, np.float64), _up(t, np.int32)
    a, b = ops.mesh_topology(dv, dt, normals=True), ops.mesh_topology(dv, dt, normals=True)
    for field in INTEGER_FIELDS + ("face_normal", "edge_normal", "vertex_normal"):
        assert torch.equal(getattr(a, field), getattr(b, field)), field


# ------------------------------------------------------------------------------------------------------------------------------------
# the sign
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sign_case(name):
    v, t = _shapes()[name]
    topo = _want(name)
    q, diag = TR.sign_queries(v, t, SIGN_SEED, n=2000)
    near = DR.closest(v, t, q)
    signed, dot = TR.signed_distance(topo, t, q, near)
    return q, near, signed, dot, diag


@gpu
@pytest.mark.parametrize("name", TR.WATERTIGHT + ("mc_sphere", "cube_open"))
def test_the_sign_of_every_query_equals_the_restatements(name):
    from gens_amd import lib as L, ops
    v, t = _shapes()[name]
    q, near, want, dot, diag = _sign_case(name)
    if name != "cube_open":
        assert TR.precondition(q, near, dot, TR.sign_normals(_want(name), t, near)[0], diag) and not np.isnan(want).any()
    else:
        assert np.isnan(want).sum() > 20 and (~np.isnan(want)).sum() > 500
    dv, dt, dq = _up(v, np.float64), _up(t, np.int32), _up(q, np.float64)
    grid, topo = ops.build_mesh_grid(dv, dt), ops.mesh_topology(dv, dt, normals=True)
    L.profile_begin(only=K37 | {"gens_mesh_closest_point"})
    signed, face = ops.signed_distance_to_mesh(dq, grid, topo)
    assert [k for k, *_ in L.profile_end(raw=True)] == ["gens_mesh_closest_point", "gens_mesh_distance_sign"]
    dist, face2, point, region = ops.closest_point_on_mesh(dq, grid, points=True, regions=True)
    assert _same(face.cpu().numpy(), near["face"]) and torch.equal(face, face2) and _same(region.cpu().numpy(), near["region"])
    got = signed.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want))                         # the NaN cases coincide
    assert np.array_equal(np.sign(got), np.sign(want), equal_nan=True)           # every sign, none left out
    assert torch.equal(signed.abs()[~signed.isnan()], dist[~signed.isnan()])     # |signed| is K36's distance, bit for bit
    for chunk in (64, 1000):
        again, again_face = ops.signed_distance_to_mesh(dq, grid, topo, chunk=chunk)
        assert _same(again.cpu().numpy(), got) and torch.equal(again_face, face), chunk


@gpu
def test_zero_on_the_mesh_nan_beyond_the_cap_and_empty_inputs():
    from gens_amd import ops
    v, t = _shapes()["cube"]
    dv, dt = _up(v, np.float64), _up(t, np.int32)
    grid, topo = ops.build_mesh_grid(dv, dt), ops.mesh_topology(dv, dt, normals=True)
    q = _up(np.array([[0.5, 0.25, 0.0], [0.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, 0.5, 1.25], [9.0, 9.0, 9.0], [np.nan, 0.0, 0.0]]), np.float64)
    signed, face = ops.signed_distance_to_mesh(q, grid, topo, max_dist=2.0)
    got = signed.cpu().numpy()
    assert got[0] == 0.0 and got[1] == 0.0 and not np.signbit(got[:2]).any() and got[2] == -0.5 and got[3] == 0.25
    assert np.isnan(got[4]) and np.isnan(got[5]) and face.cpu().tolist()[4:] == [-1, -1]
    none, none_face = ops.signed_distance_to_mesh(q[:0], grid, topo)
    assert none.shape == (0,) and none.dtype == torch.float64 and none_face.shape == (0,)
    ev, et = _up(np.zeros((3, 3)), np.float64), _up(np.zeros((0, 3)), np.int32)
    signed, face = ops.signed_distance_to_mesh(q, ops.build_mesh_grid(ev, et), ops.mesh_topology(ev, et, normals=True))
    assert signed.isnan().all() and (face == -1).all()
    with pytest.raises(ValueError, match="without normals"):
        ops.signed_distance_to_mesh(q, grid, ops.mesh_topology(dv, dt))
    with pytest.raises(ValueError, match="another mesh"):
        ops.signed_distance_to_mesh(q, grid, ops.mesh_topology(dv, dt[:10].contiguous(), normals=True))


# ------------------------------------------------------------------------------------------------------------------------------------
# mesh_distance(signed=True)
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_mesh_distance_says_which_side_the_other_mesh_lies_on():
    from gens_amd import lib as L, ops
    v, t = _shapes()["mc_sphere"]
    outward = _want("mc_sphere")["report"]["volume"] > 0
    centre = 0.5 * (v.min(axis=0) + v.max(axis=0))
    dv, dt = _up(v, np.float64), _up(t, np.int32)
    means = {}
    for scale in (1.05, 0.95):
        other = _up(centre + scale * (v - centre), np.float64)
        plain = ops.mesh_distance(dv, dt, other, dt, samples=3000)
        out = ops.mesh_distance(dv, dt, other, dt, samples=3000, signed=True, return_samples=True)
        assert set(plain) == TOP_KEYS and set(plain["a_to_b"]) == set(plain["b_to_a"]) == DIRECTION_KEYS
        assert set(out) == TOP_KEYS | {f"{k}_{s}" for k in ("samples", "dist", "face", "signed") for s in "ab"}
        for side in ("a_to_b", "b_to_a"):
            assert set(out[side]) == DIRECTION_KEYS | SIGNED_KEYS and {k: out[side][k] for k in DIRECTION_KEYS} == plain[side]
            assert out[side]["no_sign"] == 0 and out[side]["unmatched"] == 0 and type(out[side]["inside"]) is int
        # A inside the larger copy and around the smaller one; "inside" follows the other mesh's orientation
        a_inside_b, b_inside_a = scale > 1.0, scale < 1.0
        for side, is_inside, s in (("a_to_b", a_inside_b, "a"), ("b_to_a", b_inside_a, "b")):
            negative = is_inside == outward
            assert out[side]["inside"] == (out[side]["n"] if negative else 0), (scale, side)
            assert (out[side]["signed_mean"] < 0) == negative and abs(abs(out[side]["signed_mean"]) - out[side]["mean"]) <= 1e-12 * out[side]["mean"]
            assert torch.equal(out["signed_" + s].abs(), out["dist_" + s])
        means[scale] = out["a_to_b"]["signed_mean"]
    assert means[1.05] * means[0.95] < 0
    L.profile_begin(only=K37)
    ops.mesh_distance(dv, dt, dv, dt, samples=500)
    ops.mesh_distance(dv, dt, dv, dt, samples=500, signed=False)
    assert not L.profile_end(raw=True)                                           # off: not one more launch


@gpu
def test_io_mesh_report_and_the_command_lines(tmp_path, capsys):
    from gens_amd import compare_meshes as compare_cli, io as gio, mesh_report as cli
    v, t = _shapes()["torus"]
    got = gio.mesh_report(v, t.astype(np.int64))
    _check_report(got, _want("torus")["report"], "torus")
    _check_report(gio.mesh_report(torch.from_numpy(v), torch.from_numpy(t)), _want("torus")["report"], "torus")
    odd_v, odd_t = _shapes()["odd_faces"]
    _check_report(gio.mesh_report(odd_v, odd_t), _want("odd_faces")["report"], "odd_faces")      # any indices are accepted
    path = str(tmp_path / "torus.ply")
    gio.write_ply(path, v, t)
    assert cli.main([path]) == 0
    line = capsys.readouterr().out.strip()
    assert "\n" not in line
    fv, ft = gio.read_ply(path)                                                  # the file holds float32 vertices
    assert json.loads(line) == gio.mesh_report(fv, ft) and json.loads(line)["genus"] == 1
    assert compare_cli.main([path, path, "--samples", "500", "--signed"]) == 0
    lines = capsys.readouterr().out.strip().split("\n")
    assert len(lines) == 3 and "signed_mean" in lines[0] and "no_sign" in lines[1]
    signed = gio.compare_meshes(v, t, v, t, samples=500, signed=True)
    assert set(signed["a_to_b"]) == DIRECTION_KEYS | SIGNED_KEYS and set(gio.compare_meshes(v, t, v, t, samples=500)["a_to_b"]) == DIRECTION_KEYS


# ------------------------------------------------------------------------------------------------------------------------------------
# the model: the g23 surface of tests/test_hip_mesh_simplify.py, R = 64
# ------------------------------------------------------------------------------------------------------------------------------------
R = 64
COUNTS = ("vertices", "vertices_referenced", "faces", "faces_invalid", "edges", "edges_boundary", "edges_manifold", "edges_flipped",
          "edges_nonmanifold", "vertices_pinched", "vertices_nonmanifold", "components", "largest_component_faces", "boundary_components", "euler",
          "closed", "oriented", "manifold", "watertight", "genus")


@gpu
def test_extract_geometry_reports_the_topology_on_request():
    from gens_amd import io as gio, lib as L
    from .test_hip_mesh_simplify import ROUTES, _model, _world
    from .test_hip_vertex_attrs import _validate_args
    m = _model()
    surf, vols, lo, hi = m["surf"], m["vols"], m["lo"], m["hi"]
    full_report, simple_report = gio.mesh_report(*m["full"]), gio.mesh_report(*m["simple"][:2])
    v, t = surf.extract_geometry(vols, lo, hi, R, 0.0, topology=True)
    assert _same(v, _world(m["full"][0], lo, hi)) and _same(t, m["full"][1])     # the mesh is what it was without the report
    rep = surf.last_mesh_topology
    print(f"g23 R = {R}: {json.dumps(rep)}")
    assert rep == full_report and rep["edges_nonmanifold"] == 0 and rep["oriented"] and rep["faces"] == len(t) and rep["faces_invalid"] == 0
    assert surf.last_simplify_stats is None
    # with the simplification: before and after, the latter of the mesh the call returns
    surf.lattice_lipschitz = m["lipschitz"]
    try:
        for route, kw in ROUTES:
            L.profile_begin(only=K37)
            v, t = surf.extract_geometry(vols, lo, hi, R, 0.0, simplify=2, topology=True, **kw)
            assert {k for k, *_ in L.profile_end(raw=True)} == K37 - {"gens_mesh_pseudonormals", "gens_mesh_distance_sign"}, route
            assert _same(v, _world(m["simple"][0], lo, hi)) and _same(t, m["simple"][1]), route
            assert surf.last_simplify_stats["topology_before"] == full_report and surf.last_mesh_topology == simple_report, route
            assert {k: x for k, x in surf.last_simplify_stats.items() if k != "topology_before"} == m["simple"][3], route
    finally:
        surf.lattice_lipschitz = 2.0
    returned = gio.mesh_report(v, t)                                             # world coordinates: the counts are the same, the sizes are not
    assert {k: returned[k] for k in COUNTS} == {k: surf.last_mesh_topology[k] for k in COUNTS}
    print(f"g23 R = {R}, cell 2: {json.dumps(surf.last_mesh_topology)}")
    # the attribute and validate
    surf.mesh_topology = True
    try:
        surf.extract_geometry(vols, lo, hi, R, 0.0, simplify=2)
        assert surf.last_mesh_topology == simple_report
        surf.extract_geometry(vols, lo, hi, R, 0.0, simplify=2, topology=False)
        assert surf.last_mesh_topology is None and "topology_before" not in surf.last_simplify_stats
    finally:
        del surf.mesh_topology
    torch.manual_seed(3)
    out = surf.validate(*_validate_args(surf, vols), extract_geometry=True, mesh_resolution=R, mesh_simplify=2, mesh_topology=True)
    assert _same(out["vertices"], v) and surf.last_mesh_topology == simple_report


@gpu
def test_simplify_error_takes_the_sign_on_request():
    from gens_amd import ops
    from .test_hip_mesh_simplify import _model
    m = _model()
    surf, vols, lo, hi = m["surf"], m["vols"], m["lo"], m["hi"]
    full = [_up(m["full"][0], np.float64), _up(m["full"][1], np.int32)]
    simple = [_up(m["simple"][0], np.float64), _up(m["simple"][1], np.int32)]
    surf.extract_geometry(vols, lo, hi, R, 0.0, simplify=2, simplify_error={"signed": True, "samples": 5000})
    err = surf.last_simplify_stats["error"]
    print(f"g23 R = {R}, cell 2: {json.dumps(err)}")
    assert err == ops.mesh_distance(*full, *simple, samples=5000, signed=True)
    for side in ("a_to_b", "b_to_a"):
        assert SIGNED_KEYS <= set(err[side]) and 0 <= err[side]["inside"] <= err[side]["n"] and 0 <= err[side]["no_sign"] <= err[side]["n"]
    surf.extract_geometry(vols, lo, hi, R, 0.0, simplify=2, simplify_error={"samples": 5000})
    assert not SIGNED_KEYS & set(surf.last_simplify_stats["error"]["a_to_b"])
    assert surf.last_simplify_stats["error"] == {k: ({j: y for j, y in x.items() if j not in SIGNED_KEYS} if isinstance(x, dict) else x)
                                                 for k, x in err.items()}


@gpu
def test_nothing_changes_when_the_options_are_unset():
    from gens_amd import lib as L
    from gens_amd.config import Conf, gens_model_conf
    from gens_amd.models.gens import GenS
    from gens_amd.models.modules.implicit_surface import ImplicitSurface
    from .test_hip_mesh_simplify import _model, _world
    from .test_hip_vertex_attrs import TODAYS_KEYS, _validate_args
    assert ImplicitSurface.mesh_topology is None and ImplicitSurface.last_mesh_topology is None
    m = _model()
    surf, vols, lo, hi = m["surf"], m["vols"], m["lo"], m["hi"]
    assert "mesh_topology" not in vars(surf)
    L.profile_begin(only=K37)
    for off in ({}, {"topology": None}, {"topology": False}):
        got = surf.extract_geometry(vols, lo, hi, R, 0.0, simplify=2, simplify_error=True, **off)
        assert len(got) == 2 and _same(got[0], _world(m["simple"][0], lo, hi)) and _same(got[1], m["simple"][1]), off
        assert set(surf.last_simplify_stats) == set(m["simple"][3]) | {"error"} and surf.last_mesh_topology is None
        assert set(surf.last_simplify_stats["error"]) == TOP_KEYS and set(surf.last_simplify_stats["error"]["a_to_b"]) == DIRECTION_KEYS
        plain = surf.extract_geometry(vols, lo, hi, R, 0.0, **off)
        assert _same(plain[0], _world(m["full"][0], lo, hi)) and _same(plain[1], m["full"][1])
        assert surf.last_simplify_stats is None and surf.last_mesh_topology is None
    args = _validate_args(surf, vols)
    torch.manual_seed(3)
    ref = surf.validate(*args, extract_geometry=True, mesh_resolution=33, mesh_simplify=2)
    torch.manual_seed(3)
    off = surf.validate(*args, extract_geometry=True, mesh_resolution=33, mesh_simplify=2, mesh_topology=False)
    assert not L.profile_end(raw=True)
    assert set(ref) == set(off) == TODAYS_KEYS
    for k in TODAYS_KEYS:
        assert torch.equal(torch.as_tensor(off[k]), torch.as_tensor(ref[k])), k
    conf = gens_model_conf(volume_dims=(16, 8, 4), has_vol=True)
    assert "mesh_topology" not in vars(GenS(conf).implicit_surface)
    assert GenS(Conf({**conf, "mesh_topology": True})).implicit_surface.mesh_topology is True


@gpu
def test_refusals_come_before_any_launch():
    from gens_amd import lib as L, ops
    from .test_hip_mesh_simplify import K33, _model
    from .test_hip_vertex_attrs import NETWORK, _validate_args
    m = _model()
    surf, vols, lo, hi = m["surf"], m["vols"], m["lo"], m["hi"]
    v, t = _shapes()["cube"]
    dv, dt = _up(v, np.float64), _up(t, np.int32)
    L.profile_begin(only=K37 | K33 | NETWORK | {"gens_mesh_closest_point", "gens_mesh_grid_count", "gens_mc_classify", "gens_lattice_points"})
    for bad in (1, "yes", {"normals": True}, 2.0):
        with pytest.raises(ValueError, match="topology"):
            surf.extract_geometry(vols, lo, hi, 33, 0.0, topology=bad)
        with pytest.raises(ValueError, match="topology"):
            surf.validate(*_validate_args(surf, vols), extract_geometry=True, mesh_resolution=33, mesh_topology=bad)
    with pytest.raises(ValueError, match="signed"):
        surf.extract_geometry(vols, lo, hi, 33, 0.0, simplify=2, simplify_error={"signed": 1})
    for bad_v, bad_t in ((dv.float(), dt), (dv, dt.long()), (dv[:, :2], dt), (dv, dt.reshape(-1)), (dv.cpu(), dt)):
        with pytest.raises(ValueError):
            ops.mesh_topology(bad_v, bad_t)
    with pytest.raises(ValueError, match="normals"):
        ops.mesh_topology(dv, dt, normals=1)
    with pytest.raises(ValueError, match="signed"):
        ops.mesh_distance(dv, dt, dv, dt, signed="yes")
    assert not L.profile_end(raw=True)
