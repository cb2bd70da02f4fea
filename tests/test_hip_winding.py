"""GPU tests of the generalised winding number (K40): exact mode against the longdouble sum of tests/winding_reference.py inside the
rounding bracket the reference derives; the plan's moments against the restatement; the far field against the traversal reference fed the
plan's own arrays, against the exact sum within the bound the kernel reports, and not vacuously; the same bits alone, in a batch, reversed,
chunked and twice; mesh_inside never guessing; the sign it gives K36's distance, mesh_distance(sign="winding"), the model option and the
command line.  Every comparison's tolerance is decided by the reference alone."""
import functools
import json

import numpy as np
import pytest
import torch

from . import mesh_repair_reference as RR
from . import mesh_smooth_reference as SM
from . import mesh_topology_reference as TR
from . import winding_reference as WR

gpu = pytest.mark.gpu
K40 = {"gens_mesh_winding_moments", "gens_mesh_winding_number"}
COUNTS = (1, 63, 64, 65, 257, 1000)
STRIPS = (1, 63, 64, 65, 4095, 4096, 4097, 8193)             # the leaf and node boundaries and a second node
SOUP_SEED = 35                                                # a multiple of 5 and of 7: both kinds of planted invalid faces
QUERY_SEED = 7
MARGIN = 1e-9                                                 # accept tests closer than this to equality may legitimately go either way
SIGNED_KEYS = {"signed_mean", "inside", "no_sign"}
MOMENT_FIELDS = tuple(f"{level}_{name}" for level in ("leaf", "node") for name in ("count", "area", "normal", "centre", "radius2"))


def _up(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def _meshes():
    cube = TR.cube()
    ico = SM.icosphere(3)
    out = {"tetrahedron": TR.tetrahedron(), "cube": cube, "cube reversed": TR.reversed_faces(cube),
           "cube doubled": (cube[0], np.concatenate([cube[1], cube[1]])), "cube open": RR.cube_minus_square(),
           "icosphere": ico, "icosphere open": WR.without_cap(ico), "soup": RR.random_soup(SOUP_SEED)}
    for n in STRIPS:
        out[f"strip {n}"] = WR.planar_strip(n)
    return {k: (np.asarray(v, dtype=np.float64), np.asarray(t, dtype=np.int32)) for k, (v, t) in out.items()}


MESH_NAMES = ("tetrahedron", "cube", "cube reversed", "cube doubled", "cube open", "icosphere", "icosphere open", "soup") + tuple(
    f"strip {n}" for n in STRIPS)
FAR_NAMES = ("strip 4097", "strip 8193", "icosphere")        # where the far field must really be taken


@functools.lru_cache(maxsize=None)
def _case(name):
    """The mesh's 1000 queries (every smaller batch is a prefix), their solid angles, brackets and exact winding numbers: computed once."""
    v, t = _meshes()[name]
    q, omega, tol = WR.queries_with_bracket(v, t, max(COUNTS), QUERY_SEED)
    assert tol.max() < 1e-9                                   # the test's own precondition, decided by the reference alone
    return {"q": q, "omega": omega, "tol": tol, "w": omega.sum(axis=1) / WR.FOUR_PI}


@functools.lru_cache(maxsize=None)
def _plan(name):
    from gens_amd import ops
    v, t = _meshes()[name]
    dv, dt = _up(v, np.float64), _up(t, np.int32)
    plan = ops.build_winding_plan(dv, dt)
    back = {k: getattr(plan, k).cpu().numpy() for k in MOMENT_FIELDS + ("face_order", "corners")}
    return {"dv": dv, "dt": dt, "plan": plan, "back": back, "dq": _up(_case(name)["q"], np.float64)}


def _err(got, want):
    return np.abs(np.asarray(got.astype(WR.LD) - want, dtype=np.float64))


@gpu
def test_soup_has_invalid_faces_and_the_strips_are_planar():
    v, t = _meshes()["soup"]
    ok = WR.face_valid(v, t)
    assert 0 < ok.sum() < len(t) and (t < 0).any() and (t >= len(v)).any()
    assert all((_meshes()[f"strip {n}"][0][:, 2] == 0.0).all() and len(_meshes()[f"strip {n}"][1]) == n for n in STRIPS)
    assert 0 < len(_meshes()["icosphere open"][1]) < len(_meshes()["icosphere"][1]) == 1280


@gpu
@pytest.mark.parametrize("name", MESH_NAMES)
def test_exact_mode_equals_the_longdouble_sum_within_the_bracket(name):
    from gens_amd import ops
    case, p = _case(name), _plan(name)
    for n in COUNTS:
        w, bound = ops.winding_number(p["dq"][:n], p["plan"], bound=True)
        assert w.shape == (n,) and w.dtype == torch.float64 and (bound == 0.0).all()
        err = _err(w.cpu().numpy(), case["w"][:n])
        print(f"{name} n = {n}: max |w - exact| {err.max():.3e}, max err / tol {np.max(err / case['tol'][:n]):.3e}")
        assert (err <= case["tol"][:n]).all(), (name, n)
    assert torch.equal(ops.winding_number(p["dq"], p["plan"]), ops.winding_number(p["dq"], p["plan"], bound=True)[0])


@gpu
def test_hand_known_answers_and_queries_that_are_not_finite():
    from gens_amd import lib as L, ops
    centre = [0.5, 0.5, 0.5]
    q = _up(np.array([centre, [1.7, 0.4, 0.3], [np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.0, 0.0, 0.0], [0.5, 0.5, 0.0]]), np.float64)
    for name, inside in (("cube", 1.0), ("cube reversed", -1.0), ("cube doubled", 2.0), ("cube open", 5.0 / 6.0)):
        for beta in (None, 2.0):
            w, bound = (x.cpu().numpy() for x in ops.winding_number(q, _plan(name)["plan"], beta=beta, bound=True))
            assert abs(w[0] - inside) < 1e-14 and np.isnan(w[2:4]).all() and np.isnan(bound[2:4]).all()
            assert abs(w[1]) < 1e-14 or name == "cube open"                                    # (outside an open mesh: a fraction)
            assert np.isfinite(w[4:]).all() and (bound[[0, 1, 4, 5]] == 0.0).all()       # on a vertex, on a face: finite, whatever the formula gives
    # no faces, no queries: nothing is launched
    ev, et = _up(np.zeros((3, 3)), np.float64), _up(np.zeros((0, 3)), np.int32)
    L.profile_begin(only=K40)
    empty = ops.build_winding_plan(ev, et)
    w, bound = ops.winding_number(q, empty, beta=3.0, bound=True)
    none = ops.winding_number(q[:0], _plan("cube")["plan"])
    inside = ops.mesh_inside(q, empty)
    assert not L.profile_end(raw=True)
    assert empty.n_faces == empty.n_leaves == empty.n_nodes == 0 and none.shape == (0,) and none.dtype == torch.float64
    assert w.cpu().tolist()[:2] == [0.0, 0.0] and w.isnan().cpu().tolist() == [False, False, True, True, False, False]
    assert bound.isnan().cpu().tolist() == w.isnan().cpu().tolist() and inside.cpu().tolist() == [0, 0, -1, -1, 0, 0]
    with pytest.raises(ValueError, match="not finite"):
        ops.build_winding_plan(_up(np.array([[0, 0, 0], [1, 0, 0], [0, np.nan, 0], [np.inf, 0, 0]]), np.float64), _up([[0, 1, 2]], np.int32))
    ops.build_winding_plan(_up(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.inf, 0, 0]]), np.float64), _up([[0, 1, 2], [0, 3, 3]], np.int32))


@gpu
@pytest.mark.parametrize("name", MESH_NAMES)
def test_the_plan_and_its_moments_equal_the_restatement(name):
    v, t = _meshes()[name]
    p = _plan(name)
    plan, back = p["plan"], p["back"]
    nt = len(t)
    assert (plan.n_faces, plan.n_leaves, plan.n_nodes) == (nt, -(-nt // 64), -(-(-(-nt // 64)) // 64))
    order = back["face_order"]
    assert order.dtype == np.int32 and sorted(order.tolist()) == list(range(nt))            # a permutation
    ok = WR.face_valid(v, t)
    assert not ok[order[int(ok.sum()):]].any()                                                # faces that are not valid come last
    corners = np.zeros((64 * plan.n_leaves, 9))
    corners[:nt][ok[order]] = v[t[order[ok[order]]]].reshape(-1, 9)
    assert _same(back["corners"], corners)                                                    # leaf k holds positions 64 k ..., zeros elsewhere
    want = WR.moments(v, t, order)
    for level in ("leaf", "node"):
        assert np.array_equal(back[level + "_count"], want[level + "_count"]), level
        area, r2 = want[level + "_area"], want[level + "_radius2"]
        # relative 1e-12: the area to itself, the area vector to the area (the sum of its terms' lengths), the centre to the cluster's
        # extent (the larger of |p| and r)
        assert (np.abs(back[level + "_area"] - area) <= 1e-12 * area).all(), level
        assert (np.abs(back[level + "_normal"] - want[level + "_normal"]).max(axis=1) <= 1e-12 * area).all(), level
        extent = np.maximum(np.linalg.norm(want[level + "_centre"], axis=1), np.sqrt(r2))
        assert (np.abs(back[level + "_centre"] - want[level + "_centre"]).max(axis=1) <= 1e-12 * extent).all(), level
    assert (np.abs(back["leaf_radius2"] - want["leaf_radius2"]) <= 1e-12 * want["leaf_radius2"]).all()
    r = np.sqrt(back["node_radius2"])
    assert (r >= want["node_true_radius"] * (1 - 1e-12)).all() and (r <= np.sqrt(want["node_radius2"]) * (1 + 1e-12)).all()
    empty = want["leaf_count"] == 0
    assert all((back["leaf_" + k][empty] == 0).all() for k in ("area", "normal", "centre", "radius2"))


@functools.lru_cache(maxsize=None)
def _traversal(name, beta):
    case, back = _case(name), _plan(name)["back"]
    return WR.traverse(case["omega"], back["face_order"], back, case["q"], beta)


@gpu
@pytest.mark.parametrize("beta", (2.0, 4.0))
@pytest.mark.parametrize("name", MESH_NAMES)
def test_fast_mode_against_the_traversal_and_the_exact_sum(name, beta):
    from gens_amd import ops
    case, p, ref = _case(name), _plan(name), _traversal(name, beta)
    w, bound = (x.cpu().numpy() for x in ops.winding_number(p["dq"], p["plan"], beta=beta, bound=True))
    keep = ref["margin"] >= MARGIN
    assert (~keep).mean() <= 0.01 and keep.all(), (name, beta, int((~keep).sum()))           # (the seed is one for which the reference shows none)
    err = _err(w, ref["w"])
    print(f"{name} beta = {beta}: far-accepted {ref['far'].mean():.1f} a query, max bound {bound.max():.3e}, max |w - traversal| {err.max():.3e}, "
          f"max |w - exact| {_err(w, case['w']).max():.3e}")
    assert (err[keep] <= case["tol"][keep]).all()                                             # (a)
    assert (np.abs(bound - ref["bound"])[keep] <= 1e-12 * ref["bound"][keep]).all()
    assert (_err(w, case["w"]) <= bound + case["tol"]).all()                                  # (b)
    if name in FAR_NAMES and beta == 2.0:                                                     # (c)
        assert (ref["far"] > 0).mean() > 0.5 and (bound > 0).mean() > 0.5
    if name == "strip 8193" and beta == 2.0:
        assert ref["node_accepts"].sum() > 0 and ref["leaf_accepts"].sum() > 0
    for n in COUNTS[:-1]:
        again = ops.winding_number(p["dq"][:n], p["plan"], beta=beta)
        assert _same(again.cpu().numpy(), w[:n]), n


@gpu
@pytest.mark.parametrize("beta", (None, 2.0))
@pytest.mark.parametrize("name", ("icosphere open", "strip 4097"))
def test_the_same_bits_alone_in_a_batch_reversed_chunked_and_twice(name, beta):
    from gens_amd import ops
    p = _plan(name)
    dq, plan = p["dq"][:257], p["plan"]
    w, bound = ops.winding_number(dq, plan, beta=beta, bound=True)
    for i in (0, 1, 63, 64, 200, 256):
        one, one_bound = ops.winding_number(dq[i:i + 1], plan, beta=beta, bound=True)
        assert torch.equal(one, w[i:i + 1]) and torch.equal(one_bound, bound[i:i + 1]), i
    back, back_bound = ops.winding_number(dq.flip(0).contiguous(), plan, beta=beta, bound=True)
    assert torch.equal(back.flip(0), w) and torch.equal(back_bound.flip(0), bound)
    for chunk in (1, 64, 1000):
        again, again_bound = ops.winding_number(dq, plan, beta=beta, bound=True, chunk=chunk)
        assert torch.equal(again, w) and torch.equal(again_bound, bound), chunk
    twice = ops.winding_number(dq, plan, beta=beta, bound=True)
    assert torch.equal(twice[0], w) and torch.equal(twice[1], bound)
    assert torch.equal(ops.winding_number(p["dq"], plan, beta=beta)[:257], w)


@gpu
@pytest.mark.parametrize("beta", (None, 2.0, 4.0))
@pytest.mark.parametrize("name", ("cube", "cube open", "icosphere", "icosphere open", "soup", "strip 4097"))
def test_mesh_inside_never_guesses(name, beta):
    from gens_amd import ops
    case, p = _case(name), _plan(name)
    got = ops.mesh_inside(p["dq"], p["plan"], beta=beta).cpu().numpy()
    w, bound = (x.cpu().numpy() for x in ops.winding_number(p["dq"], p["plan"], beta=beta, bound=True))
    assert got.dtype == np.int8 and np.array_equal(got, WR.inside(w, bound))
    truth = WR.inside(np.asarray(case["w"], dtype=np.float64), np.zeros(len(w)))
    sure = np.abs(np.asarray(case["w"], dtype=np.float64) - 0.5) > case["tol"]                # (the truth itself is beyond rounding)
    decided = got >= 0
    print(f"{name} beta = {beta}: inside {int((got == 1).sum())}, outside {int((got == 0).sum())}, undecided {int((got < 0).sum())}")
    assert np.array_equal(got[decided & sure], truth[decided & sure])                         # wherever it decides, it is right
    assert (np.abs(w - 0.5)[~decided] <= bound[~decided] + case["tol"][~decided]).all()       # undecided only where the bound straddles a half
    if beta is None:
        assert decided[sure].all()


@gpu
@pytest.mark.parametrize("name", ("tetrahedron", "cube", "icosphere", "cube open"))
def test_signed_distance_with_the_winding_sign(name):
    from gens_amd import lib as L, ops
    p = _plan(name)
    dq, plan = p["dq"], p["plan"]
    grid, topo = ops.build_mesh_grid(p["dv"], p["dt"]), ops.mesh_topology(p["dv"], p["dt"], normals=True)
    dist, face = ops.closest_point_on_mesh(dq, grid)
    pseudo, pseudo_face = ops.signed_distance_to_mesh(dq, grid, topo)
    for beta in (None, 4.0):
        L.profile_begin(only=K40 | {"gens_mesh_closest_point", "gens_mesh_distance_sign"})
        signed, signed_face = ops.signed_distance_to_mesh(dq, grid, sign="winding", winding=plan, beta=beta)
        assert [k for k, *_ in L.profile_end(raw=True)] == ["gens_mesh_closest_point", "gens_mesh_winding_number"]
        has = ~signed.isnan()
        assert torch.equal(signed.abs()[has], dist[has]) and torch.equal(signed_face, face)  # |signed| is K36's distance, bit for bit
        inside = ops.mesh_inside(dq, plan, beta=beta)
        assert torch.equal(has, inside >= 0) and torch.equal(signed[has] < 0, (inside == 1)[has])
        both = has & ~pseudo.isnan()
        if name != "cube open":                                                               # watertight, outward: K37's sign wherever it has one
            assert beta is not None or has.all()
            assert both.sum() > 900 and torch.equal(torch.sign(signed[both]), torch.sign(pseudo[both]))
        elif beta is None:                                                                    # a closest point on the rim: a sign where K37 has none
            assert has.all() and int(pseudo.isnan().sum()) > 20
    # the default route: not one more launch, the same bits
    L.profile_begin(only=K40 | {"gens_mesh_closest_point", "gens_mesh_distance_sign"})
    named, named_face = ops.signed_distance_to_mesh(dq, grid, topo, sign="pseudonormal")
    assert [k for k, *_ in L.profile_end(raw=True)] == ["gens_mesh_closest_point", "gens_mesh_distance_sign"]
    assert _same(named.cpu().numpy(), pseudo.cpu().numpy()) and torch.equal(named_face, pseudo_face)
    on = ops.signed_distance_to_mesh(p["dv"][:3].contiguous(), grid, sign="winding", winding=plan, max_dist=1.0)[0].cpu().numpy()
    assert (on == 0.0).all() and not np.signbit(on).any()                                     # +0 on the mesh
    far = ops.signed_distance_to_mesh(_up([[50.0, 50.0, 50.0]], np.float64), grid, sign="winding", winding=plan, max_dist=1.0)[0]
    assert far.isnan().all()                                                                  # nothing within max_dist
    with pytest.raises(ValueError, match="another mesh"):
        ops.signed_distance_to_mesh(dq, grid, sign="winding", winding=_plan("strip 65")["plan"])
    with pytest.raises(ValueError, match="WindingPlan"):
        ops.signed_distance_to_mesh(dq, grid, topo, sign="winding")


@gpu
def test_mesh_distance_with_the_winding_sign():
    from gens_amd import lib as L, ops
    v, t = _meshes()["icosphere"]
    dv, dt = _up(v, np.float64), _up(t, np.int32)
    for scale in (1.05, 0.95):
        other = _up(scale * v, np.float64)
        plain = ops.mesh_distance(dv, dt, other, dt, samples=3000)
        out = ops.mesh_distance(dv, dt, other, dt, samples=3000, signed=True, sign="winding", return_samples=True)
        for side, is_inside, s in (("a_to_b", scale > 1.0, "a"), ("b_to_a", scale < 1.0, "b")):
            assert SIGNED_KEYS <= set(out[side]) and {k: out[side][k] for k in plain[side]} == plain[side]
            print(f"sphere x {scale} {side}: {json.dumps(out[side])}")
            assert out[side]["no_sign"] == 0 and out[side]["inside"] == (out[side]["n"] if is_inside else 0), (scale, side)   # all or none
            assert (out[side]["signed_mean"] < 0) == is_inside and abs(abs(out[side]["signed_mean"]) - out[side]["mean"]) <= 1e-12 * out[side]["mean"]
            assert torch.equal(out["signed_" + s].abs(), out["dist_" + s])
    # the open icosphere against itself: every sample but the removed cap's vertices (still in the vertex list) is on the mesh up to rounding; +0 where the distance is 0, and a sample a rounding
    # error off the sheet is inside or outside as that error has it (the winding number jumps across the sheet)
    ov, ot = (_up(x, d) for x, d in zip(_meshes()["icosphere open"], (np.float64, np.int32)))
    own = ops.mesh_distance(ov, ot, ov, ot, samples=2000, signed=True, sign="winding", beta=3.0, return_samples=True)
    for side, s in (("a_to_b", "a"), ("b_to_a", "b")):
        d = own["dist_" + s]
        assert own[side]["unmatched"] == 0 and float(d.median()) < 1e-7 and int((d == 0.0).sum()) > 0
        assert (own["signed_" + s][d == 0.0] == 0.0).all() and not torch.signbit(own["signed_" + s][d == 0.0]).any()
        assert own[side]["inside"] + own[side]["no_sign"] <= int((d > 0).sum())
    # off: not one more launch, the same figures
    L.profile_begin(only=K40)
    assert ops.mesh_distance(dv, dt, dv, dt, samples=500, signed=True) == ops.mesh_distance(dv, dt, dv, dt, samples=500, signed=True, sign="pseudonormal")
    assert not L.profile_end(raw=True)


@gpu
def test_the_model_option_and_the_command_line(tmp_path, capsys):
    from gens_amd import compare_meshes as cli, io as gio, ops
    from .test_hip_mesh_simplify import _model
    m = _model()
    surf, vols, lo, hi = m["surf"], m["vols"], m["lo"], m["hi"]
    full = [_up(m["full"][0], np.float64), _up(m["full"][1], np.int32)]
    simple = [_up(m["simple"][0], np.float64), _up(m["simple"][1], np.int32)]
    surf.extract_geometry(vols, lo, hi, 64, 0.0, simplify=2, simplify_error={"signed": True, "sign": "winding", "samples": 5000})
    err = surf.last_simplify_stats["error"]
    print(f"g23 R = 64, cell 2, sign winding: {json.dumps(err)}")
    assert err == ops.mesh_distance(*full, *simple, samples=5000, signed=True, sign="winding")
    pseudo = ops.mesh_distance(*full, *simple, samples=5000, signed=True)
    for side in ("a_to_b", "b_to_a"):
        assert SIGNED_KEYS <= set(err[side]) and 0 <= err[side]["inside"] <= err[side]["n"] and 0 <= err[side]["no_sign"] <= err[side]["n"]
        assert {k: x for k, x in err[side].items() if k not in SIGNED_KEYS} == {k: x for k, x in pseudo[side].items() if k not in SIGNED_KEYS}
    with pytest.raises(ValueError, match="signed=True"):
        surf.extract_geometry(vols, lo, hi, 64, 0.0, simplify=2, simplify_error={"sign": "winding"})
    v, t = _meshes()["icosphere"]
    a, b, out = str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), str(tmp_path / "out.json")
    gio.write_ply(a, v, t)
    gio.write_ply(b, 1.05 * v, t)
    capsys.readouterr()
    assert cli.main([a, b, "--samples", "500", "--signed", "--sign", "winding", "--beta", "4", "--json", out]) == 0
    lines = capsys.readouterr().out.strip().split("\n")
    assert len(lines) == 3 and "signed_mean" in lines[0] and "no_sign" in lines[1]
    got = json.load(open(out))
    fa, fb = gio.read_ply(a), gio.read_ply(b)
    assert {k: got[k] for k in ("a_to_b", "b_to_a", "hausdorff", "chamfer")} == {
        k: x for k, x in gio.compare_meshes(*fa, *fb, samples=500, signed=True, sign="winding", beta=4.0).items() if k in ("a_to_b", "b_to_a", "hausdorff", "chamfer")}
    assert got["a_to_b"]["inside"] == got["a_to_b"]["n"] and got["b_to_a"]["inside"] == 0 and got["triangles_a"] == len(t)
