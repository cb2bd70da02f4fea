"""K36 without a GPU: the rule's numpy restatement (tests/mesh_distance_reference.py) on one triangle, on degenerate triangles and on planted
ties; against an independent longdouble formulation on the white-noise and sphere meshes; the properties a distance must have; the bound
K33's guarantee implies for a simplified mesh; the refusals of the entry point through ctypes and of the Python layers."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from . import mesh_distance_reference as DR
from . import mesh_simplify_reference as SR

EPS = 2.0 ** -52
# |sqrt(d2 of the rule) - the longdouble distance| <= K eps S, S = the largest |coordinate| among the query and the winning face.  The worst
# ratio measured over the two meshes below at these seeds is 0.56 (noise mesh 0.422, sphere 0.557): K is four times that.
K_MEASURED = 0.56
K_BOUND = 4 * K_MEASURED


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_one_triangle_every_region_above_and_below():
    v, t = DR.TRIANGLE
    q, want = DR.region_queries()
    got = DR.closest(v, t, q)
    assert got["region"].tolist() == want.tolist() and (got["face"] == 0).all()
    ref = DR.exact_closest(v, t, q)
    assert np.abs(np.sqrt(got["dist2"]) - ref.astype(np.float64)).max() <= K_BOUND * EPS * 4.0
    # the point is the one the distance is measured to, and it lies in the face's plane
    a, b, c = v
    n = np.cross(b - a, c - a)
    assert np.abs((got["point"] - a) @ n).max() <= 64 * EPS * np.abs(n).max() * 4.0
    u = q - got["point"]
    assert _same((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2], got["dist2"])
    # vertex regions return the vertex itself
    for code, corner in ((1, a), (2, b), (3, c)):
        assert (got["point"][want == code] == corner).all()


def test_points_of_the_triangle_are_at_exactly_zero():
    v, t = DR.TRIANGLE
    q = DR.zero_queries()
    got = DR.closest(v, t, q)
    assert (got["dist2"] == 0.0).all() and not np.signbit(got["dist2"]).any() and _same(got["point"], q)
    assert got["region"][:3].tolist() == [1, 2, 3] and (got["region"][3:] <= 6).all()


def test_degenerate_triangles_take_the_degenerate_path():
    v, t = DR.degenerate_mesh()
    rng = np.random.default_rng(0)
    q = rng.uniform(-2.0, 8.0, (64, 3))
    for f in range(3):
        d2, p, region = DR.face_rule(q, v[t[f, 0]], v[t[f, 1]], v[t[f, 2]])
        assert (region == 7).all() and np.isfinite(d2).all() and np.isfinite(p).all()
        ref = DR.exact_distance(q, v[t[f, 0]], v[t[f, 1]], v[t[f, 2]]).astype(np.float64)
        assert np.abs(np.sqrt(d2) - ref).max() <= K_BOUND * EPS * 8.0
    d2, p, region = DR.face_rule(q, v[9], v[10], v[11])
    assert (region != 7).all()
    # three equal points: the point itself; a zero edge: its other segment
    assert (DR.face_rule(q, v[0], v[1], v[2])[1] == v[0]).all()
    # no NaN from any division, whatever the face: a zero-length segment is its end point
    assert DR.face_rule(v[0], v[0], v[0], v[0])[0] == 0.0


def test_the_smaller_face_index_wins_a_tie():
    v, t = DR.tie_mesh()
    q = np.array([[0.25, 0.25, 0.5], [0.25, 0.25, -0.5], [-1.0, -1.0, 0.0],      # the duplicated face: interior and a vertex region
                  [2.0, 4.5, 1.5], [2.0, 4.0, 1.0], [2.0, 6.0, 0.0]])          # the mirror plane
    got = DR.closest(v, t, q)
    assert got["face"].tolist() == [0, 0, 0, 3, 3, 3]
    for f0, f1, rows in ((0, 2, slice(0, 3)), (3, 4, slice(3, 6))):
        d_a = DR.face_rule(q[rows], *[v[t[f0, k]] for k in range(3)])[0]
        d_b = DR.face_rule(q[rows], *[v[t[f1, k]] for k in range(3)])[0]
        assert _same(d_a, d_b) and _same(d_a, got["dist2"][rows])               # a tie in every bit, not nearly one
    # the order of the faces decides, nothing else: swap the mirrored pair
    t2 = t[[0, 1, 2, 4, 3]]
    assert DR.closest(v, t2, q)["face"].tolist() == [0, 0, 0, 3, 3, 3] and _same(DR.closest(v, t2, q)["dist2"], got["dist2"])


def test_the_cap_non_finite_queries_and_the_empty_mesh():
    v, t = DR.TRIANGLE
    q = np.array([[1.0, 1.0, 4.0], [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0]])
    d = float(np.sqrt(DR.closest(v, t, q[:1])["dist2"][0]))
    # the boundary itself, at a distance known exactly: the plane z = 0 from z = 0.375 (d2 = 0.140625 = the rounded product 0.375 * 0.375);
    # the cap is NON-strict, so `at` keeps the query, one ulp below loses it
    pv, pt = SR.grid_mesh(6, 5, 0.5)
    pq = np.array([[1.1, 0.9, 0.375], [0.3, 1.7, -0.375], [1.1, 0.9, 0.25], [9.0, 9.0, 9.0]])
    at, under, over = (DR.closest(pv, pt, pq, max_dist=float(c)) for c in (0.375, np.nextafter(0.375, 0.0), np.nextafter(0.375, 1.0)))
    assert (at["face"] >= 0).tolist() == [True, True, True, False] and (at["dist2"][:2] == 0.140625).all() and at["dist2"][3] == np.inf
    assert (under["face"] >= 0).tolist() == [False, False, True, False] and (under["dist2"][:2] == np.inf).all()
    assert (over["face"] >= 0).tolist() == [True, True, True, False] and _same(over["dist2"], at["dist2"])
    above, below = DR.closest(v, t, q, max_dist=d * (1 + 1e-9)), DR.closest(v, t, q, max_dist=d * (1 - 1e-9))
    assert above["face"].tolist() == [0, -1, -1] and below["face"].tolist() == [-1, -1, -1]
    assert below["dist2"][0] == np.inf and np.isnan(below["dist2"][1:]).all() and np.isnan(below["point"]).all() and (below["region"] == 255).all()
    none = DR.closest(np.zeros((0, 3)), np.zeros((0, 3), np.int32), q)
    assert none["dist2"][0] == np.inf and np.isnan(none["dist2"][1:]).all() and (none["face"] == -1).all()


def _k_of(v, t, seed, n=200):
    rng = np.random.default_rng(seed)
    lo, hi = v.min(axis=0), v.max(axis=0)
    q = np.concatenate([rng.uniform(lo - 2.0, hi + 2.0, (n - 60, 3)), v[rng.integers(0, len(v), 60)] + rng.normal(0, 0.05, (60, 3))])
    got = DR.closest(v, t, q)
    ref = DR.exact_closest(v, t, q)
    scale = np.maximum(np.abs(q).max(axis=1), np.abs(v[t[got["face"]]]).max(axis=(1, 2)))
    err = np.abs(np.sqrt(got["dist2"]).astype(np.longdouble) - ref).astype(np.float64)
    return float((err / (EPS * scale)).max())


@pytest.mark.parametrize("name", ["noise", "sphere"])
def test_the_rule_agrees_with_the_longdouble_formulation(name):
    v, t = DR.noise_mesh() if name == "noise" else DR.sphere_mesh()
    k = _k_of(v, t, seed=11 if name == "noise" else 12)
    print(f"{name}: worst |d_rule - d_ref| / (eps S) = {k:.3f} over 200 queries, {len(t)} faces")
    assert k <= K_BOUND


def test_a_shifted_patch_is_exactly_the_shift_away_and_a_mesh_is_at_zero_from_itself():
    v, t = SR.grid_mesh(6, 5, 0.5)
    h = 0.375
    shifted = v + np.array([0.0, 0.0, h])
    rng = np.random.default_rng(3)
    inner = np.stack([rng.uniform(0.1, 2.4, 200), rng.uniform(0.1, 1.9, 200), np.zeros(200)], axis=1)       # projections interior to the patch
    got = DR.closest(shifted, t, np.concatenate([inner, v[[7, 8, 13]]]))
    assert (got["dist2"] == h * h).all() and (np.sqrt(got["dist2"]) == h).all()
    stats = DR.direction_stats(got["dist2"])
    assert stats["mean"] == h and stats["rms"] == h and stats["max"] == h and stats["q50"] == h and stats["unmatched"] == 0
    # A against A: every figure exactly 0 (samples are points of A: its vertices and points of its triangles)
    nv, nt = DR.noise_mesh()
    pick = rng.integers(0, len(nt), 60)
    mids = (nv[nt[pick, 0]] + nv[nt[pick, 1]]) * 0.5
    own = DR.closest(nv, nt, np.concatenate([nv[:100], mids]))
    assert (own["dist2"][:100] == 0.0).all()
    assert np.sqrt(own["dist2"][100:]).max() <= K_BOUND * EPS * 66.0       # (an edge's midpoint is a point of A only up to its own rounding)
    same = DR.mesh_distance(nv, nt, nv, nt, nv[:100], nv[:100], 1.0, 1.0)
    assert all(same[s][k] == 0.0 for s in ("a_to_b", "b_to_a") for k in ("mean", "rms", "max", "q50", "q90", "q99"))
    assert same["hausdorff"] == 0.0 and same["chamfer"] == 0.0 and same["a_to_b"]["n"] == 100 and same["a_to_b"]["unmatched"] == 0


@pytest.mark.parametrize("cell", [2.0, 3.0, 4.0])
def test_a_simplified_vertex_is_within_root_three_cells_of_the_mesh_it_came_from(cell):
    """K33 guarantees every output vertex within sqrt(3) cell of vertices[source], and a referenced vertex is a point of the mesh: so the
    distance from a simplified vertex to the original MESH is at most sqrt(3) cell.  Loose, but derived."""
    v, t = DR.sphere_mesh()
    out = SR.simplify(v, t, cell, [-0.5] * 3)
    used = np.unique(out["triangles"])
    got = DR.closest(v, t, out["vertices"][used])
    worst = float(np.sqrt(got["dist2"].max()))
    print(f"sphere, cell {cell}: {len(used)} simplified vertices, worst distance to the original mesh {worst:.4f} (bound {3 ** 0.5 * cell:.4f})")
    assert worst <= 3 ** 0.5 * cell
    assert (np.sqrt(got["dist2"]) <= np.sqrt(((out["vertices"][used] - v[out["source"][used]]) ** 2).sum(axis=1)) * (1 + 8 * EPS)).all()


def test_direction_stats_counts_the_unmatched_and_leaves_them_out():
    d2 = np.array([4.0, np.inf, 1.0, 9.0, np.inf, 0.0])
    s = DR.direction_stats(d2)
    assert s == {"n": 6, "unmatched": 2, "mean": 1.5, "rms": float(np.sqrt(14.0 / 4)), "max": 3.0, "q50": 2.0, "q90": 3.0, "q99": 3.0}
    none = DR.direction_stats(np.array([np.inf, np.inf]))
    assert none["n"] == 2 and none["unmatched"] == 2 and all(np.isnan(none[k]) for k in ("mean", "rms", "max", "q50", "q90", "q99"))
    both = DR.summary(s, none, 0.5, 0.25)
    assert np.isnan(both["hausdorff"]) and np.isnan(both["chamfer"]) and both["density_b"] == 0.25


# ------------------------------------------------------------------------------------------------------------------------------------
# the library's host side and the Python layers, without a GPU
# ------------------------------------------------------------------------------------------------------------------------------------
def test_the_entry_point_reports_bad_arguments_without_a_gpu():
    from gens_amd import lib as L
    lib = L.load()
    p = lambda k: C.c_void_p(0x1000 + 0x100 * k)  # noqa: E731  (never dereferenced: every call below is refused, or launches nothing)

    def refused(rc, *words, code=-1):
        msg = lib.gens_last_error().decode()
        assert rc == code and all(w in msg for w in words), (rc, msg)

    def call(n=5, max_dist=float("inf"), queries=p(4), dist2=p(5), face=p(6), point=None, region=None, null_grid=False, **grid):
        g = {"vertices": p(0), "triangles": p(1), "cell_start": p(2), "cell_faces": p(3), "n_faces": 7, "lo_x": 0.0, "lo_y": 0.0, "lo_z": 0.0,
             "cell": 1.0, "nx": 4, "ny": 4, "nz": 4, **grid}
        args = L.MeshGridArgs(*[g[k] for k in ("vertices", "triangles", "cell_start", "cell_faces", "n_faces", "lo_x", "lo_y", "lo_z", "cell", "nx", "ny", "nz")])
        return lib.gens_mesh_closest_point(None if null_grid else C.byref(args), queries, n, max_dist, dist2, face, point, region, None)

    who = "gens_mesh_closest_point"
    refused(call(null_grid=True), who, "null grid")
    for name in ("queries", "dist2", "face"):
        refused(call(**{name: None}), who, "null pointer")
    for name in ("vertices", "triangles", "cell_start", "cell_faces"):
        refused(call(**{name: None}), who, "null pointer (in the grid)")
    refused(call(n=-1), who, "-1 queries")
    refused(call(n=1 << 31), who, "below 2^31", code=-2)
    refused(call(n_faces=-2), who, "-2 faces")
    refused(call(n_faces=1 << 31), who, "below 2^31", code=-2)
    for bad in (0.0, -1.0, float("nan"), -float("inf")):
        refused(call(max_dist=bad), who, "max_dist")
    for bad in ({"nx": 0}, {"ny": 513}, {"nz": -1}):
        refused(call(**bad), who, "cells per axis", code=-2)
    for bad in ({"cell": 0.0}, {"cell": float("inf")}, {"lo_y": float("nan")}):
        refused(call(**bad), who, "bad grid box", code=-2)
    refused(call(lo_x=1e9, cell=1e-3), who, "2^32 cells", code=-2)
    # no queries: no launch, no error, whatever the pointers
    assert call(n=0, queries=None, dist2=None, face=None) == 0
    assert call(n=0, queries=None, dist2=None, face=None, vertices=None, n_faces=0) == 0
    assert lib.gens_abi_version() == 12
    assert L.SIGNATURES[who][2] is C.c_int64 and L.SIGNATURES[who][3] is C.c_double and len(L.SIGNATURES[who]) == 9


def test_the_python_layers_refuse_bad_arguments_before_any_launch(tmp_path):
    from gens_amd import compare_meshes as cli, io as gio, ops
    from gens_amd.models.modules.implicit_surface import ImplicitSurface
    v, t = SR.grid_mesh(3, 3)
    host_v, host_t = torch.from_numpy(v), torch.from_numpy(t)
    with pytest.raises(ValueError, match="MeshGrid"):
        ops.closest_point_on_mesh(host_v, None)
    grid = ops.MeshGrid(host_v, host_t, torch.zeros(2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), (0.0, 0.0, 0.0, 1.0), (1, 1, 1))
    with pytest.raises(ValueError, match="no CPU path"):
        ops.closest_point_on_mesh(host_v, grid)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.closest_point_on_mesh(v, grid)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.mesh_distance(host_v, host_t, host_v, host_t)
    for bad in (0, -1.0, float("nan"), True, "far", None):
        with pytest.raises(ValueError, match="max_dist"):
            ops.distance_cap("t", bad)
    assert ops.distance_cap("t", float("inf")) == float("inf") and ops.distance_cap("t", 2) == 2.0
    assert ops.mesh_distance_request("t") == (None, 1_000_000, float("inf")) and ops.mesh_distance_request("t", density=0.5, samples=10) == (0.5, 10, float("inf"))
    for kw in ({"density": 0.0}, {"density": -1.0}, {"density": float("nan")}, {"density": float("inf")}, {"density": True}, {"density": "fine"},
               {"samples": 0}, {"samples": -5}, {"samples": 1.5}, {"samples": True}, {"max_dist": 0.0}, {"max_dist": float("nan")}):
        with pytest.raises(ValueError):
            ops.mesh_distance_request("t", **kw)
        with pytest.raises(ValueError):
            gio.compare_meshes(v, t, v, t, **kw)
    with pytest.raises(ValueError, match="unknown keyword 'chunk'"):
        gio.compare_meshes(v, t, v, t, chunk=5)
    with pytest.raises(ValueError, match="mesh B: triangle indices"):
        gio.compare_meshes(v, t, v, t + 1)
    with pytest.raises(ValueError, match="mesh A: a vertex is not finite"):
        gio.compare_meshes(np.where(v == 1.0, np.nan, v), t, v, t)
    # extract_geometry's option: None and False are off; True and a dict of mesh_distance's keywords ask; not without simplify
    surf = types.SimpleNamespace(mesh_simplify_error=None)
    req = lambda x, simplify=2.0: ImplicitSurface._simplify_error_request(surf, x, simplify)  # noqa: E731
    assert ImplicitSurface.mesh_simplify_error is None
    assert req(None) is None and req(False) is None and req(None, None) is None and req(False, None) is None
    assert req(True) == {} and req({"samples": 1000}) == {"samples": 1000} and req({"density": 0.5, "max_dist": 3}) == {"density": 0.5, "max_dist": 3}
    surf.mesh_simplify_error = {"samples": 50}
    assert req(None) == {"samples": 50} and req(False) is None and req(True) == {}
    for bad in (1, 0, "yes", 2.5, {"chunk": 4}, {"samples": 0}, {"density": -1}, {"max_dist": 0}, [("samples", 5)]):
        with pytest.raises(ValueError):
            req(bad)
    with pytest.raises(ValueError, match="needs simplify"):
        req(True, None)
    with pytest.raises(ValueError, match="needs simplify"):
        req(None, None)
    # the command line refuses bad keywords with exit status 2, before the device is looked at
    path = str(tmp_path / "a.ply")
    gio.write_ply(path, v, t)
    assert cli.main([path, str(tmp_path / "missing.ply")]) == 2 and cli.main([str(tmp_path), path]) == 2      # a file that cannot be read
    assert cli.main([path, path, "--density", "0"]) == 2 and cli.main([path, path, "--samples", "0"]) == 2 and cli.main([path, path, "--max-dist", "-1"]) == 2
    assert _same(cli.read_mesh(path)[1], t)
