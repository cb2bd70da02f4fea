"""GPU tests of the point-to-mesh distance (K36): gens_mesh_closest_point against the numpy restatement's brute force over all faces
(tests/mesh_distance_reference.py), bit for bit in dist2, face, point and region, on one triangle, a 300-triangle fan at 1 to 1000 queries,
the white-noise 7 x 19 x 66 marching-cubes mesh, the 33^3 sphere (its centre included: every ring), a one-cell grid, queries far outside the
box, two clusters of faces far apart, planted ties and degenerate faces, NaN and inf queries, a cap below, at and above a known distance,
planted face ids outside the mesh; determinism and chunking; the empty cases; ops.mesh_distance, io.compare_meshes and the command line;
extract_geometry(simplify_error=) and validate on the g23 model; nothing changes when the option is unset; the refusals."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from . import mesh_distance_reference as DR
from . import mesh_simplify_reference as SR

gpu = pytest.mark.gpu
K36 = {"gens_mesh_closest_point"}
K36_ROUTE = K36 | {"gens_mesh_grid_count", "gens_mesh_grid_fill", "gens_mesh_sample_count", "gens_mesh_sample_emit"}      # all that ops.mesh_distance launches
FIGURES = ("mean", "rms", "max", "q50", "q90", "q99")


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _up(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _around(v, n, seed, pad=2.0):
    """n seeded queries: most in the mesh's box widened by pad, a fifth within a few hundredths of vertices."""
    rng = np.random.default_rng(seed)
    near = n // 5
    lo, hi = v.min(axis=0), v.max(axis=0)
    return np.concatenate([rng.uniform(lo - pad, hi + pad, (n - near, 3)), v[rng.integers(0, len(v), near)] + rng.normal(0, 0.03, (near, 3))])


def _cases():
    """name -> (vertices, triangles, queries, max_dist)."""
    inf = np.inf
    tri_v, tri_t = DR.TRIANGLE
    odd = np.array([[np.nan, 1.0, 1.0], [1.0, np.inf, 1.0], [1.0, 1.0, -np.inf], [np.nan, np.nan, np.nan]])
    out = {"one triangle": (tri_v, tri_t, np.concatenate([DR.region_queries()[0], DR.zero_queries(), _around(tri_v, 40, 1), odd]), inf)}
    fan_v, fan_t = DR.fan_mesh()
    for n in (1, 63, 64, 65, 257, 1000):
        out[f"fan, {n} queries"] = (fan_v, fan_t, _around(fan_v, n, 100 + n, pad=1.0), inf)
    noise_v, noise_t = DR.noise_mesh()
    out["noise"] = (noise_v, noise_t, _around(noise_v, 129, 2), inf)
    sph_v, sph_t = DR.sphere_mesh()
    out["sphere"] = (sph_v, sph_t, np.concatenate([SR.CENTRE[None], sph_v[:20], _around(sph_v, 179, 3)]), inf)
    lo, hi = sph_v.min(axis=0), sph_v.max(axis=0)
    mid, ext = 0.5 * (lo + hi), (hi - lo).max()
    far = [mid + s * 100.0 * ext * np.eye(3)[a] for a in range(3) for s in (1.0, -1.0)] + [hi + 100.0 * ext, lo - 100.0 * ext]
    out["sphere, far outside"] = (sph_v, sph_t, np.array(far), inf)
    two_v, two_t = DR.two_clusters_mesh()
    rng = np.random.default_rng(4)
    between = np.stack([rng.uniform(2.0, 39.0, 65), rng.uniform(-1.0, 5.0, 65), rng.uniform(-1.0, 3.0, 65)], axis=1)
    out["two clusters"] = (two_v, two_t, np.concatenate([between, [[20.5, 2.0, 0.75]]]), inf)
    tie_v, tie_t = DR.tie_mesh()
    ties = np.array([[0.25, 0.25, 0.5], [0.25, 0.25, -0.5], [-1.0, -1.0, 0.0], [2.0, 4.5, 1.5], [2.0, 4.0, 1.0], [2.0, 6.0, 0.0]])
    out["ties"] = (tie_v, tie_t, np.concatenate([ties, _around(tie_v, 58, 5)]), inf)
    out["ties, the mirrored pair swapped"] = (tie_v, tie_t[[0, 1, 2, 4, 3]], np.concatenate([ties, _around(tie_v, 58, 5)]), inf)
    deg_v, deg_t = DR.degenerate_mesh()
    out["degenerate"] = (deg_v, deg_t, np.concatenate([_around(deg_v, 120, 6), deg_v]), inf)
    # a cap below, at and above a distance known exactly: the plane z = 0 from z = 0.375
    patch_v, patch_t = SR.grid_mesh(6, 5, 0.5)
    q_cap = np.array([[1.1, 0.9, 0.375], [0.3, 1.7, -0.375], [1.1, 0.9, 0.25], [9.0, 9.0, 9.0]])
    for name, cap in (("below", np.nextafter(0.375, 0.0)), ("at", 0.375), ("above", np.nextafter(0.375, 1.0))):
        out[f"cap {name}"] = (patch_v, patch_t, q_cap, float(cap))
    out["noise, capped"] = (noise_v, noise_t, _around(noise_v, 65, 7, pad=6.0), 1.5)
    return out


CASE_NAMES = ["one triangle", "fan, 1 queries", "fan, 63 queries", "fan, 64 queries", "fan, 65 queries", "fan, 257 queries", "fan, 1000 queries", "noise",
              "sphere", "sphere, far outside", "two clusters", "ties", "ties, the mirrored pair swapped", "degenerate", "cap below", "cap at",
              "cap above", "noise, capped"]
_CASES, _WANT = {}, {}


def _case(name):
    if not _CASES:
        _CASES.update(_cases())
    return _CASES[name]


def _want(name):
    """The restatement's result of a case, computed once and shared."""
    if name not in _WANT:
        v, t, q, cap = _case(name)
        _WANT[name] = DR.closest(v, t, q, cap)
    return _WANT[name]


def _device(grid, q, cap=np.inf, chunk=None):
    from gens_amd import ops
    d2, face, point, region = ops.mesh_closest_dist2(_up(q, np.float64), grid, cap, points=True, regions=True, chunk=chunk)
    return {"dist2": d2.cpu().numpy(), "face": face.cpu().numpy(), "point": point.cpu().numpy(), "region": region.cpu().numpy()}


def _equal(got, want):
    return all(_same(got[k], want[k]) for k in ("dist2", "face", "point", "region"))


def _grid_with(v, t, box, dims):
    """ops.build_mesh_grid's steps with a box and cell counts of the test's choosing."""
    from gens_amd import lib as L, ops
    i32 = torch.int32
    cells = dims[0] * dims[1] * dims[2]
    grid = ops.MeshGrid(_up(v, np.float64), _up(t, np.int32), torch.zeros(cells + 1, device="cuda", dtype=i32), torch.zeros(1, device="cuda", dtype=i32), box, dims)
    counts = torch.zeros(cells, device="cuda", dtype=i32)
    L.call("gens_mesh_grid_count", C.byref(grid.args()), L.ptr(counts, i32), L.stream())
    grid.cell_start[1:] = torch.cumsum(counts, 0).to(i32)
    grid.cell_faces = torch.empty(int(grid.cell_start[-1]), device="cuda", dtype=i32)
    counts.zero_()
    L.call("gens_mesh_grid_fill", C.byref(grid.args()), L.ptr(counts, i32), L.stream())
    return grid


@gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_kernel_equals_brute_force_over_all_faces(name):
    from gens_amd import ops
    v, t, q, cap = _case(name)
    want = _want(name)
    grid = ops.build_mesh_grid(_up(v, np.float64), _up(t, np.int32))
    got = _device(grid, q, cap)
    found = want["face"] >= 0
    print(f"{name}: grid {grid.dims}, {len(t)} faces, {len(q)} queries, {int(found.sum())} found, regions {np.bincount(want['region'][found], minlength=8).tolist()}")
    assert _equal(got, want)
    # the public wrapper: the root of the same numbers, and only the outputs asked for
    dist, face = ops.closest_point_on_mesh(_up(q, np.float64), grid, max_dist=cap)
    assert _same(dist.cpu().numpy(), np.sqrt(want["dist2"])) and _same(face.cpu().numpy(), want["face"])


@gpu
def test_what_the_cases_are_there_for():
    """The planted cases do what their names say (in the restatement, which the kernel equals)."""
    assert _want("ties")["face"][:6].tolist() == [0, 0, 0, 3, 3, 3] and _want("ties, the mirrored pair swapped")["face"][:6].tolist() == [0, 0, 0, 3, 3, 3]
    assert (_want("degenerate")["region"] == 7).sum() > 20 and np.isfinite(_want("degenerate")["dist2"]).all()
    assert sorted(set(_want("one triangle")["region"][:-4].tolist())) == [0, 1, 2, 3, 4, 5, 6]
    assert np.isnan(_want("one triangle")["dist2"][-4:]).all() and (_want("one triangle")["face"][-4:] == -1).all()
    assert (_want("cap below")["face"] >= 0).tolist() == [False, False, True, False]
    assert (_want("cap at")["face"] >= 0).tolist() == [True, True, True, False] and (_want("cap above")["face"] >= 0).tolist() == [True, True, True, False]
    assert (_want("cap at")["dist2"][:2] == 0.140625).all() and (_want("cap above")["dist2"][:2] == 0.140625).all()
    capped = _want("noise, capped")["face"]
    assert (capped < 0).any() and (capped >= 0).any()
    centre = _want("sphere")
    assert abs(np.sqrt(centre["dist2"][0]) - SR.SPHERE_RADIUS) < 0.05


@gpu
def test_the_walk_does_not_show_a_one_cell_grid_a_fine_grid_and_planted_face_ids():
    from gens_amd import ops
    v, t, q, _ = _case("fan, 257 queries")
    want = _want("fan, 257 queries")
    lo = v.min(axis=0) - 0.01
    one = _grid_with(v, t, (*lo.tolist(), float((v.max(axis=0) - lo).max() + 0.02)), (1, 1, 1))
    assert _equal(_device(one, q), want)
    cell = float((v.max(axis=0) - lo).max() + 0.02) / 40.0
    fine = _grid_with(v, t, (*lo.tolist(), cell), (40, 40, 8))
    assert _equal(_device(fine, q), want)
    # face ids outside 0 .. F - 1 planted into every cell's list: skipped, the answer is the same
    grid = ops.build_mesh_grid(_up(v, np.float64), _up(t, np.int32))
    start, faces = grid.cell_start.cpu().numpy(), grid.cell_faces.cpu().numpy()
    junk = np.array([-1, len(t), 2 ** 31 - 1, -2 ** 31], np.int32)
    lists = [np.concatenate([junk[:2], faces[start[c]:start[c + 1]], junk[2:]]) for c in range(len(start) - 1)]
    planted = ops.MeshGrid(grid.vertices, grid.triangles, _up(np.concatenate([[0], np.cumsum([len(x) for x in lists])]), np.int32),
                           _up(np.concatenate(lists), np.int32), grid.box, grid.dims)
    assert _equal(_device(planted, q), want)
    # the same walk over the two-cluster mesh at a forced fine grid: many empty rings between the clusters
    v2, t2, q2, _ = _case("two clusters")
    lo2 = v2.min(axis=0) - 0.01
    assert _equal(_device(_grid_with(v2, t2, (*lo2.tolist(), 0.25), (200, 20, 10)), q2), _want("two clusters"))


@gpu
def test_the_same_bits_twice_and_at_every_chunk():
    from gens_amd import lib as L, ops
    v, t, q, _ = _case("fan, 1000 queries")
    want = _want("fan, 1000 queries")
    grid = ops.build_mesh_grid(_up(v, np.float64), _up(t, np.int32))
    for chunk, launches in ((None, 1), (None, 1), (64, 16), (1000, 1), (999, 2)):
        L.profile_begin(only=K36)
        got = _device(grid, q, chunk=chunk)
        assert len(L.profile_end(raw=True)) == launches and _equal(got, want), chunk
    # outputs that are not asked for are not written, and a slot past the end stays
    d2 = torch.full((1001,), -7.0, device="cuda", dtype=torch.float64)
    face = torch.full((1001,), -7, device="cuda", dtype=torch.int32)
    L.call("gens_mesh_closest_point", C.byref(grid.args()), L.ptr(_up(q, np.float64), torch.float64), 1000, float("inf"), L.ptr(d2, torch.float64),
           L.ptr(face, torch.int32), None, None, L.stream())
    assert _same(d2[:1000].cpu().numpy(), want["dist2"]) and _same(face[:1000].cpu().numpy(), want["face"]) and float(d2[1000]) == -7.0 and int(face[1000]) == -7


@gpu
def test_empty_cases_launch_nothing():
    from gens_amd import lib as L, ops
    f64, i32 = torch.float64, torch.int32
    v, t = DR.TRIANGLE
    q = _up(np.array([[0.0, 0.0, 0.0], [np.nan, 0.0, 0.0]]), np.float64)
    L.profile_begin(only=K36)
    empty = ops.build_mesh_grid(torch.zeros(0, 3, device="cuda", dtype=f64), torch.zeros(0, 3, device="cuda", dtype=i32))
    dist, face, point, region = ops.closest_point_on_mesh(q, empty, points=True, regions=True)
    assert float(dist[0]) == float("inf") and bool(torch.isnan(dist[1])) and face.tolist() == [-1, -1] and bool(torch.isnan(point).all()) and region.tolist() == [255, 255]
    grid = ops.build_mesh_grid(_up(v, np.float64), _up(t, np.int32))
    none = ops.closest_point_on_mesh(torch.zeros(0, 3, device="cuda", dtype=f64), grid, points=True, regions=True)
    assert [tuple(x.shape) for x in none] == [(0,), (0,), (0, 3), (0,)] and none[1].dtype == i32 and none[3].dtype == torch.uint8
    assert not L.profile_end(raw=True)
    # the entry point itself: no queries is no launch whatever the pointers; a mesh without faces gets the fill
    lib = L.load()
    assert lib.gens_mesh_closest_point(C.byref(grid.args()), None, 0, 1.0, None, None, None, None, None) == 0
    d2, fc = torch.full((2,), -7.0, device="cuda", dtype=f64), torch.full((2,), -7, device="cuda", dtype=i32)
    L.call("gens_mesh_closest_point", C.byref(empty.args()), L.ptr(q, f64), 2, 1.0, L.ptr(d2, f64), L.ptr(fc, i32), None, None, L.stream())
    assert float(d2[0]) == float("inf") and bool(torch.isnan(d2[1])) and fc.tolist() == [-1, -1]
    # two meshes without faces: their vertices are the samples, everything is unmatched
    out = ops.mesh_distance(_up(v, np.float64), torch.zeros(0, 3, device="cuda", dtype=i32), _up(v, np.float64), torch.zeros(0, 3, device="cuda", dtype=i32))
    assert out["a_to_b"]["n"] == 3 and out["a_to_b"]["unmatched"] == 3 and np.isnan(out["hausdorff"]) and np.isnan(out["chamfer"])


def _close(got, want):
    """The dicts of ops.mesh_distance and of the restatement: counts, max and the order statistics exact, the moments to 1e-12 relative."""
    for side in ("a_to_b", "b_to_a"):
        g, w = got[side], want[side]
        if g["n"] != w["n"] or g["unmatched"] != w["unmatched"]:
            return False
        for k in FIGURES:
            if np.isnan(w[k]) != np.isnan(g[k]) or (not np.isnan(w[k]) and (g[k] != w[k] if k not in ("mean", "rms") else abs(g[k] - w[k]) > 1e-12 * abs(w[k]))):
                return False
    if np.isnan(want["hausdorff"]):
        return bool(np.isnan(got["hausdorff"]) and np.isnan(got["chamfer"]))
    return got["hausdorff"] == want["hausdorff"] and abs(got["chamfer"] - want["chamfer"]) <= 1e-12 * abs(want["chamfer"]) and \
        got["density_a"] == want["density_a"] and got["density_b"] == want["density_b"]


def _fan_pair():
    va, ta = DR.fan_mesh()
    rng = np.random.default_rng(8)
    vb = va + rng.normal(0, 0.02, va.shape)
    return va, ta, vb, ta[:200].copy()              # B: two thirds of a perturbed copy -- a hole, so the two directions differ


@gpu
@pytest.mark.parametrize("kw", [{"samples": 700}, {"density": 0.11}, {"density": 0.09, "max_dist": 0.06}], ids=["samples", "density", "capped"])
def test_mesh_distance_equals_the_restatement_on_the_same_samples(kw):
    from gens_amd import ops
    va, ta, vb, tb = _fan_pair()
    dev = [_up(va, np.float64), _up(ta, np.int32), _up(vb, np.float64), _up(tb, np.int32)]
    got = ops.mesh_distance(*dev, **kw, return_samples=True)
    sa, sb = got["samples_a"].cpu().numpy(), got["samples_b"].cpu().numpy()
    assert _same(sa[:len(va)], va) and _same(sb[:len(vb)], vb) and len(sa) > len(va) and len(sb) > len(vb)       # its vertices, then K24's lattice points
    if "density" in kw:
        assert got["density_a"] == got["density_b"] == kw["density"]
    else:
        assert got["density_a"] == np.sqrt(DR.mesh_area(va, ta) / kw["samples"]) or abs(got["density_a"] / np.sqrt(DR.mesh_area(va, ta) / kw["samples"]) - 1) < 1e-12
    want = DR.mesh_distance(va, ta, vb, tb, sa, sb, got["density_a"], got["density_b"], kw.get("max_dist", np.inf))
    print(f"{kw}: {json.dumps({k: v for k, v in got.items() if not torch.is_tensor(v)})}")
    assert _close(got, want)
    assert _same(got["dist_a"].cpu().numpy(), np.sqrt(DR.closest(vb, tb, sa, kw.get("max_dist", np.inf))["dist2"]))
    if "max_dist" in kw:
        assert got["a_to_b"]["unmatched"] > 0 and got["a_to_b"]["max"] <= kw["max_dist"]
    else:
        assert got["a_to_b"]["max"] > 2 * got["b_to_a"]["max"]           # the hole of B shows in a_to_b only
    plain = ops.mesh_distance(*dev, **kw)
    assert sorted(plain) == ["a_to_b", "b_to_a", "chamfer", "density_a", "density_b", "hausdorff"] and plain == {k: got[k] for k in plain}


@gpu
def test_a_mesh_is_at_zero_from_itself_and_a_shifted_patch_at_the_shift():
    from gens_amd import ops
    nv, nt = DR.noise_mesh()
    dv, dt = _up(nv, np.float64), _up(nt, np.int32)
    same = ops.mesh_distance(dv, dt, dv, dt, density=1e3)               # no lattice point at this spacing: the samples are the vertices, points of A
    assert all(same[s][k] == 0.0 for s in ("a_to_b", "b_to_a") for k in FIGURES) and same["hausdorff"] == 0.0 and same["chamfer"] == 0.0
    assert same["a_to_b"]["n"] == len(nv) and same["a_to_b"]["unmatched"] == 0
    dense = ops.mesh_distance(dv, dt, dv, dt, samples=20000)            # lattice points are points of A up to their own rounding
    assert dense["hausdorff"] <= 64 * 2.0 ** -52 * 66.0 and dense["a_to_b"]["n"] > len(nv)
    pv, pt = SR.grid_mesh(6, 5, 0.5)
    h = 0.375
    grid = ops.build_mesh_grid(_up(pv + np.array([0.0, 0.0, h]), np.float64), _up(pt, np.int32))
    rng = np.random.default_rng(3)
    inner = np.stack([rng.uniform(0.1, 2.4, 500), rng.uniform(0.1, 1.9, 500), np.zeros(500)], axis=1)
    dist, face, region = ops.closest_point_on_mesh(_up(inner, np.float64), grid, regions=True)
    assert bool((dist == h).all()) and bool((face >= 0).all()) and bool((region <= 6).all())


@gpu
def test_io_compare_meshes_and_the_command_line(tmp_path, capsys):
    from gens_amd import compare_meshes as cli, io as gio, ops
    va, ta, vb, tb = _fan_pair()
    dev = [_up(va, np.float64), _up(ta, np.int32), _up(vb, np.float64), _up(tb, np.int32)]
    want = ops.mesh_distance(*dev, samples=700)
    got = gio.compare_meshes(va, ta.astype(np.int64), torch.from_numpy(vb), tb, samples=700)
    assert got == want and type(got["hausdorff"]) is float and type(got["a_to_b"]["n"]) is int and type(got["a_to_b"]["mean"]) is float
    # the command line: a PLY against an OBJ; the files hold float32 vertices, so the figures are those of the rounded meshes
    a_path, b_path, j_path = str(tmp_path / "a.ply"), str(tmp_path / "b.obj"), str(tmp_path / "out.json")
    gio.write_ply(a_path, va, ta)
    gio.write_obj(b_path, vb, tb, np.zeros((len(tb), 3, 2), np.float32), np.zeros((2, 2, 3), np.uint8))
    assert cli.main([a_path, b_path, "--samples", "700", "--json", j_path]) == 0
    lines = capsys.readouterr().out.strip().split("\n")
    assert len(lines) == 3 and lines[0].startswith("a_to_b: n ") and lines[1].startswith("b_to_a: n ") and lines[2].startswith("hausdorff ")
    fa, fb = gio.read_ply(a_path), gio.read_obj(b_path)
    assert _same(fa[1], ta) and _same(fb["triangles"], tb)
    files = gio.compare_meshes(fa[0], fa[1], fb["vertices"], fb["triangles"], samples=700)
    with open(j_path) as f:
        written = json.load(f)
    assert {k: written[k] for k in files} == files and written["triangles_a"] == len(ta) and written["vertices_b"] == len(vb)
    assert f"hausdorff {files['hausdorff']:.6g}" in lines[2]
    assert cli.main([a_path, b_path, "--density", "0.11", "--max-dist", "0.06"]) == 0
    assert "unmatched" in capsys.readouterr().out
    assert cli.main([a_path, b_path, "--max-dist", "0"]) == 2


# ------------------------------------------------------------------------------------------------------------------------------------
# the model: the g23 surface of tests/test_hip_mesh_simplify.py, R = 64
# ------------------------------------------------------------------------------------------------------------------------------------
R = 64


@gpu
def test_extract_geometry_measures_the_simplification_on_request():
    from gens_amd import lib as L, ops
    from .test_hip_mesh_simplify import _model, _world
    from .test_hip_vertex_attrs import _validate_args
    m = _model()
    surf, vols, lo, hi = m["surf"], m["vols"], m["lo"], m["hi"]
    sv, st, _, stats = m["simple"]
    full = [_up(m["full"][0], np.float64), _up(m["full"][1], np.int32)]
    simple = [_up(sv, np.float64), _up(st, np.int32)]
    want = ops.mesh_distance(*full, *simple, return_samples=True)
    L.profile_begin(only=K36)
    v, t = surf.extract_geometry(vols, lo, hi, R, 0.0, simplify=2, simplify_error=True)
    assert len(L.profile_end(raw=True)) == 2                                   # one launch per direction
    assert _same(v, _world(sv, lo, hi)) and _same(t, st)                       # the mesh is what it was without the measurement
    err = surf.last_simplify_stats["error"]
    print(f"g23 R = {R}, cell 2: {json.dumps(err)}")
    assert err == {k: want[k] for k in err} and {k: x for k, x in surf.last_simplify_stats.items() if k != "error"} == stats
    assert err["a_to_b"]["unmatched"] == 0 and err["b_to_a"]["unmatched"] == 0 and err["a_to_b"]["n"] > 100_000 and err["hausdorff"] > 0.0
    # K33's guarantee, now measured: every simplified vertex within sqrt(3) cell of the extracted MESH
    at_vertices = want["dist_b"][:len(sv)]
    assert float(at_vertices.max()) <= 3 ** 0.5 * 2 and float(at_vertices.max()) > 0.0
    # a dict of keywords, the attribute, and validate
    small = surf.extract_geometry(vols, lo, hi, R, 0.0, simplify=2, simplify_error={"samples": 5000, "max_dist": 0.25})
    assert _same(small[0], v) and surf.last_simplify_stats["error"] == ops.mesh_distance(*full, *simple, samples=5000, max_dist=0.25)
    surf.mesh_simplify_error = {"samples": 5000}
    try:
        surf.extract_geometry(vols, lo, hi, R, 0.0, simplify=2)
        by_attribute = surf.last_simplify_stats["error"]
        assert by_attribute == ops.mesh_distance(*full, *simple, samples=5000)
        surf.extract_geometry(vols, lo, hi, R, 0.0, simplify=2, simplify_error=False)
        assert "error" not in surf.last_simplify_stats
    finally:
        del surf.mesh_simplify_error
    torch.manual_seed(3)
    out = surf.validate(*_validate_args(surf, vols), extract_geometry=True, mesh_resolution=R, mesh_simplify=2, mesh_simplify_error={"samples": 5000})
    assert _same(out["vertices"], v) and _same(out["triangles"], t) and surf.last_simplify_stats["error"] == by_attribute


@gpu
def test_nothing_changes_when_the_option_is_unset():
    from gens_amd import lib as L
    from gens_amd.config import Conf, gens_model_conf
    from gens_amd.models.gens import GenS
    from gens_amd.models.modules.implicit_surface import ImplicitSurface
    from .test_hip_mesh_simplify import _model, _world
    from .test_hip_vertex_attrs import TODAYS_KEYS, _validate_args
    assert ImplicitSurface.mesh_simplify_error is None
    m = _model()
    surf, vols, lo, hi = m["surf"], m["vols"], m["lo"], m["hi"]
    assert "mesh_simplify_error" not in vars(surf)
    L.profile_begin(only=K36)
    for off in ({}, {"simplify_error": None}, {"simplify_error": False}):
        got = surf.extract_geometry(vols, lo, hi, R, 0.0, simplify=2, **off)
        assert len(got) == 2 and _same(got[0], _world(m["simple"][0], lo, hi)) and _same(got[1], m["simple"][1]), off
        assert surf.last_simplify_stats == m["simple"][3] and "error" not in surf.last_simplify_stats
        plain = surf.extract_geometry(vols, lo, hi, R, 0.0, **off)
        assert _same(plain[0], _world(m["full"][0], lo, hi)) and _same(plain[1], m["full"][1]) and surf.last_simplify_stats is None
    args = _validate_args(surf, vols)
    torch.manual_seed(3)
    ref = surf.validate(*args, extract_geometry=True, mesh_resolution=33, mesh_simplify=2)
    torch.manual_seed(3)
    off = surf.validate(*args, extract_geometry=True, mesh_resolution=33, mesh_simplify=2, mesh_simplify_error=False)
    assert not L.profile_end(raw=True)
    assert set(ref) == set(off) == TODAYS_KEYS
    for k in TODAYS_KEYS:
        assert torch.equal(torch.as_tensor(off[k]), torch.as_tensor(ref[k])), k
    conf = gens_model_conf(volume_dims=(16, 8, 4), has_vol=True)
    assert "mesh_simplify_error" not in vars(GenS(conf).implicit_surface)
    assert GenS(Conf({**conf, "mesh_simplify": 2, "mesh_simplify_error": True})).implicit_surface.mesh_simplify_error is True
    assert GenS(Conf({**conf, "mesh_simplify_error": {"samples": 1000}})).implicit_surface.mesh_simplify_error == {"samples": 1000}


@gpu
def test_refusals_come_before_any_launch():
    from gens_amd import lib as L, ops
    from .test_hip_brick_mcubes import K29
    from .test_hip_mesh_simplify import K33, _model
    from .test_hip_sparse_lattice import K28
    from .test_hip_vertex_attrs import NETWORK, _validate_args
    m = _model()
    surf, vols, lo, hi = m["surf"], m["vols"], m["lo"], m["hi"]
    f64, i32 = torch.float64, torch.int32
    v, t = _up(DR.TRIANGLE[0], np.float64), _up(DR.TRIANGLE[1], np.int32)
    grid = ops.build_mesh_grid(v, t)
    L.profile_begin(only=K36_ROUTE | K33 | K28 | K29 | NETWORK | {"gens_compact_valid", "gens_mc_classify", "gens_mc_emit", "gens_lattice_points"})
    for bad in (1, "yes", {"chunk": 3}, {"samples": 0}, {"density": float("nan")}, {"max_dist": -1.0}):
        with pytest.raises(ValueError):
            surf.extract_geometry(vols, lo, hi, 33, 0.0, simplify=2, simplify_error=bad)
        with pytest.raises(ValueError):
            surf.validate(*_validate_args(surf, vols), extract_geometry=True, mesh_resolution=33, mesh_simplify=2, mesh_simplify_error=bad)
    for off in (None, 0, False):
        with pytest.raises(ValueError, match="needs simplify"):
            surf.extract_geometry(vols, lo, hi, 33, 0.0, simplify=off, simplify_error=True)
        with pytest.raises(ValueError, match="needs simplify"):
            surf.validate(*_validate_args(surf, vols), extract_geometry=True, mesh_resolution=33, mesh_simplify=off, mesh_simplify_error={"samples": 100})
    for q in (v.float(), v[:, :2], v.reshape(-1), v.cpu()):
        with pytest.raises(ValueError):
            ops.closest_point_on_mesh(q, grid)
    for kw in ({"max_dist": 0.0}, {"max_dist": float("nan")}, {"max_dist": -2.0}, {"chunk": 0}, {"chunk": 2.5}, {"chunk": True}):
        with pytest.raises(ValueError):
            ops.closest_point_on_mesh(v, grid, **kw)
    with pytest.raises(ValueError, match="MeshGrid"):
        ops.closest_point_on_mesh(v, (v, t))
    for meshes in ((v.float(), t, v, t), (v, t.long(), v, t), (v, t, v[:, :2], t), (v, t, v, t.cpu())):
        with pytest.raises(ValueError):
            ops.mesh_distance(*meshes)
    for kw in ({"samples": 0}, {"samples": 2.5}, {"density": 0.0}, {"density": float("inf")}, {"max_dist": 0.0}):
        with pytest.raises(ValueError):
            ops.mesh_distance(v, t, v, t, **kw)
    assert not L.profile_end(raw=True)
    with pytest.raises(ValueError, match="out of range"):
        ops.mesh_distance(v, torch.tensor([[0, 1, 3]], device="cuda", dtype=i32), v, t)
    assert ops.mesh_distance(v, t, v, t, samples=100)["hausdorff"] < 1e-14
