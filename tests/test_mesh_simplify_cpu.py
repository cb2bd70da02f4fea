"""CPU tests of the mesh simplification (K33): the numpy restatement (tests/mesh_simplify_reference.py) held to what the rule promises on
marching-cubes meshes of an analytic sphere and box, on a tilted plane, a cube corner and planted inputs; the argument checks of the three
entry points through ctypes and of the Python layers (these need the built library, not a GPU)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from . import mesh_simplify_reference as SR

ORIGIN = np.array([-0.5, -0.5, -0.5])
FIELDS = {"sphere": SR.sphere_field, "box": SR.box_field}
CELLS = (2, 3, 4)
_MESH, _CASE = {}, {}


def _mesh(name):
    if name not in _MESH:
        _MESH[name] = SR.lattice_mesh(FIELDS[name])
    return _MESH[name]


def _case(name, cell, reg=SR.REG, use_mean=False):
    """The restatement's output on a shared mesh; computed once, never modified."""
    key = (name, cell, reg, use_mean)
    if key not in _CASE:
        v, t = _mesh(name)
        _CASE[key] = SR.simplify(v, t, cell, ORIGIN, reg=reg, use_mean=use_mean)
    return _CASE[key]


def check_guarantees(v, t, out, cell, origin):
    """What the rule guarantees, for any input.  The cell test allows 8 spacings of the largest coordinate of the cell's corners: the centre
    is two rounded operations from its exact value, a member's q two more, x cell and the final sum one each, and the mean of the members'
    q leaves [-0.5, 0.5] by no more than the members' own excursion plus the sum's roundings (a fraction of a spacing for the handful of
    members a cell holds)."""
    ov, ot, src = out["vertices"], out["triangles"], out["source"]
    cc = SR.key_cell(out["cluster_keys"][out["out_clusters"]]).astype(np.float64)
    lo, hi = origin + cc * cell, origin + (cc + 1.0) * cell
    tol = 8 * np.spacing(np.maximum(np.abs(lo), np.abs(hi)))
    assert ((ov >= lo - tol) & (ov <= hi + tol)).all()
    # the source is a member of the vertex's cluster, hence within sqrt(3) cell of it (squared: no root; the same 8 spacings)
    assert np.array_equal(out["vertex_cluster"][src], out["out_clusters"])
    d2 = ((ov - v[src]) ** 2).sum(axis=1)
    assert (d2 <= 3.0 * (cell + 2 * tol.max()) ** 2).all()
    # triangles: three distinct valid indices, no two with the same vertex set, every vertex referenced
    assert ot.dtype == np.int32 and (ot >= 0).all() and (ot < len(ov)).all()
    assert ((ot[:, 0] != ot[:, 1]) & (ot[:, 1] != ot[:, 2]) & (ot[:, 0] != ot[:, 2])).all()
    assert len(np.unique(np.sort(ot, axis=1), axis=0)) == len(ot)
    assert np.array_equal(np.unique(ot), np.arange(len(ov)))
    assert (np.diff(out["cluster_keys"][out["out_clusters"]]) > 0).all()
    s = out["stats"]
    assert s["output_vertices"] == len(ov) and s["output_triangles"] == len(ot)
    assert s["input_triangles"] == s["output_triangles"] + s["collapsed_triangles"] + s["duplicate_triangles"]


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("name", sorted(FIELDS))
def test_the_guarantees_hold_and_the_counts_fall(name, cell):
    v, t = _mesh(name)
    out = _case(name, cell)
    check_guarantees(v, t, out, float(cell), ORIGIN)
    print(f"{name} cell {cell}: {len(v)} V / {len(t)} T -> {len(out['vertices'])} V / {len(out['triangles'])} T, stats {out['stats']}")
    assert 0 < len(out["vertices"]) < len(v) and 0 < len(out["triangles"]) < len(t)


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("name", sorted(FIELDS))
def test_the_quadric_is_doing_its_work(name, cell):
    """Mean |field| over 6 barycentric samples per output triangle (fixed seed): the rule's vertices against the cluster means on the same
    triangles.  Measured with this restatement: sphere 0.0167 against 0.0774 (0.215), 0.258 and 0.314 of the means' figure at cells 2, 3, 4;
    box 0.265, 0.099 and 0.015."""
    out, mean = _case(name, cell), _case(name, cell, use_mean=True)
    assert np.array_equal(out["triangles"], mean["triangles"]) and np.array_equal(mean["vertices"], out["means"])
    e = SR.field_error(FIELDS[name], out["vertices"], out["triangles"])
    e_mean = SR.field_error(FIELDS[name], out["means"], out["triangles"])
    fell = int(out["fell_back"].sum())
    print(f"{name} cell {cell}: mean |field| {e:.4f} against {e_mean:.4f} with the cluster means ({e / e_mean:.3f}); fell back {fell} of {len(out['vertices'])}")
    assert e <= 0.5 * e_mean
    assert fell <= 0.05 * len(out["vertices"])
    assert mean["fell_back"].all()


@pytest.mark.parametrize("reg", [1e-2, 1e-4])
def test_the_regulariser_hardly_moves_the_sphere(reg):
    base = SR.field_error(SR.sphere_field, _case("sphere", 2)["vertices"], _case("sphere", 2)["triangles"])
    out = _case("sphere", 2, reg=reg)
    e = SR.field_error(SR.sphere_field, out["vertices"], out["triangles"])
    print(f"reg {reg:g}: mean |field| {e:.5f} against {base:.5f} at 1e-3 ({abs(e - base) / base:.4f})")
    assert abs(e - base) < 0.05 * base


def test_a_tilted_plane_keeps_its_representatives_on_the_plane():
    v, t = SR.grid_mesh(23, 19, spacing=0.37)
    a, b = 0.41, -0.23
    rot_x = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    rot_y = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    rot = rot_y @ rot_x
    p0 = np.array([3.3, 2.1, 5.7])
    w = v @ rot.T + p0
    normal = rot[:, 2]
    for cell in (1.0, 1.7):
        out = SR.simplify(w, t, cell, origin=np.zeros(3))
        check_guarantees(w, t, out, cell, np.zeros(3))
        off = np.abs((out["vertices"] - p0) @ normal)
        print(f"cell {cell}: {len(out['vertices'])} representatives, off the plane by at most {off.max():.3e} cells x {cell}")
        assert len(out["vertices"]) > 10 and off.max() <= 1e-9 * cell
        # ... while they are not simply the means: the mean lies on the plane too, so compare in the plane -- the regulariser projects the mean
        assert not out["fell_back"].all()


def _cube_corner_mesh():
    """Three faces of an axis-aligned cube meeting at the corner (2.4, 2.6, 2.3), each a 0.25-spaced grid of 13 x 13 vertices running
    towards +; the faces do not share vertices (clustering joins them)."""
    corner = np.array([2.4, 2.6, 2.3])
    vs, ts, base = [], [], 0
    for axis in range(3):
        g, t = SR.grid_mesh(13, 13, spacing=0.25)
        p = np.zeros_like(g)
        p[:, (axis + 1) % 3], p[:, (axis + 2) % 3] = g[:, 0], g[:, 1]
        vs.append(p + corner)
        ts.append(t + base)
        base += len(g)
    return np.concatenate(vs), np.concatenate(ts).astype(np.int32), corner


def test_a_cube_corner_is_kept():
    v, t, corner = _cube_corner_mesh()
    cell = 1.0
    out = SR.simplify(v, t, cell, origin=np.zeros(3))
    check_guarantees(v, t, out, cell, np.zeros(3))
    j = int(np.nonzero((SR.key_cell(out["cluster_keys"][out["out_clusters"]]) == [2, 2, 2]).all(axis=1))[0][0])
    d_rule = np.sqrt(((out["vertices"][j] - corner) ** 2).sum())
    d_mean = np.sqrt(((out["means"][j] - corner) ** 2).sum())
    print(f"the corner's cluster: the representative is {d_rule:.3e} from the corner, the members' mean {d_mean:.3e}")
    assert not out["fell_back"][j] and d_rule <= 1e-2 * cell < d_mean
    # an edge cluster (the cell next to the corner along x): on the edge y = 2.6, z = 2.3
    e = int(np.nonzero((SR.key_cell(out["cluster_keys"][out["out_clusters"]]) == [4, 2, 2]).all(axis=1))[0][0])
    assert np.abs(out["vertices"][e][1:] - corner[1:]).max() <= 1e-2 * cell < np.abs(out["means"][e][1:] - corner[1:]).max()


def test_a_cell_larger_than_the_mesh_gives_an_empty_mesh():
    v, t = _mesh("sphere")
    out = SR.simplify(v, t, 64.0, ORIGIN)
    assert out["vertices"].shape == (0, 3) and out["triangles"].shape == (0, 3) and out["source"].shape == (0,)
    assert out["stats"]["collapsed_triangles"] == len(t) and len(out["cluster_keys"]) == 1
    none = SR.simplify(np.zeros((0, 3)), np.zeros((0, 3), np.int32), 1.0)
    assert none["vertices"].shape == (0, 3) and none["triangles"].shape == (0, 3)


def test_a_cell_smaller_than_every_edge_renumbers_the_input():
    v, t = SR.grid_mesh(9, 7)
    v = v.copy()
    v[:, 2] = 0.3 * np.sin(1.3 * v[:, 0]) * np.cos(0.7 * v[:, 1]) + 2.0
    v[:, :2] += 0.13
    cell = 0.7                                                  # below the grid's spacing 1: a cell per vertex
    out = SR.simplify(v, t, cell, origin=np.zeros(3))
    order = np.argsort(out["keys"], kind="stable")
    assert len(np.unique(out["keys"])) == len(v) and np.array_equal(out["source"], order)
    rank = np.empty(len(v), np.int64)
    rank[order] = np.arange(len(v))
    assert np.array_equal(out["triangles"], rank[t]) and out["survive"].all()
    d = np.abs(out["vertices"] - v[order]).max()
    print(f"one vertex per cell: the representatives are the vertices to {d:.3e} (cell {cell})")
    assert d <= 1e-12 * cell
    check_guarantees(v, t, out, cell, np.zeros(3))


def test_planted_inputs_take_every_branch():
    v, t, cell, origin = SR.planted_mesh()
    out = SR.simplify(v, t, cell, origin)
    check_guarantees(v, t, out, cell, origin)
    surv = out["survive"]
    assert surv[[0, 1, 2, 3, 4, 5, 6, 7, 10, 12, 13]].all() and not surv[[8, 9, 11]].any()      # repeated indices and shared cells collapse
    assert out["stats"]["collapsed_triangles"] == 3 and out["stats"]["duplicate_triangles"] == 4
    # of the five triangles on one set of three clusters the first is kept, with its own orientation
    tri0 = out["triangles"][0]
    assert np.array_equal(out["vertex_cluster"][t[0]], out["out_clusters"][tri0])
    assert len(out["triangles"]) == 7
    # boundary vertices belong to the cell above: 6 -> (2,2,2), 7 -> (3,2,2), 9 -> (3,3,3) with origin -2
    assert np.array_equal(SR.cells(v[[6, 7, 9]], cell, origin), [[2, 2, 2], [3, 2, 2], [3, 3, 3]])
    # the unreferenced vertex alone in its cell is a cluster but no output vertex; the one in vertex 0's cell counts in m
    lonely = out["vertex_cluster"][10]
    assert lonely not in out["out_clusters"]
    unused = set(range(len(out["cluster_keys"]))) - set(out["out_clusters"].tolist())      # ... like the two cells of the collapsed triangle
    assert unused == {int(lonely), int(out["vertex_cluster"][15]), int(out["vertex_cluster"][17])}
    j0 = int(np.nonzero(out["out_clusters"] == out["vertex_cluster"][0])[0][0])
    members = np.nonzero(out["vertex_cluster"] == out["vertex_cluster"][0])[0]
    assert members.tolist() == [0, 3, 11] and np.allclose(out["means"][j0], v[members].mean(axis=0), rtol=0, atol=1e-14)
    # the zero-area triangle's clusters hold no other surviving triangle except through vertices 12 and 13: cluster of 14 has tr = 0 -> the mean
    j14 = int(np.nonzero(out["out_clusters"] == out["vertex_cluster"][14])[0][0])
    assert out["fell_back"][j14] and np.array_equal(out["vertices"][j14], out["means"][j14]) and out["source"][j14] == 14
    # negative coordinates need the explicit origin: the default one is aligned to multiples of the cell and at or below the minimum
    assert np.array_equal(SR.default_origin(v, cell), [-2.0, -2.0, -2.0])
    assert np.array_equal(SR.default_origin(v, 0.75), [-2.25, -2.25, -2.25])
    again = SR.simplify(v, t, cell)
    assert np.array_equal(again["vertices"], out["vertices"]) and np.array_equal(again["triangles"], out["triangles"])
    with pytest.raises(ValueError, match="outside 0"):
        SR.simplify(v, t, cell, origin=np.zeros(3))            # a vertex below origin


def test_the_cluster_meshes_and_the_fan_have_the_shapes_the_gpu_tests_want():
    for n in (63, 64, 65, 257):
        v, t, cell, origin = SR.clusters_mesh(n)
        out = SR.simplify(v, t, cell, origin)
        assert len(out["cluster_keys"]) == n == len(out["out_clusters"])
        check_guarantees(v, t, out, cell, origin)
    v, t = SR.fan_mesh()
    out = SR.simplify(v, t, SR.FAN_CELL, np.zeros(3))
    assert out["survive"].all() and len(out["triangles"]) == 300 and len(out["vertices"]) == 301
    hub = int(np.nonzero(out["source"] == 0)[0][0])
    assert not out["fell_back"][hub] and np.abs(out["vertices"][hub] - v[0]).max() < 1e-9
    check_guarantees(v, t, out, SR.FAN_CELL, np.zeros(3))


def test_the_restatement_refuses_what_the_rule_excludes():
    v, t = SR.grid_mesh(3, 3)
    for bad in (dict(cell=0.0), dict(cell=-1.0), dict(cell=np.inf), dict(cell=np.nan), dict(cell=1.0, reg=0.0), dict(cell=1.0, reg=np.nan)):
        with pytest.raises(ValueError):
            SR.simplify(v, t, **bad)
    w = v.copy()
    w[4, 1] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        SR.simplify(w, t, 1.0)
    with pytest.raises(ValueError, match="triangle index"):
        SR.simplify(v, t + 1, 1.0)
    assert len(SR.simplify(v, t, 1e-6, origin=np.zeros(3))["cluster_keys"]) == 9       # (max - origin) / cell = 2 000 000 < 2^21
    with pytest.raises(ValueError, match="outside 0"):
        SR.simplify(v * 3.0, t, 1e-6, origin=np.zeros(3))      # 6 000 000 is not


# ------------------------------------------------------------------------------------------------------------------------------------
# the library's host side and the Python layers, without a GPU
# ------------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_report_bad_arguments_without_a_gpu():
    from gens_amd import lib as L
    lib = L.load()
    p = lambda k: C.c_void_p(0x1000 + 0x100 * k)  # noqa: E731  (never dereferenced: every call below is refused, or launches nothing)

    def refused(rc, *words, code=-1):
        msg = lib.gens_last_error().decode()
        assert rc == code and all(w in msg for w in words), (rc, msg)

    def keys(vertices=p(0), n=5, ox=0.0, oy=0.0, oz=0.0, cell=1.0, out=p(1)):
        return lib.gens_cluster_keys(vertices, n, ox, oy, oz, cell, out, None)

    refused(keys(vertices=None), "gens_cluster_keys", "null")
    refused(keys(out=None), "gens_cluster_keys", "null")
    refused(keys(n=-3), "gens_cluster_keys", "-3 vertices")
    refused(keys(n=1 << 31), "gens_cluster_keys", "below 2^31", code=-2)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        refused(keys(cell=bad), "gens_cluster_keys", "cell")
    refused(keys(oy=float("nan")), "gens_cluster_keys", "origin")
    refused(keys(oz=float("inf")), "gens_cluster_keys", "origin")
    assert keys(n=0, vertices=None, out=None) == 0

    def tris(triangles=p(0), n_t=4, vc=p(1), n_v=5, ranks=p(2), survive=p(3), triple=p(4)):
        return lib.gens_cluster_triangles(triangles, n_t, vc, n_v, ranks, survive, triple, None)

    for name in ("triangles", "vc", "ranks", "survive", "triple"):
        refused(tris(**{name: None}), "gens_cluster_triangles", "null")
    refused(tris(n_t=-1), "gens_cluster_triangles", "-1 triangles")
    refused(tris(n_v=-2), "gens_cluster_triangles", "-2 vertices")
    refused(tris(n_v=1 << 31), "gens_cluster_triangles", "below 2^31", code=-2)
    refused(tris(n_t=715827883), "gens_cluster_triangles", "below 2^31", code=-2)       # 3 T = 2^31 + 1
    refused(tris(n_t=1 << 62), "gens_cluster_triangles", "below 2^31", code=-2)
    assert tris(n_t=0, triangles=None, vc=None, ranks=None, survive=None, triple=None) == 0

    pointers = ("vertices", "triangles", "survive", "cluster_keys", "entries", "entry_start", "members", "member_start", "out_clusters", "out_vertices",
                "source", "fell_back")

    def solve(**kw):
        a = {**{name: p(k) for k, name in enumerate(pointers)}, "n_vertices": 9, "n_triangles": 4, "n_clusters": 5, "n_out": 3,
             "origin": (0.0, 0.0, 0.0), "cell": 1.0, "reg": 1e-3, **kw}
        args = L.ClusterSolveArgs(*[a[n] for n in pointers[:9]], a["n_vertices"], a["n_triangles"], a["n_clusters"], a["n_out"],
                                  (C.c_double * 3)(*a["origin"]), a["cell"], a["reg"], *[a[n] for n in pointers[9:]])
        return lib.gens_cluster_solve(C.byref(args), None)

    for name in pointers:
        refused(solve(**{name: None}), "gens_cluster_solve", "null")
    refused(lib.gens_cluster_solve(None, None), "gens_cluster_solve", "null")
    refused(solve(n_vertices=-1), "gens_cluster_solve", "-1 vertices")
    refused(solve(n_out=-1), "gens_cluster_solve", "-1 output clusters")
    refused(solve(n_vertices=1 << 31, n_clusters=5), "gens_cluster_solve", "below 2^31", code=-2)
    refused(solve(n_triangles=715827883), "gens_cluster_solve", "below 2^31", code=-2)
    refused(solve(n_clusters=10), "gens_cluster_solve", "10 clusters of 9 vertices")
    refused(solve(n_out=6), "gens_cluster_solve", "6 output clusters of 5 clusters")
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        refused(solve(cell=bad), "gens_cluster_solve", "cell")
        refused(solve(reg=bad), "gens_cluster_solve", "reg")
    refused(solve(origin=(0.0, float("nan"), 0.0)), "gens_cluster_solve", "origin")
    assert solve(n_out=0, **{name: None for name in pointers}) == 0
    assert solve(n_triangles=0, n_out=0) == 0
    assert lib.gens_abi_version() == 12
    assert L.SIGNATURES["gens_cluster_keys"][2] is C.c_double and len(L.SIGNATURES["gens_cluster_triangles"]) == 8
    assert C.sizeof(L.ClusterSolveArgs) == 9 * 8 + 4 * 8 + 5 * 8 + 3 * 8


def test_the_python_layers_refuse_bad_arguments_before_any_launch():
    from gens_amd import io as gio, ops
    from gens_amd.models.modules.implicit_surface import ImplicitSurface
    v, t = SR.grid_mesh(3, 3)
    # host tensors and arrays: there is no CPU path
    with pytest.raises(ValueError, match="no CPU path"):
        ops.simplify_mesh(torch.from_numpy(v), torch.from_numpy(t), 1.0)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.simplify_mesh(v, t, 1.0)
    assert ops.simplify_request("t", 2, 1e-3) == (2.0, 1e-3) and ops.simplify_request("t", np.float32(0.5)) == (0.5, 1e-3)
    for cell, reg in ((0, 1e-3), (-1.0, 1e-3), (float("inf"), 1e-3), (float("nan"), 1e-3), (True, 1e-3), ("two", 1e-3), (None, 1e-3), (1.0, 0.0),
                      (1.0, -1e-3), (1.0, float("nan")), (1.0, float("inf")), (1.0, False)):
        with pytest.raises(ValueError):
            ops.simplify_request("t", cell, reg)
    assert ops.simplify_origin([-1.5, 0.2, 3.0], 0.75) == [-1.5, 0.0, 3.0] and ops.simplify_origin([-1.6, 0.8, 2.9], 0.75) == [-2.25, 0.75, 2.25]
    # extract_geometry's option: None, False and 0 are off; a positive finite number is the cell edge; anything else is refused
    surf = types.SimpleNamespace(mesh_simplify=None)
    req = lambda x: ImplicitSurface._simplify_request(surf, x)  # noqa: E731
    assert ImplicitSurface.mesh_simplify is None and ImplicitSurface.last_simplify_stats is None
    assert req(None) is None and req(False) is None and req(0) is None and req(0.0) is None
    assert req(2) == 2.0 and req(1.5) == 1.5
    surf.mesh_simplify = 3
    assert req(None) == 3.0 and req(0) is None and req(False) is None and req(2) == 2.0
    for bad in (True, -1, float("nan"), float("inf"), "2x"):
        with pytest.raises(ValueError):
            req(bad)
    # io.simplify_mesh: attribute lengths, index range and cell, before the device is looked at
    with pytest.raises(ValueError, match="normals has 4 rows"):
        gio.simplify_mesh(v, t, 1.0, normals=np.zeros((4, 3), np.float32))
    with pytest.raises(ValueError, match="triangle indices"):
        gio.simplify_mesh(v, t + 1, 1.0)
    with pytest.raises(ValueError, match="cell"):
        gio.simplify_mesh(v, t, 0.0)
    with pytest.raises(ValueError, match="reg"):
        gio.simplify_mesh(v, t, 1.0, reg=-1.0)
