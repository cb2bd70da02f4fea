"""CPU tests of the mesh fairing rules (K39) on the numpy restatement (tests/mesh_smooth_reference.py) alone -- a flat lattice sheet does not
move, Taubin smoothing keeps the volume of a noisy sphere where plain Laplacian smoothing loses it, and halves its roughness; pinned and
unreferenced vertices, iterations = 0 and the triangles keep their bits -- and of the host side: the entry points' argument checks, the
Python layers' refusals before any launch, the command line's argument errors."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from . import mesh_repair_reference as RR
from . import mesh_smooth_reference as SR
from . import mesh_topology_reference as TR

KINDS = ("uniform", "cotangent")


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def _ball(kind, iterations, lam, mu):
    v, t, _ = SR.noisy_icosphere()
    return SR.smooth(v, t, iterations=iterations, lam=lam, mu=mu, weights=kind, measure=True)


def test_the_neighbours_are_the_edges_ends_in_ascending_order():
    v, t = TR.two_tetrahedra_edge()                                  # a non-manifold edge: it counts once
    topo = TR.topology(v, t, normals=False)
    start, vertex, edge = SR.neighbours(topo["edges"], len(v))
    assert len(vertex) == len(edge) == 2 * len(topo["edges"]) and start[0] == 0 and start[-1] == len(vertex)
    for i in range(len(v)):
        mine = vertex[start[i]:start[i + 1]].tolist()
        assert mine == sorted(set(mine)) and i not in mine
        for j, e in zip(mine, edge[start[i]:start[i + 1]].tolist()):
            assert topo["edges"][e].tolist() == [min(i, j), max(i, j)]
    bv, bt = TR.book(5)
    nb = SR.neighbours(TR.topology(bv, bt, normals=False)["edges"], len(bv))
    assert nb[1][nb[0][0]:nb[0][1]].tolist() == [1, 2, 3, 4, 5, 6]                 # the spine's 5 uses: one neighbour


@pytest.mark.parametrize("kind", KINDS)
def test_a_flat_lattice_sheet_does_not_move(kind):
    v, t = SR.lattice_sheet(9)
    out = SR.smooth(v, t, iterations=3, weights=kind)
    assert (out["vertices"] - v == 0.0).all() and out["stats"]["moved"] == 0 and out["stats"]["displacement_max"] == 0.0
    assert out["stats"]["pinned"] == 32 and out["pinned"].sum() == 32
    if kind == "cotangent":                                          # the diagonals face two right angles: weight exactly 0
        assert (out["weight"] == 0.0).sum() == 64 and (out["weight"] >= 0.0).all()
        inner = np.array([e for e in range(len(out["weight"])) if not out["pinned"][out["topology"]["edges"][e]].any()])
        assert set(out["weight"][inner].tolist()) == {0.0, 2.0}                       # two angles of 45 degrees face an axis edge


@pytest.mark.parametrize("kind", KINDS)
def test_taubin_keeps_the_volume_that_plain_smoothing_loses_and_halves_the_roughness(kind):
    v, t, clean = SR.noisy_icosphere()
    assert v.shape == (642, 3) and t.shape == (1280, 3)
    clean_volume = TR.topology(clean, t, normals=False)["report"]["volume"]
    taubin = _ball(kind, 10, 0.5, -0.53)["stats"]
    plain = _ball(kind, 20, 0.5, 0)["stats"]
    print(kind, "taubin", taubin["volume_after"] / clean_volume, "plain", plain["volume_after"] / clean_volume, "rms",
          taubin["roughness_before"]["rms"], "->", taubin["roughness_after"]["rms"])
    assert 0.98 <= taubin["volume_after"] / clean_volume <= 1.02
    assert plain["volume_after"] / clean_volume < 0.80
    assert taubin["roughness_after"]["rms"] < 0.5 * taubin["roughness_before"]["rms"]
    assert taubin["roughness_before"]["edges"] == 1920 and taubin["pinned"] == 0 and taubin["moved"] == 642
    assert set(taubin) == set(SR.STAT_KEYS) | set(SR.MEASURE_KEYS)
    assert taubin["displacement_max"] >= taubin["displacement_rms"] >= taubin["displacement_mean"] > 0.0


@pytest.mark.parametrize("kind", KINDS)
def test_zero_iterations_pins_unreferenced_vertices_and_triangles(kind):
    v, t = SR.unreferenced_tail(257)
    zero = SR.smooth(v, t, iterations=0, weights=kind, fix_boundary=False)
    assert _same(zero["vertices"], v) and zero["stats"]["moved"] == 0 and _same(zero["triangles"], t)
    pinned = np.zeros(len(v), dtype=bool)
    pinned[[3, 4, 9]] = True
    out = SR.smooth(v, t, iterations=4, weights=kind, fix_boundary=False, pinned=pinned)
    assert _same(out["vertices"][pinned], v[pinned]) and _same(out["vertices"][22:], v[22:]) and _same(out["triangles"], t)
    assert np.signbit(out["vertices"][22]).tolist() == [True, False, True]                 # a -0.0 stays a -0.0
    assert out["stats"]["pinned"] == 3 and 0 < out["stats"]["moved"] <= 22 - 3
    fixed = SR.smooth(v, t, iterations=4, weights=kind)              # every vertex of a strip is on its boundary
    assert _same(fixed["vertices"], v) and fixed["stats"]["pinned"] == 22 and np.isnan(fixed["stats"]["displacement_max"])
    dv, dt = RR.disk(65)
    disk = SR.smooth(dv, dt, iterations=2, weights=kind)
    assert _same(disk["vertices"][1:], dv[1:]) and disk["stats"]["moved"] <= 1 and disk["stats"]["pinned"] == 65


def test_a_step_is_a_convex_combination_and_the_weights_are_clamped():
    v, t = RR.clustered_sphere()
    out = SR.smooth(v, t, iterations=1, mu=0, lam=1.0, weights="cotangent", fix_boundary=False)
    assert (out["weight"] >= 0.0).all() and np.isfinite(out["weight"]).all()
    lo, hi = v.min(axis=0), v.max(axis=0)
    assert (out["vertices"] >= lo - 1e-12).all() and (out["vertices"] <= hi + 1e-12).all()
    obtuse = np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [2.0, 0.1, 0.0]]), np.array([[0, 1, 2]], np.int32)
    w = SR.smooth(*obtuse, iterations=0, weights="cotangent")["weight"]
    assert w[0] == 0.0 and (w[1:] > 0.0).all()                       # the edge opposite the obtuse angle: clamped


def test_the_dihedral_angle_of_a_cube_and_of_other_edges():
    v, t = TR.cube()
    topo = TR.topology(v, t, normals=True)
    angle = SR.dihedral(topo)
    assert np.isfinite(angle).all() and len(angle) == 18
    assert sorted(np.round(angle / (np.pi / 2), 12).tolist()) == [0.0] * 6 + [1.0] * 12
    rep = SR.roughness_report(angle)
    assert rep["edges"] == 18 and rep["max"] == pytest.approx(np.pi / 2, abs=1e-14) and rep["mean"] == pytest.approx(np.pi / 3, abs=1e-14)
    sv, st = TR.strip(4)
    a = SR.dihedral(TR.topology(sv, st, normals=True))
    assert np.isnan(a).sum() == 6 and np.isfinite(a).sum() == 3                           # boundary edges have none
    assert SR.roughness_report(np.full(3, np.nan)) == pytest.approx({"edges": 0, "mean": np.nan, "rms": np.nan, "max": np.nan}, nan_ok=True)
    bv, bt = TR.book(3)
    assert np.isnan(SR.dihedral(TR.topology(bv, bt, normals=True))).all()                  # class 1 and class 4 only


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

    who, fn = "gens_mesh_corner_cot", lib.gens_mesh_corner_cot
    ok = [p(0), p(1), 4, 4, p(2), None]
    nulls(fn, ok, (0, 1, 4), who)
    refused(fn(*edit(ok, a2=-4)), who, "-4 vertices")
    refused(fn(*edit(ok, a3=-1)), who, "-1 faces")
    refused(fn(*edit(ok, a2=big)), who, "below 2^31", code=-2)
    refused(fn(*edit(ok, a3=(big + 2) // 3)), who, "below 2^31", code=-2)
    assert fn(None, None, 4, 0, None, None) == 0

    who, fn = "gens_mesh_edge_weights", lib.gens_mesh_edge_weights
    ok = [p(0), p(1), p(2), 5, 9, p(3), None]
    nulls(fn, ok, (0, 1, 2, 5), who)
    refused(fn(*edit(ok, a3=-5)), who, "-5 edges")
    refused(fn(*edit(ok, a4=-3)), who, "-3 half-edges")
    refused(fn(*edit(ok, a4=10)), who, "three per face")
    refused(fn(*edit(ok, a3=10)), who, "an edge has a use")
    refused(fn(*edit(ok, a4=big + 1)), who, "below 2^31", code=-2)
    assert fn(None, None, None, 0, 9, None, None) == 0

    who, fn = "gens_mesh_laplacian_step", lib.gens_mesh_laplacian_step
    ok = [p(0), 4, p(1), p(2), p(3), 10, p(4), 5, p(5), 0.5, p(6), p(7), p(8), None]
    nulls(fn, ok, (0, 2, 3, 4), who)
    refused(fn(*edit(ok, a1=-4)), who, "-4 vertices")
    refused(fn(*edit(ok, a5=-10)), who, "-10 neighbours")
    refused(fn(*edit(ok, a7=-5)), who, "-5 edges")
    refused(fn(*edit(ok, a5=9)), who, "an edge has two ends")
    refused(fn(*edit(ok, a1=big)), who, "below 2^31", code=-2)
    refused(fn(*edit(ok, a5=big, a7=big // 2)), who, "below 2^31", code=-2)
    for bad in (float("nan"), 1.5, -2.5, float("inf")):
        refused(fn(*edit(ok, a9=bad)), who, "factor")
    refused(fn(*edit(ok, a10=p(0))), who, "out == in")               # a step reads one buffer and writes another
    refused(fn(*edit(ok, a11=p(0))), who, "out == in")
    refused(fn(*edit(ok, a12=p(0))), who, "out == in")               # (neighbours read `in`: no output may be it)
    for pair in ({"a10": p(7)}, {"a10": p(8)}, {"a11": p(8)}):
        refused(fn(*edit(ok, **pair)), who, "two outputs share a buffer")
    refused(fn(*edit(ok, a10=None, a11=None, a12=None)), who, "no output")
    assert fn(None, 0, None, None, None, 10, None, 5, None, 0.5, None, None, None, None) == 0

    who, fn = "gens_mesh_dihedral", lib.gens_mesh_dihedral
    ok = [p(0), 3, p(1), p(2), 5, p(3), None]
    nulls(fn, ok, (0, 2, 3, 5), who)
    refused(fn(*edit(ok, a1=-3)), who, "-3 faces")
    refused(fn(*edit(ok, a4=-5)), who, "-5 edges")
    refused(fn(*edit(ok, a4=10)), who, "an edge has a use")
    refused(fn(*edit(ok, a1=big)), who, "below 2^31", code=-2)
    assert fn(None, 3, None, None, 0, None, None) == 0
    assert lib.gens_abi_version() == 12
    for name, n_args in (("gens_mesh_corner_cot", 6), ("gens_mesh_edge_weights", 7), ("gens_mesh_laplacian_step", 14), ("gens_mesh_dihedral", 7)):
        assert len(L.SIGNATURES[name]) == n_args and set(L.SIGNATURES[name]) <= {C.c_void_p, C.c_int64, C.c_double}


BAD_OPTIONS = [{"iterations": -1}, {"iterations": 1001}, {"iterations": 2.0}, {"iterations": True}, {"lam": 0}, {"lam": 1.5}, {"lam": "0.5"},
               {"lam": float("nan")}, {"mu": 0.3}, {"mu": -0.5}, {"mu": -2.5}, {"mu": None}, {"mu": -0.3, "lam": 0.3}, {"weights": "cot"},
               {"weights": 1}, {"fix_boundary": 1}, {"measure": "yes"}, {"rounds": 3}, {"pinned": None}]


def test_the_python_layers_refuse_bad_arguments_before_any_launch(tmp_path):
    from gens_amd import io as gio, ops, smooth_mesh as cli
    from gens_amd.models.modules.implicit_surface import ImplicitSurface
    v, t = TR.cube()
    host_v, host_t = torch.from_numpy(v), torch.from_numpy(t)
    for fn in (ops.smooth_mesh, ops.mesh_laplacian, ops.mesh_roughness):
        with pytest.raises(ValueError, match="no CPU path"):
            fn(host_v, host_t)
        with pytest.raises(ValueError, match="no CPU path"):
            fn(v, t)
    with pytest.raises(ValueError, match="MeshTopology"):
        ops.smoothing_weights(None, "uniform")
    with pytest.raises(ValueError, match="weights"):
        ops.smoothing_weights(None, "cot")
    defaults = {"iterations": 10, "lam": 0.5, "mu": -0.53, "weights": "uniform", "fix_boundary": True, "measure": False}
    assert ops.smooth_request(True) == ops.smooth_request({}) == defaults and tuple(defaults) == ops.SMOOTH_KEYS
    assert ops.smooth_request({"mu": 0, "lam": 1, "iterations": 1000, "weights": "cotangent"}) == {**defaults, "mu": 0.0, "lam": 1.0, "iterations": 1000,
                                                                                                   "weights": "cotangent"}
    assert ops.smooth_request({"mu": -2, "lam": 1.0})["mu"] == -2.0
    for bad in BAD_OPTIONS:
        with pytest.raises(ValueError, match="lam|mu" if len(bad) == 2 else next(iter(bad))):
            ops.smooth_request(bad)
        if "pinned" not in bad:
            with pytest.raises(ValueError):
                gio.smooth_mesh(v, t, **bad)                                         # (before the device is looked at)
    for bad in (None, False, 1, "yes", 2.5, [], {1: 2}):
        with pytest.raises(ValueError):
            ops.smooth_request(bad)
    # extract_geometry's option: None and False are off, True the defaults, a dict the keywords
    surf = types.SimpleNamespace(mesh_smooth=None)
    req = lambda x: ImplicitSurface._smooth_request(surf, x)  # noqa: E731
    assert ImplicitSurface.mesh_smooth is None and ImplicitSurface.last_smooth_stats is None
    assert req(None) is None and req(False) is None and req(True) == defaults and req({"iterations": 3})["iterations"] == 3
    surf.mesh_smooth = {"weights": "cotangent"}
    assert req(None)["weights"] == "cotangent" and req(False) is None and req(True)["weights"] == "uniform"
    for bad in (1, 0, "yes", 2.5, [], {1: 2}) + tuple(BAD_OPTIONS):
        with pytest.raises(ValueError):
            req(bad)
    # the host entry point
    with pytest.raises(ValueError, match="expected"):
        gio.smooth_mesh(v[:, :2], t)
    with pytest.raises(ValueError, match="whole numbers"):
        gio.smooth_mesh(v, t.astype(np.float64))
    with pytest.raises(ValueError, match="int32"):
        gio.smooth_mesh(v, t.astype(np.int64) + 2 ** 31)
    with pytest.raises(ValueError, match="normals are not carried"):
        gio.smooth_mesh(v, t, normals=np.zeros((8, 3)))
    with pytest.raises(ValueError, match="colors has 7 rows"):
        gio.smooth_mesh(v, t, colors=np.zeros((7, 3), np.uint8))
    with pytest.raises(ValueError, match="pinned has 7 rows"):
        gio.smooth_mesh(v, t, pinned=np.zeros(7, dtype=bool))
    with pytest.raises(ValueError, match="pinned is"):
        gio.smooth_mesh(v, t, pinned=np.zeros(8))
    with pytest.raises(ValueError, match="roughness"):
        gio.mesh_report(v, t, roughness=1)
    path = str(tmp_path / "a.ply")
    gio.write_ply(path, v, t)
    out = str(tmp_path / "b.ply")
    assert cli.main([str(tmp_path / "missing.ply"), out]) == 2 and cli.main([str(tmp_path), out]) == 2
    for bad in (["--iterations", "-1"], ["--iterations", "1001"], ["--lambda", "0"], ["--lambda", "1.5"], ["--mu", "0.3"], ["--mu", "-0.4"],
                ["--weights", "cot"]):
        assert cli.main([path, out] + bad) == 2, bad
    with pytest.raises(SystemExit):
        cli.main([path, out, "--iterations", "2.5"])


def test_extract_geometry_refuses_a_bad_smooth_option_before_any_launch():
    from gens_amd.config import Conf, gens_model_conf
    from gens_amd.models.gens import GenS
    from gens_amd.models.modules.implicit_surface import ImplicitSurface
    surf = ImplicitSurface(gens_model_conf(volume_dims=(16, 8, 4))["implicit_surface"])
    lo, hi = torch.full((3,), -1.0), torch.full((3,), 1.0)
    for bad in (1, "yes", {"rounds": 3}, {"mu": 0.3}, {"iterations": 1001}):
        with pytest.raises(ValueError, match="smooth|mu|iterations"):
            surf.extract_geometry([], lo, hi, 8, 0.0, smooth=bad)
        with pytest.raises(ValueError, match="smooth|mu|iterations"):
            surf.validate(*[None] * 11, lo, hi, (4, 4), mesh_smooth=bad)
    assert surf.last_smooth_stats is None
    conf = gens_model_conf(volume_dims=(16, 8, 4), has_vol=True)
    assert "mesh_smooth" not in vars(GenS(conf).implicit_surface)
    assert GenS(Conf({**conf, "mesh_smooth": True})).implicit_surface.mesh_smooth is True
    assert GenS(Conf({**conf, "mesh_smooth": {"iterations": 3}})).implicit_surface.mesh_smooth == {"iterations": 3}


def test_the_topology_report_is_what_it_was():
    """area_volume is report()'s own expression, factored out: on the host the same tensors give the same bits either way."""
    from gens_amd import ops
    v, t = (torch.from_numpy(x) for x in SR.noisy_icosphere()[:2])
    valid = torch.ones(len(t), dtype=torch.bool)
    valid[5] = False
    a, b, c = (v[torch.where(valid, t[:, k], torch.zeros_like(t[:, k])).long()] for k in range(3))
    keep = valid.to(torch.float64)
    area = (0.5 * torch.linalg.cross(b - a, c - a).square().sum(dim=1).sqrt() * keep).sum()
    volume = ((a * torch.linalg.cross(b, c)).sum(dim=1) * keep).sum() / 6.0
    got = ops.area_volume(v, t, valid)
    assert got[0].item() == area.item() and got[1].item() == volume.item()
