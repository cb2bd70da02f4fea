"""GPU tests of the mesh fairing (K39) against the numpy restatement (tests/mesh_smooth_reference.py): neighbour lists, pinned mask and counts
exactly; positions, Laplacians and weight sums bit for bit (with cotangent weights: against the restatement's step fed the device's
weights, and the weights themselves to 8 ulp of the sum of their terms); dihedral angles to 1e-12; displacement figures, area and volume to
1e-12 relative (eight open shapes whose volume cancels: see OPEN_VOLUME); neighbour walks across wave sizes (a cone apex, a disk's hub), long half-edge runs (a book's spine), invalid faces and
non-manifold edges (soups), empty meshes and unreferenced vertices; the topology is untouched; io.smooth_mesh and the command line in a
child process; extract_geometry(smooth=) on the g23 model on the three lattice routes; nothing changes when the option is unset; the
refusals."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from . import mesh_repair_reference as RR
from . import mesh_smooth_reference as SR
from . import mesh_topology_reference as TR

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K39 = {"gens_mesh_corner_cot", "gens_mesh_edge_weights", "gens_mesh_laplacian_step", "gens_mesh_dihedral"}
KINDS = ("uniform", "cotangent")
COUNTS = ("vertices", "vertices_referenced", "faces", "faces_invalid", "edges", "edges_boundary", "edges_manifold", "edges_flipped",
          "edges_nonmanifold", "vertices_pinched", "vertices_nonmanifold", "components", "largest_component_faces", "boundary_components", "euler",
          "closed", "oriented", "manifold", "watertight", "genus")
MODEL_SMOOTH = {"iterations": 3, "measure": True}


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _up(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _close(got, want, rel=1e-12):
    return (np.isnan(got) and np.isnan(want)) or abs(got - want) <= rel * abs(want)


@functools.lru_cache(maxsize=None)
def _cases():
    """name -> (vertices, triangles, fix_boundary)."""
    out = {name: (v, t, True) for name, (v, t, _) in RR.hand_cases().items()}
    for n in (63, 64, 65, 257):
        out[f"cones {n}"] = (*RR.cones(n), False)
    out["book 65"] = (*TR.book(65), False)
    for n in (63, 64, 65, 1000):
        out[f"disk {n}"] = (*RR.disk(n), True)
        out[f"disk {n} free"] = (*RR.disk(n), False)
    out["strip 1000"] = (*RR.strip_alternating(1000), True)
    out["strip 1000 free"] = (*RR.strip_alternating(1000), False)
    out["islands 65"] = (*RR.islands(65), False)
    out["clustered sphere"] = (*RR.clustered_sphere(), True)
    for seed in (2, 6, 9, 10, 35):
        out[f"soup {seed}"] = (*RR.random_soup(seed), seed % 2 == 0)
    out["noisy icosphere"] = (*SR.noisy_icosphere()[:2], True)
    out["one vertex"] = (np.array([[1.0, -0.0, 2.0]]), np.zeros((0, 3), np.int32), True)
    out["unreferenced tail"] = (*SR.unreferenced_tail(257), False)
    return out


CASE_NAMES = tuple(RR.hand_cases()) + tuple(f"cones {n}" for n in (63, 64, 65, 257)) + ("book 65",) + tuple(
    f"disk {n}{free}" for n in (63, 64, 65, 1000) for free in ("", " free")) + ("strip 1000", "strip 1000 free", "islands 65", "clustered sphere") + tuple(
    f"soup {s}" for s in (2, 6, 9, 10, 35)) + ("noisy icosphere", "one vertex", "unreferenced tail")


@functools.lru_cache(maxsize=None)
def _want_topology(name):
    v, t, _ = _cases()[name]
    return TR.topology(v, t, normals=True)


def _volume_scale(vertices, triangles, valid):
    """The sum over the valid faces of |a| . (|b| x' |c|) / 6, with x' the cross product with its differences made sums: the magnitudes
    that the six products of every a . (b x c) have before they cancel."""
    t = np.asarray(triangles).reshape(-1, 3)[np.asarray(valid, dtype=bool)]
    a, b, c = (np.abs(np.asarray(vertices)[t[:, k]]) for k in range(3))
    cross = np.stack([b[:, 1] * c[:, 2] + b[:, 2] * c[:, 1], b[:, 2] * c[:, 0] + b[:, 0] * c[:, 2], b[:, 0] * c[:, 1] + b[:, 1] * c[:, 0]], axis=1)
    return float((a * cross).sum() / 6.0)


# The open shapes whose "volume" cancels: name -> the largest |difference| between ops.smooth_mesh's figure and the restatement's that was
# measured, with the figure.  A volume is a sum of a . (b x c) over the faces; on these meshes, none of them closed, it is what is left of
# products many times its size (a strip with coordinates up to 10^4; fans, cones and a book whose hub or spine sits at the origin, so that
# every term is nearly 0), torch adds the terms as a tree and the restatement one after the other, and no two orders agree to 1e-12 of the
# remainder -- a book's 0 against 4e-19 meets no relative bound at all.  For these, and for these alone, the bound is 1e-12 of the figure plus
# 2^-50 of the magnitudes that cancel (_volume_scale).  Every other case, the closed meshes and the model among them, is held to 1e-12 of
# the figure; the largest relative difference measured there is 8.9e-13 (strip 1000, boundary fixed), then 8.9e-14.
OPEN_VOLUME = {"cones 63": (1.9e-17, 4.76e-06), "cones 64": (1.2e-17, 4.94e-06), "cones 65": (1.9e-17, 5.13e-06), "cones 257": (5.4e-18, 1.26e-06),
               "book 65": (7.2e-20, 4.5e-20), "disk 65": (1.6e-35, 6.4e-35), "strip 1000 free": (1.5e-10, -0.831), "islands 65": (1.8e-11, -4.08)}


def _check_stats(got, want, name, volume_scale=None):
    """Counts exactly; displacement figures, area and volume to 1e-12 of the figure.  volume_scale (before, after), given for the cases
    of OPEN_VOLUME alone: 2^-50 of it is added to the volume's bound (see there)."""
    assert tuple(got)[:7] == SR.STAT_KEYS and set(got) == set(want), (name, got)
    for k in ("iterations", "weights", "pinned", "moved"):
        assert got[k] == want[k] and type(got[k]) is type(want[k]), (name, k, got[k], want[k])
    for k in ("displacement_max", "displacement_mean", "displacement_rms"):
        assert _close(got[k], want[k]), (name, k, got[k], want[k])
    if "area_before" in want:
        for k in ("area_before", "area_after"):
            assert _close(got[k], want[k]), (name, k, got[k], want[k])
        for k, scale in zip(("volume_before", "volume_after"), volume_scale or (0.0, 0.0)):
            bound = 1e-12 * abs(want[k]) + 2.0 ** -50 * scale
            print(f"{name}: {k} {got[k]!r} against {want[k]!r}, |difference| {abs(got[k] - want[k]):.3e}, bound {bound:.3e}")
            assert abs(got[k] - want[k]) <= bound, (name, k, got[k], want[k], scale)
        for k in ("roughness_before", "roughness_after"):
            assert tuple(got[k]) == ("edges", "mean", "rms", "max") and got[k]["edges"] == want[k]["edges"], (name, k, got[k], want[k])
            for f in ("mean", "rms", "max"):            # each is 1-Lipschitz in the largest error of an angle
                assert (np.isnan(got[k][f]) and np.isnan(want[k][f])) or abs(got[k][f] - want[k][f]) <= 1e-12, (name, k, f, got[k], want[k])


@gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_every_output_equals_the_restatement(name):
    from gens_amd import ops
    v, t, fix = _cases()[name]
    want_topo = _want_topology(name)
    dv, dt = _up(v, np.float64), _up(t, np.int32)
    topo = ops.mesh_topology(dv, dt, normals=True)
    before = topo.report()
    # 1: the neighbour lists and the pinned mask
    nbrs = SR.neighbours(want_topo["edges"], len(v))
    for got, want in zip(ops.mesh_neighbours(topo), nbrs):
        assert _same(got.cpu().numpy(), want), name
    assert _same(((topo.vertex_flags & 2) != 0).cpu().numpy(), (want_topo["vertex_flags"] & 2) != 0)
    # 2: the weights
    uniform = ops.smoothing_weights(topo, "uniform").cpu().numpy()
    assert _same(uniform, np.ones(len(want_topo["edges"])))
    device_w = ops.smoothing_weights(topo, "cotangent").cpu().numpy()
    want_w, mag = SR.edge_weights(want_topo, SR.corner_cot(v, t, want_topo["face_valid"]), "cotangent")
    bound = 8.0 * 2.0 ** -52 * mag
    assert device_w.shape == want_w.shape and (np.abs(device_w - want_w) <= bound).all() and (device_w >= 0.0).all(), name
    print(f"{name}: {len(v)} vertices, {len(want_w)} edges; cotangent weights {'identical' if _same(device_w, want_w) else 'within the bound'}")
    # 3: the Laplacian
    for kind, w in (("uniform", uniform), ("cotangent", device_w)):
        delta, wsum = ops.mesh_laplacian(dv, dt, weights=kind, topology=topo)
        want_delta, want_sum, _ = SR.laplacian(v, nbrs, w)
        assert _same(delta.cpu().numpy(), want_delta) and _same(wsum.cpu().numpy(), want_sum), (name, kind)
    # 7: the dihedral angles
    angle, rough = ops.mesh_roughness(dv, dt, topology=topo)
    angle, want_angle = angle.cpu().numpy(), SR.dihedral(want_topo)
    assert _same(np.isnan(angle), np.isnan(want_angle)), name
    err = np.abs(angle - want_angle)[np.isfinite(want_angle)].max(initial=0.0)
    print(f"{name}: {int(np.isfinite(want_angle).sum())} dihedral angles, max error {err:.3e}")
    assert err <= 1e-12, (name, err)
    want_rough = SR.roughness_report(want_angle)
    assert rough["edges"] == want_rough["edges"] and all(_close(rough[k], want_rough[k], 1e-12) or abs(rough[k] - want_rough[k]) <= 1e-12
                                                        for k in ("mean", "rms", "max")), (name, rough, want_rough)
    plain_angle = ops.mesh_roughness(dv, dt)[0]                      # (its own topology; a topology without normals)
    assert torch.equal(plain_angle.isnan(), torch.from_numpy(np.isnan(want_angle)).cuda())
    assert torch.equal(ops.mesh_roughness(dv, dt, topology=ops.mesh_topology(dv, dt))[0].nan_to_num(-1.0), plain_angle.nan_to_num(-1.0))
    # 4 - 6, 8: the smoothing
    for kind, w in (("uniform", None), ("cotangent", device_w)):
        for iterations in (0, 1, 10):
            for mu in (0, -0.53):
                if iterations == 0 and mu == 0:
                    continue
                measure = iterations == 10 and mu != 0
                kw = {"iterations": iterations, "mu": mu, "weights": kind, "fix_boundary": fix, "measure": measure}
                got_v, got_t, stats = ops.smooth_mesh(dv, dt, topology=topo if iterations else None, **kw)
                want = SR.smooth(v, t, weight_override=w, topology=want_topo, **kw)
                tag = (name, kind, iterations, mu)
                assert got_t is dt and _same(got_v.cpu().numpy(), want["vertices"]), tag          # bit for bit
                valid = want_topo["face_valid"]
                cancels = measure and name in OPEN_VOLUME
                assert not (cancels and want_topo["report"]["watertight"])                        # (an open shape)
                _check_stats(stats, want["stats"], tag, (_volume_scale(v, t, valid), _volume_scale(want["vertices"], t, valid)) if cancels else None)
                if iterations == 0:
                    assert got_v is not dv and (len(v) == 0 or got_v.data_ptr() != dv.data_ptr()) and stats["moved"] == 0      # a copy
                if measure and len(t):
                    after = ops.mesh_topology(got_v, dt).report()
                    assert all(after[k] == before[k] for k in COUNTS), tag                         # the topology is untouched


@gpu
def test_what_the_walk_shapes_are_there_for():
    for n in (63, 64, 65, 257):
        start = SR.neighbours(_want_topology(f"cones {n}")["edges"], 2 * n + 1)[0]
        assert start[1] - start[0] == 2 * n                           # the apex walks 2 n neighbours
    book = _want_topology("book 65")
    assert book["edge_count"][0] == 65 and book["edge_class"][0] == 4 and SR.neighbours(book["edges"], 67)[0][1] == 66
    for n in (63, 64, 65, 1000):
        assert SR.neighbours(_want_topology(f"disk {n}")["edges"], n + 1)[0][1] == n
        v, t, _ = _cases()[f"disk {n}"]
        assert SR.smooth(v, t, iterations=1, mu=0, topology=_want_topology(f"disk {n}"))["stats"]["pinned"] == n
    assert sum(_want_topology(f"soup {s}")["report"]["faces_invalid"] for s in (2, 6, 9, 10, 35)) > 0
    assert sum(_want_topology(f"soup {s}")["report"]["edges_nonmanifold"] for s in (2, 6, 9, 10, 35)) > 0
    tail = _want_topology("unreferenced tail")
    assert tail["report"]["vertices"] == 257 and tail["report"]["vertices_referenced"] == 22 and tail["report"]["faces_invalid"] == 1
    assert len(_cases()["strip 1000"][0]) > 256 * 3 and len(_want_topology("disk 1000")["edges"]) > 256 * 7


@gpu
def test_the_same_bits_twice_and_the_callers_pins():
    from gens_amd import ops
    v, t, _ = _cases()["noisy icosphere"]
    dv, dt = _up(v, np.float64), _up(t, np.int32)
    pinned = np.zeros(len(v), dtype=bool)
    pinned[::7] = True
    for kind in KINDS:
        a = ops.smooth_mesh(dv, dt, weights=kind, pinned=_up(pinned, np.bool_))
        b = ops.smooth_mesh(dv, dt, weights=kind, pinned=_up(pinned, np.bool_))
        assert torch.equal(a[0], b[0]) and a[2] == b[2] and a[2]["pinned"] == int(pinned.sum())
        assert _same(a[0].cpu().numpy()[pinned], v[pinned]) and a[2]["moved"] == len(v) - int(pinned.sum())
        w = ops.smoothing_weights(ops.mesh_topology(dv, dt), kind).cpu().numpy()
        want = SR.smooth(v, t, weights=kind, pinned=pinned, weight_override=w, topology=_want_topology("noisy icosphere"))
        assert _same(a[0].cpu().numpy(), want["vertices"]), kind
        # only a topology's connectivity is used: the unsmoothed mesh's serves the smoothed vertices
        old = ops.mesh_topology(dv, dt, normals=True)
        with_old, alone = ops.smooth_mesh(a[0], dt, weights=kind, measure=True, topology=old), ops.smooth_mesh(a[0], dt, weights=kind, measure=True)
        assert torch.equal(with_old[0], alone[0]) and with_old[2] == alone[2], kind
        assert torch.equal(ops.mesh_roughness(a[0], dt, topology=old)[0], ops.mesh_roughness(a[0], dt)[0])
        assert all(torch.equal(x, y) for x, y in zip(ops.mesh_laplacian(a[0], dt, weights=kind, topology=old), ops.mesh_laplacian(a[0], dt, weights=kind)))


@gpu
def test_the_noisy_sphere_is_faired_on_the_device():
    from gens_amd import ops
    v, t, clean = SR.noisy_icosphere()
    clean_volume = TR.topology(clean, t, normals=False)["report"]["volume"]
    dv, dt = _up(v, np.float64), _up(t, np.int32)
    for kind in KINDS:
        taubin = ops.smooth_mesh(dv, dt, weights=kind, measure=True)[2]
        plain = ops.smooth_mesh(dv, dt, iterations=20, mu=0, weights=kind, measure=True)[2]
        print(kind, json.dumps(taubin), plain["volume_after"] / clean_volume)
        assert 0.98 <= taubin["volume_after"] / clean_volume <= 1.02 and plain["volume_after"] / clean_volume < 0.80
        assert taubin["roughness_after"]["rms"] < 0.5 * taubin["roughness_before"]["rms"]


@gpu
def test_io_smooth_mesh_and_the_command_line_in_a_child_process(tmp_path):
    from gens_amd import io as gio
    v, t, _ = SR.noisy_icosphere()
    topo = _want_topology("noisy icosphere")
    want = SR.smooth(v, t, iterations=2, topology=topo)
    colors = (np.arange(3 * len(v)).reshape(-1, 3) % 251).astype(np.uint8)
    seen = np.arange(len(v)) % 3 != 0
    out_v, out_t, attrs = gio.smooth_mesh(v, t.astype(np.int64), colors=colors, seen=seen, iterations=2)
    assert _same(out_v, want["vertices"]) and _same(out_t, t.astype(np.int64)) and set(attrs) == {"colors", "seen", "stats"}
    assert _same(attrs["colors"], colors) and _same(attrs["seen"], seen)
    _check_stats(attrs["stats"], want["stats"], "io")
    pinned = np.arange(len(v)) < 100
    tensors = gio.smooth_mesh(torch.from_numpy(v), torch.from_numpy(t), iterations=2, pinned=pinned)
    assert _same(tensors[0], SR.smooth(v, t, iterations=2, pinned=pinned, topology=topo)["vertices"]) and tensors[2]["stats"]["pinned"] == 100
    rep = gio.mesh_report(v, t, roughness=True)
    plain = gio.mesh_report(v, t)
    assert {k: x for k, x in rep.items() if k != "roughness"} == plain and "roughness" not in plain
    assert rep["roughness"]["edges"] == 1920 and abs(rep["roughness"]["rms"] - SR.roughness_report(SR.dihedral(topo))["rms"]) <= 1e-12
    # the command line, each in a fresh process
    src, out = str(tmp_path / "ball.ply"), str(tmp_path / "out.ply")
    gio.write_ply(src, v, t, colors=colors)
    run = subprocess.run([sys.executable, "-m", "gens_amd.smooth_mesh", src, out, "--iterations", "2", "--weights", "cotangent", "--measure"],
                         cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.strip().split("\n")
    assert len(lines) == 1
    stats = json.loads(lines[0])
    assert stats["iterations"] == 2 and stats["weights"] == "cotangent" and stats["moved"] == 642 and stats["roughness_before"]["edges"] == 1920
    assert stats["roughness_after"]["rms"] < stats["roughness_before"]["rms"]
    rv, rt, rattrs = gio.read_ply(out, attributes=True)
    assert np.array_equal(rt, t) and len(rv) == 642 and np.array_equal(rattrs["colors"], colors)
    run = subprocess.run([sys.executable, "-m", "gens_amd.mesh_report", src, "--roughness"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and json.loads(run.stdout)["roughness"]["edges"] == 1920, run.stderr[-2000:]


# ------------------------------------------------------------------------------------------------------------------------------------
# the model: the g23 surface of tests/test_hip_mesh_repair.py, R = 64, simplified at cell 4 and repaired
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_extract_geometry_smooths_on_every_route():
    from gens_amd import lib as L, ops
    from .test_hip_mesh_repair import MODEL_REPAIR, R, SIMPLIFY, _model_want
    from .test_hip_mesh_simplify import ROUTES, _model, _world
    from .test_hip_vertex_attrs import _same as same_attrs, _validate_args
    m = _model()
    surf, vols, views, lo, hi = m["surf"], m["vols"], m["views"], m["lo"], m["hi"]
    _, repaired, _ = _model_want()
    rv, rt = repaired[0], repaired[1]                                # ops.repair_mesh of the simplified mesh, in index coordinates
    got_v, _, stats = ops.smooth_mesh(rv, rt, **MODEL_SMOOTH)
    want = SR.smooth(rv.cpu().numpy(), rt.cpu().numpy(), **MODEL_SMOOTH)
    assert _same(got_v.cpu().numpy(), want["vertices"]) and stats["moved"] > 0                      # bit for bit
    _check_stats(stats, want["stats"], "g23")
    print(f"g23 R = {R}, cell {SIMPLIFY}: {json.dumps(stats)}")
    assert stats["roughness_after"]["rms"] < stats["roughness_before"]["rms"]
    after = ops.mesh_topology(got_v, rt).report()
    surf.lattice_lipschitz = m["lipschitz"]
    try:
        for route, kw in ROUTES:
            plain = surf.extract_geometry(vols, lo, hi, R, 0.0, simplify=SIMPLIFY, repair=MODEL_REPAIR, **kw)
            assert _same(plain[0], _world(rv.cpu().numpy(), lo, hi)) and _same(plain[1], rt.cpu().numpy()) and surf.last_smooth_stats is None
            L.profile_begin(only=K39)
            v, t, attrs = surf.extract_geometry(vols, lo, hi, R, 0.0, simplify=SIMPLIFY, repair=MODEL_REPAIR, smooth=MODEL_SMOOTH, topology=True,
                                                views=views, attributes=("normals", "colors"), **kw)
            launched = [k for k, *_ in L.profile_end(raw=True)]
            assert set(launched) == {"gens_mesh_laplacian_step", "gens_mesh_dihedral"} and launched.count("gens_mesh_laplacian_step") == 6, route
            assert _same(v, _world(got_v.cpu().numpy(), lo, hi)) and _same(t, plain[1]), route     # ops.smooth_mesh of the unsmoothed call's mesh
            assert surf.last_smooth_stats == stats and surf.last_mesh_topology == after, route
            assert surf.last_repair_stats is not None and surf.last_simplify_stats["output_triangles"] > 0
            # the attribute points are those of the smoothed vertices
            assert same_attrs(attrs, surf.vertex_attributes(v, vols, views)) and len(attrs["normals"]) == len(v), route
        two = surf.extract_geometry(vols, lo, hi, R, 0.0, simplify=SIMPLIFY, repair=MODEL_REPAIR, smooth=True)
        defaults = ops.smooth_mesh(rv, rt)
        assert len(two) == 2 and _same(two[0], _world(defaults[0].cpu().numpy(), lo, hi)) and surf.last_smooth_stats == defaults[2]
        surf.mesh_smooth = MODEL_SMOOTH
        try:
            again = surf.extract_geometry(vols, lo, hi, R, 0.0, simplify=SIMPLIFY, repair=MODEL_REPAIR)
            assert _same(again[0], v) and _same(again[1], t) and surf.last_smooth_stats == stats
            off = surf.extract_geometry(vols, lo, hi, R, 0.0, simplify=SIMPLIFY, repair=MODEL_REPAIR, smooth=False)
            assert _same(off[0], plain[0]) and surf.last_smooth_stats is None
        finally:
            del surf.mesh_smooth
        torch.manual_seed(3)
        out = surf.validate(*_validate_args(surf, vols), extract_geometry=True, mesh_resolution=R, mesh_simplify=SIMPLIFY, mesh_repair=MODEL_REPAIR,
                            mesh_smooth=MODEL_SMOOTH)
        assert _same(out["vertices"], v) and _same(out["triangles"], t) and surf.last_smooth_stats == stats
    finally:
        surf.lattice_lipschitz = 2.0


@gpu
def test_nothing_changes_when_the_option_is_unset():
    from gens_amd import lib as L
    from gens_amd.models.modules.implicit_surface import ImplicitSurface
    from .test_hip_mesh_repair import R
    from .test_hip_mesh_simplify import _model, _world
    from .test_hip_vertex_attrs import TODAYS_KEYS, _validate_args
    assert ImplicitSurface.mesh_smooth is None and ImplicitSurface.last_smooth_stats is None
    m = _model()
    surf, vols, lo, hi = m["surf"], m["vols"], m["lo"], m["hi"]
    assert "mesh_smooth" not in vars(surf)
    L.profile_begin(only=K39)
    for off in ({}, {"smooth": None}, {"smooth": False}):
        got = surf.extract_geometry(vols, lo, hi, R, 0.0, simplify=2, topology=True, **off)
        assert len(got) == 2 and _same(got[0], _world(m["simple"][0], lo, hi)) and _same(got[1], m["simple"][1]), off
        assert surf.last_smooth_stats is None
        plain = surf.extract_geometry(vols, lo, hi, R, 0.0, **off)
        assert _same(plain[0], _world(m["full"][0], lo, hi)) and _same(plain[1], m["full"][1]) and surf.last_smooth_stats is None
    args = _validate_args(surf, vols)
    torch.manual_seed(3)
    ref = surf.validate(*args, extract_geometry=True, mesh_resolution=33, mesh_simplify=2)
    torch.manual_seed(3)
    off = surf.validate(*args, extract_geometry=True, mesh_resolution=33, mesh_simplify=2, mesh_smooth=False)
    assert not L.profile_end(raw=True)                                           # not one K39 launch
    assert set(ref) == set(off) == TODAYS_KEYS
    for k in TODAYS_KEYS:
        assert torch.equal(torch.as_tensor(off[k]), torch.as_tensor(ref[k])), k


@gpu
def test_refusals_come_before_any_launch():
    from gens_amd import io as gio, lib as L, ops
    from .test_hip_mesh_simplify import K33, _model
    from .test_hip_mesh_topology import K37
    from .test_hip_vertex_attrs import NETWORK, _validate_args
    from .test_mesh_smooth_cpu import BAD_OPTIONS
    m = _model()
    surf, vols, lo, hi = m["surf"], m["vols"], m["lo"], m["hi"]
    v, t = TR.cube()
    dv, dt = _up(v, np.float64), _up(t, np.int32)
    other = ops.mesh_topology(*(_up(x, d) for x, d in zip(TR.tetrahedron(), (np.float64, np.int32))))
    L.profile_begin(only=K39 | K33 | NETWORK | {"gens_face_cc_hook", "gens_compact_valid", "gens_mc_classify", "gens_lattice_points"})
    for bad in (1, "yes", 2.0) + tuple(BAD_OPTIONS):
        with pytest.raises(ValueError):
            surf.extract_geometry(vols, lo, hi, 33, 0.0, smooth=bad)
        with pytest.raises(ValueError):
            surf.validate(*_validate_args(surf, vols), extract_geometry=True, mesh_resolution=33, mesh_smooth=bad)
    L.profile_end(raw=True)
    L.profile_begin(only=K39 | K37 | {"gens_face_cc_hook"})
    for fn in (ops.smooth_mesh, ops.mesh_laplacian, ops.mesh_roughness):
        for bad_v, bad_t in ((dv.float(), dt), (dv, dt.long()), (dv[:, :2], dt), (dv, dt.reshape(-1)), (dv.cpu(), dt)):
            with pytest.raises(ValueError):
                fn(bad_v, bad_t)
        with pytest.raises(ValueError, match="another mesh"):
            fn(dv, dt, topology=other)
        with pytest.raises(ValueError, match="MeshTopology"):
            fn(dv, dt, topology="yes")
    for bad in BAD_OPTIONS:
        if set(bad) <= set(ops.SMOOTH_KEYS):
            with pytest.raises(ValueError):
                ops.smooth_mesh(dv, dt, **bad)
        if "pinned" not in bad:
            with pytest.raises(ValueError):
                gio.smooth_mesh(v, t, **bad)
    for bad in (torch.zeros(8, device="cuda"), torch.zeros(7, dtype=torch.bool, device="cuda"), torch.zeros(8, dtype=torch.bool), [False] * 8):
        with pytest.raises(ValueError, match="pinned"):
            ops.smooth_mesh(dv, dt, pinned=bad)
    with pytest.raises(ValueError, match="weights"):
        ops.mesh_laplacian(dv, dt, weights="cot")
    assert not L.profile_end(raw=True)
    # the entry point itself: a step reads one buffer and writes another
    topo = ops.mesh_topology(dv, dt)
    nbrs = ops.mesh_neighbours(topo)
    with pytest.raises(RuntimeError, match="out == in"):
        L.call("gens_mesh_laplacian_step", L.ptr(dv, torch.float64), 8, *(L.ptr(x, torch.int32) for x in nbrs), 2 * topo.n_edges, None, topo.n_edges, None,
               0.5, L.ptr(dv, torch.float64), None, None, L.stream())
