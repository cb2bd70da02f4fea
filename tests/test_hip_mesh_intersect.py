"""GPU tests of K41 (mesh self-intersections) against the rational reference of tests/mesh_intersect_reference.py.  The contract, for every
mesh: candidates, duplicate pairs, invalid and degenerate faces equal the reference exactly (every candidate pair once: the broad phase);
every pair reported intersecting intersects, and no intersecting candidate is missing from intersecting + undecided; every undecided pair is
delicate or has an uncertain face, every uncertain face is delicate; nothing is undecided on a SHORT mesh; pairs ascend with s < t and the
face flags agree with them; the same bits twice and with the face order reversed; max_pairs gives the prefix and pairs=False the same
counts.  Whether a pair is delicate, and every expected count, is the reference's alone."""
import functools
import json

import numpy as np
import pytest
import torch

from . import mesh_intersect_reference as IR
from . import mesh_repair_reference as RR
from . import mesh_smooth_reference as SM
from . import mesh_topology_reference as TR
from . import winding_reference as WR

gpu = pytest.mark.gpu
K41 = {"gens_mesh_isect_faces", "gens_mesh_isect_count", "gens_mesh_isect_emit"}
FANS = (1, 63, 64, 65, 127, 128, 129, 257)                   # a cell list around the wave (64) and the slice of the pair walk (128), and three slices
SOUP_SEED = 35


def _up(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


@functools.lru_cache(maxsize=None)
def _meshes():
    cube, ico = TR.cube(), SM.icosphere(2)
    calm = SM.noisy_icosphere(2, 0.02, 7)[:2]
    out = {"cube": cube, "cubes overlapping": IR.joined(cube, IR.shifted(cube, (0.5, 0.5, 0.5))),
           "cubes touching": IR.joined(cube, IR.shifted(cube, (1, 0, 0))), "cubes apart": IR.joined(cube, IR.shifted(cube, (3, 0, 0))),
           "strip 65": WR.planar_strip(65), "lattice sheet": SM.lattice_sheet(), "book 5": TR.book(5),
           "tetrahedra at a vertex": TR.two_tetrahedra_vertex(), "tetrahedra at an edge": TR.two_tetrahedra_edge(),
           "flat fold": IR.flat_fold(), "fold lifted": IR.flat_fold(0.0625), "pierced at a vertex": IR.pierced_at_vertex(),
           "coplanar wedges": IR.coplanar_wedges(), "unwelded touch": IR.unwelded_touch(), "degenerate faces": IR.degenerate_faces(),
           "one face": (cube[0], cube[1][:1]), "big face": IR.big_face_beside_small(),
           "clustered sphere": RR.clustered_sphere(), "noisy sphere": SM.noisy_icosphere(2, 0.2, 7)[:2],
           "noisy spheres crossing": IR.joined(calm, IR.shifted(calm, (0.7, 0.1, 0.2))), "soup": RR.random_soup(SOUP_SEED),
           "torus": TR.torus(), "icosphere": ico, "mc sphere": TR.mc_sphere(),
           "icospheres crossing": IR.joined(ico, IR.shifted(ico, (0.7, 0.1, 0.2))),
           "near miss above": IR.near_miss(1), "near miss on": IR.near_miss(0), "near miss below": IR.near_miss(-1)}
    for n in FANS:
        out[f"fan {n}"] = IR.fan_through_cell(n)
    return {k: (np.asarray(v, dtype=np.float64), np.asarray(t, dtype=np.int32)) for k, (v, t) in out.items()}


SHORT = ("cube", "cubes overlapping", "cubes touching", "cubes apart", "strip 65", "lattice sheet", "tetrahedra at a vertex",
         "tetrahedra at an edge", "flat fold", "fold lifted", "pierced at a vertex", "coplanar wedges", "unwelded touch", "degenerate faces",
         "one face", "big face")
NONE_INTERSECTING = ("cube", "cubes apart", "strip 65", "lattice sheet", "book 5", "tetrahedra at a vertex", "tetrahedra at an edge",
                     "fold lifted", "clustered sphere", "noisy sphere", "one face", "near miss above")
SOME_INTERSECTING = ("cubes overlapping", "cubes touching", "flat fold", "pierced at a vertex", "coplanar wedges", "unwelded touch",
                     "noisy spheres crossing", "soup", "icospheres crossing", "big face")
NO_DELICATE_PAIR = ("clustered sphere", "noisy sphere", "noisy spheres crossing", "soup", "book 5")      # so nothing may be undecided there
SYMMETRIC = ("torus", "icosphere", "mc sphere", "icospheres crossing")                                     # these do have delicate pairs
NAMES = SHORT + ("book 5", "clustered sphere", "noisy sphere", "noisy spheres crossing", "soup") + SYMMETRIC + (
    "near miss above", "near miss on", "near miss below") + tuple(f"fan {n}" for n in FANS)


@functools.lru_cache(maxsize=None)
def _device(name):
    v, t = _meshes()[name]
    return _up(v, np.float64), _up(t, np.int32)


def _pairs_of(found):
    p, k = found.pairs.cpu().numpy(), found.kinds.cpu().numpy()
    return {(int(a), int(b)): int(c) for (a, b), c in zip(p, k)}


def _flags_from(pairs, n_faces):
    flags = np.zeros(n_faces, dtype=np.uint8)
    for (s, t), kind in pairs.items():
        flags[s] |= kind
        flags[t] |= kind
    return flags


@gpu
def test_the_meshes_are_what_the_tests_take_them_for():
    m = _meshes()
    assert set(NAMES) == set(m) and len(set(NAMES)) == len(NAMES)
    for name in NAMES:
        assert IR.is_short(m[name][0]) == (name in SHORT), name
    soup = IR.analyse(*m["soup"])
    assert soup.invalid_faces > 0 and soup.duplicate_pairs > 0 and soup.intersecting > 0
    assert (m["soup"][1] < 0).any() or (m["soup"][1] >= len(m["soup"][0])).any()
    assert IR.analyse(*m["degenerate faces"]).degenerate_faces == 2
    for name in NO_DELICATE_PAIR:                              # the precondition of "nothing undecided" there, decided by the reference alone
        r = IR.analyse(*m[name])
        assert r.delicate == 0 and not r.face_delicate.any() and r.candidates > 0, name
    for name in SYMMETRIC:
        assert IR.analyse(*m[name]).delicate > 0, name
    for name in NONE_INTERSECTING:
        assert IR.analyse(*m[name]).intersecting == 0, name
    for name in SOME_INTERSECTING:
        assert IR.analyse(*m[name]).intersecting > 0, name


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_the_contract(name):
    from gens_amd import lib as L, ops
    v, t = _meshes()[name]
    dv, dt = _device(name)
    rep = IR.analyse(v, t)
    found = ops.self_intersections_of(dv, dt)
    c = found.counts
    print(f"{name}: {json.dumps(c)}; reference: {rep.candidates} candidates, {rep.intersecting} intersecting, {rep.delicate} delicate")
    assert set(ops.SELF_INTERSECTION_KEYS) <= set(c) and all(isinstance(c[k], int) for k in ops.SELF_INTERSECTION_KEYS)
    assert (c["faces"], c["invalid_faces"], c["degenerate_faces"], c["duplicate_pairs"], c["candidates"]) == (
        rep.faces, rep.invalid_faces, rep.degenerate_faces, rep.duplicate_pairs, rep.candidates)
    cls = found.face_class.cpu().numpy()
    valid = IR.face_valid(v, t)
    assert ((cls == 0) == ~valid).all() and ((cls == 2) == rep.degenerate).all() and c["uncertain_faces"] == int((cls == 3).sum())
    assert rep.face_delicate[cls == 3].all()                                        # every uncertain face is delicate
    assert found.pairs.dtype == torch.int32 and found.kinds.dtype == torch.uint8 and found.pairs.shape == (len(found.kinds), 2)
    raw = found.pairs.cpu().numpy().astype(np.int64)
    key = (raw[:, 0] << 32) | raw[:, 1]
    assert (raw[:, 0] < raw[:, 1]).all() and (np.diff(key) > 0).all()               # s < t, ascending, no pair twice
    pairs = _pairs_of(found)
    assert set(pairs.values()) <= {1, 2} and set(pairs) <= set(rep.pairs)
    assert all(rep.pairs[p][0] for p, kind in pairs.items() if kind == 1)           # reported intersecting: it does
    assert all(p in pairs for p, (hit, _, _) in rep.pairs.items() if hit)           # intersecting: reported, as such or as undecided
    unsure = [p for p, kind in pairs.items() if kind == 2]
    assert all(rep.pairs[p][1] or cls[p[0]] == 3 or cls[p[1]] == 3 for p in unsure)  # undecided: delicate, or a face is uncertain
    assert all(p in unsure for p in rep.pairs if cls[p[0]] == 3 or cls[p[1]] == 3)
    assert (c["intersecting"], c["undecided"]) == (sum(k == 1 for k in pairs.values()), len(unsure))
    assert c["undecided"] <= sum(1 for p, (_, delicate, _) in rep.pairs.items() if delicate or cls[p[0]] == 3 or cls[p[1]] == 3)
    flags = found.face_flags.cpu().numpy()
    assert flags.dtype == np.uint8 and (flags == _flags_from(pairs, len(t))).all()
    assert (c["faces_intersecting"], c["faces_undecided"]) == (int((flags & 1 != 0).sum()), int((flags & 2 != 0).sum()))
    if name in SHORT or name in NO_DELICATE_PAIR or name.startswith("fan"):         # (the fans' coordinates keep every operation exact too)
        assert c["undecided"] == 0 and c["uncertain_faces"] == 0, name
        assert c["intersecting"] == rep.intersecting
    # the same bits twice, and with the faces in reverse order after mapping the ids back
    again = ops.self_intersections_of(dv, dt)
    assert torch.equal(again.pairs, found.pairs) and torch.equal(again.kinds, found.kinds) and torch.equal(again.face_flags, found.face_flags)
    assert again.counts == c
    back = ops.self_intersections_of(dv, dt.flip(0).contiguous())
    n = len(t)
    assert {(n - 1 - b, n - 1 - a): k for (a, b), k in _pairs_of(back).items()} == pairs
    assert torch.equal(back.face_flags.flip(0), found.face_flags) and {k: x for k, x in back.counts.items()} == c
    # max_pairs: the prefix; pairs=False: the same counts and no emit
    if pairs:
        few = ops.self_intersections_of(dv, dt, max_pairs=3)
        assert torch.equal(few.pairs, found.pairs[:3]) and torch.equal(few.kinds, found.kinds[:3]) and few.counts == c
    L.profile_begin(only=K41)
    bare = ops.self_intersections_of(dv, dt, pairs=False)
    launched = [k for k, *_ in L.profile_end(raw=True)]
    assert launched == ["gens_mesh_isect_faces", "gens_mesh_isect_count"] and bare.pairs is None and bare.kinds is None
    assert bare.counts == c and torch.equal(bare.face_flags, found.face_flags)


@gpu
def test_the_expected_verdicts_of_the_small_cases():
    from gens_amd import ops
    def kinds(name):
        return _pairs_of(ops.self_intersections_of(*_device(name)))
    assert kinds("flat fold") == {(0, 1): 1} and kinds("fold lifted") == {}
    assert kinds("pierced at a vertex") == {(0, 1): 1} and kinds("coplanar wedges") == {(0, 1): 1} and kinds("unwelded touch") == {(0, 1): 1}
    assert kinds("cube") == {} and kinds("cubes apart") == {} and kinds("one face") == {}
    assert ops.self_intersections_of(*_device("cube")).counts["candidates"] == 54
    assert ops.self_intersections_of(*_device("one face")).counts["candidates"] == 0
    degenerate = ops.self_intersections_of(*_device("degenerate faces"))
    assert degenerate.face_class.cpu().tolist() == [1, 2, 2] and degenerate.counts["degenerate_faces"] == 2
    # a corner one ulp above, on and one ulp below a plane: right or undecided, never wrong
    assert kinds("near miss above") in ({}, {(0, 1): 2})
    assert kinds("near miss on") in ({(0, 1): 1}, {(0, 1): 2}) and kinds("near miss below") in ({(0, 1): 1}, {(0, 1): 2})


@gpu
def test_the_result_does_not_depend_on_the_grid():
    from gens_amd import lib as L, ops
    for n in FANS:                                            # the fans do put n faces into one cell
        dv, dt = _device(f"fan {n}")
        grid = ops.build_mesh_grid(dv, dt)
        assert int((grid.cell_start[1:] - grid.cell_start[:-1]).max()) == n
    for name in ("cubes overlapping", "big face", "fan 257", "soup", "torus"):
        dv, dt = _device(name)
        v, t = _meshes()[name]
        dt = torch.where(((dt >= 0) & (dt < len(v))).all(dim=1, keepdim=True), dt, torch.zeros_like(dt))
        built = ops.mesh_self_intersections(ops.build_mesh_grid(dv, dt))
        # one cell that holds every face, made by hand
        lo = v.min(axis=0) - 1.0
        n = len(t)
        one = ops.MeshGrid(dv, dt, _up([0, n], np.int32), torch.arange(n, device="cuda", dtype=torch.int32).flip(0).contiguous(),
                           (lo[0], lo[1], lo[2], float((v.max(axis=0) - lo).max() + 1.0)), (1, 1, 1))
        alone = ops.mesh_self_intersections(one)
        assert torch.equal(alone.pairs, built.pairs) and torch.equal(alone.kinds, built.kinds) and torch.equal(alone.face_flags, built.face_flags)
        assert {k: alone.counts[k] for k in ops.SELF_INTERSECTION_KEYS} == {k: built.counts[k] for k in ops.SELF_INTERSECTION_KEYS}
    # no faces: nothing is launched
    L.profile_begin(only=K41)
    none = ops.self_intersections_of(_up(np.zeros((3, 3)), np.float64), _up(np.zeros((0, 3)), np.int32))
    empty = ops.mesh_self_intersections(ops.build_mesh_grid(_up(np.zeros((3, 3)), np.float64), _up(np.zeros((0, 3)), np.int32)), pairs=False)
    assert not L.profile_end(raw=True)
    assert none.counts["faces"] == 0 and none.pairs.shape == (0, 2) and none.kinds.shape == (0,) and empty.pairs is None
    assert all(x == 0 for x in empty.counts.values())


@gpu
def test_the_mesh_report_and_the_command_line(tmp_path, capsys):
    from gens_amd import io as gio, lib as L, mesh_report as cli, ops
    v, t = _meshes()["cubes overlapping"]
    L.profile_begin(only=K41)
    plain = gio.mesh_report(v, t)
    assert not L.profile_end(raw=True)                        # the default launches nothing of K41 ...
    assert plain == ops.mesh_topology(*_device("cubes overlapping")).report() and "self_intersections" not in plain
    full = gio.mesh_report(v, t, self_intersections=True)
    counts = ops.self_intersections_of(*_device("cubes overlapping")).counts
    assert {k: x for k, x in full.items() if k != "self_intersections"} == plain      # ... and is what it was
    assert full["self_intersections"] == {k: counts[k] for k in ops.SELF_INTERSECTION_KEYS} and full["self_intersections"]["intersecting"] == 18
    assert json.dumps(plain) == json.dumps(gio.mesh_report(v, t, self_intersections=False))
    both = gio.mesh_report(v, t, roughness=True, self_intersections=True, max_pairs=4)
    assert both["roughness"] == gio.mesh_report(v, t, roughness=True)["roughness"] and len(both["pairs"]["pairs"]) == 4
    sv, st = _meshes()["soup"]                                # any indices, as the report takes them
    soup = gio.mesh_report(sv, st, self_intersections=True)["self_intersections"]
    assert soup["invalid_faces"] == IR.analyse(sv, st).invalid_faces and soup["candidates"] == IR.analyse(sv, st).candidates
    path = str(tmp_path / "cubes.ply")
    gio.write_ply(path, v, t)
    capsys.readouterr()
    assert cli.main([path]) == 0
    assert json.loads(capsys.readouterr().out) == json.loads(json.dumps(plain))
    assert cli.main([path, "--self-intersections", "--max-pairs", "5"]) == 0
    got = json.loads(capsys.readouterr().out)
    found = ops.self_intersections_of(*_device("cubes overlapping"), max_pairs=5)
    assert got["self_intersections"] == full["self_intersections"]
    assert got["pairs"] == {"pairs": found.pairs.cpu().tolist(), "kinds": found.kinds.cpu().tolist()} and len(got["pairs"]["kinds"]) == 5
    assert cli.main([path, "--self-intersections"]) == 0
    got = json.loads(capsys.readouterr().out)
    assert "pairs" not in got and got["self_intersections"] == full["self_intersections"]


@gpu
def test_the_model_option():
    from gens_amd import lib as L, ops
    from .test_hip_mesh_simplify import _model
    m = _model()
    surf, vols, lo, hi = m["surf"], m["vols"], m["lo"], m["hi"]
    full = [_up(m["full"][0], np.float64), _up(m["full"][1], np.int32)]
    simple = [_up(m["simple"][0], np.float64), _up(m["simple"][1], np.int32)]
    # off (None, False): not one launch of K41, launch for launch the same call
    L.profile_begin()
    surf.extract_geometry(vols, lo, hi, 64, 0.0, simplify=2)
    default = [k for k, *_ in L.profile_end(raw=True)]
    L.profile_begin()
    surf.extract_geometry(vols, lo, hi, 64, 0.0, simplify=2, self_intersections=False)
    off = [k for k, *_ in L.profile_end(raw=True)]
    assert off == default and not (set(default) & K41) and surf.last_mesh_self_intersections is None
    assert "self_intersections_before" not in surf.last_simplify_stats
    # on: the returned mesh's counts, and the mesh before each stage
    surf.extract_geometry(vols, lo, hi, 64, 0.0, simplify=2, repair=True, smooth=True, self_intersections=True)
    last = surf.last_mesh_self_intersections
    print(f"g23 R = 64: extracted {json.dumps(surf.last_simplify_stats['self_intersections_before'])}\n  simplified "
          f"{json.dumps(surf.last_repair_stats['self_intersections_before'])}\n  repaired {json.dumps(surf.last_smooth_stats['self_intersections_before'])}\n"
          f"  smoothed {json.dumps(last)}")
    assert tuple(last) == ops.SELF_INTERSECTION_KEYS and last["faces"] > 0
    assert surf.last_simplify_stats["self_intersections_before"] == ops.self_intersection_counts(*full)
    assert surf.last_repair_stats["self_intersections_before"] == ops.self_intersection_counts(*simple)
    assert tuple(surf.last_smooth_stats["self_intersections_before"]) == ops.SELF_INTERSECTION_KEYS
    surf.extract_geometry(vols, lo, hi, 64, 0.0, self_intersections=True)
    assert surf.last_mesh_self_intersections == ops.self_intersection_counts(*full) and surf.last_simplify_stats is None
    surf.mesh_self_intersections = True                       # the attribute is the default
    try:
        surf.extract_geometry(vols, lo, hi, 64, 0.0)
        assert surf.last_mesh_self_intersections == ops.self_intersection_counts(*full)
        surf.extract_geometry(vols, lo, hi, 64, 0.0, self_intersections=False)
        assert surf.last_mesh_self_intersections is None
    finally:
        del surf.mesh_self_intersections
