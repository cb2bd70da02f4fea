"""CPU-side tests of K41 (mesh self-intersections): the rational reference of tests/mesh_intersect_reference.py against cases derived by hand,
every refusal of the three entry points through ctypes, and every refusal of the Python layers and of the command line, before the device
is looked at."""
import ctypes as C

import numpy as np
import pytest

from . import mesh_intersect_reference as IR
from . import mesh_smooth_reference as SM
from . import mesh_topology_reference as TR
from . import winding_reference as WR


def _figures(mesh):
    r = IR.analyse(*mesh)
    return r.candidates, r.intersecting


def test_the_reference_on_cases_derived_by_hand():
    cube = TR.cube()
    # a cube: 12 faces, 66 pairs; a pair has no candidate box overlap only if the faces lie in opposite sides' planes (3 opposite pairs of
    # sides x 2 x 2 faces = 12): 54 candidates; its surface does not cross itself
    assert _figures(cube) == (54, 0) and IR.is_short(cube[0])
    far = IR.analyse(*IR.joined(cube, IR.shifted(cube, (3, 0, 0))))
    assert (far.candidates, far.intersecting) == (108, 0)                  # two cubes apart: each one's own 54
    assert IR.analyse(*IR.joined(cube, IR.shifted(cube, (0.5, 0.5, 0.5)))).intersecting > 0
    touching = IR.analyse(*IR.joined(cube, IR.shifted(cube, (1, 0, 0))))
    assert touching.intersecting > 0 and all(k == 0 for hit, _, k in touching.pairs.values() if hit)      # no index is shared between the cubes
    for flat in (WR.planar_strip(65), SM.lattice_sheet()):                 # coplanar neighbours touch along shared edges and vertices only
        r = IR.analyse(*flat)
        assert r.candidates > 0 and r.intersecting == 0
    for mesh in (TR.book(5), TR.two_tetrahedra_vertex(), TR.two_tetrahedra_edge()):
        assert IR.analyse(*mesh).intersecting == 0
    fold = IR.analyse(*IR.flat_fold())
    assert fold.pairs == {(0, 1): (True, True, 2)}                         # folded flat onto its neighbour: coplanar, so delicate
    assert IR.analyse(*IR.flat_fold(0.0625)).pairs == {(0, 1): (False, False, 2)}
    assert IR.analyse(*IR.pierced_at_vertex()).pairs == {(0, 1): (True, False, 1)}
    assert IR.analyse(*IR.coplanar_wedges()).pairs == {(0, 1): (True, True, 1)}
    assert IR.analyse(*IR.unwelded_touch()).pairs == {(0, 1): (True, True, 0)}   # they meet in one point, which no index shares
    degenerate = IR.analyse(*IR.degenerate_faces())
    assert degenerate.degenerate.tolist() == [False, True, True] and degenerate.candidates == 0 and degenerate.degenerate_faces == 2
    one = IR.analyse(cube[0], cube[1][:1])
    assert (one.faces, one.candidates, one.duplicate_pairs) == (1, 0, 0)
    twice = IR.analyse(cube[0], np.concatenate([cube[1][:1], cube[1][:1, [1, 2, 0]], np.array([[0, 0, 1], [0, 1, 99]])]))
    assert (twice.invalid_faces, twice.duplicate_pairs, twice.candidates) == (2, 1, 0)
    for ulps, hit in ((1, False), (0, True), (-1, True)):                  # a corner an ulp above, on and an ulp below a plane
        assert IR.analyse(*IR.near_miss(ulps)).pairs == {(0, 1): (hit, True, 0)}
    assert not IR.is_short(IR.near_miss(0)[0]) and not IR.is_short(TR.book(5)[0]) and IR.is_short(IR.big_face_beside_small()[0])


def test_the_clipping_itself():
    from fractions import Fraction as F
    tri = [(0, 0, 0), (4, 0, 0), (0, 4, 0)]
    through = [(1, 1, -1), (1, 1, 1), (2, 1, 1)]                          # cuts the plane z = 0 in the segment (1, 1) .. (1.5, 1)
    got = set(IR.common_points(through, tri))
    assert got == {(F(1), F(1), F(0)), (F(3, 2), F(1), F(0))}
    assert IR.common_points([(9, 9, -1), (9, 9, 1), (8, 9, 1)], tri) == []               # crosses the plane outside the face
    assert IR.common_points([(0, 0, 1), (4, 0, 1), (0, 4, 1)], tri) == []                # parallel, above
    inside = IR.common_points([(1, 1, 0), (2, 1, 0), (1, 2, 0)], tri)                    # coplanar and inside: itself
    assert set(inside) == {(1, 1, 0), (2, 1, 0), (1, 2, 0)}
    assert set(IR.common_points([(4, 0, 0), (8, 0, 0), (4, 4, 0)], tri)) == {(4, 0, 0)}  # coplanar, touching at one corner


def _grid_args(**kw):
    from gens_amd import lib as L
    fake = 0x7E0000100000
    fields = dict(vertices=fake, triangles=fake + 0x1000, cell_start=fake + 0x2000, cell_faces=fake + 0x3000, n_faces=10, lo_x=0.0, lo_y=0.0,
                  lo_z=0.0, cell=1.0, nx=2, ny=2, nz=2)
    fields.update(kw)
    return L.MeshGridArgs(*(fields[n] for n, _ in L.MeshGridArgs._fields_))


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from gens_amd import lib as L
    lib = L.load()
    p = [C.c_void_p(0x7E0000200000 + 0x1000 * i) for i in range(8)]

    def faces(vertices=p[0], nv=8, triangles=p[1], nt=10, cls=p[2], box=p[3]):
        return lib.gens_mesh_isect_faces(vertices, nv, triangles, nt, cls, box, None)

    def count(grid, nv=8, entries=20, longest=5, cls=p[0], box=p[1], cells=p[2], totals=p[3], flags=p[4]):
        return lib.gens_mesh_isect_count(None if grid is None else C.byref(grid), nv, entries, longest, cls, box, cells, totals, flags, None)

    def emit(grid, nv=8, entries=20, longest=5, cls=p[0], box=p[1], start=p[2], cursor=p[3], n_out=4, pairs=p[4], kinds=p[5]):
        return lib.gens_mesh_isect_emit(None if grid is None else C.byref(grid), nv, entries, longest, cls, box, start, cursor, n_out, pairs, kinds,
                                        None)

    def refused(rc, code, word):
        assert rc == code, (rc, lib.gens_last_error())
        assert word.encode() in lib.gens_last_error(), lib.gens_last_error()
    for kw in (dict(nv=-1), dict(nt=-1)):
        refused(faces(**kw), -1, "vertices")
    for kw in (dict(vertices=None), dict(triangles=None), dict(cls=None), dict(box=None)):
        refused(faces(**kw), -1, "null pointer")
    refused(faces(nv=2 ** 31), -2, "below 2^31")
    refused(faces(nt=2 ** 31), -2, "below 2^31")
    assert faces(nt=0, triangles=None, cls=None, box=None) == 0                                      # nothing to do is no error
    for fn in (count, emit):
        refused(fn(None), -1, "null grid")
        for kw in (dict(nv=-1), dict(entries=-1), dict(longest=-1)):
            refused(fn(_grid_args(), **kw), -1, "entries")
        refused(fn(_grid_args(n_faces=-1)), -1, "faces")
        refused(fn(_grid_args(n_faces=2 ** 31)), -2, "below 2^31")
        refused(fn(_grid_args(), nv=2 ** 31), -2, "below 2^31")
        refused(fn(_grid_args(), entries=2 ** 31), -2, "below 2^31")
        for kw in (dict(nx=0), dict(ny=513), dict(nz=-1)):
            refused(fn(_grid_args(**kw)), -2, "cells per axis")
        for kw in (dict(cell=0.0), dict(cell=float("nan")), dict(lo_x=float("inf"))):
            refused(fn(_grid_args(**kw)), -2, "bad grid box")
        for kw in (dict(vertices=None), dict(triangles=None), dict(cell_start=None), dict(cell_faces=None)):
            refused(fn(_grid_args(**kw)), -1, "null pointer")
        for kw in (dict(cls=None), dict(box=None)):
            refused(fn(_grid_args(), **kw), -1, "null pointer")
        assert fn(_grid_args(n_faces=0)) == 0 and fn(_grid_args(), entries=0) == 0                   # nothing to do is no error
    for kw in (dict(cells=None), dict(totals=None), dict(flags=None)):
        refused(count(_grid_args(), **kw), -1, "null pointer")
    refused(count(_grid_args(), flags=C.c_void_p(0x7E0000300002)), -1, "aligned")
    refused(count(_grid_args(), totals=C.c_void_p(0x7E0000300004)), -1, "aligned")
    for kw in (dict(start=None), dict(cursor=None), dict(pairs=None), dict(kinds=None)):
        refused(emit(_grid_args(), **kw), -1, "null pointer")
    refused(emit(_grid_args(), n_out=-1), -1, "pairs")
    refused(emit(_grid_args(), n_out=2 ** 31), -2, "below 2^31")
    assert emit(_grid_args(), n_out=0, pairs=None, kinds=None) == 0


def test_python_layers_and_the_command_line_refuse_before_the_device(tmp_path, capsys):
    import torch
    from gens_amd import io as gio, mesh_report as cli, ops
    from gens_amd.config import gens_model_conf
    from gens_amd.models.modules.implicit_surface import ImplicitSurface
    v, t = TR.cube()
    for grid in (None, object(), (v, t), torch.from_numpy(v)):
        with pytest.raises(ValueError, match="MeshGrid"):
            ops.mesh_self_intersections(grid)
    grid = ops.MeshGrid(torch.zeros(0, 3, dtype=torch.float64), torch.zeros(0, 3, dtype=torch.int32), torch.zeros(2, dtype=torch.int32),
                        torch.zeros(1, dtype=torch.int32), (0.0, 0.0, 0.0, 1.0), (1, 1, 1))
    for bad in (None, 1, 0, "yes"):
        with pytest.raises(ValueError, match="pairs"):
            ops.mesh_self_intersections(grid, pairs=bad)
    for bad in (0, -1, 2.0, True, "3", [1]):
        with pytest.raises(ValueError, match="max_pairs"):
            ops.mesh_self_intersections(grid, max_pairs=bad)
        with pytest.raises(ValueError, match="max_pairs"):
            gio.mesh_report(v, t, self_intersections=True, max_pairs=bad)
    for args in ((torch.from_numpy(v), torch.from_numpy(t)), (v, t)):
        with pytest.raises(ValueError, match="not a tensor on the device"):
            ops.self_intersections_of(*args)
    for bad in (None, 1, "on"):
        with pytest.raises(ValueError, match="self_intersections"):
            gio.mesh_report(v, t, self_intersections=bad)
    with pytest.raises(ValueError, match="goes with"):
        gio.mesh_report(v, t, max_pairs=5)
    with pytest.raises(ValueError, match=r"\(V, 3\)"):
        gio.mesh_report(v[:, :2], t, self_intersections=True)
    assert ops.SELF_INTERSECTION_KEYS == ("faces", "invalid_faces", "degenerate_faces", "uncertain_faces", "duplicate_pairs", "candidates",
                                          "intersecting", "undecided", "faces_intersecting", "faces_undecided")
    # the model option: None or a bool, as `topology`, which keeps taking nothing else
    surf = ImplicitSurface(gens_model_conf(volume_dims=(16, 8, 4))["implicit_surface"])
    assert surf.mesh_self_intersections is None and surf.last_mesh_self_intersections is None
    assert surf._self_intersections_request(None) is False and surf._self_intersections_request(True) is True
    surf.mesh_self_intersections = True
    assert surf._self_intersections_request(None) is True and surf._self_intersections_request(False) is False
    for bad in (1, "yes", {"pairs": True}, 0):
        with pytest.raises(ValueError, match="self_intersections"):
            surf._self_intersections_request(bad)
        with pytest.raises(ValueError, match="self_intersections"):
            surf.extract_geometry(None, None, None, 8, 0.0, self_intersections=bad)
        with pytest.raises(ValueError, match="topology"):
            surf._topology_request(bad)
    # the command line
    path = str(tmp_path / "cube.ply")
    gio.write_ply(path, v, t)
    capsys.readouterr()
    assert cli.main([path, "--max-pairs", "3", "--device", "cpu"]) == 2 and "goes with" in capsys.readouterr().err
    assert cli.main([path, "--self-intersections", "--max-pairs", "0", "--device", "cpu"]) == 2 and "max_pairs" in capsys.readouterr().err
    with pytest.raises(SystemExit) as stop:
        cli.main([path, "--self-intersections", "--max-pairs", "many"])
    assert stop.value.code == 2
