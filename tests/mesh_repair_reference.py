"""K38 restated in numpy float64 (the comment of K38 in include/gens_hip.h is the definition): dedupe, split, small components, orient and
fill, as brute force with dicts and loops over the topology of tests/mesh_topology_reference.py.  Shared by tests/test_mesh_repair_cpu.py
and tests/test_hip_mesh_repair.py, which also take their shapes from here."""
import math

import numpy as np

from . import mesh_topology_reference as TR

STAT_KEYS = ("faces_invalid", "faces_duplicate", "faces_small_component", "vertices_split", "components_flipped", "components_nonorientable",
             "loops_filled", "loops_open", "fill_faces", "fill_vertices", "split_rounds")


def _empty(stats):
    return {"vertices": np.zeros((0, 3)), "triangles": np.zeros((0, 3), np.int32), "vertex_source": np.zeros(0, np.int32),
            "face_source": np.zeros(0, np.int32), "face_flipped": np.zeros(0, bool), "stats": stats}


def repair(vertices, triangles, split=True, orient=True, min_component_faces=0, max_hole_edges=0, dedupe=True):
    """-> {"vertices", "triangles", "vertex_source", "face_source", "face_flipped", "stats"} as ops.repair_mesh returns them."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    nv = len(v)
    if max_hole_edges and not (split and orient):
        raise ValueError("fill needs the split and the orientation")
    stats = dict.fromkeys(STAT_KEYS, 0)
    # a. dedupe
    faces, seen = [], set()                         # faces: (original id, (a, b, c))
    for f in range(len(t)):
        tri = tuple(int(i) for i in t[f])
        if not (all(0 <= i < nv for i in tri) and len(set(tri)) == 3):
            stats["faces_invalid"] += 1
            continue
        if dedupe:
            if frozenset(tri) in seen:
                stats["faces_duplicate"] += 1
                continue
            seen.add(frozenset(tri))
        faces.append((f, tri))
    source = [f for f, _ in faces]
    tris = [list(tri) for _, tri in faces]
    vsource = list(range(nv))
    # b. split
    if split:
        stats["split_rounds"] = 1
        topo = TR.topology(v, np.array(tris, dtype=np.int64).reshape(-1, 3), normals=False)
        new_id, vsource = {}, []                    # (vertex, fan label) -> new id
        at = {}                                     # vertex -> the labels of its corners
        for f, tri in enumerate(tris):
            for k in range(3):
                at.setdefault(tri[k], set()).add(int(topo["corner_label"][3 * f + k]))
        for x in range(nv):
            labels = sorted(at.get(x, ()))
            for lab in labels:
                new_id[(x, lab)] = len(vsource)
                vsource.append(x)
            stats["vertices_split"] += max(len(labels) - 1, 0)
        tris = [[new_id[(tri[k], int(topo["corner_label"][3 * f + k]))] for k in range(3)] for f, tri in enumerate(tris)]
    # c. small components
    if min_component_faces > 0 and tris:
        comp = TR.topology(v[vsource], np.array(tris, dtype=np.int64).reshape(-1, 3), normals=False)["face_component"]
        size = {}
        for c in comp:
            size[int(c)] = size.get(int(c), 0) + 1
        keep = [f for f in range(len(tris)) if size[int(comp[f])] >= min_component_faces]
        stats["faces_small_component"] = len(tris) - len(keep)
        tris, source = [tris[f] for f in keep], [source[f] for f in keep]
        used = sorted({i for tri in tris for i in tri})
        remap = {old: new for new, old in enumerate(used)}
        tris, vsource = [[remap[i] for i in tri] for tri in tris], [vsource[i] for i in used]
    nt = len(tris)
    flipped = [False] * nt
    nonorientable = [False] * nt
    # d. orient
    if orient and nt:
        topo = TR.topology(v[vsource], np.array(tris, dtype=np.int64).reshape(-1, 3), normals=False)
        sets = TR._Sets(2 * nt)
        for e in range(len(topo["edges"])):
            cls = int(topo["edge_class"][e])
            if cls not in (2, 3):
                continue
            fa, fb = int(topo["edge_halfedges"][e, 0]) // 3, int(topo["edge_halfedges"][e, 1]) // 3
            cross = 1 if cls == 3 else 0
            sets.join(2 * fa, 2 * fb + cross)
            sets.join(2 * fa + 1, 2 * fb + 1 - cross)
        label = sets.labels()
        sides = {}                                  # the component's smallest face -> [faces on its side, faces on the other]
        for f in range(nt):
            l0, l1 = int(label[2 * f]), int(label[2 * f + 1])
            if l0 == l1:
                nonorientable[f] = True
                continue
            sides.setdefault(min(l0, l1) // 2, [0, 0])[0 if l0 < l1 else 1] += 1
        stats["components_nonorientable"] = len({int(label[2 * f]) for f in range(nt) if nonorientable[f]})
        for f in range(nt):
            l0, l1 = int(label[2 * f]), int(label[2 * f + 1])
            if l0 == l1:
                continue
            mine, other = sides[min(l0, l1) // 2]
            flipped[f] = (other > mine) if l0 < l1 else (mine >= other)
        stats["components_flipped"] = len({min(int(label[2 * f]), int(label[2 * f + 1])) // 2 for f in range(nt) if flipped[f]})
        tris = [[a, c, b] if flipped[f] else [a, b, c] for f, (a, b, c) in enumerate(tris)]
    # e. fill
    out_v = v[vsource]
    if max_hole_edges > 0 and nt:
        topo = TR.topology(out_v, np.array(tris, dtype=np.int64).reshape(-1, 3), normals=False)
        rim = TR._Sets(len(vsource))
        half = []                                   # the boundary half-edges in ascending id
        for e in range(len(topo["edges"])):
            if topo["edge_class"][e] == 1:
                rim.join(int(topo["edges"][e, 0]), int(topo["edges"][e, 1]))
                half.append(int(topo["edge_halfedges"][e, 0]))
        half.sort()
        name = rim.labels()
        loops = {}                                  # loop name -> its vertices in ascending id
        for x in range(len(vsource)):
            if topo["vertex_flags"][x] & 2:
                loops.setdefault(int(name[x]), []).append(x)
        barred = {int(name[tris[h // 3][h % 3]]) for h in half if nonorientable[h // 3]}
        faces_of = {}                               # loop name -> the faces its edges belong to
        for h in half:
            faces_of.setdefault(int(name[tris[h // 3][h % 3]]), set()).add(h // 3)
        barred |= {lab for lab, fs in faces_of.items() if len(fs) == 1}       # a lone triangle: its closing face would be its duplicate
        apex, extra = {}, []
        for lab in sorted(loops):
            members = loops[lab]
            if not 3 <= len(members) <= max_hole_edges or lab in barred:
                stats["loops_open"] += 1
                continue
            stats["loops_filled"] += 1
            if len(members) == 3:
                apex[lab] = None
                continue
            total = np.zeros(3)
            for x in members:
                total = total + out_v[x]
            apex[lab] = len(vsource) + len(extra)
            extra.append(total / float(len(members)))
        done = set()
        for h in half:
            a, b = tris[h // 3][h % 3], tris[h // 3][(h % 3 + 1) % 3]
            lab = int(name[a])
            if lab not in apex or lab in done:
                continue
            if apex[lab] is None:
                done.add(lab)
                c = [x for x in loops[lab] if x != a and x != b][0]
            else:
                c = apex[lab]
            tris.append([b, a, c])
            source.append(-1)
            flipped.append(False)
        stats["fill_faces"], stats["fill_vertices"] = len(tris) - nt, len(extra)
        if extra:
            out_v = np.concatenate([out_v, np.array(extra).reshape(-1, 3)])
            vsource = vsource + [-1] * len(extra)
    if not vsource and not tris:
        return _empty(stats)
    return {"vertices": np.ascontiguousarray(out_v).reshape(-1, 3), "triangles": np.array(tris, dtype=np.int32).reshape(-1, 3),
            "vertex_source": np.array(vsource, dtype=np.int32).reshape(-1), "face_source": np.array(source, dtype=np.int32).reshape(-1),
            "face_flipped": np.array(flipped, dtype=bool).reshape(-1), "stats": stats}


def report(out):
    return TR.topology(out["vertices"], out["triangles"], normals=False)["report"]


# ------------------------------------------------------------------------------------------------ shapes
def fin_octahedron():
    """A closed octahedron with one more triangle on its edge (0, 2)."""
    v, t = TR.octahedron()
    return np.concatenate([v, [[2.0, 2.0, 0.0]]]), np.concatenate([t, [[0, 2, 6]]]).astype(np.int32)


def cube_one_reversed():
    v, t = TR.cube()
    t = t.copy()
    t[5] = t[5, ::-1]
    return v, t


def cube_all_but_one_reversed():
    v, t = TR.cube()
    t = t[:, ::-1].copy()
    t[7] = t[7, ::-1]
    return v, t


def two_face_tie():
    v, _ = TR.tetrahedron()
    return v, np.array([[0, 1, 2], [0, 1, 3]], dtype=np.int32)          # both run 0 -> 1: a class-3 edge, one face a side


def moebius(n=9):
    """A strip of n quads closed with a half twist: 2 n vertices, 2 n faces, one boundary loop of 2 n edges."""
    v = []
    for i in range(n):
        ang = 2 * math.pi * i / n
        for s in (-0.3, 0.3):
            r = 1.0 + s * math.cos(0.5 * ang)
            v.append([r * math.cos(ang), r * math.sin(ang), s * math.sin(0.5 * ang)])
    t = []
    for i in range(n):
        a, b = 2 * i, 2 * i + 1
        c, d = (2 * (i + 1), 2 * (i + 1) + 1) if i + 1 < n else (1, 0)
        t += [(a, c, b), (b, c, d)]
    return np.array(v), np.array(t, dtype=np.int32)


def cube_minus_square():
    v, t = TR.cube()
    return v, t[2:].copy()


def tetrahedron_minus_face():
    v, t = TR.tetrahedron()
    return v, t[1:].copy()


def odd_soup():
    """A duplicated face, a reversed duplicate, [a, a, b], an index out of range, an unreferenced vertex."""
    v = np.concatenate([TR.tetrahedron()[0], [[2.0, 2.0, 2.0], [3.0, 3.0, 3.0]]])
    t = np.array([[0, 2, 1], [0, 2, 1], [1, 2, 0], [3, 3, 4], [0, 2, 9], [-1, 2, 3], [0, 1, 3], [2, 1, 0]], dtype=np.int32)
    return v, t


def cones(n):
    """n separate triangles that share vertex 0: n fans."""
    v = [[0.0, 0.0, 0.0]]
    for i in range(n):
        ang = 2 * math.pi * i / n
        v += [[math.cos(ang), math.sin(ang), 1.0], [math.cos(ang + 0.01), math.sin(ang + 0.01), 1.0 + 0.001 * i]]
    return np.array(v), np.array([(0, 1 + 2 * i, 2 + 2 * i) for i in range(n)], dtype=np.int32)


def disk(n):
    """A fan of n triangles about a hub: a rim of n edges."""
    v = [[0.0, 0.0, 0.0]] + [[math.cos(2 * math.pi * i / n), math.sin(2 * math.pi * i / n), 0.1 * math.sin(14 * math.pi * i / n)] for i in range(n)]
    return np.array(v), np.array([(0, 1 + i, 1 + (i + 1) % n) for i in range(n)], dtype=np.int32)


def strip_alternating(n):
    v, t = TR.strip(n)
    t = t.copy()
    t[1::2] = t[1::2, ::-1]
    return v, t


def islands(n):
    """n components, the k-th a strip of k faces."""
    vs, ts, base = [], [], 0
    for k in range(1, n + 1):
        v, t = TR.strip(k)
        vs.append(v + np.array([0.0, 3.0 * k, 0.0]))
        ts.append(t + base)
        base += len(v)
    return np.concatenate(vs), np.concatenate(ts).astype(np.int32)


def random_soup(seed):
    """A seeded triangle soup over few vertices: duplicates, edges with many faces, pinches, invalid faces, both windings."""
    rng = np.random.default_rng(seed)
    nv = int(rng.integers(4, 14))
    nt = int(rng.integers(1, 40))
    v = rng.uniform(-1.0, 1.0, size=(nv + 1, 3))
    t = rng.integers(0, nv, size=(nt, 3))
    if seed % 5 == 0:
        t[rng.integers(0, nt)] = [0, nv + 3, 1]
    if seed % 7 == 0:
        t[rng.integers(0, nt)] = [-2, 0, 1]
    return v, t.astype(np.int32)


def clustered_sphere(cell=2.5):
    """The marching-cubes sphere of the topology tests, vertex-clustered: pinches and non-manifold edges as the simplification makes them."""
    from . import mesh_simplify_reference as SR
    v, t = TR.mc_sphere(17)
    out = SR.simplify(v, t, cell, origin=(-0.5, -0.5, -0.5))
    return np.asarray(out["vertices"], dtype=np.float64), np.asarray(out["triangles"], dtype=np.int32)


DEFAULTS = {}
ALL_ON = {"min_component_faces": 2, "max_hole_edges": 8}


def hand_cases():
    """name -> (vertices, triangles, keywords)."""
    out = {
        "tetrahedra_vertex": (*TR.two_tetrahedra_vertex(), DEFAULTS),
        "tetrahedra_edge": (*TR.two_tetrahedra_edge(), DEFAULTS),
        "fin_dropped": (*fin_octahedron(), {"min_component_faces": 2}),
        "fin_kept": (*fin_octahedron(), DEFAULTS),
        "cube_one_reversed": (*cube_one_reversed(), DEFAULTS),
        "cube_all_but_one_reversed": (*cube_all_but_one_reversed(), DEFAULTS),
        "two_face_tie": (*two_face_tie(), DEFAULTS),
        "moebius": (*moebius(), {"max_hole_edges": 100}),
        "cube_hole_filled": (*cube_minus_square(), {"max_hole_edges": 4}),
        "cube_hole_open": (*cube_minus_square(), {"max_hole_edges": 3}),
        "tetrahedron_hole": (*tetrahedron_minus_face(), {"max_hole_edges": 3}),
        "odd_soup": (*odd_soup(), ALL_ON),
        "odd_soup_no_dedupe": (*odd_soup(), {"dedupe": False}),
        "cube_no_split_no_orient": (*cube_one_reversed(), {"split": False, "orient": False}),
        "empty": (np.zeros((0, 3)), np.zeros((0, 3), np.int32), ALL_ON),
        "no_faces": (TR.tetrahedron()[0], np.zeros((0, 3), np.int32), ALL_ON),
    }
    return out
