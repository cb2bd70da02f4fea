"""Reference for K41 (self-intersections of a triangle mesh) in exact rational arithmetic -- fractions.Fraction over the float64 coordinates --
written from the SET definition of include/gens_hip.h (K41, definitions 1 to 3), not from the predicate form the kernel evaluates:

  a face is the closed convex hull of its corners; the face Ts is clipped, as a polygon, against the two half-spaces of the plane of Tt and
  the three edge half-spaces of Tt (Sutherland-Hodgman); what survives are the corners of Ts n Tt, whose convex hull is that set.  The pair
  intersects iff there is a surviving point (k = 0 shared indices), one that is not the shared vertex's position (k = 1), one that is not on
  the shared edge (k = 2): a convex set lies inside a point or a segment iff its corners do.

Brute force over all pairs behind a numpy AABB prefilter (float64 min / max and <= are exact).  Results are cached per mesh.

DELICATE (part of the contract, not a measurement): a candidate pair is delicate when some orient3d over four distinct corners of the pair has
|D| <= 2^-40 P, or, for k = 2, the dot product of the two normals about the shared edge is that close to zero; D is the exact value and P the
exact permanent, the sum of the absolute values of the terms of the expansion in coordinate differences against a pivot corner.  An orient3d
of four corners can be written with any of them as the pivot -- the same D up to sign, another P -- and "some orient3d" takes them all: the
largest P counts.  A face is delicate when every component of (b - a) x (c - a) has |D| <= 2^-40 P in the same sense -- the analogue of
the kernel's UNCERTAIN, "no component is certainly non-zero" (a degenerate face is delicate too).  2^-40 leaves a factor of
about a thousand over any sound c 2^-53 of a float64 filter.

SHORT: every coordinate is k 2^-4 with |k| <= 2^10; every float64 operation of every predicate (degree <= 4: 12 + 12 + 1 + 12 + 2 bits for
orient3d, 2 (12 + 12 + 1) + 2 for the dot product) is then exact."""
import functools
import itertools
from fractions import Fraction

import numpy as np

DELICATE = Fraction(1, 2 ** 40)
INTERSECTING, DISJOINT = 1, 0


def face_valid(vertices, triangles):
    nv = len(np.asarray(vertices).reshape(-1, 3))
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    return ((t >= 0) & (t < nv)).all(axis=1) & (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 2] != t[:, 0])


def is_short(vertices):
    v = np.asarray(vertices, dtype=np.float64)
    k = v * 16.0
    return bool(np.isfinite(v).all() and (k == np.round(k)).all() and (np.abs(k) <= 1024).all())


def _sub(p, q):
    return (p[0] - q[0], p[1] - q[1], p[2] - q[2])


def _cross(u, w):
    return (u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0])


def _dot(u, w):
    return u[0] * w[0] + u[1] * w[1] + u[2] * w[2]


def _clip(poly, normal, origin):
    """Sutherland-Hodgman: the closed polygon `poly` (a list of points; one or two points are a point or a segment) against the closed
    half-space normal . (x - origin) >= 0."""
    out = []
    side = [_dot(normal, _sub(p, origin)) for p in poly]
    for i, p in enumerate(poly):
        j = (i + 1) % len(poly)
        if side[i] >= 0:
            out.append(p)
        if (side[i] > 0 and side[j] < 0) or (side[i] < 0 and side[j] > 0):
            s = Fraction(side[i], side[i] - side[j])
            q = poly[j]
            out.append((p[0] + s * (q[0] - p[0]), p[1] + s * (q[1] - p[1]), p[2] + s * (q[2] - p[2])))
    return out


def common_points(ts, tt):
    """The corners of Ts n Tt (maybe repeated; empty: disjoint): ts, tt triples of exact points, tt not degenerate."""
    a, b, c = tt
    n = _cross(_sub(b, a), _sub(c, a))
    poly = _clip(list(ts), n, a)
    poly = _clip(poly, (-n[0], -n[1], -n[2]), a) if poly else poly
    for p, q in ((a, b), (b, c), (c, a)):
        if not poly:
            break
        poly = _clip(poly, _cross(n, _sub(q, p)), p)      # in the plane, at right angles to the edge, towards the third corner
    return poly


def _on_segment(x, a, b):
    u, w = _sub(b, a), _sub(x, a)
    return _cross(u, w) == (0, 0, 0) and 0 <= _dot(u, w) <= _dot(u, u)


def pair_intersects(points, s_row, t_row):
    """points: exact positions by vertex index; s_row, t_row: the index rows of two valid faces that are not degenerate, sharing k < 3."""
    shared = [i for i in s_row if i in t_row]
    common = common_points([points[i] for i in s_row], [points[i] for i in t_row])
    if len(shared) == 0:
        return bool(common)
    if len(shared) == 1:
        return any(p != points[shared[0]] for p in common)
    return any(not _on_segment(p, points[shared[0]], points[shared[1]]) for p in common)


def _orient3d_terms(a, b, c, d):
    """-> (D, P) of orient3d with the pivot d: D the determinant of (a - d, b - d, c - d), P its permanent."""
    u, v, w = _sub(a, d), _sub(b, d), _sub(c, d)
    det = u[2] * (v[0] * w[1] - w[0] * v[1]) + v[2] * (w[0] * u[1] - u[0] * w[1]) + w[2] * (u[0] * v[1] - v[0] * u[1])
    perm = (abs(u[2]) * (abs(v[0] * w[1]) + abs(w[0] * v[1])) + abs(v[2]) * (abs(w[0] * u[1]) + abs(u[0] * w[1])) +
            abs(w[2]) * (abs(u[0] * v[1]) + abs(v[0] * u[1])))
    return det, perm


def orient3d_delicate(quad):
    det = abs(_orient3d_terms(*quad)[0])
    return any(det <= DELICATE * _orient3d_terms(*(quad[:p] + quad[p + 1:] + quad[p:p + 1]))[1] for p in range(4))


def _fold_dot_terms(a, b, c, d):
    u, w, x = _sub(b, a), _sub(c, a), _sub(d, a)
    det = perm = 0
    for k in range(3):
        i, j = (k + 1) % 3, (k + 2) % 3
        det += (u[i] * w[j] - u[j] * w[i]) * (u[i] * x[j] - u[j] * x[i])
        perm += (abs(u[i] * w[j]) + abs(u[j] * w[i])) * (abs(u[i] * x[j]) + abs(u[j] * x[i]))
    return det, perm


def pair_delicate(points, s_row, t_row):
    corners = sorted(set(s_row) | set(t_row))
    if any(orient3d_delicate(tuple(points[i] for i in quad)) for quad in itertools.combinations(corners, 4)):
        return True
    shared = [i for i in s_row if i in t_row]
    if len(shared) == 2:
        c = next(i for i in s_row if i not in shared)
        d = next(i for i in t_row if i not in shared)
        for a, b in (shared, shared[::-1]):
            det, perm = _fold_dot_terms(points[a], points[b], points[c], points[d])
            if abs(det) <= DELICATE * perm:
                return True
    return False


def _normal_components(a, b, c):
    """-> [(D, P)] of the three components of (b - a) x (c - a), pivot a."""
    u, w = _sub(b, a), _sub(c, a)
    return [(u[i] * w[j] - u[j] * w[i], abs(u[i] * w[j]) + abs(u[j] * w[i])) for i, j in ((1, 2), (2, 0), (0, 1))]


def face_delicate(a, b, c):
    """No component of the normal is robustly away from zero: each has |D| <= 2^-40 P for some pivot."""
    by_pivot = [_normal_components(*pivot) for pivot in ((a, b, c), (b, c, a), (c, a, b))]
    return all(any(abs(parts[k][0]) <= DELICATE * parts[k][1] for parts in by_pivot) for k in range(3))


class Report:
    """faces, invalid_faces, degenerate_faces, duplicate_pairs, candidates: ints; degenerate (T) bool; face_delicate (T) bool (False for
    faces that are not valid); pairs: {(s, t): (intersects, delicate, k)} over all candidates, s < t."""


def _key(vertices, triangles):
    v, t = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3), np.ascontiguousarray(triangles, dtype=np.int64).reshape(-1, 3)
    return v.tobytes(), t.tobytes()


@functools.lru_cache(maxsize=None)
def _analyse(vbytes, tbytes):
    v = np.frombuffer(vbytes, dtype=np.float64).reshape(-1, 3)
    t = np.frombuffer(tbytes, dtype=np.int64).reshape(-1, 3)
    rep = Report()
    valid = face_valid(v, t)
    rep.faces, rep.invalid_faces = len(t), int((~valid).sum())
    # every finite float64 is an integer over a power of two: over the largest such power the coordinates are Python integers, which all
    # the tests below are homogeneous in (only the cut points of the clipping are fractions)
    scale = max([Fraction(float(x)).denominator for x in v[np.isfinite(v)].ravel()], default=1)
    points = [tuple(int(Fraction(float(x)) * scale) for x in row) if np.isfinite(row).all() else None for row in v]
    rep.degenerate = np.zeros(len(t), dtype=bool)
    rep.face_delicate = np.zeros(len(t), dtype=bool)
    for f in np.nonzero(valid)[0]:
        a, b, c = (points[i] for i in t[f])
        rep.degenerate[f] = _cross(_sub(b, a), _sub(c, a)) == (0, 0, 0)
        rep.face_delicate[f] = face_delicate(a, b, c)
    rep.degenerate_faces = int(rep.degenerate.sum())
    live = np.nonzero(valid & ~rep.degenerate)[0]
    rep.pairs, rep.duplicate_pairs = {}, 0
    if len(live):
        corners = v[t[live]]
        lo, hi = corners.min(axis=1), corners.max(axis=1)
        for n, s in enumerate(live):
            near = ((lo[n] <= hi[n + 1:]) & (lo[n + 1:] <= hi[n])).all(axis=1)
            s_row = tuple(int(i) for i in t[s])
            for f in live[n + 1:][near]:
                t_row = tuple(int(i) for i in t[f])
                k = len(set(s_row) & set(t_row))
                if k == 3:
                    rep.duplicate_pairs += 1
                    continue
                rep.pairs[(int(s), int(f))] = (pair_intersects(points, s_row, t_row), pair_delicate(points, s_row, t_row), k)
    rep.candidates = len(rep.pairs)
    rep.intersecting = sum(1 for hit, _, _ in rep.pairs.values() if hit)
    rep.delicate = sum(1 for _, d, _ in rep.pairs.values() if d)
    return rep


def analyse(vertices, triangles):
    """-> Report of the mesh (cached).  Indices outside the vertices make a face not valid."""
    return _analyse(*_key(vertices, triangles))


# ------------------------------------------------------------------------------------------------ small meshes of the tests
def joined(*meshes):
    """Meshes side by side, no vertex shared."""
    vs, ts, base = [], [], 0
    for v, t in meshes:
        vs.append(np.asarray(v, dtype=np.float64).reshape(-1, 3))
        ts.append(np.asarray(t, dtype=np.int64).reshape(-1, 3) + base)
        base += len(vs[-1])
    return np.concatenate(vs), np.concatenate(ts).astype(np.int32)


def shifted(mesh, offset):
    return np.asarray(mesh[0], dtype=np.float64) + np.asarray(offset, dtype=np.float64)[None, :], mesh[1]


def flat_fold(lift=0.0):
    """Two faces on the edge (0, 1) with the opposite corners on the same side in one plane (lift = 0): a fold; lift raises one corner."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0.25, 1, 0], [0.75, 0.5, lift]], dtype=np.float64)
    return v, np.array([(0, 1, 2), (1, 0, 3)], dtype=np.int32)


def pierced_at_vertex():
    """k = 1: the faces share vertex 0 and the edge (3, 4) of the second pierces the first."""
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [0.5, 0.5, -1], [0.5, 0.5, 1]], dtype=np.float64)
    return v, np.array([(0, 1, 2), (0, 3, 4)], dtype=np.int32)


def coplanar_wedges():
    """k = 1: two faces in the plane z = 0 about vertex 0 whose wedges overlap."""
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [2, 1, 0], [1, 2, 0]], dtype=np.float64)
    return v, np.array([(0, 1, 2), (0, 3, 4)], dtype=np.int32)


def unwelded_touch():
    """Two faces that touch at one position held by two vertices (2 and 3): no index is shared, so they intersect (k = 0)."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 1, 0], [0, 2, 0], [0, 1, 1]], dtype=np.float64)
    return v, np.array([(0, 1, 2), (3, 4, 5)], dtype=np.int32)


def degenerate_faces():
    """An ordinary face, a face with two corners at one position (vertices 3 and 4) and a collinear face."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 2, 2], [2, 2, 2], [3, 0, 1], [0, 0, 4], [1, 1, 5], [2, 2, 6]], dtype=np.float64)
    return v, np.array([(0, 1, 2), (3, 4, 5), (6, 7, 8)], dtype=np.int32)


def fan_through_cell(n):
    """n thin faces through the z axis, no vertex shared: face i runs from (x_i, 8, z_i) to (-x_i, -8, z_i) with x_i = -8 + i / 16, so all
    of them cross the grid's middle cell; z_i = i / 1024 and a third corner 3 / 1024 higher, so only neighbours in i have overlapping
    boxes (the exact reference stays quick).  Coordinates are multiples of 2^-10 below 2^4: every float64 operation of every predicate is
    still exact (15 + 15 + 1 + 15 + 2 bits)."""
    v, t = [], []
    for i in range(n):
        x, z = -8.0 + i / 16.0, i / 1024.0
        v += [[x, 8.0, z], [-x, -8.0, z], [-x + 0.0625, -8.0, z + 3.0 / 1024.0]]
        t.append((3 * i, 3 * i + 1, 3 * i + 2))
    return np.array(v, dtype=np.float64), np.array(t, dtype=np.int32)


def big_face_beside_small():
    """One face spanning the whole grid under a lattice sheet of small ones (at z = 0.5 above it, so nothing intersects) and cutting a second
    small sheet that crosses it."""
    v, t = [], []
    n = 7
    for z in (0.5,):
        base = len(v)
        v += [[float(x), float(y), z] for y in range(n) for x in range(n)]
        for y in range(n - 1):
            for x in range(n - 1):
                a = base + y * n + x
                t += [(a, a + 1, a + n + 1), (a, a + n + 1, a + n)]
    base = len(v)
    v += [[-1.0, -1.0, 0.0], [15.0, -1.0, 0.0], [-1.0, 15.0, 0.0]]
    t.append((base, base + 1, base + 2))
    base = len(v)
    v += [[1.0, 1.0, -0.5], [2.0, 1.0, 0.25], [1.0, 2.0, 0.25]]          # a small face through the big one
    t.append((base, base + 1, base + 2))
    return np.array(v, dtype=np.float64), np.array(t, dtype=np.int32)


def near_miss(ulps):
    """A face at coordinates that are not short in the plane z = x / 4 -- exactly: a quarter of a float64 is one -- and a second face one of
    whose corners lies `ulps` units in the last place above (below: negative; 0: exactly on) that plane, over the inside of the first face;
    the second face's other corners are well above it.  Above: disjoint; on or below: they intersect."""
    px = 1.0101017
    z = px / 4.0
    for _ in range(abs(ulps)):
        z = float(np.nextafter(z, np.inf if ulps > 0 else -np.inf))
    v = np.array([[0.1234567, 0.2345678, 0.1234567 / 4.0], [3.1415926, 0.3456789, 3.1415926 / 4.0], [0.4567891, 2.7182818, 0.4567891 / 4.0],
                  [px, 0.9090909, z], [1.3131313, 1.0101013, 1.3131313 / 4.0 + 0.37], [0.9191919, 1.2121212, 0.9191919 / 4.0 + 0.41]],
                 dtype=np.float64)
    return v, np.array([(0, 1, 2), (3, 4, 5)], dtype=np.int32)
