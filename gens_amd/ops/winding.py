"""K40: generalised winding numbers of a triangle mesh -- the sum of the solid angles its faces subtend at a point, over 4 pi -- exactly
or with a far field over clusters of 64 and 4096 faces whose error is bounded per query (build_winding_plan, winding_number), the inside
test built on them that never guesses (mesh_inside) and the sign it gives K36's distance (winding_sign; ops.signed_distance_to_mesh and
ops.mesh_distance with sign="winding").  Needs no connectivity: open, pinched, folded meshes and triangle soups all have a winding number.
The definition is the comment of K40 in include/gens_hip.h; tests/winding_reference.py restates it in numpy.

Part of gens_amd.ops (see ops/__init__.py)."""
import ctypes as C
import numbers

from .base import *  # noqa: F401,F403

_f64, _i32, _i64, _i8 = torch.float64, torch.int32, torch.int64, torch.int8
WINDING_LEAF = 64                      # faces per leaf, leaves per node (csrc/k40_mesh_winding.hip: K40_LEAF)
WINDING_SIGNS = ("pseudonormal", "winding")
MESH_DISTANCE_BETA = 6.0               # mesh_distance(sign="winding")'s default beta (the table that decided it)
_MORTON_INVALID = 1 << 30              # the key of a face that is not valid: after every 30-bit key


class WindingPlan:
    """What ops.build_winding_plan made, as device tensors (T faces, L = ceil(T / 64) leaves, K = ceil(L / 64) nodes; the definitions:
    include/gens_hip.h, K40): vertices (V, 3) float64, triangles (T, 3) int32; face_order (T) int32: the faces in Morton order of their
    centroids, faces that are not valid last; corners (64 L, 9) float64: the corners of the face at each position of that order (zeros for
    faces that are not valid); leaf_count (L) int32 (0: an empty leaf), leaf_area (L), leaf_normal (L, 3), leaf_centre (L, 3), leaf_radius2
    (L) float64, and the same five as node_* (K); n_vertices, n_faces, n_leaves, n_nodes."""

    def __init__(self, vertices, triangles):
        dev = vertices.device
        self.vertices, self.triangles = vertices, triangles
        self.n_vertices, self.n_faces = vertices.shape[0], triangles.shape[0]
        self.n_leaves = -(-self.n_faces // WINDING_LEAF)
        self.n_nodes = -(-self.n_leaves // WINDING_LEAF)
        self.face_order = torch.zeros(self.n_faces, device=dev, dtype=_i32)
        self.corners = torch.zeros(WINDING_LEAF * self.n_leaves, 9, device=dev, dtype=_f64)
        for level, m in (("leaf", self.n_leaves), ("node", self.n_nodes)):
            setattr(self, level + "_count", torch.zeros(m, device=dev, dtype=_i32))
            setattr(self, level + "_area", torch.zeros(m, device=dev, dtype=_f64))
            setattr(self, level + "_normal", torch.zeros(m, 3, device=dev, dtype=_f64))
            setattr(self, level + "_centre", torch.zeros(m, 3, device=dev, dtype=_f64))
            setattr(self, level + "_radius2", torch.zeros(m, device=dev, dtype=_f64))

    def args(self):
        a = L.WindingPlanArgs()
        a.vertices, a.triangles = self.vertices.data_ptr(), self.triangles.data_ptr()
        a.face_order, a.corners = self.face_order.data_ptr(), self.corners.data_ptr()
        for level in ("leaf", "node"):
            for name in ("count", "area", "normal", "centre", "radius2"):
                setattr(a, f"{level}_{name}", getattr(self, f"{level}_{name}").data_ptr())
        a.n_vertices, a.n_faces, a.n_leaves, a.n_nodes = self.n_vertices, self.n_faces, self.n_leaves, self.n_nodes
        return a


def _spread3(x):
    """The low 10 bits of x (int64) with two zero bits between neighbours."""
    x = x & 0x3FF
    x = (x | (x << 16)) & 0x30000FF
    x = (x | (x << 8)) & 0x300F00F
    x = (x | (x << 4)) & 0x30C30C3
    return (x | (x << 2)) & 0x9249249


def winding_face_order(vertices, triangles):
    """-> (face_order (T) int32, valid (T) bool): the faces stably sorted by the 30-bit Morton key of their centroid over the bounding box
    of the valid faces' centroids (x the most significant bit of each triple), faces that are not valid (K37's rule) last."""
    nv = vertices.shape[0]
    t = triangles.long()
    valid = ((t >= 0) & (t < nv)).all(dim=1) & (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 2] != t[:, 0])
    safe = torch.where(valid[:, None], t, torch.zeros_like(t))
    if nv == 0:
        return torch.arange(t.shape[0], device=t.device, dtype=_i32), valid
    a, b, c = vertices[safe[:, 0]], vertices[safe[:, 1]], vertices[safe[:, 2]]
    centroid = ((a + b) + c) / 3.0
    inf = torch.full_like(centroid, float("inf"))
    lo = torch.where(valid[:, None], centroid, inf).amin(dim=0)
    hi = torch.where(valid[:, None], centroid, -inf).amax(dim=0)
    span = hi - lo
    ok = torch.isfinite(span) & (span > 0.0)
    lo, span = torch.where(torch.isfinite(lo), lo, torch.zeros_like(lo)), torch.where(ok, span, torch.ones_like(span))
    cell = torch.nan_to_num((centroid - lo) / span * 1024.0, nan=0.0, posinf=1023.0, neginf=0.0).floor().clamp(0.0, 1023.0).to(_i64)
    key = (_spread3(cell[:, 0]) << 2) | (_spread3(cell[:, 1]) << 1) | _spread3(cell[:, 2])
    key = torch.where(valid, key, torch.full_like(key, _MORTON_INVALID))
    return torch.sort(key, stable=True)[1].to(_i32), valid


def build_winding_plan(vertices, triangles):
    """K40.  vertices (V, 3) float64, triangles (T, 3) int32 on the device -> WindingPlan: the faces in Morton order (keys and the stable
    sort in torch), and in one call of gens_mesh_winding_moments the faces' corners packed in that order and the area, area vector, centre
    and radius of every leaf (64 faces) and node (64 leaves).  Any indices are accepted: a face with an index outside the vertices or a
    repeated one has no solid angle and takes part in nothing.  The orientation is taken as given: an inside-out mesh has w = -1 inside and
    reads as "outside everywhere" (ops.repair_mesh re-orients).  One read-back (a flag).  ValueError before any launch of K40 for anything but
    such tensors, or a vertex of a valid face that is not finite."""
    who = "build_winding_plan"
    for name, t, dtype in (("vertices", vertices, _f64), ("triangles", triangles, _i32)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError(f"{who}: {name} is not a tensor on the device (gens_amd kernels have no CPU path)")
        if t.dtype != dtype or t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{who}: {name} is {tuple(t.shape)} {t.dtype}, expected (n, 3) {dtype}")
    if triangles.device != vertices.device:
        raise ValueError(f"{who}: vertices on {vertices.device}, triangles on {triangles.device}")
    if vertices.shape[0] >= 2 ** 31 or 3 * triangles.shape[0] >= 2 ** 31:
        raise ValueError(f"{who}: {vertices.shape[0]} vertices, {triangles.shape[0]} triangles (V and 3 T below 2^31)")
    plan = WindingPlan(_c(vertices.detach()), _c(triangles.detach()))
    if plan.n_faces == 0:
        return plan
    order, valid = winding_face_order(plan.vertices, plan.triangles)
    if plan.n_vertices:
        used = plan.vertices[torch.where(valid[:, None], plan.triangles, torch.zeros_like(plan.triangles)).long()]
        if not bool((torch.isfinite(used).all(dim=2).all(dim=1) | ~valid).all()):
            raise ValueError(f"{who}: a vertex of a valid face is not finite")
    plan.face_order = _c(order)
    L.call("gens_mesh_winding_moments", C.byref(plan.args()), L.stream(), nbytes=plan.n_faces * (16 + 72 + 72))
    return plan


def winding_beta(who, beta):
    """beta checked on the host -> 0.0 for None (exact), else the float.  ValueError unless it is None or a finite number > 1."""
    if beta is None:
        return 0.0
    value = float(beta) if isinstance(beta, numbers.Real) and not isinstance(beta, bool) else float("nan")
    if not (value > 1.0 and math.isfinite(value)):
        raise ValueError(f"{who}: beta = {beta!r}: None (exact) or a finite number > 1 (a cluster is replaced by its dipole beyond beta radii)")
    return value


def mesh_sign_request(who, signed=False, sign="pseudonormal", beta=None):
    """The sign keywords of mesh_distance, checked on the host -> (sign, beta as gens_mesh_winding_number takes it or None).  sign:
    "pseudonormal" (K37) or "winding" (K40); anything but the default needs signed=True; beta goes with "winding" only (None: the default,
    MESH_DISTANCE_BETA)."""
    if sign not in WINDING_SIGNS:
        raise ValueError(f"{who}: sign = {sign!r}: one of {', '.join(WINDING_SIGNS)}")
    if sign != "pseudonormal" and signed is not True:
        raise ValueError(f"{who}: sign = {sign!r} needs signed=True")
    if sign != "winding":
        if beta is not None:
            raise ValueError(f"{who}: beta goes with sign=\"winding\"")
        return sign, None
    return sign, winding_beta(who, MESH_DISTANCE_BETA if beta is None else beta)


def _check_queries(who, queries, plan, chunk):
    if not isinstance(plan, WindingPlan):
        raise ValueError(f"{who}: plan is {type(plan).__name__}, expected ops.build_winding_plan's WindingPlan")
    if not torch.is_tensor(queries) or not queries.is_cuda:
        raise ValueError(f"{who}: queries is not a tensor on the device (gens_amd kernels have no CPU path)")
    if queries.dtype != _f64 or queries.dim() != 2 or queries.shape[1] != 3:
        raise ValueError(f"{who}: queries is {tuple(queries.shape)} {queries.dtype}, expected (n, 3) {_f64}")
    if queries.device != plan.vertices.device:
        raise ValueError(f"{who}: queries on {queries.device}, the mesh on {plan.vertices.device}")
    if chunk is not None and (isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1):
        raise ValueError(f"{who}: chunk = {chunk!r}: a positive whole number of queries per launch, or None")
    if queries.shape[0] >= 2 ** 31:
        raise ValueError(f"{who}: {queries.shape[0]} queries (below 2^31)")


def winding_number(queries, plan, beta=None, bound=False, chunk=None, who="winding_number"):
    """K40.  queries (n, 3) float64 on the device, plan = ops.build_winding_plan(vertices, triangles) -> w (n) float64 [, bound (n) float64]:
    the generalised winding number of the mesh at every query -- 1 inside a closed mesh whose normals point outwards, 0 outside, -1 inside
    an inside-out one, a smooth fraction near holes; NaN for a query with a coordinate that is not finite.  A query on a vertex or a face
    gets what Van Oosterom and Strackee's formula gives there, which is finite (include/gens_hip.h, K40 (1)); nothing is special-cased.
    beta=None: exact, every face for every query -- T solid angles a query.  beta > 1: a node (4096 faces), else a leaf (64 faces), whose
    centre is farther than beta radii is replaced by its dipole; `bound` then holds, per query, a bound on |w - exact| that the kernel
    summed over the clusters it accepted (zeros in exact mode).  chunk: queries per launch (None: all in one); a query's bits depend on
    neither chunk, nor the other queries, nor the run.  Exact mode against a large mesh is long: give a chunk so that no launch holds the
    device for seconds.  No queries, or a mesh without faces, launch nothing: zeros (NaN for a query that is not finite).
    ValueError before any launch for queries that are not an (n, 3) float64 tensor on the mesh's device, a plan that is no WindingPlan, a
    beta that is neither None nor a finite number > 1, a bound that is no bool, a chunk that is no positive int."""
    _check_queries(who, queries, plan, chunk)
    b = winding_beta(who, beta)
    if not isinstance(bound, bool):
        raise ValueError(f"{who}: bound = {bound!r}: True or False")
    q = _c(queries.detach())
    n, dev = q.shape[0], q.device
    w = torch.zeros(n, device=dev, dtype=_f64)
    err = torch.zeros(n, device=dev, dtype=_f64) if bound else None
    if n and plan.n_faces == 0:
        bad = ~torch.isfinite(q).all(dim=1)
        w[bad] = float("nan")
        if bound:
            err[bad] = float("nan")
    elif n:
        args = plan.args()
        step = n if chunk is None else chunk
        for s in range(0, n, step):
            m = min(step, n - s)
            L.call("gens_mesh_winding_number", C.byref(args), C.c_void_p(q.data_ptr() + 24 * s), m, b, C.c_void_p(w.data_ptr() + 8 * s),
                   None if err is None else C.c_void_p(err.data_ptr() + 8 * s), L.stream(), nbytes=m * (32 + (8 if bound else 0)))
    return (w, err) if bound else w


def mesh_inside(queries, plan, beta=None, chunk=None, who="mesh_inside"):
    """K40's inside test.  -> (n) int8: 1 (inside) where w - bound >= 0.5, 0 (outside) where w + bound < 0.5, -1 (undecided) otherwise --
    the far field's bound straddles one half, or the query is not finite.  With beta=None the bound is zero and only such queries are
    undecided.  It never guesses: an undecided query is one that a smaller error (a larger beta, or None) would decide.  The orientation
    is taken as given: everything is outside an inside-out mesh.  Arguments and refusals: winding_number's."""
    w, err = winding_number(queries, plan, beta, True, chunk, who=who)
    out = torch.full(w.shape, -1, device=w.device, dtype=_i8)
    out[w - err >= 0.5] = 1
    out[w + err < 0.5] = 0
    return out


def winding_sign(dist2, inside):
    """K36's squared distances with mesh_inside's verdicts -> signed (n) float64: -d where inside is 1, +d where it is 0, NaN where it is -1
    or dist2 is not finite (nothing within max_dist), +0 where d is 0 (on the mesh)."""
    d = torch.sqrt(dist2)
    nan = torch.full_like(d, float("nan"))
    signed = torch.where(inside == 1, -d, torch.where(inside == 0, d, nan))
    signed = torch.where(torch.isfinite(dist2), signed, nan)
    return torch.where(d == 0.0, torch.zeros_like(d), signed)


__all__ = [n_ for n_ in dir() if not n_.startswith("__")]
