"""K39: mesh fairing on the device: Laplacian and Taubin smoothing with uniform or cotangent weights (smooth_mesh), the vertex Laplacian
(mesh_laplacian), the per-edge weights (smoothing_weights) and the dihedral roughness of the edges (mesh_roughness).  The rules are the
comment of K39 in include/gens_hip.h; tests/mesh_smooth_reference.py restates them in numpy with dicts and loops.

Part of gens_amd.ops (see ops/__init__.py)."""
from .base import *  # noqa: F401,F403
from .mesh_topology import VERTEX_BOUNDARY, VERTEX_REFERENCED, MeshTopology, _check_mesh, area_volume, mesh_topology

_f64, _i32, _i64, _u8 = torch.float64, torch.int32, torch.int64, torch.uint8
SMOOTH_KEYS = ("iterations", "lam", "mu", "weights", "fix_boundary", "measure")
SMOOTH_WEIGHTS = ("uniform", "cotangent")
ROUGHNESS_KEYS = ("edges", "mean", "rms", "max")

smooth_section_hook = None             # a callable(name), called where a stage of smooth_mesh begins (scripts/mesh_smooth_bench.py records HIP events there)


def _smooth_section(name):
    if smooth_section_hook is not None:
        smooth_section_hook(name)


def _real(x):
    return isinstance(x, (int, float)) and not isinstance(x, bool) and x == x and abs(x) != float("inf")


def smooth_request(x, who="smooth"):
    """The options of smooth_mesh, checked: True (the defaults) or a dict of iterations, lam, mu, weights, fix_boundary, measure -> the dict
    with every key.  ValueError for anything else, an unknown keyword, iterations that are no whole number in 0 ... 1000, a lam outside
    (0, 1], a mu that is neither 0 nor in [-2, -lam), weights that are neither "uniform" nor "cotangent", a switch that is no bool."""
    if x is True:
        x = {}
    if not isinstance(x, dict) or not all(isinstance(k, str) for k in x):
        raise ValueError(f"{who} = {x!r}: True, or a dict of {', '.join(SMOOTH_KEYS)}")
    unknown = sorted(set(x) - set(SMOOTH_KEYS))
    if unknown:
        raise ValueError(f"{who}: unknown keyword {unknown[0]!r} (smoothing takes {', '.join(SMOOTH_KEYS)})")
    opt = {"iterations": 10, "lam": 0.5, "mu": -0.53, "weights": "uniform", "fix_boundary": True, "measure": False, **x}
    n, lam, mu = opt["iterations"], opt["lam"], opt["mu"]
    if isinstance(n, bool) or not isinstance(n, int) or not 0 <= n <= 1000:
        raise ValueError(f"{who}: iterations = {n!r}: a whole number from 0 to 1000")
    if not _real(lam) or not 0.0 < lam <= 1.0:
        raise ValueError(f"{who}: lam = {lam!r}: a number above 0 and up to 1")
    if not _real(mu) or not (mu == 0 or -2.0 <= mu < -lam):
        raise ValueError(f"{who}: mu = {mu!r}: 0 (plain Laplacian smoothing) or a number from -2 to below -lam = {-lam!r}")
    if not isinstance(opt["weights"], str) or opt["weights"] not in SMOOTH_WEIGHTS:
        raise ValueError(f"{who}: weights = {opt['weights']!r}: one of {', '.join(SMOOTH_WEIGHTS)}")
    for name in ("fix_boundary", "measure"):
        if not isinstance(opt[name], bool):
            raise ValueError(f"{who}: {name} = {opt[name]!r}: True or False")
    opt["lam"], opt["mu"] = float(lam), float(mu)
    return {k: opt[k] for k in SMOOTH_KEYS}


def _check_weights(who, weights):
    if not isinstance(weights, str) or weights not in SMOOTH_WEIGHTS:
        raise ValueError(f"{who}: weights = {weights!r}: one of {', '.join(SMOOTH_WEIGHTS)}")


def _check_topology(who, vertices, triangles, topology):
    """The topology a fairing call was given: ValueError unless it is ops.mesh_topology's of a mesh of these sizes on this device."""
    if not isinstance(topology, MeshTopology):
        raise ValueError(f"{who}: topology is {type(topology).__name__}, expected ops.mesh_topology's MeshTopology")
    if topology.n_vertices != vertices.shape[0] or topology.n_faces != triangles.shape[0]:
        raise ValueError(f"{who}: the topology is of another mesh ({topology.n_vertices} vertices, {topology.n_faces} faces; this mesh has "
                         f"{vertices.shape[0]} and {triangles.shape[0]})")
    if topology.vertices.device != vertices.device:
        raise ValueError(f"{who}: the topology on {topology.vertices.device}, the mesh on {vertices.device}")


def mesh_neighbours(topology):
    """Definition 1: the neighbour lists of K37's edge table -> (nbr_start (V + 1) int32, nbr_vertex (2 E) int32, nbr_edge (2 E) int32), the
    neighbours of a vertex in ascending index.  One sort of the 2 E keys (from << 32) | to; cached on the topology."""
    if getattr(topology, "_neighbours", None) is not None:
        return topology._neighbours
    dev, nv, ne = topology.vertices.device, topology.n_vertices, topology.n_edges
    lo, hi = topology.edges[:, 0].long(), topology.edges[:, 1].long()
    key, order = torch.sort(torch.cat([(lo << 32) | hi, (hi << 32) | lo]))                  # (the keys are distinct: no ties to break)
    edge_id = torch.arange(ne, device=dev, dtype=_i32)
    nbr_vertex = _c((key & 0xFFFFFFFF).to(_i32))
    nbr_edge = _c(torch.cat([edge_id, edge_id])[order])
    nbr_start = _c(torch.searchsorted(key, torch.arange(nv + 1, device=dev, dtype=_i64) << 32).to(_i32))
    topology._neighbours = (nbr_start, nbr_vertex, nbr_edge)
    return topology._neighbours


def smoothing_weights(topology, weights="uniform"):
    """Definition 2: the weight of every edge of `topology` (ops.mesh_topology's) from the positions it was built with -> (E) float64: ones for
    "uniform"; for "cotangent" the clamped sum of the cotangents opposite the edge, over its uses in ascending half-edge
    (gens_mesh_corner_cot, gens_mesh_edge_weights).  ValueError before any launch for another name or another type."""
    who = "smoothing_weights"
    _check_weights(who, weights)
    if not isinstance(topology, MeshTopology):
        raise ValueError(f"{who}: topology is {type(topology).__name__}, expected ops.mesh_topology's MeshTopology")
    if weights == "uniform":
        return torch.ones(topology.n_edges, device=topology.vertices.device, dtype=_f64)
    return _cotangent_weights(topology, topology.vertices)


def _cotangent_weights(tp, vertices):
    """The cotangent weights of tp's edges at the positions `vertices` (V, 3) float64 (the topology gives the triangles and the runs)."""
    dev, nv, nt, ne = vertices.device, tp.n_vertices, tp.n_faces, tp.n_edges
    cot = torch.empty(3 * nt, device=dev, dtype=_f64)
    weight = torch.empty(ne, device=dev, dtype=_f64)
    if nt:
        L.call("gens_mesh_corner_cot", L.ptr(vertices, _f64), L.ptr(tp.triangles, _i32), nv, nt, L.ptr(cot, _f64), L.stream(), nbytes=nt * 156)
    if ne:
        L.call("gens_mesh_edge_weights", L.ptr(cot, _f64), L.ptr(tp.edge_start, _i32), L.ptr(tp.halfedge_order, _i32), ne, 3 * nt,
               L.ptr(weight, _f64), L.stream(), nbytes=ne * 12 + nt * 36)
    return weight


def step_bytes(n_vertices, n_edges, weighted):
    """The algorithmic bytes of one gens_mesh_laplacian_step: a position read and written and the segment bounds per vertex, an index, an
    edge id and a position (and a weight) per neighbour."""
    return n_vertices * (48 + 8) + 2 * n_edges * (4 + 4 + 24 + (8 if weighted else 0))


def _step(src, nbrs, weight, n_edges, pinned, factor, out=None, delta=None, weight_sum=None):
    nv = src.shape[0]
    L.call("gens_mesh_laplacian_step", L.ptr(src, _f64), nv, L.ptr(nbrs[0], _i32), L.ptr(nbrs[1], _i32), L.ptr(nbrs[2], _i32), 2 * n_edges,
           L.ptr(weight, _f64), n_edges, L.ptr(pinned, _u8), float(factor), L.ptr(out, _f64), L.ptr(delta, _f64), L.ptr(weight_sum, _f64),
           L.stream(), nbytes=step_bytes(nv, n_edges, weight is not None))


def mesh_laplacian(vertices, triangles, weights="uniform", topology=None):
    """Definition 3.  vertices (V, 3) float64, triangles (T, 3) int32 on the device -> (delta (V, 3) float64, weight_sum (V) float64): for
    every vertex the weighted mean of its neighbours minus the vertex, and the sum of the weights; zeros where the sum is not positive and
    finite.  One gens_mesh_laplacian_step launch with no `out`.  topology: ops.mesh_topology's of these triangles, if the caller has it;
    only its connectivity is used: positions, cotangent weights included, are taken from `vertices`.  ValueError before any launch for what ops.mesh_topology refuses, other weights or a topology of another mesh."""
    who = "mesh_laplacian"
    _check_mesh(who, vertices, triangles)
    _check_weights(who, weights)
    if topology is not None:
        _check_topology(who, vertices, triangles, topology)
    v = _c(vertices.detach())
    topo = mesh_topology(v, _c(triangles.detach())) if topology is None else topology
    nv = v.shape[0]
    delta, weight_sum = torch.zeros(nv, 3, device=v.device, dtype=_f64), torch.zeros(nv, device=v.device, dtype=_f64)
    if nv:
        weight = _cotangent_weights(topo, v) if weights == "cotangent" else None
        _step(v, mesh_neighbours(topo), weight, topo.n_edges, None, 0.0, delta=delta, weight_sum=weight_sum)
    return delta, weight_sum


def _face_normals(topo, vertices):
    """K37's unit face normals of topo's triangles at `vertices` (gens_mesh_pseudonormals over the topology's own segments)."""
    nv, nt, ne = topo.n_vertices, topo.n_faces, topo.n_edges
    dev = vertices.device
    face, edge, vert = (torch.empty(n, 3, device=dev, dtype=_f64) for n in (nt, ne, nv))
    if nt or nv:
        L.call("gens_mesh_pseudonormals", L.ptr(vertices, _f64), L.ptr(topo.triangles, _i32), nv, nt, ne, L.ptr(topo.edge_start, _i32),
               L.ptr(topo.halfedge_order, _i32), L.ptr(topo.corner_start, _i32), L.ptr(topo.corner_order, _i32), L.ptr(face, _f64),
               L.ptr(edge, _f64), L.ptr(vert, _f64), L.stream(), nbytes=nt * 108 + ne * 24 + nv * 24 + nt * 96)
    return face


def _dihedral(topo, face_normal):
    ne = topo.n_edges
    angle = torch.empty(ne, device=face_normal.device, dtype=_f64)
    if ne:
        L.call("gens_mesh_dihedral", L.ptr(face_normal, _f64), topo.n_faces, L.ptr(topo.edge_halfedges, _i32), L.ptr(topo.edge_class, _u8), ne,
               L.ptr(angle, _f64), L.stream(), nbytes=ne * 65)
    return angle


def _roughness_figures(angle):
    """(edges, mean, rms, max) over the finite angles as a (4) float64 device tensor (NaN where there are none)."""
    finite = torch.isfinite(angle)
    n = finite.sum().to(_f64)
    a = torch.where(finite, angle, torch.zeros_like(angle))
    nan = torch.full((), float("nan"), device=angle.device, dtype=_f64)
    some = n > 0
    return torch.stack([n, torch.where(some, a.sum() / n, nan), torch.where(some, (a.square().sum() / n).sqrt(), nan),
                        torch.where(some, a.max() if angle.numel() else nan, nan)])


def _roughness_report(figures):
    return {"edges": int(figures[0]), "mean": float(figures[1]), "rms": float(figures[2]), "max": float(figures[3])}


def mesh_roughness(vertices, triangles, topology=None):
    """Definition 7.  vertices (V, 3) float64, triangles (T, 3) int32 on the device -> (angle (E) float64, report): per edge of K37's table
    the angle between the unit normals of its two faces (0 on a flat mesh), NaN unless the edge has class 2 and both normals are non-zero;
    report = {"edges", "mean", "rms", "max"} over the finite angles (NaN with "edges" 0 where there are none), in one read-back.
    topology: ops.mesh_topology's of these triangles, with or without normals; only its connectivity is used: the face normals are
    computed from `vertices` (so the topology of a mesh before it was smoothed serves the smoothed one).  ValueError before any launch for
    what ops.mesh_topology refuses or a topology of another mesh."""
    who = "mesh_roughness"
    _check_mesh(who, vertices, triangles)
    if topology is not None:
        _check_topology(who, vertices, triangles, topology)
    v = _c(vertices.detach())
    topo = mesh_topology(v, _c(triangles.detach()), normals=True) if topology is None else topology
    angle = _dihedral(topo, topo.face_normal if topology is None else _face_normals(topo, v))
    return angle, _roughness_report(_roughness_figures(angle).cpu().tolist())


def smooth_mesh(vertices, triangles, iterations=10, lam=0.5, mu=-0.53, weights="uniform", fix_boundary=True, pinned=None, measure=False,
                topology=None):
    """K39.  vertices (V, 3) float64, triangles (T, 3) int32 on the device, any indices -> (vertices' (V, 3) float64, triangles, stats).
    `iterations` times: every vertex moves by lam times its Laplacian (the weighted mean of its neighbours over K37's edges, minus the
    vertex), then, unless mu == 0, by mu times the Laplacian of the moved mesh (Taubin's lambda | mu smoothing, which does not shrink; mu = 0
    is plain Laplacian smoothing, which does).  weights: "uniform" or "cotangent" (from the input positions, kept through all iterations,
    negative sums clamped to 0).  Pinned vertices stay bit for bit: pinned (V) bool, if given, and with fix_boundary every vertex on a
    boundary edge; so do unreferenced vertices.  The triangles come back as they came.  stats: iterations, weights, pinned, moved
    (vertices with a changed bit), displacement_max / _mean / _rms over the vertices that are neither pinned nor unreferenced (NaN if none);
    with measure=True also area_before / _after, volume_before / _after (report()'s expressions) and roughness_before / _after
    (mesh_roughness's report); one read-back.  topology: ops.mesh_topology's of these triangles, if the caller has it; only its
    connectivity is used: weights, areas, volumes and normals are computed from `vertices`.  Deterministic: two
    buffers, one thread per vertex, no atomics.  ValueError before any launch for what ops.mesh_topology or smooth_request refuses, a
    `pinned` that is no (V) bool tensor on the device, or a topology of another mesh."""
    who = "smooth_mesh"
    _check_mesh(who, vertices, triangles)
    opt = smooth_request({"iterations": iterations, "lam": lam, "mu": mu, "weights": weights, "fix_boundary": fix_boundary, "measure": measure}, who)
    if pinned is not None and (not torch.is_tensor(pinned) or pinned.dtype != torch.bool or pinned.shape != (vertices.shape[0],)
                               or pinned.device != vertices.device):
        raise ValueError(f"{who}: pinned is not a ({vertices.shape[0]},) bool tensor on {vertices.device}")
    if topology is not None:
        _check_topology(who, vertices, triangles, topology)
    v, t = _c(vertices.detach()), _c(triangles.detach())
    dev, nv, nt = v.device, v.shape[0], t.shape[0]
    n, lam, mu = opt["iterations"], opt["lam"], opt["mu"]
    _smooth_section("topology")
    topo = mesh_topology(v, t) if topology is None else topology
    ne = topo.n_edges
    _smooth_section("neighbours")
    nbrs = mesh_neighbours(topo)
    _smooth_section("weights")
    weight = _cotangent_weights(topo, v) if opt["weights"] == "cotangent" else None
    fixed = pinned.clone() if pinned is not None else torch.zeros(nv, device=dev, dtype=torch.bool)
    if opt["fix_boundary"]:
        fixed |= (topo.vertex_flags & VERTEX_BOUNDARY) != 0
    fixed_u8 = _c(fixed.view(_u8))
    _smooth_section("steps")
    cur, other = v.clone(), torch.empty_like(v)
    if nv:
        for _ in range(n):
            for f in (lam, mu):
                if f != 0.0:
                    _step(cur, nbrs, weight, ne, fixed_u8, f, out=other)
                    cur, other = other, cur
    del other
    _smooth_section("stats")
    free = ~fixed & ((topo.vertex_flags & VERTEX_REFERENCED) != 0)
    d = cur - v
    dist = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).sqrt()
    n_free = free.sum().to(_f64)
    dist_free = torch.where(free, dist, torch.zeros_like(dist))
    nan = torch.full((), float("nan"), device=dev, dtype=_f64)
    some = n_free > 0
    moved = (cur.view(_i64) != v.view(_i64)).any(dim=1).sum().to(_f64)
    figures = [fixed.sum().to(_f64), moved, torch.where(some, dist_free.max() if nv else nan, nan), torch.where(some, dist_free.sum() / n_free, nan),
               torch.where(some, (dist_free.square().sum() / n_free).sqrt(), nan)]
    if opt["measure"]:
        zero = torch.zeros((), device=dev, dtype=_f64)
        before = area_volume(v, t, topo.face_valid) if nt else (zero, zero)
        after = area_volume(cur, t, topo.face_valid) if nt else (zero, zero)
        rough_before = _roughness_figures(_dihedral(topo, _face_normals(topo, v)))
        rough_after = _roughness_figures(_dihedral(topo, _face_normals(topo, cur)))
        figures += [before[0], after[0], before[1], after[1], *rough_before, *rough_after]
    figures = torch.stack(figures).cpu().tolist()
    stats = {"iterations": n, "weights": opt["weights"], "pinned": int(figures[0]), "moved": int(figures[1]), "displacement_max": figures[2],
             "displacement_mean": figures[3], "displacement_rms": figures[4]}
    if opt["measure"]:
        stats.update(area_before=figures[5], area_after=figures[6], volume_before=figures[7], volume_after=figures[8],
                     roughness_before=_roughness_report(figures[9:13]), roughness_after=_roughness_report(figures[13:17]))
    _smooth_section("end")
    return cur, triangles, stats


__all__ = [n_ for n_ in dir() if not n_.startswith("__")]
