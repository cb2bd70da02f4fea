"""K36: exact point-to-mesh distance over K23's grid (closest_point_on_mesh) and the two-sided comparison of two meshes built on it
(mesh_distance: what MeshLab's Hausdorff filter and Metro report).  The definition is the comment of K36 in include/gens_hip.h (DESIGN.md,
section 5m); tests/mesh_distance_reference.py restates it in numpy as brute force over all faces.

Part of gens_amd.ops (see ops/__init__.py)."""
import ctypes as C

from .base import *  # noqa: F401,F403
from .geometry import MeshGrid, build_mesh_grid
from .points import sample_mesh_points
from .winding import build_winding_plan, mesh_inside, mesh_sign_request, winding_sign

_f64, _i32, _u8 = torch.float64, torch.int32, torch.uint8
MESH_DISTANCE_SAMPLES = 1_000_000
MESH_DISTANCE_KEYS = ("density", "samples", "max_dist", "signed", "sign", "beta")      # what extract_geometry(simplify_error=dict) may name
WINDING_SIGN_CHUNK = 1 << 18         # queries per K40 launch of mesh_distance(sign="winding"): no launch holds the device for long
NO_REGION = 255                                                # the region code of a query without a face

distance_section_hook = None         # a callable(name), called where a part of mesh_distance begins (scripts/mesh_distance_bench.py records HIP events there)


def _distance_section(name):
    if distance_section_hook is not None:
        distance_section_hook(name)


def distance_cap(who, max_dist):
    """max_dist checked on the host -> float.  ValueError unless it is a number > 0 (+inf: no cap)."""
    try:
        cap = float("nan") if isinstance(max_dist, bool) else float(max_dist)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: max_dist = {max_dist!r}: a positive number (+inf: no cap)") from None
    if not cap > 0.0:
        raise ValueError(f"{who}: max_dist = {max_dist!r}: a positive number (+inf: no cap)")
    return cap


def mesh_closest_dist2(queries, grid, max_dist=float("inf"), points=False, regions=False, chunk=None):
    """gens_mesh_closest_point as it writes: queries (n, 3) float64 on the device, grid: a MeshGrid -> (dist2 (n) float64, face (n) int32,
    point (n, 3) float64 or None, region (n) uint8 or None).  chunk: queries per launch (None: all in one); queries are independent, so the
    result does not depend on it.  No queries, or a mesh without faces, launch nothing: +inf / -1 (NaN for a query that is not finite)."""
    who = "closest_point_on_mesh"
    if not isinstance(grid, MeshGrid):
        raise ValueError(f"{who}: grid is {type(grid).__name__}, expected ops.build_mesh_grid's MeshGrid")
    if not torch.is_tensor(queries) or not queries.is_cuda:
        raise ValueError(f"{who}: queries is not a tensor on the device (gens_amd kernels have no CPU path)")
    if queries.dtype != _f64 or queries.dim() != 2 or queries.shape[1] != 3:
        raise ValueError(f"{who}: queries is {tuple(queries.shape)} {queries.dtype}, expected (n, 3) {_f64}")
    if queries.device != grid.vertices.device:
        raise ValueError(f"{who}: queries on {queries.device}, the mesh on {grid.vertices.device}")
    cap = distance_cap(who, max_dist)
    if chunk is not None and (isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1):
        raise ValueError(f"{who}: chunk = {chunk!r}: a positive whole number of queries per launch, or None")
    q = _c(queries.detach())
    n, dev = q.shape[0], q.device
    if n >= 2 ** 31:
        raise ValueError(f"{who}: {n} queries (below 2^31)")
    dist2 = torch.full((n,), float("inf"), device=dev, dtype=_f64)
    face = torch.full((n,), -1, device=dev, dtype=_i32)
    point = torch.full((n, 3), float("nan"), device=dev, dtype=_f64) if points else None
    region = torch.full((n,), NO_REGION, device=dev, dtype=_u8) if regions else None
    if n == 0:
        return dist2, face, point, region
    if grid.n_faces == 0:
        dist2[~torch.isfinite(q).all(dim=1)] = float("nan")
        return dist2, face, point, region
    args = grid.args()
    step = n if chunk is None else chunk
    for s in range(0, n, step):
        m = min(step, n - s)
        off = lambda t, row: None if t is None else C.c_void_p(t.data_ptr() + s * row)  # noqa: E731
        L.call("gens_mesh_closest_point", C.byref(args), off(q, 24), m, cap, off(dist2, 8), off(face, 4), off(point, 24), off(region, 1), L.stream(),
               nbytes=m * (36 + (24 if points else 0) + (1 if regions else 0)))
    return dist2, face, point, region


def closest_point_on_mesh(queries, grid, max_dist=float("inf"), points=False, regions=False, chunk=None):
    """K36.  queries (n, 3) float64 on the device, grid = ops.build_mesh_grid(vertices, triangles) -> (dist (n) float64, face (n) int32
    [, point (n, 3) float64][, region (n) uint8]): the distance to the nearest point of the mesh (torch.sqrt of the kernel's squared
    distance), the face it lies on -- the smallest index among faces at exactly the same distance --, that point, and where on the face it
    lies (0 interior, 1 - 3 vertex a / b / c, 4 - 6 edge ab / bc / ca, 7 the degenerate path).  Exactly the brute-force minimum over all
    faces, whatever the grid.  max_dist: a cap; where nothing lies within it (d^2 <= max_dist^2), and for a mesh without faces: +inf, -1,
    NaNs, 255.  A query with a coordinate that is not finite: NaN, -1.  Unsigned.
    Cost: a query next to the mesh costs about a microsecond of a launch's share, a query with nothing near it walks rings of empty cells
    until it meets a face -- about 0.2 ms EACH against a 930 000-face mesh.  All queries go into ONE launch unless
    `chunk` says otherwise, so a million points far from the mesh are one kernel that runs for minutes: for clouds that may lie far from the
    mesh give max_dist (the walk stops once nothing unvisited can be within it) and a chunk, so that no single launch holds the device.
    ValueError before any launch for queries that are not an
    (n, 3) float64 device tensor on the mesh's device, a grid that is no MeshGrid, max_dist not > 0, a chunk that is no positive int."""
    dist2, face, point, region = mesh_closest_dist2(queries, grid, max_dist, points, regions, chunk)
    return (torch.sqrt(dist2), face) + ((point,) if points else ()) + ((region,) if regions else ())


def _mesh_area(v, t):
    if t.shape[0] == 0:
        return torch.zeros((), device=v.device, dtype=_f64)
    a, b, c = v[t[:, 0].long()], v[t[:, 1].long()], v[t[:, 2].long()]
    return 0.5 * torch.linalg.cross(b - a, c - a).square().sum(dim=1).sqrt().sum()


def _direction_figures(dist2):
    """(7,) float64 on the device: matched count m, sum of d, sum of d^2, max, q50, q90, q99 over the finite entries (see direction_stats in
    tests/mesh_distance_reference.py: the order statistic at index (p m) // 100)."""
    n = dist2.shape[0]
    if n == 0:
        return torch.zeros(7, device=dist2.device, dtype=_f64)
    keep = torch.isfinite(dist2)
    m = keep.sum()
    d2 = torch.where(keep, dist2, torch.zeros_like(dist2))
    d = torch.sqrt(d2)
    ordered = torch.sort(torch.where(keep, torch.sqrt(dist2), torch.full_like(dist2, float("inf"))))[0]     # the unmatched sort to the end
    last = torch.clamp(m - 1, min=0)
    idx = torch.stack([last] + [torch.minimum(last, (p * m) // 100) for p in (50, 90, 99)])
    return torch.cat([torch.stack([m.to(_f64), d.sum(), d2.sum()]), ordered[idx]])


def _direction_dict(n, figures):
    m = int(figures[0])
    out = {"n": n, "unmatched": n - m}
    if m == 0:
        out.update({k: float("nan") for k in ("mean", "rms", "max", "q50", "q90", "q99")})
        return out
    out.update(mean=figures[1] / m, rms=math.sqrt(figures[2] / m), max=figures[3], q50=figures[4], q90=figures[5], q99=figures[6])
    return out


def _signed_figures(dist2, signed):
    """(3,) float64 on the device over the matched samples (finite dist2): the sum of the signed distances that have a sign, the count of
    negative ones, the count without a sign (NaN)."""
    if dist2.shape[0] == 0:
        return torch.zeros(3, device=dist2.device, dtype=_f64)
    matched = torch.isfinite(dist2)
    none = torch.isnan(signed)
    return torch.stack([torch.where(matched & ~none, signed, torch.zeros_like(signed)).sum(), (matched & (signed < 0.0)).sum().to(_f64),
                        (matched & none).sum().to(_f64)])


def mesh_distance_request(who, density=None, samples=MESH_DISTANCE_SAMPLES, max_dist=float("inf"), signed=False):
    """The comparison's keywords, checked on the host -> (density or None, samples, max_dist)."""
    if not isinstance(signed, bool):
        raise ValueError(f"{who}: signed = {signed!r}: True or False")
    if density is not None:
        try:
            density = float("nan") if isinstance(density, bool) else float(density)
        except (TypeError, ValueError):
            density = float("nan")
        if not (density > 0.0 and math.isfinite(density)):
            raise ValueError(f"{who}: density: the sample spacing, positive and finite (None: sqrt(area / samples) per mesh)")
    if isinstance(samples, bool) or not isinstance(samples, int) or samples < 1:
        raise ValueError(f"{who}: samples = {samples!r}: a positive whole number")
    return density, samples, distance_cap(who, max_dist)


def mesh_distance_keywords(who, kw):
    """A dict of mesh_distance's keywords (MESH_DISTANCE_KEYS), checked on the host: mesh_distance_request for the first four,
    mesh_sign_request for `sign` and `beta`.  ValueError for what either refuses."""
    mesh_distance_request(who, **{k: v for k, v in kw.items() if k not in ("sign", "beta")})
    mesh_sign_request(who, kw.get("signed", False), kw.get("sign", "pseudonormal"), kw.get("beta", None))


def mesh_distance(va, ta, vb, tb, density=None, samples=MESH_DISTANCE_SAMPLES, max_dist=float("inf"), return_samples=False, signed=False,
                  sign="pseudonormal", beta=None):
    """The two-sided distance between the meshes A = (va, ta) and B = (vb, tb): vertices (V, 3) float64 and triangles (T, 3) int32 on the
    device.  Each mesh is sampled with ops.sample_mesh_points -- ALL its vertices, then K24's lattice points at spacing `density` (the DTU
    score's sampler; the vertices come on top of the area-uniform lattice, so regions of small triangles weigh more: on a mesh whose
    triangles are about `density` wide, vertices are about a third of the samples) -- and every sample is given its exact distance to the
    OTHER mesh (closest_point_on_mesh).  density = None: sqrt(area / samples) per mesh, i.e. about `samples` lattice points on each
    (fewer on slivers narrower than the spacing).
    -> {"a_to_b": figures of A's samples against B, "b_to_a": the reverse, "hausdorff": the larger of the two `max`, "chamfer": the mean of
    the two `mean`, "density_a", "density_b"}; a direction's figures: n (samples), unmatched (samples with nothing within max_dist: counted
    here and left out of the rest), mean, rms, max, q50, q90, q99 (order statistics at index (p m) // 100 of the m matched distances);
    NaN where m = 0.  Python numbers: the sums are float64 on the device and the figures come back in one read (building the grids and
    sampling read sizes and extents back as they always do, and density = None reads the two areas).  return_samples: also
    "samples_a", "dist_a", "face_a" (and _b): the device tensors behind the figures.  One-sided figures differ: a hole in B
    shows in a_to_b only.  signed=True (K37; off: not one more launch or key): each sample's distance also gets the sign that the OTHER mesh's
    orientation gives it (ops.signed_distance_to_mesh: positive on the side its face normals point to) and a direction gains signed_mean
    (the mean over the matched samples that have a sign; NaN if none has), inside (the count of negative ones) and no_sign (matched samples
    whose closest point has no sign: on a boundary, flipped or non-manifold edge, a pinched vertex, a degenerate face); with return_samples
    also "signed_a" / "signed_b".  sign="winding" (K40; needs signed=True) takes the sign from the OTHER mesh's generalised winding number
    instead (ops.mesh_inside with `beta`, default MESH_DISTANCE_BETA): negative where the sample is inside, whatever the mesh's edges are
    like -- open, pinched, folded, a soup --, the same three keys, no_sign now counting the samples the far field's bound leaves undecided;
    an inside-out mesh has nothing inside it (ops.repair_mesh re-orients).  ValueError before any launch for what closest_point_on_mesh, build_mesh_grid's inputs and the keywords exclude."""
    who = "mesh_distance"
    for name, t, dtype in (("va", va, _f64), ("ta", ta, _i32), ("vb", vb, _f64), ("tb", tb, _i32)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError(f"{who}: {name} is not a tensor on the device (gens_amd kernels have no CPU path)")
        if t.dtype != dtype or t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{who}: {name} is {tuple(t.shape)} {t.dtype}, expected (n, 3) {dtype}")
        if t.device != va.device:
            raise ValueError(f"{who}: va on {va.device}, {name} on {t.device}")
    density, samples, cap = mesh_distance_request(who, density, samples, max_dist, signed)
    sign, beta = mesh_sign_request(who, signed, sign, beta)
    pseudo = signed and sign == "pseudonormal"
    _distance_section("grids")
    meshes = [(_c(va.detach()), _c(ta.detach())), (_c(vb.detach()), _c(tb.detach()))]
    grids = [build_mesh_grid(v, t) for v, t in meshes]
    _distance_section("sampling")
    if density is None:
        areas = torch.stack([_mesh_area(v, t) for v, t in meshes]).cpu().tolist()
        if not all(math.isfinite(a) for a in areas):
            raise ValueError(f"{who}: a mesh's area is not finite")
        densities = [math.sqrt(a / samples) if a > 0.0 else 1.0 for a in areas]      # (a mesh without area has no lattice points at any spacing)
    else:
        densities = [density, density]
    points = [sample_mesh_points(v, t, d) for (v, t), d in zip(meshes, densities)]
    results = []
    for k in (0, 1):
        _distance_section("query_a_to_b" if k == 0 else "query_b_to_a")
        results.append(mesh_closest_dist2(points[k], grids[1 - k], cap, pseudo, pseudo))
    signs = None
    if signed and not pseudo:
        _distance_section("sign")
        signs = [winding_sign(results[k][0], mesh_inside(points[k], build_winding_plan(*meshes[1 - k]), beta, WINDING_SIGN_CHUNK, who=who))
                 for k in (0, 1)]
    elif signed:
        from .mesh_topology import distance_sign, mesh_topology
        _distance_section("sign")
        signs = [distance_sign(points[k], *results[k], mesh_topology(*meshes[1 - k], normals=True)) for k in (0, 1)]
    _distance_section("reduce")
    figures = [_direction_figures(r[0]) for r in results]
    if signed:
        figures = [torch.cat([f, _signed_figures(r[0], s)]) for f, r, s in zip(figures, results, signs)]
    figures = torch.stack(figures).cpu().tolist()
    _distance_section("end")
    sides = [_direction_dict(points[k].shape[0], figures[k]) for k in (0, 1)]
    if signed:
        for side, f in zip(sides, figures):
            with_sign = int(f[0]) - int(f[9])
            side.update(signed_mean=f[7] / with_sign if with_sign else float("nan"), inside=int(f[8]), no_sign=int(f[9]))
    ha, hb = sides[0]["max"], sides[1]["max"]
    out = {"a_to_b": sides[0], "b_to_a": sides[1], "hausdorff": float("nan") if ha != ha or hb != hb else max(ha, hb),
           "chamfer": 0.5 * (sides[0]["mean"] + sides[1]["mean"]), "density_a": densities[0], "density_b": densities[1]}
    if return_samples:
        for k, s in enumerate("ab"):
            out["samples_" + s], out["dist_" + s], out["face_" + s] = points[k], torch.sqrt(results[k][0]), results[k][1]
            if signed:
                out["signed_" + s] = signs[k]
    return out


__all__ = [n_ for n_ in dir() if not n_.startswith("__")]
