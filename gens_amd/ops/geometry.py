"""K11 (lattice points), K12 (iso-surface extraction on the device) and K23 / K25's mesh culling (ray casting against the extracted mesh,
the view rays of both cleaning scripts, face components and the culling tail the two share).

Part of gens_amd.ops (see ops/__init__.py); citations are relative to /root/reference."""
from .base import *  # noqa: F401,F403

# ------------------------------------------------------------------------------------------------------------------
# K11  lattice (implicit_surface.py:407-418)
# ------------------------------------------------------------------------------------------------------------------
def lattice_points(bound_min, bound_max, resolution, first, count, device):
    lo = (C.c_float * 3)(*[float(v) for v in bound_min])
    hi = (C.c_float * 3)(*[float(v) for v in bound_max])
    pts = torch.empty(count, 3, device=device, dtype=_f32)
    L.call("gens_lattice_points", lo, hi, int(resolution), int(first), int(count), L.ptr(pts), L.stream())
    return pts


# ------------------------------------------------------------------------------------------------------------------
# K12  iso-surface extraction (mcubes.marching_cubes at implicit_surface.py:423)
# ------------------------------------------------------------------------------------------------------------------
_MC_TABLES = {}


def _mc_tables(dev):
    """The case table (256, 16) int8 and the triangle counts (256,) uint8 of gens_amd/mc_tables.py on `dev`, copied there once."""
    from .. import mc_tables
    if dev not in _MC_TABLES:
        _MC_TABLES[dev] = (torch.from_numpy(mc_tables.TRI_TABLE.copy()).to(dev), torch.from_numpy(mc_tables.TRI_COUNT.copy()).to(dev))
    return _MC_TABLES[dev]


def marching_cubes(u, threshold=0.0):
    """u (X,Y,Z) float32 device tensor -> (vertices (V,3) float64 in index coordinates, triangles (T,3) int32), both on the
    device.  Classic marching cubes with the case table of gens_amd/mc_tables.py; order as in oracle/mc_oracle.py."""
    dev = u.device
    table, count = _mc_tables(dev)
    u = _c(u.detach().to(_f32))
    x, y, z = u.shape
    total = x * y * z
    vmask, vcount, cases, tcount = (torch.empty(total, device=dev, dtype=torch.uint8) for _ in range(4))
    u8 = torch.uint8
    L.call("gens_mc_classify", L.ptr(u), x, y, z, float(threshold), L.ptr(count, u8), L.ptr(vmask, u8), L.ptr(vcount, u8), L.ptr(cases, u8),
           L.ptr(tcount, u8), L.stream(), nbytes=total * 8)
    vend = torch.cumsum(vcount, 0, dtype=torch.int32)
    tend = torch.cumsum(tcount, 0, dtype=torch.int32)
    nv, nt = int(vend[-1]), int(tend[-1])
    vertices = torch.empty(nv, 3, device=dev, dtype=torch.float64)
    triangles = torch.empty(nt, 3, device=dev, dtype=torch.int32)
    if nv == 0:
        return vertices, triangles
    voff = vend - vcount        # exclusive scans
    toff = tend - tcount
    del vend, tend
    i32 = torch.int32
    L.call("gens_mc_emit", L.ptr(u), x, y, z, float(threshold), L.ptr(table, torch.int8), table.shape[1], L.ptr(vmask, u8), L.ptr(voff, i32),
           L.ptr(cases, u8), L.ptr(tcount, u8), L.ptr(toff, i32), L.ptr(vertices, torch.float64),
           L.ptr(triangles, i32) if nt else L.ptr(torch.empty(1, 3, device=dev, dtype=i32), i32), L.stream(),
           nbytes=total * 15 + nv * 24 + nt * 12)
    return vertices, triangles


# ------------------------------------------------------------------------------------------------------------------
# K23  first hits against a triangle mesh and its face components (utils/clean_mesh.py:38-106: pyembree's intersects_first, trimesh's
#      face_adjacency + connected_components); the same kernels under K25's ray step (evaluation/clean_meshes.py:212-281)
# ------------------------------------------------------------------------------------------------------------------
class MeshGrid:
    """A triangle mesh on the device with the uniform grid of K23 over it: about two cubic cells per face (at most 512 per axis), every
    face listed in every cell its closed AABB overlaps.  vertices (V,3) float64, triangles (F,3) int32, cell_start (cells + 1) int32,
    cell_faces int32; box = (lo_x, lo_y, lo_z, cell edge) float32, dims = (nx, ny, nz)."""

    def __init__(self, vertices, triangles, cell_start, cell_faces, box, dims):
        self.vertices, self.triangles, self.cell_start, self.cell_faces = vertices, triangles, cell_start, cell_faces
        self.box, self.dims = tuple(float(b) for b in box), tuple(int(d) for d in dims)

    @property
    def n_faces(self):
        return self.triangles.shape[0]

    def args(self):
        i32 = torch.int32
        return L.MeshGridArgs(L.ptr(self.vertices, torch.float64), L.ptr(self.triangles, i32), L.ptr(self.cell_start, i32),
                              L.ptr(self.cell_faces, i32), self.n_faces, *self.box, *self.dims)


def _grid_box(vmin, vmax, n_faces):
    """Box and cell count of the grid: the referenced vertices' bounding box padded by 1e-4 of its extent (float32 corner at or below it),
    cubic cells of volume (box volume) / (2 F), at most 512 per axis -> ((lo_x, lo_y, lo_z, cell) float32 values, (nx, ny, nz))."""
    import numpy as np
    vmin, vmax = np.asarray(vmin, dtype=np.float64), np.asarray(vmax, dtype=np.float64)
    ext = float((vmax - vmin).max())
    scale = max(float(np.abs(vmin).max()), float(np.abs(vmax).max()), ext, 1e-30)
    pad = 1e-4 * ext + 1e-6 * scale
    lo = (vmin - pad).astype(np.float32)
    span = (vmax + pad) - lo.astype(np.float64)
    full = np.maximum(span, 1e-3 * span.max())
    cell = (float(np.prod(full)) / (2.0 * max(n_faces, 1))) ** (1.0 / 3.0)
    cell = max(cell, float(span.max()) / 512.0 * (1.0 + 1e-6))
    c32 = np.float32(cell)
    if float(c32) < cell:
        c32 = np.nextafter(c32, np.float32(np.inf))
    dims = np.clip(np.ceil(span / float(c32) * (1.0 + 1e-9)), 1, 512).astype(int)
    return (float(lo[0]), float(lo[1]), float(lo[2]), float(c32)), tuple(int(d) for d in dims)


def build_mesh_grid(vertices, triangles):
    """vertices (V,3), triangles (F,3) device tensors -> MeshGrid (counting sort: count, exclusive scan, fill)."""
    dev = vertices.device
    v = _c(vertices.detach().to(torch.float64)).reshape(-1, 3)
    t = _c(triangles.detach().to(device=dev, dtype=torch.int32)).reshape(-1, 3)
    nf = t.shape[0]
    if nf:
        lim = torch.stack([t.min(), t.max()]).cpu()
        if int(lim[0]) < 0 or int(lim[1]) >= v.shape[0]:
            raise ValueError("build_mesh_grid: triangle index out of range")
        used = v[t.reshape(-1).long()]
        ext = torch.stack([used.amin(0), used.amax(0)]).cpu().numpy()
        if not (abs(ext) < float("inf")).all():
            raise ValueError("build_mesh_grid: non-finite vertex")
        box, dims = _grid_box(ext[0], ext[1], nf)
    else:
        box, dims = (0.0, 0.0, 0.0, 1.0), (1, 1, 1)
    cells = dims[0] * dims[1] * dims[2]
    i32 = torch.int32
    counts = torch.zeros(cells, device=dev, dtype=i32)
    grid = MeshGrid(v, t, torch.zeros(cells + 1, device=dev, dtype=i32), torch.zeros(1, device=dev, dtype=i32), box, dims)
    if nf == 0:
        return grid
    L.call("gens_mesh_grid_count", C.byref(grid.args()), L.ptr(counts, i32), L.stream())
    ends = torch.cumsum(counts, 0, dtype=torch.int64)
    total = int(ends[-1])
    if total >= 2 ** 31:
        raise RuntimeError(f"build_mesh_grid: {total} face-cell overlaps exceed int32")
    grid.cell_start[1:] = ends.to(i32)
    grid.cell_faces = torch.empty(max(total, 1), device=dev, dtype=i32)
    counts.zero_()                              # (now the fill's cursor)
    L.call("gens_mesh_grid_fill", C.byref(grid.args()), L.ptr(counts, i32), L.stream())
    return grid


def ray_mesh_first_hit(rays_o, rays_d, grid):
    """trimesh's intersects_first: rays (N,3) -> (face (N,) int32, -1 on a miss; t (N,) float32 along rays_d, +inf on a miss).  The first
    hit is the smallest (t, face) over the faces hit at t > 0 from either side (watertight test in float64)."""
    ro = _c(rays_o.detach().to(_f32)).reshape(-1, 3)
    rd = _c(rays_d.detach().to(_f32)).reshape(-1, 3)
    n = ro.shape[0]
    face = torch.empty(n, device=ro.device, dtype=torch.int32)
    t = torch.empty(n, device=ro.device, dtype=_f32)
    L.call("gens_ray_first_hit", C.byref(grid.args()), L.ptr(ro), L.ptr(rd), n, L.ptr(face, torch.int32), L.ptr(t), L.stream())
    return face, t


def view_ray_cams(intrs, c2ws, invert="4x4"):
    """(nv,4,4) intrinsics and camera-to-world -> (nv,21) float32 on the host: K^-1[:3,:3] and c2w[:3,:4].  K^-1 is torch.inverse on the
    CPU of each float32 4x4 (invert="4x4", as clean_mesh.py:60 takes it) or of its 3x3 block (invert="3x3", as clean_meshes.py:51 takes it
    from the [:3,:3] it is handed at :223); the two differ in the last bits, and each script's rays need its own."""
    if invert not in ("4x4", "3x3"):
        raise ValueError(f"view_ray_cams: invert={invert!r} (4x4 or 3x3)")
    intrs, c2ws = torch.as_tensor(intrs).detach().cpu(), torch.as_tensor(c2ws).detach().cpu().float()
    def kinv(k):
        # each matrix goes to float32 where its script converts it, the 3x3 block once it is cut out: the last bits of torch.inverse
        # depend on the memory layout it is handed, and the block of a float64 input reaches it as a contiguous copy
        if invert == "4x4":
            return k.float().inverse()[:3, :3]
        return torch.inverse(k[:3, :3].float())

    return torch.stack([torch.cat([kinv(intrs[i]).reshape(-1), c2ws[i][:3, :4].reshape(-1)]) for i in range(intrs.shape[0])])


def _cast_view_rays(entry, grid, masks, intrs, c2ws, *shape, invert, rows):
    """The launch both view-ray operators share: the camera table, zeroed flags (rows, F) and any_miss (rows,), and `entry` on masks
    (nv,H,W) with `shape` = its arguments between (nv, H, W) and the outputs -> (flags, any_miss)."""
    dev = grid.vertices.device
    nv, h, w = masks.shape
    cams = view_ray_cams(intrs, c2ws, invert).to(dev)
    flags = torch.zeros(rows, max(grid.n_faces, 1), device=dev, dtype=torch.uint8)
    any_miss = torch.zeros(rows, device=dev, dtype=torch.int32)
    L.call(entry, C.byref(grid.args()), L.ptr(masks, masks.dtype), L.ptr(cams), nv, h, w, *shape, L.ptr(flags, torch.uint8),
           L.ptr(any_miss, torch.int32), L.stream())
    return flags[:, :grid.n_faces], any_miss


def visible_faces(grid, masks, intrs, c2ws, upscale):
    """The first-hit half of clean_mesh_outside_frustum (clean_mesh.py:45-78) in one launch: every pixel of every view upsampled by
    `upscale` whose nearest-upsampled mask is > 0 casts the ray clean_mesh.py:50-66 builds.  masks (nv,H,W) (the raw, view-averaged masks),
    intrs / c2ws (nv,4,4) -> (flags (F,) uint8: 1 for every face some ray hits first, any_miss (1,) int32: 1 if some cast ray missed)."""
    m = _c(masks.detach().to(device=grid.vertices.device, dtype=_f32))
    _, h, w = m.shape
    inv_scale = float(torch.tensor(1.0 / upscale, dtype=torch.float32))
    flags, any_miss = _cast_view_rays("gens_view_rays_hit_faces", grid, m, intrs, c2ws, int(h * upscale), int(w * upscale), inv_scale,
                                      invert="4x4", rows=1)
    return flags[0], any_miss


def view_rays_hit_counts(grid, masks, intrs, c2ws, dep_min=425):
    """The ray loop of clean_mesh_faces_outside_frustum (clean_meshes.py:212-246) in one launch: every pixel of every view whose uint8
    mask is > 128 casts gen_rays_from_single_image's ray from o + d * dep_min.  masks (nv,H,W) uint8, intrs / c2ws (nv,4,4) ->
    (counts (F,) int32: the number of views in which some ray hits the face first; flags (nv,F) uint8: per view; any_miss (nv,) int32: 1
    where a cast ray of the view missed)."""
    m = _c(masks.detach().to(grid.vertices.device))
    if m.dtype != torch.uint8 or m.dim() != 3:
        raise ValueError("view_rays_hit_counts: (nv,H,W) uint8 masks")
    if grid.n_faces:
        flags, any_miss = _cast_view_rays("gens_view_rays_hit_counts", grid, m, intrs, c2ws, float(dep_min), invert="3x3", rows=m.shape[0])
    else:                                       # (an empty mesh has no arrays to hand the kernel: every cast ray misses)
        flags = torch.zeros(m.shape[0], 0, device=m.device, dtype=torch.uint8)
        any_miss = (m > 128).reshape(m.shape[0], -1).any(1).to(torch.int32)
    return flags.sum(0, dtype=torch.int32), flags, any_miss


def face_adjacency(triangles, n_vertices):
    """trimesh's face_adjacency: the pairs (P,2) int32 of faces that share an edge used by EXACTLY two faces (group_rows(edges,
    require_count=2)), without the pairs of a face with itself (a face with a repeated vertex, [a, a, b], uses its edge (a, b) twice;
    trimesh drops those pairs too); edge key min(v) * V + max(v), sorted by torch.sort."""
    t = triangles.detach().reshape(-1, 3).to(torch.int64)
    if t.shape[0] == 0:
        return torch.zeros(0, 2, device=t.device, dtype=torch.int32)
    e = torch.stack([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]], 1).reshape(-1, 2)
    key = torch.minimum(e[:, 0], e[:, 1]) * int(n_vertices) + torch.maximum(e[:, 0], e[:, 1])
    key, order = torch.sort(key)
    face = order // 3
    same = key[1:] == key[:-1]
    no = torch.zeros(1, device=t.device, dtype=torch.bool)
    first = same & ~torch.cat([no, same[:-1]]) & ~torch.cat([same[1:], no])      # runs of length exactly two start here
    i = torch.nonzero(first).reshape(-1)
    i = i[face[i] != face[i + 1]]
    return _c(torch.stack([face[i], face[i + 1]], 1).to(torch.int32))


def face_components(triangles, n_vertices, pairs=None):
    """Connected components of the face-adjacency graph (face_adjacency's pairs) -> labels (F,) int32 = the smallest face index of each
    face's component.  Union-find on the device: a hook launch, then a compress launch."""
    dev = triangles.device
    nf = triangles.reshape(-1, 3).shape[0]
    if pairs is None:
        pairs = face_adjacency(triangles, n_vertices)
    i32 = torch.int32
    parent = torch.arange(nf, device=dev, dtype=i32)
    label = torch.empty(nf, device=dev, dtype=i32)
    if nf == 0:
        return label
    pairs = _c(pairs.to(i32))
    if pairs.shape[0]:
        L.call("gens_face_cc_hook", L.ptr(pairs, i32), pairs.shape[0], L.ptr(parent, i32), nf, L.stream())
    L.call("gens_face_cc_compress", L.ptr(parent, i32), nf, L.ptr(label, i32), L.stream())
    return label


def kept_after_quirk(counts, any_miss, num_com_vis=2):
    """The `values[1:]` of both cleaning scripts (clean_mesh.py:80-90 with num_com_vis = 1, clean_meshes.py:248-260) on device tensors:
    counts (F,) views that hit each face first, any_miss (nv,) -> (keep (F,) bool, len(values)).  values = the sorted faces with counts >=
    num_com_vis, with -1 in front if at least num_com_vis views had a miss; values[1:] is kept."""
    keep = counts >= num_com_vis
    n_values = int(keep.sum())
    if int((any_miss > 0).sum()) >= num_com_vis:
        return keep, n_values + 1               # values[0] is the -1 of the misses
    hit = torch.nonzero(keep).reshape(-1)
    if len(hit):
        keep = keep.clone()
        keep[hit[0]] = False                    # values[1:] drops the smallest hit face instead
    return keep, n_values


def large_components(v_np, t_dtype, t, min_faces, return_index=False):
    """The tail of both cleaning scripts (clean_mesh.py:101-106, clean_meshes.py:268-281) on device triangles t (F,3) int64 over the host
    vertices v_np: the components of at least `min_faces` faces by trimesh's rule (a face without a neighbour across an edge of exactly
    two faces is in no component), then the referenced vertices in their order -> (vertices, triangles of t_dtype) numpy.
    return_index: also the (V',) int64 indices of the kept vertices in v_np, for per-vertex attributes to follow the compaction."""
    dev, n_v = t.device, len(v_np)
    if len(t):
        pairs = face_adjacency(t, n_v)
        label = face_components(t, n_v, pairs).long()
        in_graph = torch.zeros(len(t), device=dev, dtype=torch.bool)
        in_graph[pairs.reshape(-1).long()] = True
        t = t[in_graph & (torch.bincount(label, minlength=len(t))[label] >= min_faces)]
    used = torch.zeros(n_v, device=dev, dtype=torch.bool)
    used[t.reshape(-1)] = True
    remap = torch.cumsum(used, 0) - 1
    used_np = used.cpu().numpy()
    mesh = v_np.reshape(-1, 3)[used_np], remap[t].cpu().numpy().astype(t_dtype)
    if return_index:
        import numpy as np
        return mesh + (np.flatnonzero(used_np).astype(np.int64),)
    return mesh


__all__ = [n_ for n_ in dir() if not n_.startswith("__")]      # private helpers travel too: the package namespace is the old module's
