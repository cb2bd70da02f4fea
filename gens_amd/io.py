"""Writers for what `runner.py` stores per validated view, without trimesh / OpenCV:

    meshes/{scene}_epoch{e}.ply            the extracted surface, moved back to world coordinates by scale_mat   (runner.py:229-236)
    val_img/…png, val_normal/…png          rendered colour and normal images                                      (runner.py:243-244)
    val_render_depth/…png, val_sdf_depth/… depth maps through the magma colour map, fixed range [0, 2.5]          (runner.py:245-246, 379-392)

and the reference's mesh cleaning (utils/clean_mesh.py): the mask half (:9-35, drop faces with a vertex that fewer than two source masks
see) on the host, the ray-cast half (clean_mesh_outside_frustum, :38-106: pyembree through trimesh, then trimesh's face components) on the
device (K23), and the chain of both (`clean_mesh`, :109-130).  `drop_small_components` is a host restatement of the component step."""
import os

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image


# ------------------------------------------------------------------------------------------------------------------ meshes
def transform_vertices(vertices, matrix):
    """vertices (V,3), matrix (4,4) -> (V,3): what trimesh.Trimesh.apply_transform does to the vertices (runner.py:232)."""
    m = np.asarray(matrix, dtype=np.float64)
    v = np.asarray(vertices, dtype=np.float64)
    return v @ m[:3, :3].T + m[:3, 3]


def transform_normals(normals, matrix):
    """normals (V,3), matrix (4,4) -> (V,3) float64: the normals of a surface moved by transform_vertices(., matrix).  Normals go with the
    inverse transpose of the linear part -- `n @ inv(M[:3, :3])` on row vectors -- and are renormalised: scale_mat need not be a uniform
    scale.  Zero rows (no normal) stay zero."""
    m = np.asarray(matrix, dtype=np.float64)
    n = np.asarray(normals, dtype=np.float64).reshape(-1, 3) @ np.linalg.inv(m[:3, :3])
    length = np.linalg.norm(n, axis=1, keepdims=True)
    return np.divide(n, length, out=np.zeros_like(n), where=length > 0)


def write_ply(path, vertices, triangles, normals=None, colors=None):
    """Binary little-endian PLY with float32 vertices and int32 triangles (the layout trimesh exports for a bare mesh).
    normals (V,3) / colors (V,3): optional per-vertex properties, written as float nx ny nz / uchar red green blue after x y z (the names
    MeshLab, Open3D and trimesh read)."""
    v = np.ascontiguousarray(vertices, dtype="<f4").reshape(-1, 3)
    t = np.ascontiguousarray(triangles, dtype="<i4").reshape(-1, 3)
    if t.size and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError("write_ply: triangle index out of range")
    fields, names = [("xyz", "<f4", (3,))], "property float x\nproperty float y\nproperty float z\n"
    if normals is not None:
        normals = np.asarray(normals).reshape(-1, 3)
        fields.append(("n", "<f4", (3,)))
        names += "property float nx\nproperty float ny\nproperty float nz\n"
    if colors is not None:
        colors = np.asarray(colors).reshape(-1, 3)
        fields.append(("c", "u1", (3,)))
        names += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    for what, a in (("normals", normals), ("colors", colors)):
        if a is not None and len(a) != len(v):
            raise ValueError(f"write_ply: {len(a)} {what} for {len(v)} vertices")
    header = ("ply\nformat binary_little_endian 1.0\ncomment gens_amd\n"
              f"element vertex {len(v)}\n{names}"
              f"element face {len(t)}\nproperty list uchar int vertex_indices\nend_header\n")
    if len(fields) > 1:
        rows = np.empty(len(v), dtype=fields)
        rows["xyz"] = v
        if normals is not None:
            rows["n"] = normals
        if colors is not None:
            rows["c"] = colors
        v = rows
    faces = np.empty(len(t), dtype=[("n", "u1"), ("idx", "<i4", (3,))])
    faces["n"] = 3
    faces["idx"] = t
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(v.tobytes())
        f.write(faces.tobytes())


def write_point_cloud(path, points, normals=None, colors=None):
    """A point cloud as write_ply writes a mesh, with an empty face element (read_ply reads it back: triangles of shape (0, 3)): float32
    x y z, optional float nx ny nz and uchar red green blue.  What evaluate_dtu(mode="pcd") reads as pcd/scan{n}.ply."""
    write_ply(path, points, np.zeros((0, 3), np.int32), normals=normals, colors=colors)


def _obj_stem(path):
    path = os.fspath(path)
    return path[:-4] if path.lower().endswith(".obj") else path


def write_obj(path, vertices, triangles, uv, texture, normals=None, seen=None):
    """A textured mesh as Wavefront OBJ: `path`.obj (`path` may carry the extension), with its material `path`.mtl (map_Kd) and its texture
    `path`.png beside it -- what MeshLab, Blender and Open3D open.  vertices (V,3) and optional per-vertex normals (V,3) are written as
    float32 (`v`, `vn`), uv (T,3,2) (texture_mesh's "texture_uv": one coordinate pair per corner, origin bottom-left) as one `vt` per
    corner, faces as `f a/ta[/na]`.  texture (H,W,3) uint8 (row 0 at the top); seen (H,W) bool, where given: texels no source view sees
    (the network's output is arbitrary there) and texels no triangle owns are written mid-grey (128).  -> the three paths."""
    stem = _obj_stem(path)
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(triangles, dtype=np.int64).reshape(-1, 3)
    uv = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 3, 2)
    texture = np.asarray(texture)
    if t.size and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError("write_obj: triangle index out of range")
    if len(uv) != len(t):
        raise ValueError(f"write_obj: {len(uv)} rows of corner coordinates for {len(t)} triangles")
    if texture.ndim != 3 or texture.shape[2] != 3 or texture.dtype != np.uint8:
        raise ValueError(f"write_obj: texture is {texture.shape} {texture.dtype}, expected (H, W, 3) uint8")
    if normals is not None:
        normals = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        if len(normals) != len(v):
            raise ValueError(f"write_obj: {len(normals)} normals for {len(v)} vertices")
    if seen is not None:
        seen = np.asarray(seen, dtype=bool)
        if seen.shape != texture.shape[:2]:
            raise ValueError(f"write_obj: seen is {seen.shape} for a texture of {texture.shape[:2]}")
        texture = np.where(seen[:, :, None], texture, np.uint8(128))
    name = os.path.basename(stem)
    corner = 3 * np.arange(len(t), dtype=np.int64)[:, None] + np.arange(1, 4, dtype=np.int64)[None]
    if normals is None:
        faces, fmt = np.stack([t + 1, corner], axis=-1).reshape(-1, 6), "f %d/%d %d/%d %d/%d"
    else:
        faces, fmt = np.stack([t + 1, corner, t + 1], axis=-1).reshape(-1, 9), "f %d/%d/%d %d/%d/%d %d/%d/%d"
    with open(stem + ".obj", "w") as f:
        f.write(f"# gens_amd\nmtllib {name}.mtl\nusemtl {name}\n")
        np.savetxt(f, v, fmt="v %.9g %.9g %.9g")
        np.savetxt(f, uv.reshape(-1, 2), fmt="vt %.9g %.9g")
        if normals is not None:
            np.savetxt(f, normals, fmt="vn %.9g %.9g %.9g")
        np.savetxt(f, faces, fmt=fmt)
    with open(stem + ".mtl", "w") as f:
        f.write(f"newmtl {name}\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {name}.png\n")
    Image.fromarray(np.ascontiguousarray(texture)).save(stem + ".png")
    return stem + ".obj", stem + ".mtl", stem + ".png"


def read_obj(path):
    """Inverse of write_obj -> dict: "vertices" (V,3) float32, "triangles" (T,3) int32, "uv" (T,3,2) float32, "normals" (V,3) float32 or
    None, "texture" (H,W,3) uint8 (through the material's map_Kd; None if the file names none).  Reads what write_obj writes: triangles
    whose corners are a/ta or a/ta/na, with the normal index equal to the vertex index."""
    stem = _obj_stem(path)
    rows = {"v": [], "vt": [], "vn": [], "f": []}
    mtl = None
    with open(stem + ".obj") as f:
        for line in f:
            words = line.split()
            if not words or words[0].startswith("#"):
                continue
            if words[0] == "mtllib":
                mtl = words[1]
            elif words[0] in rows:
                rows[words[0]].append(words[1:])
    v = np.array(rows["v"], dtype=np.float64).astype(np.float32).reshape(-1, 3)
    vt = np.array(rows["vt"], dtype=np.float64).astype(np.float32).reshape(-1, 2)
    vn = np.array(rows["vn"], dtype=np.float64).astype(np.float32).reshape(-1, 3) if rows["vn"] else None
    if any(len(face) != 3 for face in rows["f"]):
        raise ValueError(f"{stem}.obj: non-triangular face")
    corners = np.array([[c.split("/") for c in face] for face in rows["f"]], dtype=np.int64).reshape(len(rows["f"]), 3, -1)
    if corners.shape[2] < 2 and len(corners):
        raise ValueError(f"{stem}.obj: faces without texture coordinates")
    tri = (corners[:, :, 0] - 1).astype(np.int32) if len(corners) else np.zeros((0, 3), np.int32)
    uv = vt[corners[:, :, 1] - 1] if len(corners) else np.zeros((0, 3, 2), np.float32)
    if vn is not None and len(corners) and not (corners[:, :, 2] == corners[:, :, 0]).all():
        raise ValueError(f"{stem}.obj: normals are read per vertex (f a/ta/a)")
    texture = None
    if mtl is not None:
        with open(os.path.join(os.path.dirname(stem), mtl)) as f:
            maps = [line.split()[1] for line in f if line.split()[:1] == ["map_Kd"]]
        if maps:
            texture = np.asarray(Image.open(os.path.join(os.path.dirname(stem), maps[0])).convert("RGB"))
    return {"vertices": v, "triangles": tri, "uv": uv, "normals": vn, "texture": texture}


_PLY_TYPES = {b"char": "i1", b"int8": "i1", b"uchar": "u1", b"uint8": "u1", b"short": "<i2", b"int16": "<i2", b"ushort": "<u2", b"uint16": "<u2",
              b"int": "<i4", b"int32": "<i4", b"uint": "<u4", b"uint32": "<u4", b"float": "<f4", b"float32": "<f4", b"double": "<f8",
              b"float64": "<f8"}


def read_ply(path, attributes=False):
    """Inverse of write_ply (binary little-endian, x/y/z vertices, uchar-counted int triangles) -> (vertices, triangles).  Also reads what
    the DTU scoring reads (evaluation/dtu_eval.py:84, 122): a file whose vertices carry further scalar properties (normals, colours), and a
    point cloud without a face element, which gives triangles of shape (0, 3).  The vertices keep the file's x/y/z type.
    attributes=True: -> (vertices, triangles, attrs), attrs holding "normals" (V,3) from nx ny nz and "colors" (V,3) from red green blue, in
    the file's types, where the file has them."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        nv, nf, element, props, face_props = None, 0, None, [], []
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: truncated header")
            words = line.split()
            if words[:1] == [b"format"] and words[1] != b"binary_little_endian":
                raise ValueError(f"{path}: only binary_little_endian is read")
            if words[:1] == [b"element"]:
                element = words[1]
                if element == b"vertex":
                    nv = int(words[2])
                elif element == b"face":
                    nf = int(words[2])
                elif int(words[2]):
                    raise ValueError(f"{path}: element {element.decode()} is not read")
            if words[:1] == [b"property"]:
                if element == b"vertex":
                    if words[1] == b"list" or words[1] not in _PLY_TYPES:
                        raise ValueError(f"{path}: vertex property {line.decode().strip()!r} is not read")
                    props.append((words[2].decode(), _PLY_TYPES[words[1]]))
                elif element == b"face":
                    face_props.append(words[1:])
            if words[:1] == [b"end_header"]:
                break
        if nv is None or not all(c in [p for p, _ in props] for c in "xyz"):
            raise ValueError(f"{path}: no vertex element with x, y, z")
        rows = np.frombuffer(f.read(np.dtype(props).itemsize * nv), dtype=props)
        v = np.stack([rows["x"], rows["y"], rows["z"]], axis=-1) if nv else np.zeros((0, 3), dtype=props[0][1])
        if nf and (len(face_props) != 1 or face_props[0][0] != b"list" or _PLY_TYPES.get(face_props[0][1]) != "u1" or
                   _PLY_TYPES.get(face_props[0][2]) not in ("<i4", "<u4")):
            raise ValueError(f"{path}: faces must be one uchar-counted list of int")
        faces = np.frombuffer(f.read(13 * nf), dtype=[("n", "u1"), ("idx", "<i4", (3,))])
        if nf and not (faces["n"] == 3).all():
            raise ValueError(f"{path}: non-triangular face")
    if not attributes:
        return v.copy(), faces["idx"].copy()
    have, attrs = [p for p, _ in props], {}
    for key, cols in (("normals", ("nx", "ny", "nz")), ("colors", ("red", "green", "blue"))):
        if all(c in have for c in cols):
            attrs[key] = np.stack([rows[c] for c in cols], axis=-1)
    return v.copy(), faces["idx"].copy(), attrs


@torch.no_grad()
def clean_mesh_by_mask(vertices, triangles, masks, intrs, c2ws, min_nb_visible=1):
    """utils/clean_mesh.py:9-35: keep the triangles whose three vertices project inside the (dilated) object mask of more than
    `min_nb_visible` views.  vertices (V,3) in the cameras' frame, masks (nv,H,W), intrs (nv,4,4), c2ws (nv,4,4) -> kept triangles."""
    points = torch.from_numpy(np.asarray(vertices)).float().permute(1, 0)
    masks, intrs, c2ws = masks.cpu(), intrs.cpu(), c2ws.cpu()
    nv, h, w = masks.shape
    pts_cam = torch.matmul(c2ws.inverse(), torch.cat([points, torch.ones_like(points[:1])], dim=0)[None])[:, :3]
    pts_img = torch.matmul(intrs[:, :3, :3], pts_cam)
    pts_xy = pts_img[:, :2] / torch.clamp(pts_img[:, 2:], 1e-8)
    pts_xy[:, 0] = 2 * pts_xy[:, 0] / (w - 1) - 1
    pts_xy[:, 1] = 2 * pts_xy[:, 1] / (h - 1) - 1
    in_mask = (pts_xy.abs() <= 1).all(dim=1) & (pts_img[:, -1] > 1e-8)
    grid = torch.clamp(pts_xy.permute(0, 2, 1).unsqueeze(1), -10, 10)
    warp_mask = F.grid_sample(masks.unsqueeze(1).float(), grid, align_corners=True).squeeze(1).squeeze(1)
    valid = ((warp_mask > 0) * in_mask).sum(dim=0) > min_nb_visible
    tri = torch.from_numpy(np.asarray(triangles).astype(np.int64))
    return np.asarray(triangles)[valid[tri].all(dim=-1).numpy()]


def drop_small_components(vertices, triangles, min_faces=500, return_index=False):
    """utils/clean_mesh.py:101-106 without trimesh, on the host: keep the connected components (faces sharing an edge) of at least
    `min_faces` faces and drop the vertices nothing references any more -> (vertices, triangles) re-indexed.  Faces are joined across
    every shared edge, also one that more than two faces share; trimesh's face_adjacency (and clean_mesh_outside_frustum) joins only
    across edges of exactly two faces.  On manifold meshes the two agree.
    return_index: also the (V',) int64 indices of the kept vertices in `vertices` (per-vertex attributes follow with attrs[index])."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    v = np.asarray(vertices)
    if len(tri) == 0:
        return (v[:0], tri, np.zeros(0, dtype=np.int64)) if return_index else (v[:0], tri)
    # faces adjacent through a shared (undirected) edge: sort the three edges of every face, group equal edges
    edges = np.sort(np.stack([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]], 1).reshape(-1, 2), axis=1)
    face_of = np.repeat(np.arange(len(tri)), 3)
    order = np.lexsort((edges[:, 1], edges[:, 0]))
    e, f = edges[order], face_of[order]
    same = (e[1:] == e[:-1]).all(axis=1)
    a, b = f[:-1][same], f[1:][same]
    n_comp, label = connected_components(coo_matrix((np.ones(len(a), dtype=np.int8), (a, b)), shape=(len(tri), len(tri))), directed=False)
    keep = np.bincount(label, minlength=n_comp)[label] >= min_faces
    tri = tri[keep]
    used = np.zeros(len(v), dtype=bool)
    used[tri.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    mesh = v[used], remap[tri].astype(np.asarray(triangles).dtype if len(tri) else np.int64)
    return mesh + (np.flatnonzero(used).astype(np.int64),) if return_index else mesh


def as_numpy(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def device_of(*xs, device=None):
    """`device` if given, else the device of the first HIP tensor among xs, else the current one."""
    if device is not None:
        return torch.device(device)
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    return torch.device("cuda", torch.cuda.current_device())


@torch.no_grad()
def clean_mesh_outside_frustum(vertices, triangles, masks, intrs, c2ws, upscale=4, min_faces=500, return_index=False):
    """utils/clean_mesh.py:38-106 on the device (K23): keep the faces that some masked pixel of some view (upsampled by `upscale`) sees
    first, then the connected components of at least `min_faces` faces, then the referenced vertices (in their order, as trimesh's
    remove_unreferenced_vertices).  vertices (V,3), triangles (F,3) (arrays or tensors), masks (nv,H,W) raw (a pixel casts iff its
    nearest-upsampled value is > 0), intrs / c2ws (nv,4,4) -> (vertices, triangles) as numpy arrays of the inputs' dtypes.

    Faithful to the reference's quirks: the sorted list of hit faces has its first entry dropped (`values[1:]`) -- that is the -1 of the
    misses when some masked ray missed, and otherwise the smallest face index hit; a face is seen if one view sees it (num_com_vis = 1);
    components come from trimesh's face_adjacency (edges shared by exactly two faces), and a face without such a neighbour is in no
    component at all (trimesh takes the graph's nodes from its edges).  One deliberate deviation: where no component survives, the
    reference raises inside np.concatenate([]); this returns an empty mesh.  trimesh also merges coincident vertices when it loads a
    mesh; K12 emits one vertex per lattice edge, so vertices coincide only where a lattice value equals the threshold exactly, and no
    merge is done here.
    return_index: also the (V',) int64 indices of the returned vertices in `vertices`."""
    from . import ops
    v_np, t_np = as_numpy(vertices), as_numpy(triangles)
    dev = device_of(vertices, triangles, masks)
    v = torch.as_tensor(v_np, dtype=torch.float64).reshape(-1, 3).to(dev)
    t = torch.as_tensor(t_np.astype(np.int64)).reshape(-1, 3).to(dev)
    if len(t):
        grid = ops.build_mesh_grid(v, t)
        flags, any_miss = ops.visible_faces(grid, masks, intrs, c2ws, upscale)       # the union over the views: one view's counts
        t = t[ops.kept_after_quirk(flags, any_miss, 1)[0]]
    return ops.large_components(v_np, t_np.dtype, t, min_faces, return_index=return_index)


@torch.no_grad()
def _drop_small_components_device(vertices, triangles, min_faces=500, return_index=False):
    """clean_mesh.py:101-106 on the device (K23), trimesh's rule: faces are joined across edges of exactly two faces, and a face without
    such a neighbour is in no component -> (vertices, triangles) numpy, unreferenced vertices removed in their order.  Equal to
    `drop_small_components` on manifold meshes (for min_faces >= 2).  return_index: also the kept vertices' (V',) int64 indices."""
    from . import ops
    v_np, t_np = as_numpy(vertices), as_numpy(triangles)
    dev = device_of(vertices, triangles)
    return ops.large_components(v_np, t_np.dtype, torch.as_tensor(t_np.astype(np.int64)).reshape(-1, 3).to(dev), min_faces, return_index=return_index)


@torch.no_grad()
def clean_mesh(vertices, triangles, masks, intrs, c2ws, dilation_radius=11, min_nb_visible=1, upscale=2, min_faces=500, return_index=False):
    """utils/clean_mesh.py:109-130: masks (nv,H,W[,3]) are averaged over a trailing channel axis; the faces outside the dilated (> 0.5)
    masks go (clean_mesh_by_mask, on the host), then clean_mesh_outside_frustum runs with the un-dilated averaged masks -> (vertices,
    triangles) numpy, unreferenced vertices removed (see clean_mesh_outside_frustum for the quirks kept and the one deviation).
    min_faces: the component size of clean_mesh.py:102 (500 there, not an argument of the reference's clean_mesh).
    return_index: also the (V',) int64 indices of the returned vertices in `vertices` (the mask half drops faces only)."""
    masks = masks.detach().cpu()
    if masks.dim() > 3:
        masks = masks.mean(dim=-1)
    v_np = as_numpy(vertices)
    kept = clean_mesh_by_mask(v_np, as_numpy(triangles), dilate_masks(masks, dilation_radius), intrs, c2ws, min_nb_visible)
    return clean_mesh_outside_frustum(v_np, kept, masks, intrs, c2ws, upscale=upscale, min_faces=min_faces, return_index=return_index)


@torch.no_grad()
def simplify_mesh(vertices, triangles, cell, origin=None, normals=None, colors=None, seen=None, device=None, reg=1e-3):
    """ops.simplify_mesh (K33: vertex clustering with quadric-optimal representatives) for host meshes, numpy in and out like the cleaners:
    vertices (V,3), triangles (F,3) (arrays or tensors), cell: the edge of the clustering cells in the vertices' units; origin, reg:
    ops.simplify_mesh's -> (vertices' (V',3) float64, triangles' (F',3) of the input's integer type, attrs).  attrs["source"] (V',) int64:
    per returned vertex the input vertex nearest to it within its cluster; normals / colors / seen (V, ...), where given, come back in attrs
    under those names gathered by it (attributes are never averaged: a colour stays a colour some vertex had).  attrs["stats"]:
    ops.simplify_mesh's counts.  ValueError for what ops.simplify_mesh refuses, and for an attribute whose length is not V."""
    from . import ops
    v_np, t_np = as_numpy(vertices), as_numpy(triangles)
    v_np = np.ascontiguousarray(v_np, dtype=np.float64).reshape(-1, 3)
    given = {name: as_numpy(a) for name, a in (("normals", normals), ("colors", colors), ("seen", seen)) if a is not None}
    for name, a in given.items():
        if len(a) != len(v_np):
            raise ValueError(f"simplify_mesh: {name} has {len(a)} rows for {len(v_np)} vertices")
    t_int = np.asarray(t_np).reshape(-1, 3)
    if t_int.size and (t_int.min() < 0 or t_int.max() >= len(v_np)):
        raise ValueError(f"simplify_mesh: triangle indices {t_int.min()} .. {t_int.max()} outside the {len(v_np)} vertices")
    if len(v_np) >= 2 ** 31:
        raise ValueError(f"simplify_mesh: {len(v_np)} vertices (below 2^31)")
    ops.simplify_request("simplify_mesh", cell, reg)
    dev = device_of(vertices, triangles, device=device)
    out_v, out_t, source, stats = ops.simplify_mesh(torch.from_numpy(v_np).to(dev), torch.from_numpy(np.ascontiguousarray(t_int, dtype=np.int32)).to(dev),
                                                    cell, origin=origin, reg=reg)
    source = source.cpu().numpy()
    attrs = {name: a[source] for name, a in given.items()}
    attrs["source"], attrs["stats"] = source, stats
    return out_v.cpu().numpy(), out_t.cpu().numpy().astype(t_int.dtype if np.issubdtype(t_int.dtype, np.integer) else np.int32), attrs


@torch.no_grad()
def compare_meshes(va, ta, vb, tb, device=None, **kw):
    """ops.mesh_distance (K36: exact point-to-triangle distances, both ways) for host meshes, numpy in like the cleaners: vertices (V,3),
    triangles (F,3) of the meshes A and B (arrays or tensors); kw: ops.mesh_distance's density, samples, max_dist, signed, sign, beta (sign="winding":
    the sign from generalised winding numbers, K40, for meshes whose edges give K37 none) -> its dict as plain
    Python numbers (a_to_b / b_to_a with n, unmatched, mean, rms, max, q50, q90, q99 and, with signed=True, signed_mean, inside, no_sign (K37);
    hausdorff; chamfer; density_a, density_b).  ValueError for what
    ops.mesh_distance refuses, for triangle indices outside the vertices and for vertices that are not finite, before the device is
    looked at."""
    from . import ops
    unknown = sorted(set(kw) - set(ops.MESH_DISTANCE_KEYS))
    if unknown:
        raise ValueError(f"compare_meshes: unknown keyword {unknown[0]!r} (ops.mesh_distance's {', '.join(ops.MESH_DISTANCE_KEYS)})")
    ops.mesh_distance_keywords("compare_meshes", kw)
    meshes = []
    for name, v, t in (("A", va, ta), ("B", vb, tb)):
        v_np = np.ascontiguousarray(as_numpy(v), dtype=np.float64).reshape(-1, 3)
        t_np = np.asarray(as_numpy(t)).reshape(-1, 3)
        if t_np.size and (t_np.min() < 0 or t_np.max() >= len(v_np)):
            raise ValueError(f"compare_meshes: mesh {name}: triangle indices {t_np.min()} .. {t_np.max()} outside the {len(v_np)} vertices")
        if not np.isfinite(v_np).all():
            raise ValueError(f"compare_meshes: mesh {name}: a vertex is not finite")
        meshes.append((v_np, np.ascontiguousarray(t_np, dtype=np.int32)))
    dev = device_of(va, ta, vb, tb, device=device)
    out = ops.mesh_distance(*[torch.from_numpy(x).to(dev) for mesh in meshes for x in mesh], **kw)

    def plain(x):
        return {k: plain(v) for k, v in x.items()} if isinstance(x, dict) else (int(x) if isinstance(x, (int, np.integer)) else float(x))
    return plain(out)


@torch.no_grad()
def mesh_report(vertices, triangles, device=None, roughness=False, self_intersections=False, max_pairs=None):
    """ops.mesh_topology(...).report() (K37) for a host mesh, numpy in like the cleaners: vertices (V,3), triangles (F,3) (arrays or tensors)
    -> the dict of Python numbers: vertices, vertices_referenced, faces, faces_invalid, edges and their counts by class (boundary, manifold,
    flipped, non-manifold), vertices_pinched, vertices_nonmanifold, components, largest_component_faces, boundary_components, euler, closed,
    oriented, manifold, watertight, genus (None unless watertight), area, volume.  Any indices are accepted: a face with an index outside
    the vertices or a repeated one is counted as invalid and takes part in nothing else.  roughness=True: a further key "roughness", ops.
    mesh_roughness's report {edges, mean, rms, max} of the dihedral angles (K39).  self_intersections=True: a further key
    "self_intersections", the counts of ops.mesh_self_intersections (K41: candidates, intersecting and undecided pairs, degenerate and
    uncertain faces, ...); with max_pairs=N also "pairs": {"pairs": the first N (s, t), "kinds": 1 intersecting / 2 undecided}.  The
    defaults launch nothing of K41 and return what they did.  ValueError, before the device is looked at, for arrays that are not (n, 3),
    indices that are not whole numbers or do not fit int32, a `roughness` or `self_intersections` that is no bool, a max_pairs that is no
    positive int or None, or that comes without self_intersections=True."""
    from . import ops
    if not isinstance(roughness, bool):
        raise ValueError(f"mesh_report: roughness = {roughness!r}: True or False")
    if not isinstance(self_intersections, bool):
        raise ValueError(f"mesh_report: self_intersections = {self_intersections!r}: True or False")
    ops.check_intersect_request("mesh_report", True, max_pairs)
    if max_pairs is not None and not self_intersections:
        raise ValueError("mesh_report: max_pairs goes with self_intersections=True")
    v_np, t_np = np.asarray(as_numpy(vertices)), np.asarray(as_numpy(triangles))
    if any(x.size and (x.ndim != 2 or x.shape[1] != 3) for x in (v_np, t_np)):
        raise ValueError(f"mesh_report: vertices {v_np.shape}, triangles {t_np.shape}: expected (V, 3) and (F, 3)")
    if t_np.size and not np.issubdtype(t_np.dtype, np.integer):
        raise ValueError(f"mesh_report: triangles of {t_np.dtype}: whole numbers")
    if t_np.size and (t_np.min() < -2 ** 31 or t_np.max() >= 2 ** 31):
        raise ValueError("mesh_report: a triangle index does not fit int32")
    v_np = np.ascontiguousarray(v_np, dtype=np.float64).reshape(-1, 3)
    t_np = np.ascontiguousarray(t_np.reshape(-1, 3), dtype=np.int32)
    dev = device_of(vertices, triangles, device=device)
    if not roughness and not self_intersections:
        return ops.mesh_topology(torch.from_numpy(v_np).to(dev), torch.from_numpy(t_np).to(dev)).report()
    dv, dt = torch.from_numpy(v_np).to(dev), torch.from_numpy(t_np).to(dev)
    topo = ops.mesh_topology(dv, dt, normals=roughness)
    out = topo.report()
    if roughness:
        out["roughness"] = ops.mesh_roughness(dv, dt, topology=topo)[1]
    if self_intersections:
        if max_pairs is None:
            out["self_intersections"] = ops.self_intersection_counts(dv, dt, who="mesh_report")
        else:
            found = ops.self_intersections_of(dv, dt, max_pairs=max_pairs, who="mesh_report")
            out["self_intersections"] = {k: found.counts[k] for k in ops.SELF_INTERSECTION_KEYS}
            out["pairs"] = {"pairs": found.pairs.cpu().tolist(), "kinds": found.kinds.cpu().tolist()}
    return out


def _mesh_arrays(who, vertices, triangles):
    """Host arrays of a mesh with any indices -> (vertices (V, 3) float64, triangles (F, 3) int32, the input's integer type); ValueError for
    arrays that are not (n, 3), indices that are not whole numbers or do not fit int32."""
    v_np, t_np = np.asarray(as_numpy(vertices)), np.asarray(as_numpy(triangles))
    if any(x.size and (x.ndim != 2 or x.shape[1] != 3) for x in (v_np, t_np)):
        raise ValueError(f"{who}: vertices {v_np.shape}, triangles {t_np.shape}: expected (V, 3) and (F, 3)")
    if t_np.size and not np.issubdtype(t_np.dtype, np.integer):
        raise ValueError(f"{who}: triangles of {t_np.dtype}: whole numbers")
    if t_np.size and (t_np.min() < -2 ** 31 or t_np.max() >= 2 ** 31):
        raise ValueError(f"{who}: a triangle index does not fit int32")
    kind = t_np.dtype if np.issubdtype(t_np.dtype, np.integer) else np.dtype(np.int32)
    return np.ascontiguousarray(v_np, dtype=np.float64).reshape(-1, 3), np.ascontiguousarray(t_np.reshape(-1, 3), dtype=np.int32), kind


def carry_repair_attributes(triangles, vertex_source, face_source, normals=None, colors=None, seen=None):
    """The attributes of a repaired mesh (ops.repair_mesh's triangles', vertex_source, face_source as host arrays) from those of its input:
    a kept vertex takes its source's row; a centroid, whose fill faces (b, a, centroid) name its loop once per vertex, takes the loop's
    mean normal, renormalised (a zero row if the mean is zero), the mean colour rounded to the nearest whole number, and `seen` only if
    the whole loop is seen -> {name: array} for the attributes given."""
    kept = vertex_source >= 0
    fill = triangles[face_source < 0]
    fill = fill[~kept[fill[:, 2]]] if len(fill) else fill          # (a loop of three has no centroid: its face carries nothing)
    count = np.zeros(len(vertex_source))
    np.add.at(count, fill[:, 2], 1.0)
    out = {}
    for name, a in (("normals", normals), ("colors", colors), ("seen", seen)):
        if a is None:
            continue
        a = np.asarray(a)
        rows = np.zeros((len(vertex_source),) + a.shape[1:], dtype=a.dtype)
        rows[kept] = a[vertex_source[kept]]
        if len(fill):
            total = np.zeros(rows.shape, dtype=np.float64)
            np.add.at(total, fill[:, 2], a[vertex_source[fill[:, 1]]].astype(np.float64))
            mean = total[~kept] / count[~kept].reshape((-1,) + (1,) * (a.ndim - 1))
            if name == "normals":
                length = np.sqrt((mean * mean).sum(axis=-1, keepdims=True))
                mean = np.where(length > 0.0, mean / np.where(length > 0.0, length, 1.0), 0.0)
            elif name == "colors":
                mean = np.rint(mean) if np.issubdtype(a.dtype, np.integer) else mean
            else:
                mean = mean == 1.0                                 # every vertex of the loop is seen
            rows[~kept] = mean.astype(a.dtype)
        out[name] = rows
    return out


@torch.no_grad()
def repair_mesh(vertices, triangles, normals=None, colors=None, seen=None, device=None, **kw):
    """ops.repair_mesh (K38: duplicate and invalid faces dropped, pinches and non-manifold edges split, small components dropped,
    components re-oriented, small holes closed) for host meshes, numpy in and out like the cleaners: vertices (V,3), triangles (F,3) (arrays
    or tensors, any indices); kw: ops.repair_mesh's split, orient, min_component_faces, max_hole_edges, dedupe -> (vertices' (V',3) float64,
    triangles' (F',3) of the input's integer type, attrs).  attrs["vertex_source"] (V',), attrs["face_source"] (F',) int32 (-1: a centroid
    / a fill face), attrs["face_flipped"] (F',) bool, attrs["stats"]: ops.repair_mesh's counts; normals / colors / seen (V, ...), where given,
    come back under those names carried through vertex_source (carry_repair_attributes: a centroid takes its loop's renormalised mean
    normal, rounded mean colour and the AND of `seen`).  ValueError, before the device is looked at, for what ops.repair_request refuses, for
    arrays that are not (n, 3), indices that are not whole numbers or do not fit int32, and for an attribute whose length is not V."""
    from . import ops
    who = "repair_mesh"
    opt = ops.repair_request(who, **kw)
    v_np, t_np, kind = _mesh_arrays(who, vertices, triangles)
    given = {name: as_numpy(a) for name, a in (("normals", normals), ("colors", colors), ("seen", seen)) if a is not None}
    for name, a in given.items():
        if len(a) != len(v_np):
            raise ValueError(f"{who}: {name} has {len(a)} rows for {len(v_np)} vertices")
    dev = device_of(vertices, triangles, device=device)
    out_v, out_t, vertex_source, face_source, flipped, stats = ops.repair_mesh(torch.from_numpy(v_np).to(dev), torch.from_numpy(t_np).to(dev), **opt)
    out_t, vertex_source, face_source = out_t.cpu().numpy(), vertex_source.cpu().numpy(), face_source.cpu().numpy()
    attrs = carry_repair_attributes(out_t, vertex_source, face_source, **given)
    attrs.update(vertex_source=vertex_source, face_source=face_source, face_flipped=flipped.cpu().numpy(), stats=stats)
    return out_v.cpu().numpy(), out_t.astype(kind), attrs


@torch.no_grad()
def smooth_mesh(vertices, triangles, colors=None, seen=None, device=None, **kw):
    """ops.smooth_mesh (K39: Laplacian / Taubin smoothing with uniform or cotangent weights) for host meshes, numpy in and out like the
    cleaners: vertices (V,3), triangles (F,3) (arrays or tensors, any indices); kw: ops.smooth_mesh's iterations, lam, mu, weights,
    fix_boundary, measure and pinned ((V,) bool) -> (vertices' (V,3) float64, triangles (F,3) as they came, attrs).  attrs["stats"]:
    ops.smooth_mesh's stats; colors / seen (V, ...), where given, come back under those names unchanged (the vertex count does not change).
    Normals are not accepted: they no longer describe the surface (recompute them: vertex_attributes, or ops.mesh_topology(normals=True)).
    ValueError, before the device is looked at, for what ops.smooth_request refuses, a `normals` keyword, arrays that are not (n, 3),
    indices that are not whole numbers or do not fit int32, and for an attribute or a `pinned` whose length is not V."""
    from . import ops
    who = "smooth_mesh"
    if "normals" in kw:
        raise ValueError(f"{who}: normals are not carried: after smoothing they no longer describe the surface (recompute them)")
    pinned = kw.pop("pinned", None)
    opt = ops.smooth_request(kw, who)
    v_np, t_np, _ = _mesh_arrays(who, vertices, triangles)
    given = {name: as_numpy(a) for name, a in (("colors", colors), ("seen", seen)) if a is not None}
    if pinned is not None:
        pinned = np.asarray(as_numpy(pinned))
        if pinned.dtype != np.bool_ or pinned.ndim != 1:
            raise ValueError(f"{who}: pinned is {pinned.shape} {pinned.dtype}, expected (V,) bool")
    for name, a in {**given, **({} if pinned is None else {"pinned": pinned})}.items():
        if len(a) != len(v_np):
            raise ValueError(f"{who}: {name} has {len(a)} rows for {len(v_np)} vertices")
    dev = device_of(vertices, triangles, device=device)
    out_v, _, stats = ops.smooth_mesh(torch.from_numpy(v_np).to(dev), torch.from_numpy(t_np).to(dev),
                                      pinned=None if pinned is None else torch.from_numpy(np.ascontiguousarray(pinned)).to(dev), **opt)
    return out_v.cpu().numpy(), as_numpy(triangles), {**given, "stats": stats}


def dilate_masks(masks, radius=11):
    """utils/clean_mesh.py:119-125: masks (nv,H,W[,3]) > 0.5, dilated by a disk of `radius` pixels (skimage.morphology.disk)."""
    from scipy import ndimage
    masks = masks.cpu()
    if masks.dim() > 3:
        masks = masks.mean(dim=-1)
    yy, xx = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    disk = (xx * xx + yy * yy) <= radius * radius
    return torch.stack([torch.from_numpy(ndimage.binary_dilation((m > 0.5).numpy(), structure=disk)) for m in torch.unbind(masks)])


# ------------------------------------------------------------------------------------------------------------------ images
def depth_to_rgb(depth, vmin=0.0, vmax=2.5):
    """runner.py:379-390: (H,W) depth -> (H,W,3) uint8 through matplotlib's magma map, linear in [vmin, vmax]."""
    import matplotlib as mpl
    import matplotlib.cm as cm
    mapper = cm.ScalarMappable(norm=mpl.colors.Normalize(vmin=vmin, vmax=vmax), cmap="magma")
    return (mapper.to_rgba(np.asarray(depth))[:, :, :3] * 255).astype(np.uint8)


def save_depth(depth, file_path):
    Image.fromarray(depth_to_rgb(depth)).save(file_path)


def save_validation_outputs(base_exp_dir, outputs, inputs, tag, image_tag=None, clean=False, clean_frustum=False):
    """Store one validated view the way runner.py:215-246 (tag = "epoch{e}", image names from inputs["file_name"]) and
    runner.py:349-375 (tag = "step{s}", image_tag = the view index) do.  Returns the written paths.
    clean=True: the mask half of the cleaning only; clean=True, clean_frustum=True: the whole of utils/clean_mesh.py's clean_mesh
    (`clean_mesh`, what runner.py --clean_mesh scores).  clean_frustum=True without clean=True is an error (the frustum step runs on
    the mask half's result).
    outputs["vertex_normals"] / ["vertex_colors"] (validate's mesh_attributes), where present, follow the mesh: through the cleaning's
    vertex index, the normals through transform_normals; colours of vertices no source view sees (outputs["vertex_seen"] False: the network's
    output is arbitrary there) are written mid-grey (128, 128, 128).
    outputs["surface_depth"] / ["surface_normal_img"] / ["surface_img"] (validate's surface_render), where present, are written under
    val_surface_depth/, val_surface_normal/ and val_surface_img/ by the writers of their volume-rendered counterparts; pixels whose ray did
    not hit the surface are black.
    outputs["mesh_depth"] / ["mesh_normal_img"] / ["mesh_img"] (validate's mesh_render, K35), where present, are written in the same way
    under val_mesh_depth/, val_mesh_normal/ and val_mesh_img/; pixels whose ray did not hit the mesh (outputs["mesh_hit"]) are black.
    outputs["fused_points"] (validate's surface_fusion), where present, is written as pcd/{scene}_{tag}.ply (write_point_cloud) in world
    coordinates (transform_vertices / transform_normals with scale_mat), with fused_normals and fused_colors where present; colours of points
    no source view sees (fused_seen False) are written mid-grey.  Copied to pcd/scan{n}.ply it is what evaluate_dtu(mode="pcd") reads.
    outputs["texture"] (validate's mesh_texture), where present, is written with the mesh as meshes/{scene}_{tag}.obj, its .mtl and its
    .png beside the PLY (write_obj), in world coordinates, with outputs["texture_uv"] and the vertex normals where present; texels no
    source view sees (outputs["texture_seen"] False) are mid-grey.  Not together with clean=True (ValueError before anything is written):
    cleaning drops faces and the atlas is indexed by face, so texture the cleaned mesh afterwards (ImplicitSurface.texture_mesh)."""
    if clean_frustum and not clean:
        raise ValueError("save_validation_outputs: clean_frustum=True needs clean=True")
    if clean and outputs.get("texture") is not None:
        raise ValueError("save_validation_outputs: clean=True drops faces and the texture atlas is indexed by face: clean the mesh, then "
                         "texture it with ImplicitSurface.texture_mesh")
    scene = inputs["scene"]
    image_tag = inputs["file_name"] if image_tag is None else image_tag
    vertices, triangles = outputs["vertices"], outputs["triangles"]
    normals, colors = outputs.get("vertex_normals"), outputs.get("vertex_colors")
    if colors is not None and outputs.get("vertex_seen") is not None:
        colors = np.where(np.asarray(outputs["vertex_seen"], dtype=bool)[:, None], colors, np.uint8(128))
    if clean and clean_frustum:
        vertices, triangles, index = clean_mesh(vertices, triangles, inputs["masks"], inputs["intrs"], inputs["c2ws"], return_index=True)
        normals, colors = (None if a is None else np.asarray(a)[index] for a in (normals, colors))
    elif clean:
        triangles = clean_mesh_by_mask(vertices, triangles, dilate_masks(inputs["masks"]), inputs["intrs"], inputs["c2ws"])
    scale_mat = inputs["scale_mat"].detach().cpu().numpy()
    vertices = transform_vertices(vertices, scale_mat)
    if normals is not None:
        normals = transform_normals(normals, scale_mat)
    paths = {}
    for sub in ("meshes", "val_img", "val_normal", "val_sdf_depth", "val_render_depth"):
        os.makedirs(os.path.join(base_exp_dir, sub), exist_ok=True)
    paths["mesh"] = os.path.join(base_exp_dir, "meshes", f"{scene}_{tag}.ply")
    write_ply(paths["mesh"], vertices, triangles, normals=normals, colors=colors)
    if outputs.get("texture") is not None:
        paths["obj"], paths["mtl"], paths["texture"] = write_obj(os.path.join(base_exp_dir, "meshes", f"{scene}_{tag}.obj"), vertices, triangles,
                                                                 outputs["texture_uv"], outputs["texture"], normals=normals,
                                                                 seen=outputs.get("texture_seen"))
    paths["img"] = os.path.join(base_exp_dir, "val_img", f"{image_tag}_{tag}.png")
    Image.fromarray(outputs["img_fine"].astype(np.uint8)).save(paths["img"])
    paths["normal"] = os.path.join(base_exp_dir, "val_normal", f"{image_tag}_{tag}.png")
    Image.fromarray(outputs["normal_img"].astype(np.uint8)).save(paths["normal"])
    paths["render_depth"] = os.path.join(base_exp_dir, "val_render_depth", f"{image_tag}_{tag}.png")
    save_depth(outputs["render_depth"], paths["render_depth"])
    paths["sdf_depth"] = os.path.join(base_exp_dir, "val_sdf_depth", f"{image_tag}_{tag}.png")
    save_depth(outputs["sdf_depth"], paths["sdf_depth"])
    for key, sub, name in (("surface_depth", "val_surface_depth", "surface_depth"), ("surface_normal_img", "val_surface_normal", "surface_normal"),
                           ("surface_img", "val_surface_img", "surface_img"), ("mesh_depth", "val_mesh_depth", "mesh_depth"),
                           ("mesh_normal_img", "val_mesh_normal", "mesh_normal"), ("mesh_img", "val_mesh_img", "mesh_img")):
        if key not in outputs:
            continue
        os.makedirs(os.path.join(base_exp_dir, sub), exist_ok=True)
        paths[name] = os.path.join(base_exp_dir, sub, f"{image_tag}_{tag}.png")
        rgb = depth_to_rgb(outputs[key]) if key.endswith("_depth") else np.asarray(outputs[key]).astype(np.uint8)
        hit = outputs.get(key.split("_")[0] + "_hit")
        if hit is not None:                               # (the colour map's lowest entry is not quite black)
            rgb = np.where(np.asarray(hit, dtype=bool)[:, :, None], rgb, np.uint8(0))
        Image.fromarray(rgb).save(paths[name])
    if "fused_points" in outputs:
        os.makedirs(os.path.join(base_exp_dir, "pcd"), exist_ok=True)
        paths["pcd"] = os.path.join(base_exp_dir, "pcd", f"{scene}_{tag}.ply")
        cloud_normals, cloud_colors = outputs.get("fused_normals"), outputs.get("fused_colors")
        if cloud_colors is not None and outputs.get("fused_seen") is not None:
            cloud_colors = np.where(np.asarray(outputs["fused_seen"], dtype=bool)[:, None], cloud_colors, np.uint8(128))
        write_point_cloud(paths["pcd"], transform_vertices(outputs["fused_points"], scale_mat),
                          normals=None if cloud_normals is None else transform_normals(cloud_normals, scale_mat), colors=cloud_colors)
    return paths
