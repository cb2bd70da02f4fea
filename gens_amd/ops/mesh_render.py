"""K35: depth, normal and colour maps of a triangle mesh as rays see it -- the shading launch behind K23's first hits (shade_mesh_hits), the
chain grid -> first hit -> shade (render_mesh), and the comparison of two such maps (compare_maps, plain torch).  The definition is the
comment of K35 in include/gens_hip.h; tests/mesh_render_reference.py restates it in numpy.

Part of gens_amd.ops (see ops/__init__.py)."""

from .base import *  # noqa: F401,F403
from .geometry import MeshGrid, build_mesh_grid, ray_mesh_first_hit
from .texture import TEXTURE_MAX_TEXELS, TEXTURE_MIN_TEXELS, texture_layout

_i32, _u8 = torch.int32, torch.uint8
MESH_SHADINGS = ("flat", "smooth")
MESH_ORIENT = 0                      # ops.marching_cubes / brick_marching_cubes wind their triangles so that (B - A) x (C - A) points along + grad sdf


def _dev(who, name, t, dtype, shape):
    """A device tensor of `dtype` whose shape matches `shape` (None entries are free) -> contiguous."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise ValueError(f"{who}: {name} is not a tensor on the device (gens_amd kernels have no CPU path)")
    t = t.detach()
    t = t.view(_u8) if t.dtype == torch.bool and dtype == _u8 else t
    if t.dtype != dtype or t.dim() != len(shape) or any(s is not None and s != d for s, d in zip(shape, t.shape)):
        raise ValueError(f"{who}: {name} is {tuple(t.shape)} {t.dtype}, expected {tuple('n' if s is None else s for s in shape)} {dtype}")
    return _c(t)


def _shading(who, shading, orient, normals):
    if shading not in MESH_SHADINGS:
        raise ValueError(f"{who}: shading = {shading!r}: one of {MESH_SHADINGS!r}")
    if orient not in (0, 1) or isinstance(orient, bool):
        raise ValueError(f"{who}: orient = {orient!r}: 0 (as wound) or 1 (reversed)")
    if shading == "smooth" and normals is None:
        raise ValueError(f"{who}: smooth shading needs the vertex normals")
    return MESH_SHADINGS.index(shading), int(orient)


def atlas_texels(n_faces, shape):
    """The tile edge S whose K34 layout of n_faces triangles is an image of `shape` (H, W, ...): W = cols (S + 1) fixes it.  ValueError when
    there is none (the image is not this mesh's atlas)."""
    shape = tuple(int(v) for v in shape[:2])
    fits = [s for s in range(TEXTURE_MIN_TEXELS, TEXTURE_MAX_TEXELS + 1) if texture_layout(n_faces, s)[:2] == shape]
    if len(fits) != 1:
        raise ValueError(f"a texture of {shape} is not the atlas of {n_faces} triangles for any tile edge (K34's layout)")
    return fits[0]


def shade_mesh_hits(grid, rays_o, rays_d, face, t, rot, normals=None, colors=None, seen=None, texture=None, texture_seen=None, texels=None,
                    shading="flat", orient=MESH_ORIENT, outputs=None):
    """The shading of K35 at the first hits (face, t) of ops.ray_mesh_first_hit on `grid` (an ops.MeshGrid: the mesh on the device).
    rays_o / rays_d (n, 3) float32, face (n) int32, t (n) float32, rot (9 floats: inverse(c2ws[0][:3,:3]) row-major, K31's); optional
    normals (V, 3) float32, colors (V, 3) uint8, seen (V) uint8 / bool (K30's vertex attributes); texture (H, W, 3) uint8, texture_seen
    (H, W) uint8 / bool and texels (K34's atlas of this mesh; it takes precedence over the vertex colours).  All device tensors.
    shading "flat" (the face's own normal; orient 1 reverses it) or "smooth" (the vertex normals interpolated).
    -> dict of device tensors: "hit" (n) uint8, "bary" (n, 3), "depth" (n) = t (rot d)_z, "normal" (n, 3), "normal_img" (n, 3) float32, and
    with colours or an atlas "img" (n, 3) uint8, with their seen flags "seen" (n) uint8.  Everything is 0 where the ray is not a hit.
    outputs: the names to produce (default: all the inputs allow).  ValueError before any launch for shapes and types that do not fit."""
    who = "shade_mesh_hits"
    if not isinstance(grid, MeshGrid):
        raise ValueError(f"{who}: grid is {type(grid).__name__}, expected ops.MeshGrid (ops.build_mesh_grid)")
    shade, orient = _shading(who, shading, orient, normals)
    o, d = _dev(who, "rays_o", rays_o, _f32, (None, 3)), _dev(who, "rays_d", rays_d, _f32, (None, 3))
    n, dev = o.shape[0], o.device
    d, face, t = _dev(who, "rays_d", d, _f32, (n, 3)), _dev(who, "face", face, _i32, (n,)), _dev(who, "t", t, _f32, (n,))
    rot = _dev(who, "rot", rot.reshape(-1) if torch.is_tensor(rot) else rot, _f32, (9,))
    n_v, n_f = grid.vertices.shape[0], grid.n_faces
    normals = None if normals is None else _dev(who, "normals", normals, _f32, (n_v, 3))
    colors = None if colors is None else _dev(who, "colors", colors, _u8, (n_v, 3))
    seen = None if seen is None else _dev(who, "seen", seen, _u8, (n_v,))
    if seen is not None and colors is None:
        raise ValueError(f"{who}: seen flags come with the vertex colours")
    h = w = s = 0
    if texture is not None:
        if texels is None:
            raise ValueError(f"{who}: a texture comes with its texels (the tile edge it was made with)")
        h, w = texture_layout(n_f, texels)[:2]
        s = int(texels)
        texture = _dev(who, "texture", texture, _u8, (h, w, 3))
        texture_seen = None if texture_seen is None else _dev(who, "texture_seen", texture_seen, _u8, (h, w))
    elif texture_seen is not None:
        raise ValueError(f"{who}: texture_seen without a texture")
    have = ["hit", "bary", "depth", "normal", "normal_img"]
    if texture is not None or colors is not None:
        have.append("img")
    if (texture_seen if texture is not None else seen) is not None:
        have.append("seen")
    names = have if outputs is None else [k for k in have if k in outputs]
    unknown = [] if outputs is None else [k for k in outputs if k not in have]
    if unknown:
        raise ValueError(f"{who}: outputs {unknown!r} are not available: {have!r} are")
    shapes = {"hit": ((n,), _u8), "bary": ((n, 3), _f32), "depth": ((n,), _f32), "normal": ((n, 3), _f32), "normal_img": ((n, 3), _f32),
              "img": ((n, 3), _u8), "seen": ((n,), _u8)}
    out = {k: torch.empty(shapes[k][0], device=dev, dtype=shapes[k][1]) for k in names}
    if n and names:                                                # (no ray or nothing asked for launches nothing)
        p8 = lambda v: L.ptr(v, _u8)  # noqa: E731
        args = L.MeshShadeArgs(L.ptr(grid.vertices, torch.float64), L.ptr(grid.triangles, _i32), n_v, n_f, L.ptr(o), L.ptr(d), L.ptr(face, _i32),
                               L.ptr(t), n, L.ptr(rot), L.ptr(normals), p8(colors), p8(seen), p8(texture), p8(texture_seen), h, w, s, shade, orient,
                               p8(out.get("hit")), L.ptr(out.get("bary")), L.ptr(out.get("depth")), L.ptr(out.get("normal")),
                               L.ptr(out.get("normal_img")), p8(out.get("img")), p8(out.get("seen")))
        L.call("gens_mesh_shade", C.byref(args), L.stream(), nbytes=n * (32 + 84 + sum(out[k].element_size() * out[k][0].numel() for k in names)))
    return out


def render_mesh(vertices, triangles, rays_o, rays_d, rot, *, grid=None, chunk=None, normals=None, colors=None, seen=None, texture=None,
                texture_seen=None, texels=None, shading="flat", orient=MESH_ORIENT):
    """A triangle mesh as the rays o + t d see it: ops.build_mesh_grid (unless `grid`, the MeshGrid of this mesh, is handed in; vertices and
    triangles may then be None), ops.ray_mesh_first_hit and shade_mesh_hits, whose keywords these are.  vertices (V, 3) and triangles (T, 3)
    device tensors in the frame of the rays.  -> dict of flat per-ray device tensors: "face" (n) int32 (-1: miss), "t" (n) float32 (+inf:
    miss) and shade_mesh_hits' dict.  chunk: rays per launch pair (default: all at once); every ray is independent of the others, so the
    result does not depend on it."""
    who = "render_mesh"
    _shading(who, shading, orient, normals)
    if chunk is not None and (isinstance(chunk, bool) or int(chunk) < 1):
        raise ValueError(f"{who}: chunk = {chunk!r}: at least 1 ray")
    for name, v in (("rays_o", rays_o), ("rays_d", rays_d)):
        if not torch.is_tensor(v) or not v.is_cuda:
            raise ValueError(f"{who}: {name} is not a tensor on the device (gens_amd kernels have no CPU path)")
    if grid is None:
        grid = build_mesh_grid(vertices, triangles)
    o, d = _c(rays_o.detach().to(_f32)).reshape(-1, 3), _c(rays_d.detach().to(_f32)).reshape(-1, 3)
    if o.shape != d.shape:
        raise ValueError(f"{who}: {o.shape[0]} origins for {d.shape[0]} directions")
    n = o.shape[0]
    step = n if chunk is None else int(chunk)
    kw = dict(normals=normals, colors=colors, seen=seen, texture=texture, texture_seen=texture_seen, texels=texels, shading=shading, orient=orient)
    parts = []
    for first in range(0, n, max(step, 1)):
        oc, dc = o[first:first + step], d[first:first + step]
        face, t = ray_mesh_first_hit(oc, dc, grid)
        parts.append({"face": face, "t": t, **shade_mesh_hits(grid, oc, dc, face, t, rot, **kw)})
    if not parts:                                                  # no ray: the empty dict of the same keys
        face, t = torch.empty(0, device=o.device, dtype=_i32), torch.empty(0, device=o.device, dtype=_f32)
        parts.append({"face": face, "t": t, **shade_mesh_hits(grid, o, d, face, t, rot, **kw)})
    return parts[0] if len(parts) == 1 else {k: torch.cat([p[k] for p in parts]) for k in parts[0]}


def compare_maps(a, b):
    """Two maps of the same rays -- dicts with "hit" and "depth" and, for the colour figures, "img" (render_mesh's, ImplicitSurface.render_mesh's
    or render_surface's; tensors or numpy arrays of any leading shape) -> dict:
        "both", "only_a", "only_b", "neither": pixel counts by who hit;
        over the pixels both hit: "color_sum" (the exact integer sum of |img_a - img_b| over pixels and channels), "color_mean" (that sum
        / (3 both)), "color_max" (int), and "depth_mean", "depth_median", "depth_max" of |depth_a - depth_b| in float64 (the median is the
        lower middle value).  The colour figures are None when either map has no "img", and every figure but the counts and "color_sum" is
        None when no pixel is hit by both.  Plain torch: not a hot path."""
    def flat(m, k, cols):
        v = torch.as_tensor(m[k])
        return v.reshape((-1, cols) if cols else (-1,))
    ha, hb = flat(a, "hit", 0) != 0, flat(b, "hit", 0).to(flat(a, "hit", 0).device) != 0
    if ha.shape != hb.shape:
        raise ValueError(f"compare_maps: {ha.shape[0]} and {hb.shape[0]} pixels")
    both = ha & hb
    nb = int(both.sum())
    out = {"both": nb, "only_a": int((ha & ~hb).sum()), "only_b": int((hb & ~ha).sum()), "neither": int((~ha & ~hb).sum())}
    out.update(color_sum=None, color_mean=None, color_max=None, depth_mean=None, depth_median=None, depth_max=None)
    if "img" in a and "img" in b:
        diff = (flat(a, "img", 3).to(torch.int64) - flat(b, "img", 3).to(ha.device).to(torch.int64)).abs()[both]
        out["color_sum"] = int(diff.sum())
        if nb:
            out["color_mean"], out["color_max"] = out["color_sum"] / (3 * nb), int(diff.max())
    if nb:
        dd = (flat(a, "depth", 0).to(torch.float64) - flat(b, "depth", 0).to(ha.device).to(torch.float64)).abs()[both]
        out["depth_mean"], out["depth_median"], out["depth_max"] = float(dd.mean()), float(dd.median()), float(dd.max())
    return out


__all__ = [n_ for n_ in dir() if not n_.startswith("__")]
