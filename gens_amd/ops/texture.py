"""K34: texture atlases for triangle meshes -- the streaming launches around the network kernels of ImplicitSurface.texture_mesh: samples of
the atlas to points on their triangles, one Newton round towards the surface and its guard, colours to pixels, and the per-corner texture coordinates.
The definition is the comment of K34 in include/gens_hip.h; tests/mesh_texture_reference.py restates it in numpy.

Part of gens_amd.ops (see ops/__init__.py)."""
import numpy as np

from .base import *  # noqa: F401,F403

_i32, _u8 = torch.int32, torch.uint8
TEXTURE_MIN_TEXELS, TEXTURE_MAX_TEXELS = 3, 64
TEXTURE_MAX_EDGE = 16384             # the largest atlas edge texture_mesh builds: what viewers and image writers take


def texture_layout(n_faces, texels):
    """-> (H, W, cols, rows, P): the atlas of n_faces triangles with tile edge `texels` (3 to 64).  Every triangle gets P = S (S + 1) / 2
    texels, two triangles share a tile of S + 1 columns by S rows, and the tiles fill cols = ceil(sqrt(n_tiles)) columns.  Host only: no
    launch.  ValueError for texels that is not an integer from 3 to 64 or a negative face count."""
    if isinstance(texels, bool) or not isinstance(texels, (int, np.integer)):
        raise ValueError(f"texture_layout: texels = {texels!r}: an integer from {TEXTURE_MIN_TEXELS} to {TEXTURE_MAX_TEXELS}")
    s, t = int(texels), int(n_faces)
    if not TEXTURE_MIN_TEXELS <= s <= TEXTURE_MAX_TEXELS:
        raise ValueError(f"texture_layout: texels = {s} ({TEXTURE_MIN_TEXELS} to {TEXTURE_MAX_TEXELS})")
    if t < 0:
        raise ValueError(f"texture_layout: {t} faces")
    tiles = (t + 1) // 2
    cols = math.isqrt(tiles)
    cols += cols * cols < tiles
    rows = -(-tiles // cols) if cols else 0
    return rows * s, cols * (s + 1), cols, rows, s * (s + 1) // 2


def texture_fit(n_faces, limit=TEXTURE_MAX_EDGE):
    """The largest texels whose atlas of n_faces triangles has both edges within `limit`, or None if not even 3 fits."""
    for s in range(TEXTURE_MAX_TEXELS, TEXTURE_MIN_TEXELS - 1, -1):
        h, w = texture_layout(n_faces, s)[:2]
        if h <= limit and w <= limit:
            return s
    return None


def _mesh(who, points, triangles):
    for name, t, dtype in (("points", points, _f32), ("triangles", triangles, _i32)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError(f"{who}: {name} is not a tensor on the device (gens_amd kernels have no CPU path)")
        if t.dtype != dtype or t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{who}: {name} is {tuple(t.shape)} {t.dtype}, expected (n, 3) {dtype}")
    return _c(points.detach()), _c(triangles.detach())


def _range(who, n_faces, per_face, s0, s1):
    s0, s1 = int(s0), (n_faces * per_face if s1 is None else int(s1))
    if not 0 <= s0 <= s1 <= n_faces * per_face:
        raise ValueError(f"{who}: samples {s0} .. {s1} of {n_faces} faces x {per_face} samples")
    return s0, s1


def texture_points(points, triangles, texels, s0=0, s1=None, with_edge=False):
    """points (V, 3) float32 and triangles (T, 3) int32 on the device -> the points (s1 - s0, 3) float32 of the atlas samples s0 .. s1 - 1
    of the enumeration s = f P + k (default: all of them); a chunk may begin and end inside a triangle.  with_edge: also the longest edge
    (s1 - s0,) float32 of each sample's triangle (texture_snap's default limit).  A triangle with an index outside the vertices has NaN
    points; the index is not read through."""
    who = "texture_points"
    points, triangles = _mesh(who, points, triangles)
    n_f = triangles.shape[0]
    per_face = texture_layout(n_f, texels)[4]
    s0, s1 = _range(who, n_f, per_face, s0, s1)
    n = s1 - s0
    out = torch.empty(n, 3, device=points.device, dtype=_f32)
    edge = torch.empty(n, device=points.device, dtype=_f32) if with_edge else None
    if n:                                                          # (an empty range launches nothing)
        L.call("gens_texture_points", L.ptr(points), points.shape[0], L.ptr(triangles, _i32), n_f, int(texels), s0, s1, L.ptr(out),
               L.ptr(edge), L.stream(), nbytes=n * (16 if with_edge else 12))
    return (out, edge) if with_edge else out


def texture_snap(points, value, grad, threshold=0.0, limit=None, max_move=None):
    """One Newton round towards the zero set of g = sdf + threshold, in place: points (n, 3) float32, value (n,) or (n, 1) float32 = sdf,
    grad (n, 3) float32 (ops.sdf_mlp(want_grad=True)); limit (n,) float32, a step limit per sample, or one max_move > 0 for all.
    p <- p - g grad / |grad|^2 where g and grad are finite, |grad|^2 > 0 and the step is no longer than the limit; else p is kept.
    -> taken (n,) uint8.  One round of Newton's method: texture_keep_better turns back the steps that did not lower |g|; nothing else is
    promised about convergence."""
    who = "texture_snap"
    if limit is None and not (max_move is not None and float(max_move) > 0.0):
        raise ValueError(f"{who}: max_move = {max_move!r}: a positive length, or a limit per sample")
    if not math.isfinite(float(threshold)):
        raise ValueError(f"{who}: threshold = {threshold!r} (finite)")
    if not points.is_contiguous() or points.dtype != _f32 or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{who}: points are moved in place: a contiguous (n, 3) float32 tensor")
    n = points.shape[0]
    value, grad = _c(value.detach()).reshape(-1), _c(grad.detach()).reshape(-1, 3)
    limit = _c(limit.detach()).reshape(-1) if limit is not None else None
    if value.shape[0] != n or grad.shape[0] != n or (limit is not None and limit.shape[0] != n):
        raise ValueError(f"{who}: {n} points, {value.shape[0]} values, {grad.shape[0]} gradients"
                         f"{'' if limit is None else f', {limit.shape[0]} limits'}")
    taken = torch.empty(n, device=points.device, dtype=_u8)
    if n:
        L.call("gens_texture_snap", L.ptr(points), L.ptr(value), L.ptr(grad), L.ptr(limit), 0.0 if limit is not None else float(max_move),
               float(threshold), n, L.ptr(taken, _u8), L.stream(), nbytes=n * 45)
    return taken


def texture_keep_better(points, value, grad, prev_points, prev_value, prev_grad, threshold=0.0):
    """The snap's guard, in place: where |value + threshold| <= |prev_value + threshold| is false (a NaN included), the row of points
    (n, 3), value (n,) and grad (n, 3) is overwritten with that of prev_points, prev_value and prev_grad: the point goes back to where its
    step began, with that point's value and gradient.  All float32 and contiguous.  -> reverted (n,) uint8."""
    who = "texture_keep_better"
    if not math.isfinite(float(threshold)):
        raise ValueError(f"{who}: threshold = {threshold!r} (finite)")
    n = points.shape[0]
    for name, t, cols in (("points", points, 3), ("value", value, 1), ("grad", grad, 3), ("prev_points", prev_points, 3),
                          ("prev_value", prev_value, 1), ("prev_grad", prev_grad, 3)):
        if not t.is_contiguous() or t.dtype != _f32 or t.numel() != n * cols:
            raise ValueError(f"{who}: {name} is {tuple(t.shape)} {t.dtype}, expected {n} contiguous float32 rows of {cols}")
    reverted = torch.empty(n, device=points.device, dtype=_u8)
    if n:
        L.call("gens_texture_keep_better", L.ptr(points), L.ptr(value), L.ptr(grad), L.ptr(prev_points), L.ptr(prev_value), L.ptr(prev_grad),
               float(threshold), n, L.ptr(reverted, _u8), L.stream(), nbytes=n * 29)
    return reverted


def texture_pack(color, vis, n_faces, texels, s0=0, s1=None, atlas=None, seen=None):
    """color (n, 3) float32 and vis (n, n_src) uint8 (ops.blend_views) of the samples s0 .. s1 - 1 -> (atlas (H, W, 3) uint8, seen (H, W)
    uint8): each sample's texel gets trunc(clip(256 c, 0, 255)) (K30's rule) and its `seen` flag any(vis).  atlas / seen: the arrays a
    chunked caller fills piece by piece (default: new ones, zeroed -- texels no triangle owns stay 0 and not seen)."""
    who = "texture_pack"
    n_f = int(n_faces)
    h, w, _, _, per_face = texture_layout(n_f, texels)
    s0, s1 = _range(who, n_f, per_face, s0, s1)
    n = s1 - s0
    color = _c(color.detach()).reshape(-1, 3)
    n_src = vis.shape[-1] if vis.dim() > 1 else 1
    vis = _c(vis.detach()).reshape(-1, n_src)
    vis = vis.view(_u8) if vis.dtype == torch.bool else vis
    if color.shape[0] != n or vis.shape[0] != n or not 1 <= n_src <= 255:
        raise ValueError(f"{who}: {n} samples, {color.shape[0]} colours, {vis.shape[0]} rows of {n_src} flags (1 to 255)")
    atlas = torch.zeros(h, w, 3, device=color.device, dtype=_u8) if atlas is None else atlas
    seen = torch.zeros(h, w, device=color.device, dtype=_u8) if seen is None else seen
    if tuple(atlas.shape) != (h, w, 3) or tuple(seen.shape) != (h, w):
        raise ValueError(f"{who}: atlas {tuple(atlas.shape)} and seen {tuple(seen.shape)}, expected {(h, w, 3)} and {(h, w)}")
    if n:
        L.call("gens_texture_pack", L.ptr(color), L.ptr(vis, _u8), n_src, n_f, int(texels), s0, s1, L.ptr(atlas, _u8), L.ptr(seen, _u8),
               L.stream(), nbytes=n * (16 + n_src))
    return atlas, seen


def texture_uv(n_faces, texels, device):
    """-> uv (T, 3, 2) float32 on `device`: the texture coordinates of every triangle's corners, u = (x + 0.5) / W and
    v = 1 - (y + 0.5) / H at the corners' texel centres (origin bottom-left, as OBJ expects)."""
    n_f = int(n_faces)
    texture_layout(n_f, texels)
    uv = torch.empty(n_f, 3, 2, device=device, dtype=_f32)
    if n_f:
        L.call("gens_texture_uv", n_f, int(texels), L.ptr(uv), L.stream(), nbytes=n_f * 24)
    return uv


__all__ = [n_ for n_ in dir() if not n_.startswith("__")]
