"""K30: per-vertex attributes of an extracted mesh -- the two streaming launches around the network kernels: lattice-index vertices to
points in the model's frame, and gradient / colour / in-frustum flags to unit normals, 8-bit colours and the `seen` flag.

Part of gens_amd.ops (see ops/__init__.py); citations are relative to /root/reference."""
from .base import *  # noqa: F401,F403


def vertex_points(vertices, resolution, span, lo):
    """vertices (V,3) float64 on the device, in lattice-index coordinates (marching_cubes / brick_marching_cubes) -> (V,3) float32 points:
    the float32 rounding of `vertices / (resolution - 1.0) * span + lo` in float64 (implicit_surface.py:424-425).  span, lo: three Python
    floats each, the doubles the host expression would use (extract_geometry: its float32 `b_max - b_min` and `b_min`, widened)."""
    v = _c(vertices.detach()).reshape(-1, 3)
    span, lo = [float(s) for s in span], [float(b) for b in lo]
    if len(span) != 3 or len(lo) != 3:
        raise ValueError("vertex_points: span and lo are three numbers each")
    n = v.shape[0]
    pts = torch.empty(n, 3, device=v.device, dtype=_f32)
    L.call("gens_vertex_points", L.ptr(v, torch.float64), n, int(resolution), *span, *lo, L.ptr(pts), L.stream(), nbytes=n * 36)
    return pts


def vertex_pack(grad=None, color=None, vis=None, normals=None, colors=None, seen=None):
    """grad (V,3) float32 = d sdf / dx (sdf_mlp(want_grad=True)), color (V,3) float32 and vis (V,S) uint8 (blend_views) ->
    (normals (V,3) float32 or None, colors (V,3) uint8 or None, seen (V,) uint8 or None): unit normals (zero where the gradient is zero or
    not finite), trunc(clip(256 c, 0, 255)) (implicit_surface.py:455; 0 where c is not finite) and `any(vis)`.  grad or color may be
    None: what depends on it is not computed.  normals / colors / seen: optional output buffers (slices of the caller's arrays)."""
    if grad is None and color is None:
        raise ValueError("vertex_pack: a gradient, a colour or both")
    if color is not None and vis is None:
        raise ValueError("vertex_pack: a colour comes with its in-frustum flags")
    first = grad if grad is not None else color
    n, s = first.shape[0], 0
    if grad is not None:
        grad = _c(grad.detach()).reshape(-1, 3)
        normals = torch.empty(n, 3, device=grad.device, dtype=_f32) if normals is None else normals
    else:
        normals = None
    if color is not None:
        color = _c(color.detach()).reshape(-1, 3)
        s = vis.shape[-1] if vis.dim() > 1 else 1
        vis = _c(vis.detach()).reshape(-1, s)
        vis = vis.view(torch.uint8) if vis.dtype == torch.bool else vis
        if color.shape[0] != n or vis.shape[0] != n or s < 1:
            raise ValueError(f"vertex_pack: {n} vertices, {color.shape[0]} colours, {vis.shape[0]} rows of {s} flags")
        colors = torch.empty(n, 3, device=color.device, dtype=torch.uint8) if colors is None else colors
        seen = torch.empty(n, device=color.device, dtype=torch.uint8) if seen is None else seen
    else:
        vis = colors = seen = None
    for name, out, rows in (("normals", normals, 3 * n), ("colors", colors, 3 * n), ("seen", seen, n)):
        if out is not None and out.numel() != rows:
            raise ValueError(f"vertex_pack: {name} holds {out.numel()} elements, {rows} expected")
    u8 = torch.uint8
    L.call("gens_vertex_pack", L.ptr(grad), L.ptr(color), L.ptr(vis, u8), s, n, L.ptr(normals), L.ptr(colors, u8), L.ptr(seen, u8), L.stream(),
           nbytes=n * ((24 if grad is not None else 0) + (16 + s if color is not None else 0)))
    return normals, colors, seen


__all__ = [n_ for n_ in dir() if not n_.startswith("__")]
