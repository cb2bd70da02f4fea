"""K25: the device pieces of the DTU mesh finalising step (evaluation/clean_meshes.py) that are its own: OpenCV's elliptical dilation and
the per-vertex mask votes.  Its ray step (view_rays_hit_counts) is in ops/geometry.py, beside K23's.

Part of gens_amd.ops (see ops/__init__.py); citations are relative to /root/reference."""
from .base import *  # noqa: F401,F403

DILATE_MAX_KERNEL = 63


def opencv_ellipse(kw, kh):
    """cv.getStructuringElement(cv.MORPH_ELLIPSE, (kw, kh)) as per-row half-spans: r = kh // 2, c = kw // 2, row i has dy = i - r and
    dx = round_half_even(c * sqrt((r^2 - dy^2) / r^2)) (1 / r^2 taken as 0 for r = 0); it holds the columns max(c - dx, 0) ..
    min(c + dx + 1, kw) - 1.  -> list of kh ints dx.  11 x 11 gives the row widths 1, 7, 9, 11, 11, 11, 11, 11, 9, 7, 1."""
    import math
    kw, kh = int(kw), int(kh)
    r, c = kh // 2, kw // 2
    inv_r2 = 1.0 / (r * r) if r else 0.0
    return [int(round(c * math.sqrt((r * r - (i - r) * (i - r)) * inv_r2))) for i in range(kh)]       # (Python's round is half to even)


def ellipse_footprint(kw, kh):
    """opencv_ellipse as the (kh, kw) boolean array OpenCV returns (as uint8)."""
    import numpy as np
    c = int(kw) // 2
    fp = np.zeros((int(kh), int(kw)), dtype=bool)
    for i, dx in enumerate(opencv_ellipse(kw, kh)):
        fp[i, max(c - dx, 0):min(c + dx + 1, int(kw))] = True
    return fp


def dilate_u8(images, half_spans, kw, channels=None):
    """cv.dilate with OpenCV's defaults (anchor at the centre, pixels outside the image take no part): images (n,h,w,c) or (n,h,w) uint8
    on the device, half_spans = the element's kh rows (opencv_ellipse), kw its width -> (n,h,w,channels) uint8 (or (n,h,w) for a 3-D
    input): the first `channels` channels of every pixel dilated (default: all)."""
    squeeze = images.dim() == 3
    x = _c(images.detach().unsqueeze(-1) if squeeze else images.detach())
    if x.dtype != torch.uint8 or x.dim() != 4:
        raise ValueError("dilate_u8: (n,h,w[,c]) uint8 images")
    n, h, w, c = x.shape
    channels = c if channels is None else int(channels)
    if c not in (1, 3) or not 1 <= channels <= c:
        raise ValueError(f"dilate_u8: {channels} of {c} channels (1 or 3 interleaved, at least one dilated)")
    spans = [int(s) for s in half_spans]
    if len(spans) > DILATE_MAX_KERNEL:
        raise ValueError(f"dilate_u8: {len(spans)} kernel rows (at most {DILATE_MAX_KERNEL})")
    out = torch.empty(n, h, w, channels, device=x.device, dtype=torch.uint8)
    L.call("gens_dilate_u8", L.ptr(x, torch.uint8), L.ptr(out, torch.uint8), n, h, w, c, channels, int(kw), len(spans), L.int_table(spans),
           L.stream(), nbytes=n * h * w * 2 * channels)
    return out[..., 0] if squeeze else out


def vertex_mask_votes(points, proj, masks):
    """clean_points_by_mask's loop (clean_meshes.py:118-139): points (V,3) float64, proj (nv,>=3,4) float32 projection matrices, masks
    (nv,H,W) uint8 (dilated; set where > 128) -> votes (V,) int32: in how many views the point projects inside the mask framed by one
    pixel of ones.  No test for points behind a camera; a point that rounds onto the frame counts as inside; a point with q[2] == 0
    (numpy's int32 cast is undefined there) counts as outside."""
    dev = masks.device
    p = _c(points.detach().to(device=dev, dtype=torch.float64)).reshape(-1, 3)
    m = _c(masks.detach())
    if m.dtype != torch.uint8 or m.dim() != 3:
        raise ValueError("vertex_mask_votes: (nv,H,W) uint8 masks")
    nv, h, w = m.shape
    pr = _c(proj.detach().to(device=dev, dtype=_f32)[:, :3, :4])
    if pr.shape[0] != nv:
        raise ValueError("vertex_mask_votes: one projection per mask")
    votes = torch.empty(p.shape[0], device=dev, dtype=torch.int32)
    L.call("gens_vertex_mask_votes", L.ptr(p, torch.float64), p.shape[0], L.ptr(pr), L.ptr(m, torch.uint8), nv, h, w, L.ptr(votes, torch.int32),
           L.stream(), nbytes=p.shape[0] * 28)
    return votes


__all__ = [n_ for n_ in dir() if not n_.startswith("__")]
