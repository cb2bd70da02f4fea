"""K32: fusion of per-view depth maps into a consistency-filtered point cloud -- the camera table (fusion_cams), the per-pixel votes
(fuse_depth_maps) and the points of the kept pixels (fused_points).  The definition is the comment of K32 in include/gens_hip.h (DESIGN.md,
section 5i); tests/depth_fusion_reference.py restates it in numpy.  Evaluator-agnostic: the depth maps may come from anywhere, as
ops.sphere_trace works on any field.

Part of gens_amd.ops (see ops/__init__.py)."""
import numpy as np

from .base import *  # noqa: F401,F403
from .lookup import compact_valid
from .points import radius_downsample

_f64 = torch.float64


def fusion_cams(intrs, c2ws):
    """The camera table of K32, built on the host in numpy float64: intrs (nv, 4, 4) or (nv, 3, 3), c2ws (nv, 4, 4), tensors or arrays ->
    (nv, 24) float64 numpy array, per view P = K[:3,:3] w2c[:3,:4] (12 values), B = inverse(K[:3,:3] w2c[:3,:3]) (9) and the camera
    centre (3).  Pixel (x, y), integers, is the ray through K^-1 [x, y, 1] (synthetic.make_rays, datasets.camera.rays_from_pixels)."""
    k = np.asarray(torch.as_tensor(intrs).detach().cpu().numpy(), dtype=np.float64)
    c = np.asarray(torch.as_tensor(c2ws).detach().cpu().numpy(), dtype=np.float64)
    if k.ndim != 3 or c.ndim != 3 or c.shape[1:] != (4, 4) or k.shape[0] != c.shape[0] or k.shape[1] < 3 or k.shape[2] < 3:
        raise ValueError(f"fusion_cams: intrs {k.shape} and c2ws {c.shape}: (nv, 4, 4) or (nv, 3, 3) intrinsics and (nv, 4, 4) poses")
    if not (np.isfinite(k).all() and np.isfinite(c).all()):
        raise ValueError("fusion_cams: a camera matrix is not finite")
    out = np.zeros((c.shape[0], 24), np.float64)
    for v in range(c.shape[0]):
        try:
            w2c = np.linalg.inv(c[v])
            out[v, :12] = (k[v, :3, :3] @ w2c[:3, :4]).reshape(-1)
            out[v, 12:21] = np.linalg.inv(k[v, :3, :3] @ w2c[:3, :3]).reshape(-1)
        except np.linalg.LinAlgError:
            raise ValueError(f"fusion_cams: the pose or the intrinsics of view {v} are singular") from None
        out[v, 21:] = c[v, :3, 3]
    return out


def _cams(who, cams, nv, dev):
    cams = torch.as_tensor(cams)
    if cams.dtype != _f64 or cams.numel() != 24 * nv:
        raise ValueError(f"{who}: cams is {tuple(cams.shape)} {cams.dtype}: the (nv, 24) float64 table of fusion_cams for {nv} views")
    return _c(cams.detach().to(dev)).reshape(nv, 24)


def _map(who, name, t, shape, dtype, dev):
    if not torch.is_tensor(t) or not t.is_cuda or (dev is not None and t.device != dev):
        raise ValueError(f"{who}: {name} is not a tensor on the device of the depth maps (gens_amd kernels have no CPU path)")
    if t.dtype != dtype or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError(f"{who}: {name} is {tuple(t.shape)} {t.dtype}, expected {tuple(shape) if shape is not None else '(nv, H, W)'} {dtype}")
    return _c(t.detach())


def default_pairs(nv):
    """Every other view votes for a view: (nv, nv - 1) int32."""
    return np.array([[s for s in range(nv) if s != r] for r in range(nv)], dtype=np.int32).reshape(nv, max(nv - 1, 0))


def _pairs(pairs, nv):
    if pairs is None:
        return default_pairs(nv)
    p = np.asarray(pairs.detach().cpu().numpy() if torch.is_tensor(pairs) else pairs)
    if p.ndim != 2 or p.shape[0] != nv or not np.issubdtype(p.dtype, np.integer):
        raise ValueError(f"fuse_depth_maps: pairs is {p.shape} {p.dtype}: (nv, k) integers, row r the source views of view r ({nv} views)")
    bad = (p != -1) & ((p < 0) | (p >= nv) | (p == np.arange(nv)[:, None]))
    if bad.any():
        r, j = np.argwhere(bad)[0]
        raise ValueError(f"fuse_depth_maps: pairs[{r}][{j}] = {p[r, j]}: a source view is another of the {nv} views, or -1 (padding)")
    return np.ascontiguousarray(p, dtype=np.int32)


def _radius(who, dedupe_radius):
    if dedupe_radius is None:
        return None
    dedupe_radius = float(dedupe_radius)
    if not (dedupe_radius > 0.0 and math.isfinite(dedupe_radius)):
        raise ValueError(f"{who}: dedupe_radius = {dedupe_radius!r}, positive and finite (None: off)")
    return dedupe_radius


def fusion_request(who, nv, pairs, pix_tol, rel_tol, min_views, has_normal, normal_cos):
    """fuse_depth_maps' pairs and thresholds, checked on the host -> (pairs (nv, k) int32 numpy, pix_tol, rel_tol, min_views, normal_cos)."""
    pairs = _pairs(pairs, nv)
    pix_tol, rel_tol = float(pix_tol), float(rel_tol)
    if not (pix_tol >= 0.0 and math.isfinite(pix_tol)) or not (rel_tol >= 0.0 and math.isfinite(rel_tol)):
        raise ValueError(f"{who}: pix_tol = {pix_tol!r}, rel_tol = {rel_tol!r}: finite and at least 0")
    if isinstance(min_views, bool) or int(min_views) != min_views or int(min_views) < 1:
        raise ValueError(f"{who}: min_views = {min_views!r}, a whole number, at least 1")
    if normal_cos is not None and not has_normal:
        raise ValueError(f"{who}: normal_cos needs the normal maps")
    if normal_cos is not None:
        normal_cos = float(normal_cos)
        if not -1.0 <= normal_cos <= 1.0:
            raise ValueError(f"{who}: normal_cos = {normal_cos!r}, a cosine")
    return pairs, pix_tol, rel_tol, int(min_views), normal_cos


def fuse_depth_maps(depth, cams, pairs=None, pix_tol=1.0, rel_tol=0.01, min_views=3, normal=None, normal_cos=None):
    """The votes of K32.  depth (nv, H, W) float32 on the device: each view's z-depth in its own camera, usable where finite and > 0;
    cams: fusion_cams' table; pairs (nv, k) integers: row r the source views that vote for view r, -1 pads (default: every other view; DTU
    callers pass the pair.txt lists).  A source votes for a pixel when the pixel's point, seen through the source's depth map and brought
    back, lands within pix_tol pixels and its depth within rel_tol (relative), both strictly; with normal (nv, H, W, 3) float32 unit world
    normals and normal_cos (None: off) the two normals' dot must also reach normal_cos.
    -> (votes (nv, H, W) uint8, keep (nv, H, W) uint8 = votes >= min_views, fused (nv, H, W) float64 = the mean of the pixel's depth and its
    voters' where kept, else 0) on the device.  ValueError before any launch for bad shapes, dtypes, devices, thresholds or pairs."""
    who = "fuse_depth_maps"
    depth = _map(who, "depth", depth, None, _f32, None)
    if depth.dim() != 3:
        raise ValueError(f"{who}: depth is {tuple(depth.shape)}: (nv, H, W)")
    nv, h, w = depth.shape
    dev = depth.device
    if nv * h * w >= 2 ** 31:
        raise ValueError(f"{who}: {nv} maps of {h} x {w} pixels (nv H W below 2^31)")
    cams = _cams(who, cams, nv, dev)
    pairs, pix_tol, rel_tol, min_views, normal_cos = fusion_request(who, nv, pairs, pix_tol, rel_tol, min_views, normal is not None, normal_cos)
    normal = _map(who, "normal", normal, (nv, h, w, 3), _f32, dev) if normal_cos is not None else None      # (normal_cos None: the test is off)
    u8 = torch.uint8
    votes, keep = torch.empty(nv, h, w, device=dev, dtype=u8), torch.empty(nv, h, w, device=dev, dtype=u8)
    fused = torch.empty(nv, h, w, device=dev, dtype=_f64)
    k = pairs.shape[1]
    pairs_d = torch.from_numpy(pairs).to(dev) if k else None
    L.call("gens_fuse_depth_maps", L.ptr(depth), L.ptr(cams, _f64), L.ptr(pairs_d, torch.int32), L.ptr(normal), nv, h, w, k, pix_tol, rel_tol,
           min_views, 0.0 if normal_cos is None else normal_cos, L.ptr(votes, u8), L.ptr(keep, u8), L.ptr(fused, _f64), L.stream(),
           nbytes=nv * h * w * (14 + 16 * k), flops=nv * h * w * k * 150)
    return votes, keep, fused


def fused_points(fused, cams, keep, normal=None, img=None, dedupe_radius=None):
    """The cloud of K32: fused (nv, H, W) float64 and keep (nv, H, W) uint8 or bool from fuse_depth_maps, cams: fusion_cams' table; normal
    (nv, H, W, 3) float32 and img (nv, H, W, 3) uint8 device maps, optional -> (points (N, 3) float64, normals (N, 3) float32 or None, colors
    (N, 3) uint8 or None, pixel (N,) int64 = the flat index (r H + y) W + x of each point, increasing) on the device: the kept pixels
    compacted (ops.compact_valid; one host read, their count) and lifted, point = c_r + fused (B_r [x, y, 1]).
    Every view that keeps a surface point emits it: a surface seen by m views appears m times, a pixel apart at most.  dedupe_radius (world
    units, None: off) thins the cloud with ops.radius_downsample (K24) in index order and carries normals, colours and pixel through its
    mask.  ValueError before any launch for bad shapes, dtypes, devices or a bad radius."""
    who = "fused_points"
    fused = _map(who, "fused", fused, None, _f64, None)
    if fused.dim() != 3:
        raise ValueError(f"{who}: fused is {tuple(fused.shape)}: (nv, H, W)")
    nv, h, w = fused.shape
    dev = fused.device
    if nv * h * w >= 2 ** 31:
        raise ValueError(f"{who}: {nv} maps of {h} x {w} pixels (nv H W below 2^31)")
    cams = _cams(who, cams, nv, dev)
    if torch.is_tensor(keep) and keep.dtype == torch.bool:
        keep = keep.view(torch.uint8)
    keep = _map(who, "keep", keep, (nv, h, w), torch.uint8, dev)
    if normal is not None:
        normal = _map(who, "normal", normal, (nv, h, w, 3), _f32, dev)
    if img is not None:
        img = _map(who, "img", img, (nv, h, w, 3), torch.uint8, dev)
    dedupe_radius = _radius(who, dedupe_radius)
    n = int((keep != 0).sum())
    u8 = torch.uint8
    points = torch.empty(n, 3, device=dev, dtype=_f64)
    normals = torch.empty(n, 3, device=dev, dtype=_f32) if normal is not None else None
    colors = torch.empty(n, 3, device=dev, dtype=u8) if img is not None else None
    if n == 0:                                          # (compact_valid's rescue of an empty mask is the reference's, not a cloud's)
        return points, normals, colors, torch.empty(0, device=dev, dtype=torch.int64)
    pixel = compact_valid(keep)[0][:n]
    L.call("gens_fused_points", L.ptr(fused, _f64), L.ptr(cams, _f64), L.ptr(pixel, torch.int64), n, nv, h, w, L.ptr(normal), L.ptr(img, u8),
           L.ptr(points, _f64), L.ptr(normals), L.ptr(colors, u8), L.stream(), nbytes=n * (40 + (24 if normals is not None else 0) + (6 if colors is not None else 0)))
    if dedupe_radius is not None:
        sel = radius_downsample(points, dedupe_radius)
        points, pixel = points[sel], pixel[sel]
        normals = None if normals is None else normals[sel]
        colors = None if colors is None else colors[sel]
    return points, normals, colors, pixel


__all__ = [n_ for n_ in dir() if not n_.startswith("__")]
