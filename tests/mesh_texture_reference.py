"""K34 restated in numpy: the texture-atlas rule of include/gens_hip.h, step by step.  Arithmetic is float64 from the float32 inputs, every
operation rounded on its own in the order written (numpy never contracts), results rounded once to float32 -- so the kernels of
csrc/k34_mesh_texture.hip equal these functions bit for bit.  Shared by tests/test_mesh_texture_cpu.py and tests/test_hip_mesh_texture.py."""
import math

import numpy as np

MIN_TEXELS, MAX_TEXELS = 3, 64


def layout(n_faces, texels):
    """-> (H, W, cols, rows, P) of the atlas of n_faces triangles with tile edge `texels`."""
    s, t = int(texels), int(n_faces)
    if not MIN_TEXELS <= s <= MAX_TEXELS:
        raise ValueError(f"texels = {texels!r} ({MIN_TEXELS} to {MAX_TEXELS})")
    if t < 0:
        raise ValueError(f"{n_faces} faces")
    tiles = (t + 1) // 2
    cols = math.isqrt(tiles)
    cols += cols * cols < tiles
    rows = -(-tiles // cols) if cols else 0
    return rows * s, cols * (s + 1), cols, rows, s * (s + 1) // 2


def local_texels(texels):
    """-> (i', j') int64 arrays of length P: sample number k's local texel, j' the outer index and i' the inner."""
    s = int(texels)
    jp = np.concatenate([np.full(s - j, j, dtype=np.int64) for j in range(s)])
    ip = np.concatenate([np.arange(s - j, dtype=np.int64) for j in range(s)])
    return ip, jp


def pixel(n_faces, texels, face, ip, jp):
    """Local texel (ip, jp) of triangle `face` (arrays that broadcast) -> its pixel (x, y), int64."""
    s = int(texels)
    cols = layout(n_faces, s)[2]
    face, ip, jp = np.asarray(face, dtype=np.int64), np.asarray(ip, dtype=np.int64), np.asarray(jp, dtype=np.int64)
    q, turned = face >> 1, (face & 1) != 0
    i = np.where(turned, s - ip, ip)
    j = np.where(turned, s - 1 - jp, jp)
    return (q % max(cols, 1)) * (s + 1) + i, (q // max(cols, 1)) * s + j


def sample_faces(texels, s0, s1):
    """Samples s0 .. s1 - 1 of the enumeration s = f P + k -> (face, ip, jp), int64 arrays."""
    p = int(texels) * (int(texels) + 1) // 2
    smp = np.arange(int(s0), int(s1), dtype=np.int64)
    ip, jp = local_texels(texels)
    k = smp % p
    return smp // p, ip[k], jp[k]


def _edge2(p, q):
    d = q - p
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def texture_points(points, triangles, texels, s0=0, s1=None, with_edge=False):
    """points (V, 3) float32, triangles (T, 3) int32 -> the points (s1 - s0, 3) float32 of samples s0 .. s1 - 1 (default: all), and with
    with_edge the longest edge (s1 - s0,) float32 of each sample's triangle.  A triangle with an index outside 0 .. V - 1: NaN."""
    pts = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    tri = np.asarray(triangles, dtype=np.int32).reshape(-1, 3)
    s = int(texels)
    p = layout(tri.shape[0], s)[4]
    s1 = tri.shape[0] * p if s1 is None else s1
    face, ip, jp = sample_faces(s, s0, s1)
    idx = tri[face].astype(np.int64)
    ok = ((idx >= 0) & (idx < pts.shape[0])).all(axis=1)
    idx = np.where(ok[:, None], idx, 0)
    if pts.shape[0] == 0:
        pts = np.zeros((1, 3), dtype=np.float32)
    a3, b3, c3 = (pts[idx[:, c]].astype(np.float64) for c in range(3))
    den = np.float64(s - 2)
    a, b = (ip.astype(np.float64) / den)[:, None], (jp.astype(np.float64) / den)[:, None]
    with np.errstate(all="ignore"):
        out = ((a3 + a * (b3 - a3)) + b * (c3 - a3)).astype(np.float32)
        out[~ok] = np.nan
        if not with_edge:
            return out
        m = _edge2(a3, b3)
        e = _edge2(b3, c3)
        m = np.where(e > m, e, m)
        e = _edge2(c3, a3)
        m = np.where(e > m, e, m)
        edge = np.sqrt(m).astype(np.float32)
        edge[~ok] = np.nan
    return out, edge


def texture_uv(n_faces, texels, dtype=np.float32):
    """-> (T, 3, 2) corner coordinates: the corners sit at the local texel centres (0, 0), (S - 2, 0), (0, S - 2); u = (x + 0.5) / W,
    v = 1 - (y + 0.5) / H.  dtype=np.float64: the coordinates before their rounding to float32 (the CPU tests' exact arithmetic)."""
    s, t = int(texels), int(n_faces)
    h, w = layout(t, s)[:2]
    face = np.arange(t, dtype=np.int64)[:, None]
    x, y = pixel(t, s, face, np.array([[0, s - 2, 0]]), np.array([[0, 0, s - 2]]))
    if t == 0:
        return np.zeros((0, 3, 2), dtype=dtype)
    u = (x.astype(np.float64) + 0.5) / np.float64(w)
    v = 1.0 - (y.astype(np.float64) + 0.5) / np.float64(h)
    return np.stack([u, v], axis=-1).astype(dtype)


def texture_snap(points, value, grad, threshold=0.0, limit=None, max_move=None):
    """One Newton round: points (n, 3) float32, value (n,) float32, grad (n, 3) float32; limit (n,) float32 per sample or one max_move
    -> (points' (n, 3) float32, taken (n,) bool)."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    g = np.asarray(value, dtype=np.float32).reshape(-1).astype(np.float64) + np.float64(np.float32(threshold))
    gr = np.asarray(grad, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    mm = np.asarray(limit, dtype=np.float32).reshape(-1).astype(np.float64) if limit is not None else np.full(p.shape[0], np.float64(max_move))
    with np.errstate(all="ignore"):
        n2 = (gr[:, 0] * gr[:, 0] + gr[:, 1] * gr[:, 1]) + gr[:, 2] * gr[:, 2]
        t = g / n2
        step = t[:, None] * gr
        len2 = (step[:, 0] * step[:, 0] + step[:, 1] * step[:, 1]) + step[:, 2] * step[:, 2]
        taken = np.isfinite(g) & np.isfinite(n2) & (n2 > 0.0) & (len2 <= mm * mm)
        moved = (p.astype(np.float64) - step).astype(np.float32)
    return np.where(taken[:, None], moved, p), taken


def texture_keep_better(points, value, grad, prev_points, prev_value, prev_grad, threshold=0.0):
    """The snap's guard: where |value + threshold| <= |prev_value + threshold| is false (a NaN included) the row goes back to the previous
    point, value and gradient -> (points, value, grad, reverted (n,) bool)."""
    thr = np.float64(np.float32(threshold))
    v, pv = np.asarray(value, np.float32).reshape(-1), np.asarray(prev_value, np.float32).reshape(-1)
    with np.errstate(all="ignore"):
        back = ~(np.abs(v.astype(np.float64) + thr) <= np.abs(pv.astype(np.float64) + thr))
    pick = lambda a, b: np.where(back[:, None], np.asarray(b, np.float32).reshape(-1, 3), np.asarray(a, np.float32).reshape(-1, 3))  # noqa: E731
    return pick(points, prev_points), np.where(back, pv, v), pick(grad, prev_grad), back


def color8(color):
    """K30's rule: trunc(clip(256 c, 0, 255)) in float32, 0 where c is not finite."""
    c = np.asarray(color, dtype=np.float32)
    with np.errstate(all="ignore"):
        q = np.minimum(np.maximum(c * np.float32(256.0), np.float32(0.0)), np.float32(255.0))
    return np.where(np.isfinite(c), q, np.float32(0.0)).astype(np.uint8)


def texture_pack(color, vis, n_faces, texels, s0=0, s1=None, atlas=None, seen=None):
    """color (n, 3) float32 and vis (n, n_src) flags of samples s0 .. s1 - 1 -> (atlas (H, W, 3) uint8, seen (H, W) uint8), written into the
    arrays given or into zeros."""
    s, t = int(texels), int(n_faces)
    h, w, _, _, p = layout(t, s)
    s1 = t * p if s1 is None else s1
    atlas = np.zeros((h, w, 3), dtype=np.uint8) if atlas is None else atlas
    seen = np.zeros((h, w), dtype=np.uint8) if seen is None else seen
    face, ip, jp = sample_faces(s, s0, s1)
    if len(face) == 0:
        return atlas, seen
    x, y = pixel(t, s, face, ip, jp)
    atlas[y, x] = color8(np.asarray(color).reshape(-1, 3))
    seen[y, x] = (np.asarray(vis).reshape(len(face), -1) != 0).any(axis=1)
    return atlas, seen


def bilinear_taps(uv, h, w):
    """A texture coordinate (..., 2) in float64 -> ((x0, y0), (fx, fy)): the top-left tap's pixel and the weights of the right / lower taps,
    with texel centres at integer + 0.5 and v measured from the bottom (the convention of texture_uv)."""
    uv = np.asarray(uv, dtype=np.float64)
    xc = uv[..., 0] * w - 0.5
    yc = (1.0 - uv[..., 1]) * h - 0.5
    x0, y0 = np.floor(xc), np.floor(yc)
    return (x0.astype(np.int64), y0.astype(np.int64)), (xc - x0, yc - y0)


def bilinear_sample(image, uv):
    """image (H, W, C) float64 sampled bilinearly at uv (n, 2) float64, taps clamped to the image -> (n, C)."""
    h, w = image.shape[:2]
    (x0, y0), (fx, fy) = bilinear_taps(uv, h, w)
    cx = lambda v: np.clip(v, 0, w - 1)  # noqa: E731
    cy = lambda v: np.clip(v, 0, h - 1)  # noqa: E731
    fx, fy = fx[:, None], fy[:, None]
    top = image[cy(y0), cx(x0)] * (1.0 - fx) + image[cy(y0), cx(x0 + 1)] * fx
    bot = image[cy(y0 + 1), cx(x0)] * (1.0 - fx) + image[cy(y0 + 1), cx(x0 + 1)] * fx
    return top * (1.0 - fy) + bot * fy
