"""A float64 restatement of surface_patch_warp as the fused kernels document it (gens_patch_warp_fwd / _bwd, k19_step.hip; projector.py:46-91 is
the operator-by-operator mirror), of the K9 read (gens_patch_sample_fwd / _bwd, k9_misc.hip) and of the warp features' up-sampling
(gens_upsample2d_into / _cat), each with a running error bound, for the patch warp tests.  CPU only: numpy and torch, no GPU.  The running-bound
rules and the tap helpers are those of tests/feature_lookup_reference.py (imported, not copied).

    inputs      the evaluation's own float32 values: rays_o, rays_d (B, 3), z (B), g0 (B, 3), c2ws, intrs (nv, 4, 4), the maps (nv, C, h, w)
                and kinv_ref (3, 3) AS THE EVALUATION HOLDS IT (SceneCams.kinv_ref copied back for the kernels, torch.inverse(intrs)[0] for the
                float32 oracle): it counts as exact input.
    reference   p = o + d z; n = normalise(g0) R_ref (a zero g0: divided by 1e-8, so n = 0 and H_v = K_v R_v^T R_ref K_ref^-1); x_cam, disp,
                (u0, v0), H_v; per patch pixel (row-major: y outer, x inner, offsets -half .. half) q = H_v (u0 + ox, v0 + oy, 1), its
                de-homogenisation, the normalise / un-normalise round trip and the zero-padded bilinear read.  The reference patch is read at
                (u0 + ox, v0 + oy) through the same round trip.  Every quantity carries a first-order running bound (u = 2^-24) that covers
                any float32 evaluation in any association order, with or without FMA (feature_lookup_reference's rules).  The constants
                + 1e-8 / + 1e-10 are float32's; where the other operand carries no error the sum is ONE float32 operation on exact inputs,
                whose IEEE result is determined: the reference takes that result and adds nothing, so on inputs built so that nothing rounds
                (`exact`) every coordinate bound is zero and `inside the bound` means `equal`.
    values      |value - reference| <= e_ix Lx + e_iy Ly + 8 u max|texel| on the zero-padded map, per view and channel.
    backward    g_z[ray] = sum over views, pixels, channels of g_sampled (dv/dix dgx/dz + dv/diy dgy/dz).  The tangents du0, dv0, ddisp, dH, dq,
                dgx, dgy follow the DAG the kernel evaluates (pw_ray, pw_homography<true>, patch_warp_bwd_k) under the same rules.  A sample
                adds |sx| e_dgx + |sy| e_dgy + |dgx| e_sx + |dgy| e_sy; e_sx = (C + 8) u sum|texel g weight| (a term is rounded in its
                product, at most C + 3 additions, a difference, the two roundings of its weight, the product with it and the accumulation)
                + |second mixed difference| e_iy + for a sample whose ix lies within its bound of an integer the largest difference between
                the slopes of the candidate cells.  A ray adds (k + 4) u sum|terms| for its k = S P samples (per-lane sums and wave_sum in any
                order; 4: the two products and their sum).  Every ray is held to its own bound.
    free        a sample whose coordinate bound is not finite or not below half a texel; a ray with a free sample is free in the backward.
    PINNED      a ray with a non-finite input (NaN / inf z, NaN g0) whose float64 coordinates are non-finite has nothing to blame on rounding:
                its values are exactly 0 and its samples add nothing to g_z (so g_z is exactly 0 for a non-finite z).  This is what the
                kernels do today (bilinear_taps' `fin`, the isfinite test of patch_warp_bwd_k).
    K9 direct   given coordinates are exact: values within 8 u max|texel|, d/d(xy) within (C + 8) u sum|texel g weight|; the cell is floor.
    up-sampling F.interpolate(mode="bilinear", align_corners=False) as upsample2d_into_k restates it: bound(sy) Ly + bound(sx) Lx + 8 u max.
    generators  make_case for SHAPES x CLASSES and make_exact_case, from seeded torch.Generators: smooth maps (low-frequency sinusoids plus
                2 % noise), source views with their own intrinsics, ray origins off the reference centre (so du0, dv0 are not zero).
                texels(): the (nv, h, w, C_pad) tensor with a NaN sentinel in the pad channels.
    patch_warp_f32 / patch_warp_bwd_f32   the kernel's order of operations in numpy float32 with the seeded defects of DEFECTS / BWD_DEFECTS.
"""
import functools

import numpy as np
import torch

from tests import feature_lookup_reference as F
from tests.feature_lookup_reference import AMBIGUOUS_CAP, U, _div, _fma32, _gather, _is_f32, _mul, _near, _np, _read64, _rnd, _slopes, _sum, _taps  # noqa: F401

f32 = np.float32
E8, E10 = float(f32(1e-8)), float(f32(1e-10))
# measured on the CPU (test_patch_warp_reference_cpu.py -s): the float32 oracle's reverse-mode g_z uses at most REVERSE_MODE_MEASURED of the
# forward-mode bound over every shape of `inside` and `border`; rounded up to the next power of two
REVERSE_MODE_MEASURED = 0.012
REVERSE_MODE_FACTOR = 2.0 ** -6
BWD_FREE_CAP = 0.05

# (views, (h, w), channels, patch, rays): see tests/test_hip_patch_warp.py for what each exercises
SHAPES = ((2, (2, 2), 1, 1, 1), (3, (5, 7), 3, 3, 4), (3, (5, 7), 5, 3, 5), (5, (33, 65), 12, 11, 70), (11, (24, 32), 12, 11, 33),
          (16, (9, 12), 16, 15, 9))
SHAPE_IDS = tuple(f"v{nv}-{h}x{w}-c{c}-p{p}-b{b}" for nv, (h, w), c, p, b in SHAPES)
CLASSES = ("inside", "border", "outside", "behind", "grazing", "zero_normal", "nonfinite")
BWD_CLASSES = ("inside", "border", "zero_normal", "nonfinite")
DEFECTS = ("rows_cols_swapped", "offsets_from_zero", "tex_view_off_by_one", "intr_view_off_by_one", "rel_transposed", "normal_not_rotated",
           "normal_not_normalised", "align_corners_false", "border_clamp", "ref_through_homography")
BWD_DEFECTS = ("no_h_du0", "no_dh", "dh_sign", "slopes_swapped", "quotient_without_dq2", "border_slope_kept")
ALL_CASES = tuple((i, c) for i in range(len(SHAPES)) for c in CLASSES) + ((None, "exact"),)
K9_POINTS, K9_CHANNELS = (0, 1, 255, 256, 257), (1, 3, 5, 12, 16)
K9_CLASSES = ("inside", "border", "outside", "nonfinite", "on_grid")
UP_SIZES = (((1, 1), (2, 2)), ((3, 5), (7, 9)), ((5, 7), (5, 7)), ((12, 16), (48, 64)), ((24, 32), (48, 64)))
UP_CHANNELS = (1, 4, 5)


def case_id(shape, cls):
    return "exact" if cls == "exact" else f"{SHAPE_IDS[shape]}-{cls}"


# ------------------------------------------------------------------------------------------------------------------ pairs (value, bound)
def ex(x):
    x = np.asarray(x, np.float64)
    return x, np.zeros_like(x)


def mul(a, b):
    return _mul(a[0], a[1], b[0], b[1])


def add(*ts):
    return _sum([t[0] for t in ts], [t[1] for t in ts])


def neg(a):
    return -a[0], a[1]


def div(a, b):
    return _div(a[0], a[1], b[0], b[1])


def addc(a, c):
    """a + c for a float32 constant c.  Exact a: one IEEE operation, its float32 result and no error (see the docstring)."""
    r = a[0] + c
    exact = a[1] == 0
    return np.where(exact, r.astype(f32).astype(np.float64), r), np.where(exact, 0.0, a[1] + U * np.abs(r))


def sub1(a, c):
    r = a[0] + c
    return r, _rnd(r, a[1])


def root(a):
    r = np.sqrt(a[0])
    return r, _rnd(r, np.where(a[0] > 0, a[1] / (2 * np.where(a[0] > 0, r, 1.0)), np.sqrt(a[1])))


def at(a, idx):
    return a[0][idx], a[1][idx]


def dot(xs, ys):
    return add(*[mul(x, y) for x, y in zip(xs, ys)])


def _round_trip(g, m):
    """((2 g / m - 1) + 1) / 2 * m as the evaluation forms it."""
    b = div((2.0 * g[0], 2.0 * g[1]), ex(np.full_like(g[0], m)))
    c = sub1(sub1(b, -1.0), 1.0)
    return mul((c[0] / 2.0, c[1] / 2.0), ex(np.full_like(g[0], m)))


# ------------------------------------------------------------------------------------------------------------------ the chain
def _chain(o, d, z, g0, c2ws, intrs, kinv, h, w, patch, normals=None):
    """-> dict of pairs: coordinates (S, B, P) of the source reads and (1, B, P) of the reference read, with the tangents of the former."""
    s = c2ws.shape[0] - 1
    cr, k0 = c2ws[0], intrs[0]
    zz = ex(z)
    dd = [ex(d[:, j]) for j in range(3)]
    p = [add(ex(o[:, j]), mul(dd[j], zz)) for j in range(3)]
    g = [ex(g0[:, j]) for j in range(3)]
    gn = root(add(*[mul(a, a) for a in g]))
    floor = ~(gn[0] > 0) & ~np.isnan(gn[0])
    gn = np.where(floor, E8, gn[0]), np.where(floor, 0.0, gn[1])
    g = [div(a, gn) for a in g]
    e = lambda i, j: ex(cr[i, j])  # noqa: E731
    nrm = [add(*[mul(g[i], e(i, j)) for i in range(3)]) for j in range(3)]
    if normals is not None:
        nrm = [ex(normals[:, j]) for j in range(3)]
    t = [neg(add(*[mul(e(i, j), e(i, 3)) for i in range(3)])) for j in range(3)]
    xc = [add(*([mul(p[i], e(i, j)) for i in range(3)] + [t[j]])) for j in range(3)]
    dx = [add(*[mul(dd[i], e(i, j)) for i in range(3)]) for j in range(3)]
    pr = [add(*[mul(xc[j], ex(k0[i, j])) for j in range(3)]) for i in range(3)]
    dp = [add(*[mul(dx[j], ex(k0[i, j])) for j in range(3)]) for i in range(3)]
    disp, ddisp = dot(nrm, xc), dot(nrm, dx)
    den = addc(pr[2], E8)
    den2 = mul(den, den)
    u0, v0 = div(pr[0], den), div(pr[1], den)
    du0 = div(add(mul(dp[0], den), neg(mul(pr[0], dp[2]))), den2)
    dv0 = div(add(mul(dp[1], den), neg(mul(pr[1], dp[2]))), den2)
    # homographies: view constants (S, 1), ray quantities (1, B)
    cs = c2ws[1:]
    col = lambda a: ex(np.asarray(a, np.float64)[:, None])  # noqa: E731
    row = lambda a: (a[0][None], a[1][None])  # noqa: E731
    rel = [[add(*[mul(col(cs[:, k, i]), e(k, j)) for k in range(3)]) for j in range(3)] for i in range(3)]
    diff = []
    for k in range(3):
        r = cr[k, 3] - cs[:, k, 3]
        diff.append((r[:, None], _rnd(r, np.zeros_like(r))[:, None]))
    tv = [add(*[mul(col(cs[:, k, i]), diff[k]) for k in range(3)]) for i in range(3)]
    hden = row(addc(disp, E10))
    hden2 = mul(hden, hden)
    outer = [[mul(tv[i], row(nrm[j])) for j in range(3)] for i in range(3)]
    hom = [[add(rel[i][j], div(outer[i][j], hden)) for j in range(3)] for i in range(3)]
    dhom = [[div(neg(mul(outer[i][j], row(ddisp))), hden2) for j in range(3)] for i in range(3)]
    ks = intrs[1:]
    kk = lambda i, j: col(ks[:, i, j])  # noqa: E731
    tmp = [[add(*[mul(kk(i, m), hom[m][j]) for m in range(3)]) for j in range(3)] for i in range(3)]
    dtmp = [[add(*[mul(kk(i, m), dhom[m][j]) for m in range(3)]) for j in range(3)] for i in range(3)]
    hh = [[add(*[mul(tmp[i][m], ex(kinv[m, j])) for m in range(3)]) for j in range(3)] for i in range(3)]
    dh = [[add(*[mul(dtmp[i][m], ex(kinv[m, j])) for m in range(3)]) for j in range(3)] for i in range(3)]
    # samples (S, B, P)
    half = patch // 2
    px = np.arange(patch * patch)
    ox, oy = (px % patch - half).astype(np.float64), (px // patch - half).astype(np.float64)
    ray = lambda a: (a[0][None, :, None], a[1][None, :, None])  # noqa: E731
    smp = lambda a: (a[0][:, :, None], a[1][:, :, None])  # noqa: E731
    u, v = add(ray(u0), ex(ox[None, None])), add(ray(v0), ex(oy[None, None]))
    q = [add(mul(smp(hh[i][0]), u), mul(smp(hh[i][1]), v), smp(hh[i][2])) for i in range(3)]
    dq = [add(mul(smp(dh[i][0]), u), mul(smp(dh[i][1]), v), smp(dh[i][2]), mul(smp(hh[i][0]), ray(du0)), mul(smp(hh[i][1]), ray(dv0)))
          for i in range(3)]
    qden = addc(q[2], E8)
    qden2 = mul(qden, qden)
    gx, gy = div(q[0], qden), div(q[1], qden)
    dgx = div(add(mul(dq[0], qden), neg(mul(q[0], dq[2]))), qden2)
    dgy = div(add(mul(dq[1], qden), neg(mul(q[1], dq[2]))), qden2)
    return dict(ix=_round_trip(gx, w - 1.0), iy=_round_trip(gy, h - 1.0), dgx=dgx, dgy=dgy, rix=_round_trip(u, w - 1.0), riy=_round_trip(v, h - 1.0),
                q2=q[2][0], disp=disp[0], u0=u0[0], v0=v0[0], s=s)


def _values(m, views, ix, iy, bad_ray):
    """m (nv, C, h, w); views: the map of each row of ix; ix, iy pairs (V, B, P).  -> val, bound (V, B, P, C), dead, free (V, B, P)."""
    vv, b, p = ix[0].shape
    sv = np.broadcast_to(np.asarray(views)[:, None], (vv, b * p))
    fl = lambda a: a.reshape(vv, b * p)  # noqa: E731
    fin = np.isfinite(ix[0]) & np.isfinite(iy[0])
    dead = bad_ray[None, :, None] & ~fin
    free = ~dead & (~(ix[1] < 0.5) | ~(iy[1] < 0.5))
    val = _read64(m, sv, fl(np.where(dead, np.nan, ix[0])), fl(np.where(dead, np.nan, iy[0]))).reshape(vv, b, p, -1)
    lx, ly, top = _slopes(m)
    sel = np.asarray(views)
    bnd = ix[1][..., None] * lx[sel][:, None, None] + iy[1][..., None] * ly[sel][:, None, None] + 8 * U * top[sel][:, None, None]
    bnd = np.where(dead[..., None], 0.0, np.where(free[..., None], np.inf, bnd))
    return np.where(dead[..., None], 0.0, val), bnd, dead, free


def reference(o, d, z, g0, c2ws, intrs, kinv, maps, patch, normals=None):
    """-> dict, float64: ref, ref_bound (1, B, P, C); sampled, bound (S, B, P, C); dead, free (S, B, P) and ref_dead, ref_free (1, B, P);
    ix, iy, e_ix, e_iy (S, B, P), rix, riy (1, B, P); dgx, dgy, e_dgx, e_dgy; q2 (S, B, P), disp (B); bad_ray (B).
    normals (B, 3): the reference-camera normal given as input (projector.surface_patch_warp's calling convention) in place of g0's."""
    o, d, z, g0, c2ws, intrs, kinv, maps = (_np(t) for t in (o, d, z, g0, c2ws, intrs, kinv, maps))
    h, w = maps.shape[2:]
    with np.errstate(all="ignore"):
        ch = _chain(o, d, z, g0, c2ws, intrs, kinv, h, w, patch, None if normals is None else _np(normals))
        bad_ray = ~(np.isfinite(z) & np.isfinite(g0).all(-1) & np.isfinite(o).all(-1) & np.isfinite(d).all(-1))
        sampled, bound, dead, free = _values(maps, np.arange(1, ch["s"] + 1), ch["ix"], ch["iy"], bad_ray)
        ref, ref_bound, ref_dead, ref_free = _values(maps, np.array([0]), ch["rix"], ch["riy"], bad_ray)
    return dict(ref=ref, ref_bound=ref_bound, sampled=sampled, bound=bound, dead=dead, free=free, ref_dead=ref_dead, ref_free=ref_free,
                ix=ch["ix"][0], iy=ch["iy"][0], e_ix=ch["ix"][1], e_iy=ch["iy"][1], rix=ch["rix"][0], riy=ch["riy"][0], dgx=ch["dgx"][0],
                dgy=ch["dgy"][0], e_dgx=ch["dgx"][1], e_dgy=ch["dgy"][1], q2=ch["q2"], disp=ch["disp"], bad_ray=bad_ray, u0=ch["u0"], v0=ch["v0"])


# ------------------------------------------------------------------------------------------------------------------ slopes of the read
def _multiples(terms, sa):
    """Every term a multiple of 2^-23 of the next power of two above sa (the sum of their magnitudes): any partial sum is a float32 number."""
    quantum = 2.0 ** (np.ceil(np.log2(np.where((sa > 0) & np.isfinite(sa), sa, 1.0))) - 23)
    ok = np.ones(sa.shape, bool)
    for t in terms:
        r = t / quantum[..., None]
        ok &= (r == np.rint(r)).all(-1)
    return ok


def _cell_slopes(m, sv, ix, iy, x0, y0, cot):
    """The slopes of the zero-padded bilinear read in cell (x0, y0), contracted with cot.  m (nv, C, h, w); sv, ix, iy, x0, y0 (V, N); cot
    (V, N, C).  -> sx, sy, mixed, ax, ay (the sums of |texel cot weight| behind sx and sy), exact (nothing rounds in either)."""
    h, w = m.shape[2:]
    tap, mag, raw = [], [], []
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        xx, yy = (x0 + dx).astype(np.int64), (y0 + dy).astype(np.int64)
        ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        t = _gather(m, sv, yy, xx) * cot * ok[..., None]
        raw.append(t)
        tap.append(t.sum(-1))
        mag.append(np.abs(t).sum(-1))
    wx1, wx0, wy1, wy0 = ix - x0, (x0 + 1.0) - ix, iy - y0, (y0 + 1.0) - iy
    sx = (tap[1] - tap[0]) * wy0 + (tap[3] - tap[2]) * wy1
    sy = (tap[2] - tap[0]) * wx0 + (tap[3] - tap[1]) * wx1
    ax = (mag[0] + mag[1]) * np.abs(wy0) + (mag[2] + mag[3]) * np.abs(wy1)
    ay = (mag[0] + mag[2]) * np.abs(wx0) + (mag[1] + mag[3]) * np.abs(wx1)
    wts = _is_f32(wx1) & _is_f32(wx0) & _is_f32(wy1) & _is_f32(wy0)
    exact = wts & _multiples([raw[0] * wy0[..., None], raw[1] * wy0[..., None], raw[2] * wy1[..., None], raw[3] * wy1[..., None]], ax)
    exact &= _multiples([raw[0] * wx0[..., None], raw[2] * wx0[..., None], raw[1] * wx1[..., None], raw[3] * wx1[..., None]], ay)
    return sx, sy, (tap[3] - tap[2]) - (tap[1] - tap[0]), ax, ay, exact


def _read_slopes(m, sv, ix, iy, e_ix, e_iy, cot):
    """-> sx, sy and their bounds e_sx, e_sy (see the docstring) for reads at (ix, iy) with coordinate bounds (e_ix, e_iy); all (V, N)."""
    h, w = m.shape[2:]
    c = m.shape[1]
    x0, y0, _, _ = _taps(ix, iy, h, w)
    x0, y0 = x0.astype(np.float64), y0.astype(np.float64)
    sx, sy, mixed, ax, ay, exact = _cell_slopes(m, sv, ix, iy, x0, y0, cot)
    kx, ky = np.rint(ix), np.rint(iy)
    alt_x = np.where(_near(ix, kx, e_ix), np.where(x0 == kx, -1.0, 1.0), 0.0)
    alt_y = np.where(_near(iy, ky, e_iy), np.where(y0 == ky, -1.0, 1.0), 0.0)
    jump_x, jump_y = np.zeros_like(sx), np.zeros_like(sy)
    for a, b in ((1, 0), (0, 1), (1, 1)):
        tx, ty, tm, _, _, _ = _cell_slopes(m, sv, ix, iy, x0 + a * alt_x, y0 + b * alt_y, cot)
        jump_x, jump_y = np.maximum(jump_x, np.abs(tx - sx)), np.maximum(jump_y, np.abs(ty - sy))
        mixed = np.maximum(np.abs(mixed), np.abs(tm))
    rounds = ~(exact & (e_ix == 0) & (e_iy == 0))
    e_sx = rounds * (c + 8) * U * ax + np.abs(mixed) * e_iy + jump_x
    e_sy = rounds * (c + 8) * U * ay + np.abs(mixed) * e_ix + jump_y
    return sx, sy, e_sx, e_sy


def backward_reference(ref, maps, cot):
    """g_z (B) of sum(sampled * cot) in float64 and its bound (inf: the ray is free).  cot (S, B, P, C)."""
    maps, cot = _np(maps), _np(cot)
    s, b, p, c = cot.shape
    sv = np.broadcast_to(np.arange(1, s + 1)[:, None], (s, b * p))
    fl = lambda a: a.reshape(s, b * p)  # noqa: E731
    with np.errstate(all="ignore"):
        dead, free = fl(ref["dead"]), fl(ref["free"])
        ix, iy = np.where(dead, np.nan, fl(ref["ix"])), np.where(dead, np.nan, fl(ref["iy"]))
        e_ix, e_iy = np.where(dead | free, 0.0, fl(ref["e_ix"])), np.where(dead | free, 0.0, fl(ref["e_iy"]))
        sx, sy, e_sx, e_sy = _read_slopes(maps, sv, np.where(dead, 0.0, ix), np.where(dead, 0.0, iy), e_ix, e_iy, cot.reshape(s, b * p, c))
        dgx, dgy = fl(ref["dgx"]), fl(ref["dgy"])
        tx, ty = np.where(dead, 0.0, sx * dgx), np.where(dead, 0.0, sy * dgy)
        e = np.abs(sx) * fl(ref["e_dgx"]) + np.abs(sy) * fl(ref["e_dgy"]) + np.abs(dgx) * e_sx + np.abs(dgy) * e_sy
        e = np.where(dead, 0.0, e)
        per_ray = lambda a: a.reshape(s, b, p).transpose(1, 0, 2).reshape(b, s * p)  # noqa: E731
        tx, ty, e, free = per_ray(tx), per_ray(ty), per_ray(e), per_ray(free)
        g_z, sa, e_in = (tx + ty).sum(-1), (np.abs(tx) + np.abs(ty)).sum(-1), e.sum(-1)
        exact = (e_in == 0) & _multiples([tx, ty], sa) & _is_f32(tx).all(-1) & _is_f32(ty).all(-1)
        bound = np.where(exact, 0.0, e_in + (s * p + 4) * U * sa)
        bound = np.where(free.any(-1) | ~np.isfinite(bound) | ~np.isfinite(g_z), np.inf, bound)
    return g_z, bound


# ------------------------------------------------------------------------------------------------------------------ K9 direct, up-sampling
def k9_reference(m, xy, cot):
    """m (C, h, w), xy (N, 2) given (exact) coordinates, cot (N, C).  -> val, val_bound (N, C); g_xy, g_bound (N, 2)."""
    m, xy, cot = _np(m)[None], _np(xy), _np(cot)
    n, c = xy.shape[0], m.shape[1]
    sv = np.zeros((1, n), np.int64)
    with np.errstate(all="ignore"):
        ix, iy = xy[None, :, 0], xy[None, :, 1]
        fin = np.isfinite(ix) & np.isfinite(iy)
        val = np.where(fin[..., None], _read64(m, sv, ix, iy), 0.0)[0]
        top = _slopes(m)[2][0]
        h, w = m.shape[2:]
        x0, y0, _, _ = _taps(ix, iy, h, w)
        val_bound = np.where(fin[0][:, None], 8 * U * top[None], 0.0) + np.zeros_like(val)
        sx, sy, _, ax, ay, exact = _cell_slopes(m, sv, np.where(fin, ix, 0.0), np.where(fin, iy, 0.0), x0.astype(np.float64), y0.astype(np.float64),
                                                cot[None])
        g = np.where(fin[0][:, None], np.stack([sx[0], sy[0]], -1), 0.0)
        g_bound = np.where(fin[0][:, None], ~exact[0][:, None] * (c + 8) * U * np.stack([ax[0], ay[0]], -1), 0.0)
    return val, val_bound, g, g_bound


def _source_position(n_out, n_in):
    """max((i + 0.5) (n_in / n_out) - 0.5, 0) for i < n_out with its bound."""
    i = np.arange(n_out, dtype=np.float64)
    ratio = div(ex(np.full(n_out, float(n_in))), ex(np.full(n_out, float(n_out))))
    s = sub1(mul(ex(i + 0.5), ratio), -0.5)
    return np.maximum(s[0], 0.0), s[1]


def upsample_reference(src, h, w):
    """src (n, C, hs, ws) -> (n, C, h, w) float64 and its bound."""
    src = _np(src)
    hs, ws = src.shape[2:]
    with np.errstate(all="ignore"):
        sy, e_sy = _source_position(h, hs)
        sx, e_sx = _source_position(w, ws)
        y0, x0 = np.minimum(np.floor(sy).astype(np.int64), hs - 1), np.minimum(np.floor(sx).astype(np.int64), ws - 1)
        y1, x1 = np.minimum(y0 + 1, hs - 1), np.minimum(x0 + 1, ws - 1)
        ty, tx = (sy - y0)[:, None], (sx - x0)[None, :]
        top = src[:, :, y0][:, :, :, x0] * (1 - tx) + src[:, :, y0][:, :, :, x1] * tx
        bot = src[:, :, y1][:, :, :, x0] * (1 - tx) + src[:, :, y1][:, :, :, x1] * tx
        val = top * (1 - ty) + bot * ty
        ly = np.abs(np.diff(src, axis=2)).max((2, 3), initial=0.0)[..., None, None]
        lx = np.abs(np.diff(src, axis=3)).max((2, 3), initial=0.0)[..., None, None]
        rounds = ~(_is_f32(1 - tx) & _is_f32(1 - ty) & (e_sy[:, None] == 0) & (e_sx[None, :] == 0) & ((tx == 0) | (tx == 1)) & ((ty == 0) | (ty == 1)))
        bound = e_sy[:, None] * ly + e_sx[None, :] * lx + rounds * 8 * U * np.abs(src).max((2, 3))[..., None, None]
    return val, bound


# ------------------------------------------------------------------------------------------------------------------ checks
def use(got, want, bound):
    return F._use(got, want, bound)


def check_forward(ref, got_ref, got_sampled):
    """-> dict(use_ref, use_sampled: worst share of the bound used; finite: free samples are finite; zeros: the pinned zeros are zeros;
    n_free, n_samples)."""
    got_ref, got_sampled = _np(got_ref), _np(got_sampled)
    out = dict(use_ref=float(use(got_ref, ref["ref"], ref["ref_bound"]).max(initial=0.0)),
               use_sampled=float(use(got_sampled, ref["sampled"], ref["bound"]).max(initial=0.0)))
    out["finite"] = bool(np.isfinite(got_sampled[ref["free"]]).all() and np.isfinite(got_ref[ref["ref_free"]]).all())
    out["zeros"] = bool((got_sampled[ref["dead"]] == 0).all() and (got_ref[ref["ref_dead"]] == 0).all())
    out["n_free"], out["n_samples"] = int(ref["free"].sum() + ref["ref_free"].sum()), ref["free"].size + ref["ref_free"].size
    return out


def forward_ok(res):
    return res["use_ref"] <= 1 and res["use_sampled"] <= 1 and res["finite"] and res["zeros"]


def check_backward(g_z, bound, got, factor=1.0):
    return float(use(got, g_z, bound * factor).max(initial=0.0))


# ------------------------------------------------------------------------------------------------------------------ inputs
def kinv_of(intrs):
    """inverse(intrs)[0, :3, :3] as gens_scene_setup forms it: solved in float64, rounded once."""
    return torch.from_numpy(np.linalg.inv(_np(intrs)[0])[:3, :3].astype(f32))


def smooth_maps(nv, c, h, w, g):
    """A few low-frequency sinusoids per channel plus 2 % noise: small texel slopes and small slope jumps between cells."""
    yy, xx = np.meshgrid(np.arange(h) / max(h, 8), np.arange(w) / max(w, 8), indexing="ij")
    r = torch.rand(nv, c, 3, 4, generator=g, dtype=torch.float64).numpy()
    m = np.zeros((nv, c, h, w))
    for k in range(3):
        fx, fy, ph, am = (r[:, :, k, j][..., None, None] for j in range(4))
        m += (0.3 + 0.4 * am) * np.sin(2 * np.pi * ((0.5 + 1.5 * fx) * xx + (0.5 + 1.5 * fy) * yy + ph))
    m += 0.02 * torch.randn(nv, c, h, w, generator=g, dtype=torch.float64).numpy()
    return torch.from_numpy(m).float()


def texels(maps, pad=float("nan")):
    """(nv, C, h, w) -> (nv, h, w, C_pad) with the pad channels set to a sentinel no output may depend on."""
    nv, c, h, w = maps.shape
    t = torch.full((nv, h, w, 4 * ((c + 3) // 4)), pad, dtype=torch.float32)
    t[..., :c] = maps.permute(0, 2, 3, 1)
    return t.contiguous()


def _perp(wv, g):
    a = torch.randn(wv.shape[0], 3, generator=g, dtype=torch.float64).numpy()
    a -= (a * wv).sum(-1, keepdims=True) * wv
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def make_scene(nv, h, w, patch, g):
    """Cameras on an arc of radius ~2.2 that spans at most 40 degrees, all looking near the origin, each with its own intrinsics.  A patch wider
    than the image keeps a modest angle of view (the focal lengths grow with patch / image size), so that no homography's horizon crosses it."""
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64).numpy()  # noqa: E731
    step, zoom = min(7.0, 40.0 / (nv - 1)), max(1.0, 3.0 * patch / min(h, w))
    c2ws, intrs = [], []
    for k in range(nv):
        az = np.radians((k - (nv - 1) / 2) * step + 0.5 * step * (rnd(1)[0] - 0.5))
        el = np.radians(20.0 * (rnd(1)[0] - 0.5))
        r = 2.2 * (1 + 0.1 * (rnd(1)[0] - 0.5))
        centre = r * np.array([np.sin(az) * np.cos(el), np.sin(el), -np.cos(az) * np.cos(el)])
        c2ws.append(F._look_at(centre, 0.2 * (rnd(3) - 0.5), np.array([0.05 * (rnd(1)[0] - 0.5), 1.0, 0.0])))
        intr = np.eye(4)
        intr[0, 0], intr[1, 1] = zoom * 1.8 * w * (1 + 0.1 * (rnd(1)[0] - 0.5)), zoom * 2.4 * h * (1 + 0.1 * (rnd(1)[0] - 0.5))
        intr[0, 2], intr[1, 2] = w * (0.5 + 0.06 * (rnd(1)[0] - 0.5)), h * (0.5 + 0.06 * (rnd(1)[0] - 0.5))
        intrs.append(intr)
    return np.stack(c2ws).astype(f32).astype(np.float64), np.stack(intrs).astype(f32).astype(np.float64)


def make_case(shape, cls, seed=None):
    nv, (h, w), c, patch, b = SHAPES[shape]
    assert cls in CLASSES
    seed = 7000 + 100 * shape + CLASSES.index(cls) if seed is None else seed
    g = torch.Generator().manual_seed(seed + 50)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64).numpy()  # noqa: E731
    c2ws, intrs = make_scene(nv, h, w, patch, g)
    if cls == "behind":                                     # view 1 moves in front of the surface points: they lie behind it
        c2ws[1, :3, 3] *= 0.3
    if cls == "outside":                                    # the source views' principal points lie 3 to 60 image sizes beside their images
        intrs[1:, 0, 2] += np.where(rnd(nv - 1) < 0.5, -1, 1) * (w + patch) * np.floor(3 + 57 * rnd(nv - 1) ** 3)
        intrs = intrs.astype(f32).astype(np.float64)
    half = max(patch // 2, 1)
    if cls == "border":                                     # within half a patch of an edge, on either side of it
        edge, t, off = np.arange(b) % 4, rnd(b), half * (2 * rnd(b) - 1)
        px = np.where(edge == 0, off, np.where(edge == 1, w - 1 + off, (w - 1) * t))
        py = np.where(edge == 2, off, np.where(edge == 3, h - 1 + off, (h - 1) * t))
    else:
        px, py = (w - 1) * rnd(b), (h - 1) * rnd(b)
    depth = 0.4 + 0.6 * rnd(b) if cls == "behind" else 1.6 + 1.2 * rnd(b)
    k, cw = intrs[0], c2ws[0]
    cam = np.stack([(px - k[0, 2]) * depth / k[0, 0], (py - k[1, 2]) * depth / k[1, 1], depth], -1)
    p = cam @ cw[:3, :3].T + cw[:3, 3]
    o = cw[:3, 3] + 0.15 * (2 * rnd(b, 3) - 1)               # off the reference centre: du0, dv0 are not zero
    z = np.linalg.norm(p - o, axis=-1)
    d = (p - o) / z[:, None]
    wv = (p - cw[:3, 3]) / np.linalg.norm(p - cw[:3, 3], axis=-1, keepdims=True)
    if cls == "grazing":                                    # |disp| from 1e-3 to 0.1 of the depth
        cosine = np.where(rnd(b) < 0.5, -1, 1) * 10.0 ** (-3 + 2 * rnd(b))
    else:                                                   # within 60 degrees of the viewing ray, facing the camera
        cosine = np.cos(np.radians(60 * rnd(b)))
    n = -cosine[:, None] * wv + np.sqrt(1 - cosine[:, None] ** 2) * _perp(wv, g)
    g0 = torch.from_numpy(n * (0.5 + 1.5 * rnd(b, 1))).float()
    z = torch.from_numpy(z).float()
    if cls == "zero_normal":                                # exact zeros, and normals so short that the 1e-10 beside disp weighs a tenth of it
        g0[1::4] *= 1e-9
        g0[::2] = 0.0
    if cls == "nonfinite":
        if b >= 5:
            z[1], z[2], z[3], g0[4, 1] = float("nan"), float("inf"), -float("inf"), float("nan")
        elif b == 4:
            z[1], z[2], g0[3, 0] = float("nan"), float("inf"), float("nan")
        else:
            z[0] = float("nan")
    maps = smooth_maps(nv, c, h, w, g)
    intrs_t = torch.from_numpy(intrs).float()
    return dict(o=torch.from_numpy(o).float(), d=torch.from_numpy(d).float(), z=z, g0=g0, c2ws=torch.from_numpy(c2ws).float(), intrs=intrs_t,
                kinv=kinv_of(intrs_t), maps=maps, patch=patch, cot=torch.randn(nv - 1, b, patch * patch, c, generator=g), cls=cls, shape=shape)


EXACT_PIXELS = ((0, 0), (64, 32), (1, 31), (32, 16), (63, 1), (2, 2), (62, 30), (33, 0))


def make_exact_case():
    """Nothing rounds: identity rotations, f = 32, 33 x 65 maps (w - 1 = 64, h - 1 = 32), g0 = (0, 0, 4), depths 1, 2, 4, ray origins at the
    reference centre or 1/8 beside it (u0 moves by 4 / depth: du0 = -4 / depth^2), texels multiples of 1/8, cotangents of 1/2.  H_v is a pure
    shift: view 1 by 1/4 px per unit of inverse depth (quarter and eighth positions), view 2 by a whole pixel through its principal point
    (samples ON texel boundaries, at -1, 0, w - 1 and w), view 3 by half a row and 40 columns (beyond).  5 channels, patch 5."""
    g = torch.Generator().manual_seed(78)
    c2ws = np.stack([np.eye(4)] * 4)
    c2ws[1, :3, 3], c2ws[2, :3, 3], c2ws[3, :3, 3] = (-1 / 128, 0, 0), (0, 0, 0), (0, -1 / 64, 0)
    intrs = np.stack([np.eye(4)] * 4)
    intrs[:, 0, 0] = intrs[:, 1, 1] = 32.0
    intrs[:, 0, 2], intrs[:, 1, 2] = 32.0, 16.0
    intrs[2, 0, 2], intrs[3, 0, 2] = 31.0, 72.0
    o, d, z = [], [], []
    for i, (px, py) in enumerate(EXACT_PIXELS * 3):
        depth = (1.0, 2.0, 4.0)[(i // len(EXACT_PIXELS))]
        off = 0.125 if i % 2 else 0.0
        o.append([off, 0.0, 0.0])
        d.append([(px - 32.0) / 32.0 - off / depth, (py - 16.0) / 32.0, 1.0])
        z.append(depth)
    dy = lambda *s, q, top: (torch.randint(-top, top + 1, s, generator=g).float() / q)  # noqa: E731
    b = len(z)
    intrs_t = torch.from_numpy(intrs).float()
    return dict(o=torch.tensor(o), d=torch.tensor(d), z=torch.tensor(z), g0=torch.tensor([[0.0, 0.0, 4.0]] * b), c2ws=torch.from_numpy(c2ws).float(),
                intrs=intrs_t, kinv=kinv_of(intrs_t), maps=dy(4, 5, 33, 65, q=8, top=16), patch=5, cot=dy(3, b, 25, 5, q=2, top=2), cls="exact",
                shape=None)


def case_reference(case, kinv=None):
    ref = reference(case["o"], case["d"], case["z"], case["g0"], case["c2ws"], case["intrs"], case["kinv"] if kinv is None else kinv, case["maps"],
                    case["patch"])
    ref["g_z"], ref["g_bound"] = backward_reference(ref, case["maps"], case["cot"])
    return ref


@functools.lru_cache(maxsize=None)
def shape_case(shape, cls):
    """The case the CPU and the GPU tests share (computed once, never modified) with its reference for the float64-solved kinv_ref."""
    case = make_exact_case() if cls == "exact" else make_case(shape, cls)
    return case, case_reference(case)


def reference_for(shape, cls, kinv):
    """shape_case's reference if kinv (the evaluation's own inverse) has its bits, a fresh one otherwise."""
    case, ref = shape_case(shape, cls)
    return (case, ref) if torch.equal(kinv.cpu().reshape(-1), case["kinv"].reshape(-1)) else (case, case_reference(case, kinv.cpu()))


@functools.lru_cache(maxsize=None)
def k9_case(n, c, cls):
    """-> (map (C, 9, 12), xy (n, 2), cot (n, C)) for gens_patch_sample_fwd / _bwd."""
    h, w = 9, 12
    g = torch.Generator().manual_seed(100 * n + c + 17 * K9_CLASSES.index(cls))
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64).numpy()  # noqa: E731
    if cls == "inside":
        x, y = (w - 1) * rnd(n), (h - 1) * rnd(n)
    elif cls == "border":
        edge, t, off = np.arange(n) % 4, rnd(n), 2 * rnd(n) - 1
        x = np.where(edge == 0, off, np.where(edge == 1, w - 1 + off, (w + 1) * t - 1))
        y = np.where(edge == 2, off, np.where(edge == 3, h - 1 + off, (h + 1) * t - 1))
    elif cls == "outside":
        x = np.where(rnd(n) < 0.5, -1 - 10.0 ** (8 * rnd(n)), w + 10.0 ** (8 * rnd(n)))
        y = np.where(rnd(n) < 0.5, -1 - 10.0 ** (8 * rnd(n)), h + 10.0 ** (8 * rnd(n)))
    elif cls == "nonfinite":
        x, y = (w - 1) * rnd(n), (h - 1) * rnd(n)
        x[::3], y[1::5] = np.nan, np.inf
        x[2::7] = -np.inf
    else:                                                   # on_grid: integers and quarters from -2 to w + 1
        x = np.floor((4 * (w + 3) + 1) * rnd(n)) / 4 - 2
        y = np.floor((4 * (h + 3) + 1) * rnd(n)) / 4 - 2
    m = smooth_maps(1, c, h, w, g)[0]
    cot = torch.randn(n, c, generator=g)
    if cls == "on_grid":
        m, cot = torch.round(m * 8) / 8, torch.round(cot * 2) / 2
    return m, torch.from_numpy(np.stack([x, y], -1)).float().reshape(n, 2), cot


@functools.lru_cache(maxsize=None)
def up_case(size, c):
    (hs, ws), (h, w) = UP_SIZES[size]
    g = torch.Generator().manual_seed(31 * size + c)
    return smooth_maps(2, c, hs, ws, g), h, w


# ------------------------------------------------------------------------------------------------------------------ float32 restatement
def _taps32(ix, iy, h, w, clamp):
    x0, y0, wts, ok = _taps(ix, iy, h, w)
    if clamp:
        fin = np.isfinite(ix) & np.isfinite(iy)
        ok = [fin] * 4
    return x0, y0, wts, ok


def _read32(m, sv, ix, iy, clamp=False):
    x0, y0, wts, ok = _taps32(ix, iy, m.shape[2], m.shape[3], clamp)
    acc = np.zeros(ix.shape + (m.shape[1],), f32)
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        val = _gather(m, sv, y0 + dy, x0 + dx)
        acc = _fma32(val, np.broadcast_to(np.where(ok[k], wts[k], f32(0))[..., None], val.shape), acc)
    return acc


def _chain32(o, d, z, g0, c2ws, intrs, kinv, h, w, patch, defect):
    """pw_ray, pw_homography<true> and the per-sample chain of patch_warp_bwd_k in float32.  -> ix, iy, dgx, dgy (S, B, P), rix, riy (1, B, P)."""
    one, two = f32(1), f32(2)
    cr, k0, s = c2ws[0], intrs[0], c2ws.shape[0] - 1
    p = [o[:, j] + d[:, j] * z for j in range(3)]
    g = [g0[:, j] for j in range(3)]
    gn = np.sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2])
    gn = np.where(gn <= 0, f32(1e-8), gn)
    if defect != "normal_not_normalised":
        g = [a / gn for a in g]
    nrm = list(g) if defect == "normal_not_rotated" else [g[0] * cr[0, j] + g[1] * cr[1, j] + g[2] * cr[2, j] for j in range(3)]
    t = [-(cr[0, j] * cr[0, 3] + cr[1, j] * cr[1, 3] + cr[2, j] * cr[2, 3]) for j in range(3)]
    xc = [(p[0] * cr[0, j] + p[1] * cr[1, j] + p[2] * cr[2, j]) + t[j] for j in range(3)]
    dx = [d[:, 0] * cr[0, j] + d[:, 1] * cr[1, j] + d[:, 2] * cr[2, j] for j in range(3)]
    pr = [xc[0] * k0[i, 0] + xc[1] * k0[i, 1] + xc[2] * k0[i, 2] for i in range(3)]
    dp = [dx[0] * k0[i, 0] + dx[1] * k0[i, 1] + dx[2] * k0[i, 2] for i in range(3)]
    disp = nrm[0] * xc[0] + nrm[1] * xc[1] + nrm[2] * xc[2]
    ddisp = nrm[0] * dx[0] + nrm[1] * dx[1] + nrm[2] * dx[2]
    den = pr[2] + f32(1e-8)
    u0, v0 = pr[0] / den, pr[1] / den
    du0, dv0 = (dp[0] * den - pr[0] * dp[2]) / (den * den), (dp[1] * den - pr[1] * dp[2]) / (den * den)
    cs = c2ws[1:]
    ks = intrs[:-1] if defect == "intr_view_off_by_one" else intrs[1:]
    col = lambda a: a[:, None]  # noqa: E731
    if defect == "rel_transposed":
        rel = [[col(cs[:, i, 0]) * cr[j, 0] + col(cs[:, i, 1]) * cr[j, 1] + col(cs[:, i, 2]) * cr[j, 2] for j in range(3)] for i in range(3)]
    else:
        rel = [[col(cs[:, 0, i]) * cr[0, j] + col(cs[:, 1, i]) * cr[1, j] + col(cs[:, 2, i]) * cr[2, j] for j in range(3)] for i in range(3)]
    tv = [col(cs[:, 0, i]) * col(cr[0, 3] - cs[:, 0, 3]) + col(cs[:, 1, i]) * col(cr[1, 3] - cs[:, 1, 3]) + col(cs[:, 2, i]) * col(cr[2, 3] - cs[:, 2, 3])
          for i in range(3)]
    hden = (disp + f32(1e-10))[None]
    sign = one if defect == "dh_sign" else -one
    hom, dhom = [[None] * 3 for _ in range(3)], [[None] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            outer = tv[i] * nrm[j][None]
            hom[i][j] = rel[i][j] + outer / hden
            dhom[i][j] = sign * outer * ddisp[None] / (hden * hden)
    kk = lambda i, j: col(ks[:, i, j])  # noqa: E731
    tmp = [[kk(i, 0) * hom[0][j] + kk(i, 1) * hom[1][j] + kk(i, 2) * hom[2][j] for j in range(3)] for i in range(3)]
    dtmp = [[kk(i, 0) * dhom[0][j] + kk(i, 1) * dhom[1][j] + kk(i, 2) * dhom[2][j] for j in range(3)] for i in range(3)]
    hh = [[(tmp[i][0] * kinv[0, j] + tmp[i][1] * kinv[1, j] + tmp[i][2] * kinv[2, j])[:, :, None] for j in range(3)] for i in range(3)]
    dh = [[(dtmp[i][0] * kinv[0, j] + dtmp[i][1] * kinv[1, j] + dtmp[i][2] * kinv[2, j])[:, :, None] for j in range(3)] for i in range(3)]
    half = 0 if defect == "offsets_from_zero" else patch // 2
    px = np.arange(patch * patch)
    ox, oy = (px % patch - half).astype(f32), (px // patch - half).astype(f32)
    if defect == "rows_cols_swapped":
        ox, oy = oy, ox
    u, v = u0[None, :, None] + ox[None, None], v0[None, :, None] + oy[None, None]
    du, dv = du0[None, :, None], dv0[None, :, None]
    q = [hh[i][0] * u + hh[i][1] * v + hh[i][2] for i in range(3)]
    dq = []
    for i in range(3):
        first = (dh[i][0] * u + dh[i][1] * v + dh[i][2]) if defect != "no_dh" else np.zeros_like(q[i])
        second = (hh[i][0] * du + hh[i][1] * dv) if defect != "no_h_du0" else np.zeros_like(q[i])
        dq.append(first + second)
    qden = q[2] + f32(1e-8)
    gx, gy = q[0] / qden, q[1] / qden
    if defect == "quotient_without_dq2":
        dgx, dgy = (dq[0] * qden) / (qden * qden), (dq[1] * qden) / (qden * qden)
    else:
        dgx, dgy = (dq[0] * qden - q[0] * dq[2]) / (qden * qden), (dq[1] * qden - q[1] * dq[2]) / (qden * qden)
    wm, hm = f32(w - 1), f32(h - 1)

    def trip(a, m, size):
        n = two * a / m - one
        if defect == "align_corners_false":
            return ((n + one) * f32(size) - one) / two
        return (n + one) / two * m
    ru, rv = u, v
    if defect == "ref_through_homography":
        ru, rv = gx[:1], gy[:1]
    return trip(gx, wm, w), trip(gy, hm, h), dgx, dgy, trip(ru, wm, w), trip(rv, hm, h)


def _f32_args(o, d, z, g0, c2ws, intrs, kinv, maps):
    return tuple(_np(t, f32) for t in (o, d, z, g0, c2ws, intrs, kinv, maps))


def patch_warp_f32(o, d, z, g0, c2ws, intrs, kinv, maps, patch, defect=None):
    """-> ref (1, B, P, C), sampled (S, B, P, C) float32 tensors.  defect: None or one of DEFECTS:
        rows_cols_swapped      the patch offsets transposed                     (px % patch for the row)
        offsets_from_zero      offsets 0 .. patch - 1                           (the - half forgotten)
        tex_view_off_by_one    source view v reads view v - 1's texels          (v counts from 1)
        intr_view_off_by_one   source view v uses view v - 1's intrinsics
        rel_transposed         R_v R_ref^T in place of R_v^T R_ref
        normal_not_rotated     normalise(g0) used as the reference-camera normal
        normal_not_normalised  g0 R_ref without the division                    (H_v keeps its value but for the 1e-10 beside disp)
        align_corners_false    the read un-normalises with ((n + 1) size - 1) / 2
        border_clamp           a tap outside the image keeps its weight          (the clamped loads without the ok flags)
        ref_through_homography the reference patch sent through view 1's homography"""
    assert defect is None or defect in DEFECTS
    o, d, z, g0, c2ws, intrs, kinv, maps = _f32_args(o, d, z, g0, c2ws, intrs, kinv, maps)
    s, b, (h, w) = c2ws.shape[0] - 1, z.shape[0], maps.shape[2:]
    with np.errstate(all="ignore"):
        ix, iy, _, _, rix, riy = _chain32(o, d, z, g0, c2ws, intrs, kinv, h, w, patch, defect)
        n = b * patch * patch
        first = 0 if defect == "tex_view_off_by_one" else 1
        sv = np.broadcast_to(np.arange(first, first + s)[:, None], (s, n))
        clamp = defect == "border_clamp"
        sampled = _read32(maps, sv, ix.reshape(s, n), iy.reshape(s, n), clamp).reshape(s, b, patch * patch, -1)
        ref = _read32(maps, np.zeros((1, n), np.int64), rix.reshape(1, n), riy.reshape(1, n), clamp).reshape(1, b, patch * patch, -1)
    return torch.from_numpy(np.ascontiguousarray(ref)), torch.from_numpy(np.ascontiguousarray(sampled))


def patch_warp_bwd_f32(o, d, z, g0, c2ws, intrs, kinv, maps, patch, cot, defect=None):
    """g_z (B) float32 as patch_warp_bwd_k forms it (lane sums, then the wave's butterfly).  defect: None or one of BWD_DEFECTS:
        no_h_du0              dq without H (du0, dv0)                 no_dh                  dq without dH (u, v, 1)
        dh_sign               dhom = + outer ddisp / den^2            slopes_swapped         term = sy dgx + sx dgy
        quotient_without_dq2  dgx = dq0 den / den^2                   border_slope_kept      an out-of-image tap keeps its (clamped) texel"""
    assert defect is None or defect in BWD_DEFECTS
    o, d, z, g0, c2ws, intrs, kinv, maps = _f32_args(o, d, z, g0, c2ws, intrs, kinv, maps)
    cot = _np(cot, f32)
    s, b, (h, w), c = c2ws.shape[0] - 1, z.shape[0], maps.shape[2:], maps.shape[1]
    pp = patch * patch
    with np.errstate(all="ignore"):
        ix, iy, dgx, dgy, _, _ = _chain32(o, d, z, g0, c2ws, intrs, kinv, h, w, patch, defect)
        n = b * pp
        fl = lambda a: a.reshape(s, n)  # noqa: E731
        ix, iy, dgx, dgy = fl(ix), fl(iy), fl(dgx), fl(dgy)
        sv = np.broadcast_to(np.arange(1, s + 1)[:, None], (s, n))
        x0, y0, _, ok = _taps32(ix, iy, h, w, defect == "border_slope_kept")
        fin = np.isfinite(ix) & np.isfinite(iy)
        fx, fy = x0.astype(f32), y0.astype(f32)
        wx1, wx0, wy1, wy0 = ix - fx, (fx + f32(1)) - ix, iy - fy, (fy + f32(1)) - iy
        g = cot.reshape(s, n, c)
        sx, sy = np.zeros((s, n), f32), np.zeros((s, n), f32)
        for q in range((c + 3) // 4):
            dots = []
            for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                val = _gather(maps, sv, y0 + dy, x0 + dx)
                acc = val[..., 4 * q] * g[..., 4 * q]
                for j in range(4 * q + 1, min(4 * q + 4, c)):
                    acc = acc + val[..., j] * g[..., j]
                dots.append(np.where(ok[k], acc, f32(0)))
            sx = sx + ((dots[1] - dots[0]) * wy0 + (dots[3] - dots[2]) * wy1)
            sy = sy + ((dots[2] - dots[0]) * wx0 + (dots[3] - dots[1]) * wx1)
        term = (sy * dgx + sx * dgy) if defect == "slopes_swapped" else (sx * dgx + sy * dgy)
        term = np.where(fin & (term == term), term, f32(0)).reshape(s, b, pp).transpose(1, 0, 2).reshape(b, s * pp)
        lanes = np.zeros((b, 64), f32)
        for i in range(s * pp):
            lanes[:, i % 64] += term[:, i]
        width = 64
        while width > 1:
            width //= 2
            lanes = lanes[:, :width] + lanes[:, width:2 * width]
    return torch.from_numpy(np.ascontiguousarray(lanes[:, 0]))


def case_args(case):
    return tuple(case[k] for k in ("o", "d", "z", "g0", "c2ws", "intrs", "kinv", "maps", "patch"))


def patch_sample_f32(m, xy):
    m, xy = _np(m, f32)[None], _np(xy, f32)
    with np.errstate(all="ignore"):
        return torch.from_numpy(_read32(m, np.zeros((1, xy.shape[0]), np.int64), xy[None, :, 0], xy[None, :, 1])[0])
