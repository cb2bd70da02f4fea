"""A float64 restatement of the source-view feature look-up, lookup_feature + compute_angle (projector.py:278-349; K4, k4_feature.hip with
k4_common.h and the tap code of common.h), with a running error bound, for the feature look-up tests.  CPU only: numpy and torch, no GPU.

    inputs      the evaluation's own: pts, w2c (the INVERSE as the evaluation holds it, 16 floats per view -- SceneViews.w2c copied back for the
                kernels, torch.inverse(c2ws) for the float32 oracle), intr, c2w, the images and the feature pyramid, all float32.
    reference   per source view, point and level: px, py, d, the read position (ix, iy), the bilinear value, and a first-order running bound
                (u = 2^-24) that covers any float32 evaluation in any association order: an operation contributes the propagated input
                error plus u |result|, a k-term sum (k - 1) u sum|terms|, a quotient a / b the rigorous (e_a + |a / b| e_b) / (|b| - e_b).
                The level scale 2^-l is exact.  An operation whose inputs carry no error and whose float64 result is a float32 number adds
                nothing (a sum: when every term is a multiple of 2^-23 of the next power of two above sum|terms|, so that every partial sum
                in any order is a float32 number) -- so on inputs built so that nothing rounds (`exact`) the bound on the coordinates is
                zero, and `inside the bound` then means `equal`.
    values      |value - reference| <= e_ix Lx + e_iy Ly + 8 u max|texel|; Lx, Ly the largest horizontal / vertical difference of adjacent
                texels of that view's zero-padded map, per channel: the zero-padded bilinear read is continuous and piecewise bilinear, its
                slope in x a convex combination of two horizontal texel differences, so this also covers a tap that moves to the next
                cell.  8 u max|texel|: four weights of three roundings each (two differences, one product, 3 u sum|w v| <= 3 u max) and
                four accumulations (4 u max), and one to spare.
    mask        a (point, view, level) item is AMBIGUOUS if |d| <= e_d, or px (py) lies within its bound of 0 or of w (h) -- always with a
                non-zero bound: a coordinate that is exact is decided.  A level that is not ambiguous has a decided in-image flag; the mask
                of a (point, view) is false as soon as one decided level is outside, true when all levels are decided inside, and free
                otherwise.  An item whose float64 coordinates are non-finite with nothing to blame on rounding (d = 0 exactly, a NaN / inf
                point) has value 0 and mask false.  Values are held to the bound wherever it is finite, ambiguous or not.
    ray_diff    the same rules through the two normalisations (+ float32(1e-6)), the difference and diff / max(dn, 1e-6): the error grows
                like u / dn.  An item whose dn lies within its error of 1e-6 (or below its error) is ambiguous -- unless the source centre
                IS the reference centre, where the difference is exactly zero in any evaluation.
    backward    the float64 gradient of sum(fv * cot) for every map and the images, with a per-texel bound: a tap weight is 1-Lipschitz in
                ix and in iy, so an item adds (e_ix + e_iy) |cot| to the texels of its 2 x 2 footprint grown by one texel each way, and a
                texel that receives k float32 atomic additions in any order adds (k + 4) u sum|w cot| (4: the three roundings of a weight
                and the product with the cotangent).  An item whose e_ix + e_iy is not below half a texel frees its view's whole map.
    generators  make_case: `inside`, `border`, `behind`, `crowd`, `nonfinite` for every shape of SHAPES, and `exact` (its own scene, see
                make_exact_case), all from seeded torch.Generators; maps at most 65 wide.  Pyramids `from h x w` halve rounding up, never
                below 2 (the size a stride-2 convolution with padding leaves; 48 x 64 halves evenly, 24 x 32 ends at 2 x 2).
    lookup_f32 / lookup_bwd_f32   the same formulas in float32 (numpy: sequential sums, correctly rounded divisions, the kernel's tap and
                accumulation order), with the seeded defects of DEFECTS / BWD_DEFECTS -- mistakes this kernel's structure invites -- to
                show that the bound notices them.
"""
import functools

import numpy as np
import torch

U = 2.0 ** -24
EPS = float(np.float32(1e-6))           # the constant as float32 holds it
AMBIGUOUS_CAP = 0.005
f32 = np.float32


def pyramid(h, w, n):
    out = [(h, w)]
    for _ in range(n - 1):
        h, w = max(2, (h + 1) // 2), max(2, (w + 1) // 2)
        out.append((h, w))
    return tuple(out)


# (nv, level sizes (h, w), points): see tests/test_hip_feature_lookup.py for what each exercises
SHAPES = (
    (2, ((2, 2),), 1),
    (3, pyramid(5, 7, 2), 85),
    (4, pyramid(9, 12, 3), 85),
    (4, pyramid(9, 12, 3), 86),
    (5, pyramid(48, 64, 5), 1622),
    (16, pyramid(30, 41, 4), 33),
    (11, pyramid(24, 32, 5), 300),
    (9, ((40, 52), (20, 26), (10, 13), (5, 7), (3, 4), (2, 2), (2, 3), (3, 2)), 300),
)
SHAPE_IDS = tuple(f"v{nv}-{len(lv)}x{lv[0][0]}x{lv[0][1]}-n{n}" for nv, lv, n in SHAPES)
CLASSES = ("inside", "border", "behind", "crowd", "nonfinite")
DEFECTS = ("align_corners", "level_size", "view_off_by_one", "closed_pixel_test", "border_clamp", "pair_mixup", "rgb_from_level1",
           "no_eps_in_norm")
BWD_DEFECTS = ("taps_swapped", "bwd_level_scale")
EXACT_LEVELS = ((33, 65), (17, 33), (9, 17), (5, 9), (3, 5))
EXACT_PX = (-1.0, -0.25, 0.0, 0.25, 63.0, 64.0, 64.75, 65.0, 65.25)
EXACT_PY = (-0.5, 0.0, 32.0, 32.5, 33.0)
EXACT_D = (1.0, 2.0, 4.0, 0.0, -1.0)


def _np(t, dtype=np.float64):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(t), dtype=dtype)


# ------------------------------------------------------------------------------------------------------------------ running bound
def _is_f32(r):
    with np.errstate(over="ignore", invalid="ignore"):       # (a float64 beyond float32's range is not a float32 number)
        return r == r.astype(f32).astype(np.float64)


def _rnd(r, e_in):
    """The bound after one rounded operation with result r: e_in + u |r|; nothing where the inputs are exact and r is a float32 number."""
    return np.where((e_in == 0) & _is_f32(r), 0.0, e_in + U * np.abs(r))


def _mul(a, e_a, b, e_b):
    r = a * b
    return r, _rnd(r, np.abs(a) * e_b + np.abs(b) * e_a)


def _sum(terms, errs):
    """Sum of k terms in any order, with or without fused multiply-adds."""
    terms = np.broadcast_arrays(*terms)
    s, sa, e_in = sum(terms), sum(np.abs(t) for t in terms), sum(np.broadcast_arrays(*errs))
    quantum = 2.0 ** (np.ceil(np.log2(np.where((sa > 0) & np.isfinite(sa), sa, 1.0))) - 23)
    exact = e_in == 0
    for t in terms:
        exact = exact & (t / quantum == np.rint(t / quantum))
    return s, np.where(exact, 0.0, e_in + (len(terms) - 1) * U * sa)


def _div(a, e_a, b, e_b):
    r = a / b
    room = np.abs(b) - e_b
    e = np.where(room > 0, (e_a + np.abs(r) * e_b) / np.where(room > 0, room, 1.0), np.inf)
    return r, _rnd(r, e)


def _near(a, edge, e):
    return (e > 0) & ~(np.abs(a - edge) > e)                  # (an infinite bound, or a NaN coordinate under one, is `near`)


def _project(w2c, intr, pts):
    """-> px, py, d at level 0 and their bounds, each (S, N)."""
    x, y, z = (pts[:, k][None] for k in range(3))
    zero = np.zeros_like(x)
    cam, e_cam = [], []
    for r in range(3):
        terms = [w2c[1:, r, 0, None] * x, w2c[1:, r, 1, None] * y, w2c[1:, r, 2, None] * z, w2c[1:, r, 3, None] + zero]
        errs = [_rnd(t, zero) for t in terms[:3]] + [zero]
        c, e = _sum(terms, errs)
        cam.append(c)
        e_cam.append(e)
    rows = []
    for r in range(3):
        prods = [_mul(intr[1:, r, j, None] + zero, zero, cam[j], e_cam[j]) for j in range(3)]
        rows.append(_sum([p[0] for p in prods], [p[1] for p in prods]))
    (u, e_u), (v, e_v), (d, e_d) = rows
    px, e_px = _div(u, e_u, d, e_d)
    py, e_py = _div(v, e_v, d, e_d)
    return px, py, d, e_px, e_py, e_d


def _read_position(p, e_p, size):
    """ix = ((p / ((size - 1) / 2) - 1 + 1) * size - 1) / 2 as the evaluation forms it, with its bound."""
    c = np.full_like(p, (size - 1) / 2.0)
    zero = np.zeros_like(p)
    q, e_q = _div(p, e_p, c, zero)
    n = q - 1.0
    e_n = _rnd(n, e_q)
    a = n + 1.0
    e_a = _rnd(a, e_n)
    b, e_b = _mul(a, e_a, np.full_like(p, float(size)), zero)
    cc = b - 1.0
    e_c = _rnd(cc, e_b)
    return cc / 2.0, e_c / 2.0


def _taps(ix, iy, h, w):
    """The four taps of a zero-padded bilinear read, in the dtype of ix: x0, y0 (int64), weights [w00, w01, w10, w11] ((y, x): 00 = north-west)
    and their in-image flags.  common.h's bilinear_taps."""
    one = ix.dtype.type(1)
    fin = np.isfinite(ix) & np.isfinite(iy)
    sx, sy = np.where(fin, ix, 0).astype(ix.dtype), np.where(fin, iy, 0).astype(ix.dtype)
    fx = np.clip(np.floor(sx), -4, w + 4).astype(ix.dtype)
    fy = np.clip(np.floor(sy), -4, h + 4).astype(ix.dtype)
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    wx1, wx0 = sx - fx, (fx + one) - sx
    wy1, wy0 = sy - fy, (fy + one) - sy
    wts = [wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1]
    xin = [(x0 >= 0) & (x0 < w), (x0 + 1 >= 0) & (x0 + 1 < w)]
    yin = [(y0 >= 0) & (y0 < h), (y0 + 1 >= 0) & (y0 + 1 < h)]
    ok = [fin & xin[0] & yin[0], fin & xin[1] & yin[0], fin & xin[0] & yin[1], fin & xin[1] & yin[1]]
    return x0, y0, wts, ok


def _gather(m, sv, yy, xx):
    """m (nv, C, h, w); sv, yy, xx (S, N) -> (S, N, C), indices clamped into the image."""
    h, w = m.shape[2:]
    return m[sv, :, np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]


def _read64(m, sv, ix, iy):
    h, w = m.shape[2:]
    x0, y0, wts, ok = _taps(ix, iy, h, w)
    out = 0.0
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        out = out + _gather(m, sv, y0 + dy, x0 + dx) * (wts[k] * ok[k])[..., None]
    return out


def _slopes(m):
    """m (nv, C, h, w) -> Lx, Ly, top, each (nv, C): the largest adjacent differences of the zero-padded map and the largest |texel|."""
    p = np.pad(m, ((0, 0), (0, 0), (1, 1), (1, 1)))
    return np.abs(np.diff(p, axis=3)).max((2, 3)), np.abs(np.diff(p, axis=2)).max((2, 3)), np.abs(m).max((2, 3))


def reference(pts, w2c, intr, c2w, imgs, feats):
    """pts (N, 3); w2c, intr, c2w (nv, 4, 4); imgs (nv, 3, h, w); feats [(nv, 4, h_l, w_l)], float32 values.  -> dict, arrays in float64:
        fv, fv_bound (N, S, 3 + 4 L)      value and bound (inf where nothing can be said), columns as the kernel lays them out
        ix, iy, e_ix, e_iy, px, py [L] (S, N); d, e_d (S, N)
        inside, amb [L] (S, N) bool       the in-image flag of a level and whether it is ambiguous
        mask_true, mask_false (N, S)      decided masks; an item in neither is free
        dead (S, N)                       non-finite float64 coordinates with nothing to blame on rounding: value 0, mask false
        ray_diff, rd_bound (N, S, 4), rd_amb (N, S)"""
    pts, w2c, intr, c2w, imgs = _np(pts), _np(w2c), _np(intr), _np(c2w), _np(imgs)
    feats = [_np(f) for f in feats]
    nv, n = w2c.shape[0], pts.shape[0]
    s = nv - 1
    sv = np.broadcast_to(np.arange(1, nv)[:, None], (s, n))
    with np.errstate(all="ignore"):
        px0, py0, d, e_px0, e_py0, e_d = _project(w2c, intr, pts)
        bad_pt = ~np.isfinite(pts).all(-1)[None]
        dead = bad_pt | ((d == 0) & (e_d == 0))
        wild = ~dead & ~(np.abs(d) > e_d)                    # |d| <= e_d: the quotient is anybody's
        out = dict(d=d, e_d=e_d, dead=dead, ix=[], iy=[], e_ix=[], e_iy=[], px=[], py=[], inside=[], amb=[])
        cols, bounds = [None], [None]
        for l, m in enumerate(feats):
            h, w = m.shape[2:]
            sc = 2.0 ** -l
            px, py, e_px, e_py = px0 * sc, py0 * sc, e_px0 * sc, e_py0 * sc
            ix, e_ix = _read_position(px, e_px, w)
            iy, e_iy = _read_position(py, e_py, h)
            inside = ~dead & (d > 0) & (px >= 0) & (px < w) & (py >= 0) & (py < h)
            amb = ~dead & (wild | _near(px, 0.0, e_px) | _near(px, float(w), e_px) | _near(py, 0.0, e_py) | _near(py, float(h), e_py))
            free = wild | ~np.isfinite(e_ix) | ~np.isfinite(e_iy)
            for mm, store in ((m, True),) + (((imgs, False),) if l == 0 else ()):
                val = np.where(dead[..., None], 0.0, _read64(mm, sv, np.where(dead, np.nan, ix), np.where(dead, np.nan, iy)))
                lx, ly, top = _slopes(mm)
                bnd = e_ix[..., None] * lx[1:, None] + e_iy[..., None] * ly[1:, None] + 8 * U * top[1:, None]
                bnd = np.where(dead[..., None], 0.0, np.where(free[..., None], np.inf, bnd))
                if store:
                    cols.append(val)
                    bounds.append(bnd)
                else:
                    cols[0], bounds[0] = val, bnd
            for k, a in zip(("ix", "iy", "e_ix", "e_iy", "px", "py", "inside", "amb"), (ix, iy, e_ix, e_iy, px, py, inside, amb)):
                out[k].append(a)
        decided_out = [~a & ~i for a, i in zip(out["amb"], out["inside"])]
        decided_in = [~a & i for a, i in zip(out["amb"], out["inside"])]
        out["mask_false"] = np.logical_or.reduce(decided_out).T
        out["mask_true"] = np.logical_and.reduce(decided_in).T
        out["fv"] = np.concatenate(cols, -1).transpose(1, 0, 2)
        out["fv_bound"] = np.concatenate(bounds, -1).transpose(1, 0, 2)
        out.update(_ray_diff(pts, c2w))
    return out


def _unit(v, e_v):
    """v [3 x (S, N)] -> v / (|v| + 1e-6) with bounds."""
    sq = [_mul(c, e, c, e) for c, e in zip(v, e_v)]
    rr, e_rr = _sum([q[0] for q in sq], [q[1] for q in sq])
    nrm = np.sqrt(rr)
    e_n = _rnd(nrm, np.where(rr > 0, e_rr / (2 * np.where(rr > 0, nrm, 1.0)), np.sqrt(e_rr)))
    den = nrm + EPS
    e_den = _rnd(den, e_n)
    return [_div(c, e, den, e_den) for c, e in zip(v, e_v)]


def _ray_diff(pts, c2w):
    p = [pts[:, k][None] for k in range(3)]
    zero = np.zeros_like(p[0])
    ref_c, src_c = c2w[0, :3, 3], c2w[1:, :3, 3]
    to_ref = [ref_c[k] - p[k] + np.zeros((src_c.shape[0], 1)) for k in range(3)]
    to_src = [src_c[:, k, None] - p[k] for k in range(3)]
    r = _unit(to_ref, [_rnd(c, zero) for c in to_ref])
    q = _unit(to_src, [_rnd(c, zero) for c in to_src])
    diff = [a[0] - b[0] for a, b in zip(r, q)]
    e_diff = [_rnd(dd, a[1] + b[1]) for dd, a, b in zip(diff, r, q)]
    sq = [_mul(c, e, c, e) for c, e in zip(diff, e_diff)]
    rr, e_rr = _sum([t[0] for t in sq], [t[1] for t in sq])
    dn = np.sqrt(rr)
    e_dn = _rnd(dn, np.where(rr > 0, e_rr / (2 * np.where(rr > 0, dn, 1.0)), np.sqrt(e_rr)))
    same = (src_c == ref_c[None]).all(-1)[:, None] & np.isfinite(pts).all(-1)[None]        # the difference is exactly zero in any evaluation
    clamped = dn + e_dn < EPS
    amb = ~same & ~clamped & ~(dn - e_dn > EPS) & np.isfinite(pts).all(-1)[None]
    den = np.where(clamped, EPS, dn)
    e_den = np.where(clamped, 0.0, e_dn)
    comps = [_div(c, e, den, e_den) for c, e in zip(diff, e_diff)]
    prods = [_mul(a[0], a[1], b[0], b[1]) for a, b in zip(r, q)]
    dot, e_dot = _sum([t[0] for t in prods], [t[1] for t in prods])
    val = np.stack([np.where(same, 0.0, c[0]) for c in comps] + [dot], -1)
    bnd = np.stack([np.where(same, 0.0, np.where(amb, np.inf, c[1])) for c in comps] + [e_dot], -1)
    return dict(ray_diff=val.transpose(1, 0, 2), rd_bound=bnd.transpose(1, 0, 2), rd_amb=amb.T)


# ------------------------------------------------------------------------------------------------------------------ checks
def _use(got, want, bound):
    """|got - want| / bound per entry: 0 where they agree, inf where they differ and the bound is zero, 0 where the bound is infinite."""
    got = _np(got)
    with np.errstate(all="ignore"):
        err = np.abs(got - want)
        err = np.where(np.isnan(got) | np.isnan(want), np.where(np.isnan(got) & np.isnan(want), 0.0, np.inf), err)
        use = np.where(err == 0, 0.0, np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.inf))
    return np.where(np.isinf(bound), 0.0, use)


def ambiguous_share(ref):
    amb = np.stack(ref["amb"])
    return int(amb.sum()), amb.size


def check_forward(ref, fv, ray_diff, mask, pts):
    """-> dict(use_fv, use_rd: the worst share of the bound used; mask_bad: decided masks that differ; n_amb, n_items; n_free_masks)."""
    use_fv = _use(fv, ref["fv"], ref["fv_bound"])
    finite_pt = np.isfinite(_np(pts)).all(-1)
    use_rd = _use(ray_diff, ref["ray_diff"], ref["rd_bound"])[finite_pt]
    mask = _np(mask, bool)
    bad = (ref["mask_true"] & ~mask) | (ref["mask_false"] & mask)
    n_amb, n_items = ambiguous_share(ref)
    return dict(use_fv=float(use_fv.max(initial=0.0)), use_rd=float(use_rd.max(initial=0.0)), mask_bad=int(bad.sum()), n_amb=n_amb,
                n_items=n_items, n_free_masks=int((~ref["mask_true"] & ~ref["mask_false"]).sum()))


def forward_ok(res):
    return res["use_fv"] <= 1 and res["use_rd"] <= 1 and res["mask_bad"] == 0


def grads_reference(ref, shapes, cot, base=0.0):
    """The float64 gradient of sum(fv * cot) and its per-texel bound.  shapes: [(h, w)] per level; cot (N, S, 3 + 4 L).  base: the constant the
    buffers held before (the kernels ADD): it is part of the result, and each of a texel's k additions then also rounds at its size (k u |base|).
    -> (grads, bounds): lists [level 0 .. L - 1, images] of (nv, C, h, w) float64 (C = 4 for the maps, 3 for the images)."""
    cot = _np(cot).transpose(1, 0, 2)                        # (S, N, row)
    s, n = cot.shape[:2]
    nv = s + 1
    sv = np.broadcast_to(np.arange(1, nv)[:, None], (s, n))
    grads, bounds = [], []
    with np.errstate(all="ignore"):
        for l, (h, w) in list(enumerate(shapes)) + [(0, shapes[0])]:
            img = len(grads) == len(shapes)
            c = cot[..., :3] if img else cot[..., 3 + 4 * l:7 + 4 * l]
            nc = c.shape[-1]
            dead = ref["dead"]
            ix, iy = np.where(dead, np.nan, ref["ix"][l]), np.where(dead, np.nan, ref["iy"][l])
            e = np.where(dead, 0.0, ref["e_ix"][l] + ref["e_iy"][l])
            x0, y0, wts, ok = _taps(ix, iy, h, w)
            g, sumabs, cnt, eb = (np.zeros((nv, h, w, nc)) for _ in range(4))
            for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                at = (sv[ok[k]], (y0 + dy)[ok[k]], (x0 + dx)[ok[k]])
                term = wts[k][ok[k]][:, None] * c[ok[k]]
                np.add.at(g, at, term)
                np.add.at(sumabs, at, np.abs(term))
                np.add.at(cnt, at, (c[ok[k]] != 0).astype(np.float64))
            free = ~dead & ~(e < 0.5)
            tame = ~dead & ~free
            for oy in range(-1, 3):
                for ox in range(-1, 3):
                    yy, xx = y0 + oy, x0 + ox
                    sel = tame & (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
                    np.add.at(eb, (sv[sel], yy[sel], xx[sel]), e[sel][:, None] * np.abs(c[sel]))
            bound = eb + (cnt + 4) * U * sumabs + cnt * U * abs(base)
            hit = (free[..., None] & (c != 0)).any(1)        # (S, nc): a free item with a cotangent in this channel
            bound[1:] = np.where(hit[:, None, None, :], np.inf, bound[1:])
            grads.append(g.transpose(0, 3, 1, 2) + base)
            bounds.append(bound.transpose(0, 3, 1, 2))
    return grads, bounds


def check_grads(want, bounds, got):
    """-> the worst share of the bound used over all maps and the images (inf: outside)."""
    worst = 0.0
    for w, b, g in zip(want, bounds, got):
        worst = max(worst, float(_use(g, w, b).max(initial=0.0)))
    return worst


def adjoint_tolerance(ref, case, cot):
    """For the adjoint identity sum(fv * cot) = sum over maps of sum(map * grad): both sides are roundings of the same exact sum of terms
    w * texel * cot (one per item, tap and channel).  The forward rounds a term at most 8 times (see `values`); the backward rounds the terms
    of a texel that receives k additions at most k + 4 times each.  -> (tol, total): tol = u sum over texels of (k + 12) A, with A >= the sum
    of |w| |texel| |cot| of the texel's terms (weights raised by their error, k counted over the footprints grown by one texel), and total
    the sum of all A."""
    cot = _np(cot).transpose(1, 0, 2)
    s, n = cot.shape[:2]
    sv = np.broadcast_to(np.arange(1, s + 1)[:, None], (s, n))
    tol, total = 0.0, 0.0
    maps = [_np(f) for f in case["feats"]] + [_np(case["imgs"])]
    with np.errstate(all="ignore"):
        for j, m in enumerate(maps):
            l = j if j < len(case["feats"]) else 0
            c = np.abs(cot[..., 3 + 4 * l:7 + 4 * l] if j < len(case["feats"]) else cot[..., :3])
            h, w = m.shape[2:]
            dead = ref["dead"]
            ix, iy = np.where(dead, np.nan, ref["ix"][l]), np.where(dead, np.nan, ref["iy"][l])
            x0, y0, _, _ = _taps(ix, iy, h, w)
            e = np.where(dead, 0.0, ref["e_ix"][l] + ref["e_iy"][l])
            cnt, amount = np.zeros((s + 1, h, w)), np.zeros((s + 1, h, w))
            for oy in range(-1, 3):
                for ox in range(-1, 3):
                    yy, xx = y0 + oy, x0 + ox
                    sel = ~dead & (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
                    wt = np.clip(1 - np.abs(ix - xx), 0, 1) * np.clip(1 - np.abs(iy - yy), 0, 1)       # the tent of texel (yy, xx)
                    at = (sv[sel], yy[sel], xx[sel])
                    np.add.at(amount, at, (((wt + e)[sel])[:, None] * np.abs(_gather(m, sv, yy, xx)[sel]) * c[sel]).sum(-1))
                    np.add.at(cnt, at, 1.0)
            tol += U * float(((cnt + 12) * amount).sum())
            total += float(amount.sum())
    return tol, total


# ------------------------------------------------------------------------------------------------------------------ inputs
def w2c_of(c2ws):
    """The inverse as gens_scene_setup forms it: solved in float64, rounded once."""
    return torch.from_numpy(np.linalg.inv(_np(c2ws)).astype(f32))


def _look_at(centre, target, up):
    fwd = (target - centre) / np.linalg.norm(target - centre)
    right = np.cross(up, fwd)
    right /= np.linalg.norm(right)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, np.cross(fwd, right), fwd, centre
    return m


def make_scene(nv, levels, seed):
    """Cameras on an arc of radius ~2.2 around the unit cube, all looking near the origin; white-noise images and maps."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64).numpy()  # noqa: E731
    h, w = levels[0]
    c2ws, intrs = [], []
    for k in range(nv):
        az = np.radians((k - (nv - 1) / 2) * 7.0 + 4.0 * (rnd(1)[0] - 0.5))
        el = np.radians(20.0 * (rnd(1)[0] - 0.5))
        r = 2.2 * (1 + 0.1 * (rnd(1)[0] - 0.5))
        centre = r * np.array([np.sin(az) * np.cos(el), np.sin(el), -np.cos(az) * np.cos(el)])
        c2ws.append(_look_at(centre, 0.2 * (rnd(3) - 0.5), np.array([0.05 * (rnd(1)[0] - 0.5), 1.0, 0.0])))
        intr = np.eye(4)
        intr[0, 0], intr[1, 1] = 1.8 * w * (1 + 0.1 * (rnd(1)[0] - 0.5)), 2.4 * h * (1 + 0.1 * (rnd(1)[0] - 0.5))
        intr[0, 2], intr[1, 2] = w * (0.5 + 0.06 * (rnd(1)[0] - 0.5)), h * (0.5 + 0.06 * (rnd(1)[0] - 0.5))
        intrs.append(intr)
    imgs = torch.rand(nv, 3, h, w, generator=g)
    feats = [torch.randn(nv, 4, hh, ww, generator=g) for hh, ww in levels]
    return dict(intrs=torch.from_numpy(np.stack(intrs)).float(), c2ws=torch.from_numpy(np.stack(c2ws)).float(), imgs=imgs, feats=feats,
                levels=tuple(levels))


def _back_project(sc, view, px, py, d):
    """Points that view `view` (array of view indices) sees at pixel (px, py) and depth d, in float64 from the float32 cameras."""
    k, c2w = _np(sc["intrs"])[view], _np(sc["c2ws"])[view]
    cam = np.stack([(px - k[:, 0, 2]) * d / k[:, 0, 0], (py - k[:, 1, 2]) * d / k[:, 1, 1], d, np.ones_like(d)], -1)
    return torch.from_numpy(np.einsum("nij,nj->ni", c2w, cam)[:, :3]).float()


def make_case(shape, cls, seed=None):
    nv, levels, n = SHAPES[shape]
    assert cls in CLASSES
    seed = 1000 * shape + CLASSES.index(cls) if seed is None else seed
    sc = make_scene(nv, levels, seed)
    g = torch.Generator().manual_seed(seed + 500)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64).numpy()  # noqa: E731
    h, w = levels[0]
    view = 1 + np.arange(n) % (nv - 1)
    if cls in ("inside", "nonfinite"):
        pts = (torch.rand(n, 3, generator=g) * 1.2 - 0.6)
        if cls == "nonfinite":
            for row, (col, val) in zip((1, 2, 3, n - 1) if n >= 5 else (n - 1,), ((0, float("nan")), (1, float("inf")), (2, -float("inf")), (0, float("nan")))):
                pts[row, col] = val
    elif cls == "border":                                   # within 2 px of an edge: one or two taps are zero-padded
        edge, t, off = np.arange(n) % 4, rnd(n), 4 * rnd(n) - 2
        px = np.where(edge == 0, off, np.where(edge == 1, w + off, (w + 4) * t - 2))
        py = np.where(edge == 2, off, np.where(edge == 3, h + off, (h + 4) * t - 2))
        px, py = np.where(edge < 2, px, (w + 4) * t - 2), np.where(edge >= 2, py, (h + 4) * t - 2)
        pts = _back_project(sc, view, px, py, 1.6 + 1.2 * rnd(n))
    elif cls == "behind":                                   # d < 0, |d| from 2 down to 1e-3
        pts = _back_project(sc, view, w * rnd(n), h * rnd(n), -(10.0 ** (-3 + 3.3 * rnd(n))))
    else:                                                   # crowd: every point inside one texel of view 1
        x0, y0 = np.floor(w * (0.3 + 0.3 * rnd(1)[0])), np.floor(h * (0.3 + 0.3 * rnd(1)[0]))
        pts = _back_project(sc, np.ones(n, np.int64), x0 + rnd(n), y0 + rnd(n), 2.1 + 0.05 * rnd(n))
    row = 3 + 4 * len(levels)
    sc.update(pts=pts.contiguous(), cot=torch.randn(n, nv - 1, row, generator=g), w2c=w2c_of(sc["c2ws"]), cls=cls, shape=shape)
    return sc


def make_exact_case():
    """Nothing rounds: identity rotations, centres at z = -2 with dyadic x / y offsets, fx = fy = 32, cx = 32, cy = 16, maps of size 2^k + 1 (so
    (w - 1) / 2 is a power of two), texels, images and cotangents multiples of 1/8 (1/2), points back-projected through view 1 from quarter-pixel
    targets on and next to every edge at depths 1, 2, 4, 0 (the lateral offset of depth 1, in the camera's own plane) and -1, one point AT view
    1's centre, and view 2 with the reference view's pose."""
    g = torch.Generator().manual_seed(77)
    centres = np.array([[0.0, 0.0, -2.0], [0.5, -0.125, -2.0], [0.0, 0.0, -2.0]])   # (no grid point in the cameras' plane lies on the line through both)
    c2ws = np.stack([np.eye(4)] * 3)
    c2ws[:, :3, 3] = centres
    intr = np.eye(4)
    intr[0, 0] = intr[1, 1] = 32.0
    intr[0, 2], intr[1, 2] = 32.0, 16.0
    pts = []
    for d in EXACT_D:
        lateral = d if d != 0 else 1.0
        for py in EXACT_PY:
            for px in EXACT_PX:
                pts.append([(px - 32.0) * lateral / 32.0 + centres[1, 0], (py - 16.0) * lateral / 32.0 + centres[1, 1], d + centres[1, 2]])
    pts.append(list(centres[1]))
    dy = lambda *s, q, top: (torch.randint(-top, top + 1, s, generator=g).float() / q)  # noqa: E731
    h, w = EXACT_LEVELS[0]
    pts = torch.tensor(pts, dtype=torch.float64)
    assert torch.equal(pts.float().double(), pts)
    n, row = pts.shape[0], 3 + 4 * len(EXACT_LEVELS)
    return dict(intrs=torch.from_numpy(np.stack([intr] * 3)).float(), c2ws=torch.from_numpy(c2ws).float(), imgs=dy(3, 3, h, w, q=8, top=8).abs(),
                feats=[dy(3, 4, hh, ww, q=8, top=16) for hh, ww in EXACT_LEVELS], levels=EXACT_LEVELS, pts=pts.float().contiguous(),
                cot=dy(n, 2, row, q=2, top=2), w2c=w2c_of(c2ws), cls="exact", shape=None)


def case_reference(case, w2c=None):
    return reference(case["pts"], case["w2c"] if w2c is None else w2c, case["intrs"], case["c2ws"], case["imgs"], case["feats"])


@functools.lru_cache(maxsize=None)
def shape_case(shape, cls):
    """The case the CPU and the GPU tests share (computed once, never modified), with the reference for the float64-solved inverse.
    shape None / cls `exact`: the exact case.  -> (case, reference)."""
    case = make_exact_case() if cls == "exact" else make_case(shape, cls)
    return case, case_reference(case)


def reference_for(shape, cls, w2c):
    """shape_case's reference if w2c (the evaluation's own inverse) has its bits, a fresh one otherwise."""
    case, ref = shape_case(shape, cls)
    return (case, ref) if torch.equal(w2c.cpu().reshape(-1), case["w2c"].reshape(-1)) else (case, case_reference(case, w2c.cpu()))


@functools.lru_cache(maxsize=None)
def shape_grads(shape, cls):
    case, ref = shape_case(shape, cls)
    return grads_reference(ref, case["levels"], case["cot"])


ALL_CASES = tuple((i, c) for i in range(len(SHAPES)) for c in CLASSES) + ((None, "exact"),)


def case_id(shape, cls):
    return "exact" if cls == "exact" else f"{SHAPE_IDS[shape]}-{cls}"


# ------------------------------------------------------------------------------------------------------------------ float32 restatement
def _fma32(a, b, c):
    """float32 fma(a, b, c) through float64: the product is exact there, the sum rounded twice (which differs from one rounding only on ties
    of the float64 sum -- a last bit in one of ~2^29 results, and never where nothing rounds)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def _project32(w2c, intr, pts):
    x, y, z = (pts[:, k][None] for k in range(3))
    cam = [w2c[1:, r, 0, None] * x + w2c[1:, r, 1, None] * y + w2c[1:, r, 2, None] * z + w2c[1:, r, 3, None] for r in range(3)]
    u, v, d = (intr[1:, r, 0, None] * cam[0] + intr[1:, r, 1, None] * cam[1] + intr[1:, r, 2, None] * cam[2] for r in range(3))
    return u / d, v / d, d


def _position32(p, size, norm_size=None):
    c = f32(((size if norm_size is None else norm_size) - 1) / 2.0)
    n = p / c - f32(1)
    return ((n + f32(1)) * f32(size) - f32(1)) / f32(2)


def lookup_f32(pts, w2c, intr, c2w, imgs, feats, defect=None):
    """-> fv (N, S, 3 + 4 L) float32, ray_diff (N, S, 4) float32, mask (N, S) bool, as torch tensors.  defect: None or one of DEFECTS:
        align_corners      the maps are read at ix = px                                    (the Q6 quirk undone)
        level_size         level l >= 1 normalised with level 0's (w, h)                   (fs.cw[0] for fs.cw[l])
        view_off_by_one    taps read from view sv - 1's image                              (sv counts from 1)
        closed_pixel_test  px <= w, py <= h
        border_clamp       a tap outside the image keeps its weight                        (the clamped loads without the ok flags)
        pair_mixup         odd items take their x0 taps from the even partner's rows       (pair_taps: r0 / r1 not swapped back)
        rgb_from_level1    the colour columns are read with level 1's taps                 (q, t of the wrong trip of the level loop)
        no_eps_in_norm     ray_diff without the 1e-6 in the two normalisations"""
    assert defect is None or defect in DEFECTS
    pts, w2c, intr, c2w, imgs = (_np(t, f32) for t in (pts, w2c, intr, c2w, imgs))
    feats = [_np(t, f32) for t in feats]
    nv, n = w2c.shape[0], pts.shape[0]
    s = nv - 1
    sv = np.broadcast_to(np.arange(1, nv)[:, None], (s, n))
    item = np.arange(n)[None] * s + np.arange(s)[:, None]
    mate = np.where(item % 2 == 1, item - 1, item)            # the even lane of an odd item's pair
    mate_at = (mate % s, mate // s)
    read_view = sv - 1 if defect == "view_off_by_one" else sv
    h0, w0 = feats[0].shape[2:]
    with np.errstate(all="ignore"):
        px0, py0, d = _project32(w2c, intr, pts)
        mask = np.ones((s, n), bool)
        cols, keep = [None], {}
        for l, m in enumerate(feats):
            h, w = m.shape[2:]
            px, py = px0 * f32(2.0 ** -l), py0 * f32(2.0 ** -l)
            if defect == "closed_pixel_test":
                mask &= (d > 0) & (px >= 0) & (px <= f32(w)) & (py >= 0) & (py <= f32(h))
            else:
                mask &= (d > 0) & (px >= 0) & (px < f32(w)) & (py >= 0) & (py < f32(h))
            if defect == "align_corners":
                ix, iy = px, py
            else:
                level0 = defect == "level_size" and l >= 1
                ix, iy = _position32(px, w, w0 if level0 else None), _position32(py, h, h0 if level0 else None)
            x0, y0, wts, ok = _taps(ix, iy, h, w)
            keep[l] = (x0, y0, wts, ok)

            def read(mm, taps):
                x0, y0, wts, ok = taps
                hh, ww = mm.shape[2:]
                acc = np.zeros((s, n, mm.shape[1]), f32)
                for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                    val = _gather(mm, read_view, y0 + dy, x0 + dx)
                    if defect == "pair_mixup" and dx == 0:
                        yc = np.clip(y0 + dy, 0, hh - 1)
                        val = mm[read_view[mate_at], :, yc[mate_at], np.clip(x0, 0, ww - 1)]
                    wt = wts[k] if defect == "border_clamp" else np.where(ok[k], wts[k], f32(0))
                    wt = np.where(np.isfinite(ix) & np.isfinite(iy), wt, f32(0))
                    acc = _fma32(val, np.broadcast_to(wt[..., None], val.shape), acc)
                return acc
            cols.append(read(m, keep[l]))
            if l == 0:
                cols[0] = read(imgs, keep[0])
            if l == 1 and defect == "rgb_from_level1":
                cols[0] = read(imgs, keep[1])
        fv = np.concatenate(cols, -1).transpose(1, 0, 2)
        eps = f32(0) if defect == "no_eps_in_norm" else f32(1e-6)

        def unit(c):
            v = [c[:, k, None] - pts[:, k][None] for k in range(3)]
            nrm = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) + eps
            return [a / nrm for a in v]
        r, q = unit(np.broadcast_to(c2w[0, :3, 3], (s, 3))), unit(c2w[1:, :3, 3])
        diff = [a - b for a, b in zip(r, q)]
        dn = np.maximum(np.sqrt(diff[0] * diff[0] + diff[1] * diff[1] + diff[2] * diff[2]), f32(1e-6))
        rd = np.stack([a / dn for a in diff] + [r[0] * q[0] + r[1] * q[1] + r[2] * q[2]], -1).transpose(1, 0, 2)
    return torch.from_numpy(np.ascontiguousarray(fv)), torch.from_numpy(np.ascontiguousarray(rd)), torch.from_numpy(np.ascontiguousarray(mask.T))


def lookup_bwd_f32(pts, w2c, intr, levels, cot, defect=None):
    """The gradient of sum(fv * cot) in float32, added texel by texel in item order.  -> [level 0 .. L - 1, images] of (nv, C, h, w) float32
    tensors.  defect: None or one of BWD_DEFECTS:
        taps_swapped     the weights of the north-east and south-west taps exchanged     (tap = dy * 2 + dx read as dx * 2 + dy)
        bwd_level_scale  the backward projects level l with 2^-(l + 1)                    (its own exp2f, not the forward's)"""
    assert defect is None or defect in BWD_DEFECTS
    pts, w2c, intr, cot = (_np(t, f32) for t in (pts, w2c, intr, cot))
    cot = cot.transpose(1, 0, 2)
    nv, n = w2c.shape[0], pts.shape[0]
    s = nv - 1
    sv = np.broadcast_to(np.arange(1, nv)[:, None], (s, n))
    out = []
    with np.errstate(all="ignore"):
        px0, py0, _ = _project32(w2c, intr, pts)
        for l, (h, w) in list(enumerate(levels)) + [(0, levels[0])]:
            img = len(out) == len(levels)
            c = cot[..., :3] if img else cot[..., 3 + 4 * l:7 + 4 * l]
            sc = f32(2.0 ** -(l + 1 if defect == "bwd_level_scale" else l))
            x0, y0, wts, ok = _taps(_position32(px0 * sc, w), _position32(py0 * sc, h), h, w)
            if defect == "taps_swapped":
                wts = [wts[0], wts[2], wts[1], wts[3]]
            g = np.zeros((nv, h, w, c.shape[-1]), f32)
            for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                np.add.at(g, (sv[ok[k]], (y0 + dy)[ok[k]], (x0 + dx)[ok[k]]), wts[k][ok[k]][:, None] * c[ok[k]])
            out.append(torch.from_numpy(np.ascontiguousarray(g.transpose(0, 3, 1, 2))))
    return out
