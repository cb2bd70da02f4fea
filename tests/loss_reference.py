"""Float64 references, float32 restatements with seeded defects, case generators and the acceptance criteria for the loss kernels:
K13 compute_LNCC (k13_lncc.hip), K10 tv_regularization (k9_misc.hip scalar and four-voxel forms, k19_step.hip all-levels form) and the fused
Loss.forward (k19_step.hip loss_fwd_k / loss_bwd_k).  Plain torch / numpy on the CPU, no gens_amd import.  u = 2^-24 throughout.

CRITERIA AND WHERE THEY COME FROM

TV value.  Every term (v' - v)^2 is non-negative, so a float32 sum of them has a relative error of at most k u, k the longest chain of roundings
    on the way of one term into the total.  Four-voxel forms: the difference and the square (2), up to 16 additions into the thread's accumulator
    (4 voxels x 4 channels), 6 steps of the wave sum, 3 additions of the block's four waves: 27 < 32.  The scalar form has 4 additions per thread
    instead of 16.  The per-block partials are added in float64 (nothing), sx + sy + sz, the division and the square root (which halves what
    precedes it) are float64, the result is rounded to float32 once: well under 32 u.  tv_l and the weighted total are held to 64 u relative,
    twice the count.  The pair count is a sum of ones and exact.  A level whose mask leaves no pair has tv_l = sqrt(0 / 1e-8) = 0 exactly.
TV gradient.  g = coef_l s, s the sum of up to six terms 2 (v - v') (each: one difference, an exact doubling, one addition: at most 12
    roundings on s, relative to A = sum |2 (v - v')|, since the terms may cancel), coef_l = g_up 0.5^l / (2 tv_l den_l) in float32 from a tv_l
    that carries 32 u at most (above), the products and the division 5 more: under 50 roundings.  |g - g64| <= 128 u coef64_l A per element.
    Where no neighbour pair is active A = 0 and the device value must be 0 exactly.  On a level without any pair coef_l is infinite and every
    element is NaN in float64 too (sqrt' at 0 times 0); there the NaN patterns must agree.
Loss terms.  loss_fwd_k gives thread t the elements t, t + 1024, ...: ceil(n / 1024) additions, then 6 wave steps and 16 additions of the wave
    totals, and the element's own expression (colour: three differences and two additions; the division by the count, the 1e-5 / 1e-8 guard and
    the factor 0.5 a few more): ceil(n / 1024) + 30 roundings cover it, all terms of a sum are non-negative, and each term is held to
    2 (ceil(n / 1024) + 30) u relative with n the length of that term's sum.  The sparse term adds the rounding of expf's argument:
    fl(|x| scale) is off by u |x| scale relatively, which moves exp(-|x| scale) by that fraction: + mean(u |x| scale exp(-|x| scale)); and
    2^-126, the smallest normal float32, since expf may flush what lies below it.  eikonal / smooth / tv are copies: exact.  An absent
    target gives exactly 0.  `loss` is held to the same relative bound (with the largest n) applied to sum_k |w_k term_k|, plus w_sparse times
    the expf allowance.  The weights and sparse_scale reach the kernel as float32 arguments; the reference takes them at those values.
Loss gradients are element-wise: g_up w, the mask, the division by the count (itself an exact sum of ones plus a guard: one rounding), the sign;
    the longest chain is g_sparse (|x| scale, expf at 2 ulp, scale sign, three products, the division: k = 8).  2 (k + 8) u = 32 u relative, for
    g_sparse plus u |x| scale |g64| for expf's argument and 2^-126 (1 + |g_up w scale / n|) for the flush.  Where the float64 gradient is
    exactly zero (invalid ray, gated target, sign(0), an all-invalid batch) the bound is zero: the device value must be zero.
LNCC value (a): lncc_bound, a first-order running error bound of the one-pass formula for a float32 evaluation in ANY summation order: a sum of P
    exact terms (P - 1) u sum |t|, of P rounded products P u sum |t|; every later operation the propagated error of its operands plus
    u |result| (a b: + e_a e_b as well; a / b: (e_a + |a / b| e_b) / (|b| - e_b); unbounded once e_b >= |b| / 2); 1e-5f against 1e-5; the clamp is 1-Lipschitz; the mean over C
    channels sum e / C + C u |mean|; the mean of the two smallest of S numbers is 1-Lipschitz in the max norm, so the ray's bound is the largest
    view bound + 4 u, capped at 2 (both values lie in [0, 2]).  It is vacuous where the one-pass variance cancels (`bright`), hence
LNCC value (b): per case, worst |device - float64| <= max(4 e32, 4 u), e32 the worst error of the clean in-order float32 restatement lncc_f32 on
    the same case.  The kernel performs lncc_f32's operations in lncc_f32's order (-ffp-contract=off); 4 is the factor the suite uses where a
    device result is held to a CPU float32 evaluation of the same formulas.
LNCC gradients.  A ray is KEPT when its selection and its clamp decisions cannot differ between correct evaluations: the gap between the second
    and third smallest view mean exceeds 1e-4 (S = 2: always) and no channel's 1 - cc lies within 1e-4 of 0 or 2 -- about 60 times the worst
    float32 value error on these cases.  e = max over kept rays of max |g - g64| / max |g64| per ray, for g_ref and g_src;
    e_device <= max(4 e_oracle32, 1e-6), e_oracle32 that of float32 autograd through oracle.gens_oracle.lncc.  Gradients are compared on
    `ordinary` only: on `bright` the float32 value error itself (up to 9e-4) exceeds the 1e-4 gap, so no ray's selection is settled; `dim`
    and `constant` tie all views; on `twin` the sum of the two twins' g_src is compared, which does not depend on which twin is selected.
LNCC and NaN.  torch.clamp keeps NaN and torch.topk ranks it after every number, so lncc64 is NaN exactly where fewer than two views are
    NaN-free; lncc_f32 states the same rule (a view whose mean is NaN never displaces a number; fewer than two numbers give NaN).
"""
import functools
import math

import numpy as np
import torch

from oracle import gens_oracle as K

U = 2.0 ** -24
F64 = torch.float64
FLT_MIN = 2.0 ** -126
f32 = np.float32


def _rng(seed):
    return torch.Generator().manual_seed(seed)


# ================================================================================================================== LNCC
LNCC_SHAPES = ((257, 4, 12, 121), (5, 5, 12, 121), (3, 4, 16, 121), (4, 2, 32, 9), (257, 64, 1, 121), (6, 9, 7, 121), (1, 12, 5, 121),
               (2, 2, 1, 1), (1, 3, 12, 121))
LNCC_CLASSES = ("ordinary", "dim", "bright", "constant", "twin")
LNCC_GRAD_CLASSES = ("ordinary",)
LNCC_DEFECTS = ("short", "first2", "min", "lane")
KEEP_GAP = 1e-4


def lncc_parts(ref, src):
    """ncc.py:29-53 up to the channel mean, operation by operation as oracle.gens_oracle.lncc.  -> means (B, S), raw 1 - cc (B, S, C)."""
    p = ref.shape[2]
    r, s = ref.permute(1, 0, 3, 2), src.permute(1, 0, 3, 2)
    ref_sum, src_sum = r.sum(-1), s.sum(-1)
    u_ref, u_src = ref_sum / p, src_sum / p
    cross = (r * s).sum(-1) - u_src * ref_sum - u_ref * src_sum + u_ref * u_src * p
    ref_var = (r * r).sum(-1) - 2 * u_ref * ref_sum + u_ref * u_ref * p
    src_var = (s * s).sum(-1) - 2 * u_src * src_sum + u_src * u_src * p
    raw = 1 - cross * cross / (ref_var * src_var + 1e-5)
    return torch.clamp(raw, 0.0, 2.0).mean(dim=2), raw


def keep_mask(means, raw, twins=False):
    """The rays whose selection and clamp decisions no correct float32 evaluation can take differently.  twins: views 0 and 1 are identical,
    and a tie between THEM at ranks two and three changes nothing in the sum of their gradients."""
    b, s = means.shape
    srt = torch.sort(means, 1)[0]
    gap = torch.ones(b, dtype=torch.bool) if s == 2 else (srt[:, 2] - srt[:, 1]) > KEEP_GAP
    if twins and s > 2:
        t = means[:, 0]
        tie = (srt[:, 1] == t) & (srt[:, 2] == t) & ((srt[:, 1] - srt[:, 0]) > KEEP_GAP)
        if s > 3:
            tie = tie & ((srt[:, 3] - srt[:, 2]) > KEEP_GAP)
        gap = gap | tie
    edge = ((raw.abs() > KEEP_GAP) & ((raw - 2).abs() > KEEP_GAP)).all(-1).all(-1)
    return gap & edge & torch.isfinite(means).all(-1)


def lncc64(ref, src, twins=False):
    """-> (ncc (B, 1) = oracle.gens_oracle.lncc on the float64 inputs (differentiable), means (B, S), raw (B, S, C), keep (B,))."""
    ref, src = ref.to(F64), src.to(F64)
    out = K.lncc(ref, src)
    with torch.no_grad():
        means, raw = lncc_parts(ref.detach(), src.detach())
        keep = keep_mask(means, raw, twins)
    return out, means, raw, keep


class _E:
    """A float64 value with a running bound on the error of its float32 evaluation (first order in u; the products of two operand errors are
    kept, because cross^2 of a constant patch is nothing but such a product)."""

    def __init__(self, v, e):
        self.v, self.e = v, e

    @staticmethod
    def const(c):
        return _E(torch.tensor(float(c), dtype=F64), torch.tensor(0.0, dtype=F64))

    def __add__(self, o):
        v = self.v + o.v
        return _E(v, self.e + o.e + U * v.abs())

    def __sub__(self, o):
        v = self.v - o.v
        return _E(v, self.e + o.e + U * v.abs())

    def __mul__(self, o):
        v = self.v * o.v
        return _E(v, self.e * o.v.abs() + self.v.abs() * o.e + self.e * o.e + U * v.abs())

    def __truediv__(self, o):
        v = self.v / o.v
        e = (self.e + v.abs() * o.e) / (o.v.abs() - o.e).clamp_min(1e-300) + U * v.abs()
        return _E(v, torch.where(o.e >= 0.5 * o.v.abs(), torch.full_like(e, float("inf")), e))

    def twice(self):
        return _E(2 * self.v, 2 * self.e)


def lncc_bound(ref, src):
    """Criterion (a): (B,) bound on |ncc32 - ncc64| of any float32 evaluation of the one-pass formula (docstring of this file)."""
    ref, src = ref.detach().to(F64), src.detach().to(F64)
    p, c = ref.shape[2], ref.shape[3]
    r, s = ref.permute(1, 0, 3, 2), src.permute(1, 0, 3, 2)

    def total(t, products):
        return _E(t.sum(-1), (p - 1 + products) * U * t.abs().sum(-1))
    rs, qs, rr, qq, rq = total(r, 0), total(s, 0), total(r * r, 1), total(s * s, 1), total(r * s, 1)
    np_ = _E.const(p)
    u_ref, u_src = rs / np_, qs / np_
    cross = rq - u_src * rs - u_ref * qs + u_ref * u_src * np_
    ref_var = rr - u_ref.twice() * rs + u_ref * u_ref * np_
    src_var = qq - u_src.twice() * qs + u_src * u_src * np_
    guard = _E(torch.tensor(1e-5, dtype=F64), torch.tensor(abs(float(f32(1e-5)) - 1e-5), dtype=F64))
    x = _E.const(1.0) - cross * cross / (ref_var * src_var + guard)
    mean = torch.clamp(x.v, 0.0, 2.0).mean(2)
    e_mean = x.e.sum(2) / c + c * U * mean.abs()
    e_mean = torch.where(torch.isnan(mean) | torch.isnan(e_mean), torch.zeros_like(e_mean), e_mean)      # a NaN view is ranked out, not selected
    return (e_mean.max(1)[0] + 4 * U).clamp_max(2.0)


def lncc_f32(ref, src, defect=None):
    """lncc_fwd_k in float32: the five sums over p in index order, lncc_stat's expressions in its order, lane (s, c) = (lane / C, lane % C), the
    sequential channel mean, the two smallest views with the first index winning a tie, a NaN mean ranking after every number.  -> (B, 1) tensor.
        short    the last patch sample is dropped from the sums              first2   the first two views instead of the two smallest
        min      the smallest view instead of the mean of the two smallest   lane     the view of a lane taken as lane % S instead of lane / C"""
    assert defect is None or defect in LNCC_DEFECTS
    r, q = ref.detach().numpy().astype(f32)[0], src.detach().numpy().astype(f32)
    s_count, b, p_count, c_count = q.shape
    z = np.zeros((s_count, b, c_count), f32)
    rs, qs, rr, qq, rq = z.copy(), z.copy(), z.copy(), z.copy(), z.copy()
    with np.errstate(all="ignore"):
        for p in range(p_count - 1 if defect == "short" else p_count):
            a, bb = r[None, :, p, :], q[:, :, p, :]
            rs, qs, rr, qq, rq = rs + a, qs + bb, rr + a * a, qq + bb * bb, rq + a * bb
        n = f32(p_count)
        u_ref, u_src = rs / n, qs / n
        cross = rq - u_src * rs - u_ref * qs + u_ref * u_src * n
        ref_var = rr - f32(2) * u_ref * rs + u_ref * u_ref * n
        src_var = qq - f32(2) * u_src * qs + u_src * u_src * n
        den = ref_var * src_var + f32(1e-5)
        x = f32(1) - cross * cross / den
        ncc = np.where(x < 0, f32(0), np.where(x > 2, f32(2), x)).astype(f32)             # NaN passes
        lane = np.arange(s_count * c_count)
        view = lane % s_count if defect == "lane" else lane // c_count
        row = ncc[view, :, lane % c_count].T                                              # (B, S*C): the wave's LDS row
        best0, best1 = np.full(b, 3.4e38, f32), np.full(b, 3.4e38, f32)
        numbers = np.zeros(b, np.int64)
        first2 = []
        for v in range(s_count):
            m = np.zeros(b, f32)
            for k in range(c_count):
                m = m + row[:, v * c_count + k]
            m = m / f32(c_count)
            first2.append(m)
            numbers += ~np.isnan(m)
            c0 = m < best0
            c1 = ~c0 & (m < best1)
            best1 = np.where(c0, best0, np.where(c1, m, best1))
            best0 = np.where(c0, m, best0)
        if defect == "first2":
            best0, best1 = first2[0], first2[1]
        out = best0 if defect == "min" else (best0 + best1) / f32(2)
        out = np.where(numbers < 2, f32("nan"), out).astype(f32)
    return torch.from_numpy(out)[:, None]


@functools.lru_cache(maxsize=None)
def lncc_case(shape, cls):
    """-> (ref (1, B, P, C), src (S, B, P, C)) float32, shared by the CPU and the GPU tests and never modified."""
    b, s, c, p = LNCC_SHAPES[shape]
    g = _rng(1000 + 10 * shape + LNCC_CLASSES.index(cls))
    base = torch.rand(1, b, p, c, generator=g)
    src = base * (0.5 + torch.rand(s, b, 1, c, generator=g)) + 0.3 * torch.rand(s, b, p, c, generator=g)      # as tests/test_lncc.py
    if cls == "dim":                       # the 1e-5 guard dominates: cc ~ 0, every view ties near 1
        base, src = base * 1e-3, src * 1e-3
    elif cls == "bright":                  # mean 1, contrast 0.1: sum x^2 - (sum x)^2 / P cancels three digits
        base, src = 1.0 + 0.1 * (base - 0.5), 1.0 + 0.1 * (src - 0.5)
    elif cls == "constant":                # zero variance
        base = torch.rand(1, b, 1, c, generator=g).expand(1, b, p, c).contiguous()
        src = torch.rand(s, b, 1, c, generator=g).expand(s, b, p, c).contiguous()
    elif cls == "twin":
        src[1] = src[0]
    return base, src


LNCC_NAN_KINDS = ("one-view-of-2", "one-view-of-4", "reference-patch", "all-views")


def lncc_nan_case(kind):
    """-> (ref, src, ref_clean, src_clean, ray): ray `ray` of an ordinary case with one NaN in one source view's patch (S = 2: the ray is NaN;
    S = 4: the two smallest of the other three views), one NaN in the reference patch, or one NaN in every view."""
    shape = {"one-view-of-2": 3, "one-view-of-4": 2, "reference-patch": 1, "all-views": 2}[kind]
    ref_clean, src_clean = lncc_case(shape, "ordinary")
    ref, src, ray = ref_clean.clone(), src_clean.clone(), 1
    nan = float("nan")
    if kind == "reference-patch":
        ref[0, ray, 5, 2] = nan
    elif kind == "all-views":
        src[:, ray, 7, 3] = nan
    else:
        src[1, ray, 4, 0] = nan
    return ref, src, ref_clean, src_clean, ray


def lncc_value_errors(ref, src, got):
    """got (B, 1) float32 -> dict(err (B,) against float64, bound (B,) criterion (a), e32 the restatement's worst error, bit_equal)."""
    want = lncc64(ref, src)[0][:, 0]
    rest = lncc_f32(ref, src)[:, 0]
    got = got.detach().cpu()[:, 0]
    nan = torch.isnan(want)
    err = torch.where(nan, torch.zeros_like(want), (got.double() - want).abs())
    e32 = torch.where(nan, torch.zeros_like(want), (rest.double() - want).abs())
    return dict(err=err, bound=lncc_bound(ref, src), e32=float(e32.max()), nan_equal=bool(torch.equal(torch.isnan(got), nan)),
                bit_equal=bool(torch.equal(got.view(torch.int32), rest.view(torch.int32))))


def lncc_value_ok(res):
    """Criteria (a) and (b) on the dict of lncc_value_errors.  -> (ok, text)."""
    use_a = float((res["err"] / res["bound"]).max())
    limit_b = max(4 * res["e32"], 4 * U)
    worst = float(res["err"].max())
    text = (f"worst error {worst:.2e}, (a) use {use_a:.3f} of a bound of {float(res['bound'].min()):.1e} .. {float(res['bound'].max()):.1e}, "
            f"(b) limit {limit_b:.2e} (restatement {res['e32']:.2e}), bit-equal to the restatement: {res['bit_equal']}")
    return res["nan_equal"] and use_a <= 1.0 and worst <= limit_b, text


def lncc_grads64(ref, src, cot, twins=False):
    """-> (g_ref, g_src float64, keep)."""
    r, s = ref.double().requires_grad_(True), src.double().requires_grad_(True)
    out, _, _, keep = lncc64(r, s, twins)
    g_ref, g_src = torch.autograd.grad((out * cot.double()).sum(), [r, s])
    return g_ref, g_src, keep


def lncc_grads_oracle32(ref, src, cot):
    r, s = ref.clone().requires_grad_(True), src.clone().requires_grad_(True)
    return torch.autograd.grad((K.lncc(r, s) * cot).sum(), [r, s])


def grad_error(g, g64, keep):
    """g, g64 (V, B, P, C) -> max over kept rays of max |g - g64| / max |g64| of the ray (a ray whose float64 gradient is all zero: 0 when g
    is all zero too, else inf)."""
    if not bool(keep.any()):
        return 0.0
    d = (g.detach().cpu().double() - g64).abs().permute(1, 0, 2, 3)[keep].flatten(1).max(1)[0]
    m = g64.abs().permute(1, 0, 2, 3)[keep].flatten(1).max(1)[0]
    e = torch.where(m > 0, d / m.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))
    return float(e.max())


def lncc_cot(shape):
    return torch.rand(LNCC_SHAPES[shape][0], 1, generator=_rng(77 + shape)) + 0.25


# ================================================================================================================== TV
TV_DEFECTS = ("own_count", "z_seam", "xy_swap", "weight_shift", "bwd_seam")
MAX_LEVELS = 8
# name -> (levels [(X, Y, Z)], mask kind).  Z % 4 == 0 on every level: the four-voxel forms (and, in a list, the all-levels launch) apply.
TV_CASES = {
    "v-1x1x4-ones": ([(1, 1, 4)], "ones"),
    "v-2x3x4-rand": ([(2, 3, 4)], "rand"),
    "v-3x5x8-values": ([(3, 5, 8)], "values"),
    "v-5x2x12-slab": ([(5, 2, 12)], "slab"),
    "v-4x8x32-rand": ([(4, 8, 32)], "rand"),                      # exactly 256 threads of four voxels
    "v-1x257x4-values": ([(1, 257, 4)], "values"),
    "v-2x2x260-slab": ([(2, 2, 260)], "slab"),
    "v-4x4x8-cube-rand": ([(4, 4, 8)], "rand"),                   # X = Y: the one level on which xy_swap changes nothing
    "s-3x4x7-rand": ([(3, 4, 7)], "rand"),                        # scalar form only
    "s-2x3x1-ones": ([(2, 3, 1)], "ones"),
    "s-9x5x5-values": ([(9, 5, 5)], "values"),
    "l2-rand": ([(3, 5, 8), (2, 3, 4)], "rand"),
    "l3-values": ([(2, 3, 4), (6, 5, 8), (1, 1, 4)], "values"),
    "l3-empty-middle": ([(2, 3, 4), (6, 5, 8), (3, 2, 4)], "empty1"),
    "l5-slab": ([(2, 3, 8), (7, 2, 4), (1, 6, 12), (5, 5, 4), (3, 1, 16)], "slab"),
    "l8-rand": ([(2, 3, 4), (6, 5, 8), (1, 1, 4), (3, 7, 4), (4, 2, 12), (2, 2, 4), (5, 3, 8), (1, 4, 4)], "rand"),
    "l2-mixed-forms": ([(3, 4, 7), (2, 3, 4)], "rand"),           # a scalar-form level in a list: the per-level path
}


def tv_vectorisable(levels):
    return all(z % 4 == 0 for _, _, z in levels)


@functools.lru_cache(maxsize=None)
def tv_case(name):
    """-> (vols [(1, 4, X, Y, Z)], masks [(1, 1, X, Y, Z)]) float32.  Mask values come from {0, 0.5, 1, 2} only, so m m' > 0 is the same
    decision in float32 and float64."""
    levels, kind = TV_CASES[name]
    g = _rng(sum(ord(ch) for ch in name))
    vols, masks = [], []
    for lvl, (x, y, z) in enumerate(levels):
        vols.append(torch.randn(1, 4, x, y, z, generator=g))
        if kind == "ones":
            m = torch.ones(1, 1, x, y, z)
        elif kind in ("rand", "empty1"):
            m = (torch.rand(1, 1, x, y, z, generator=g) > 0.3).float()
            if kind == "empty1" and lvl == 1:
                m = torch.zeros(1, 1, x, y, z)
        elif kind == "values":
            m = torch.tensor([0.0, 0.5, 1.0, 2.0])[torch.randint(0, 4, (1, 1, x, y, z), generator=g)]
        else:                                  # slab: ones up to and including z = 4k - 1, the last voxel of a thread of four
            m = torch.zeros(1, 1, x, y, z)
            m[..., :4 * max(1, z // 8)] = 1.0
        masks.append(m)
    return vols, masks


def tv64(vols, masks):
    """tv_regularization of the reference project in float64 (all three axes over the x-pair count).  -> (total, [tv_l])."""
    total, per_level = 0, []
    for lvl, (v, m) in enumerate(zip(vols, masks)):
        v, m = v.to(F64), m.to(F64)
        mx = (m[:, :, 1:] * m[:, :, :-1]) > 0
        my = (m[:, :, :, 1:] * m[:, :, :, :-1]) > 0
        mz = (m[..., 1:] * m[..., :-1]) > 0
        den = mx.sum().to(F64) + 1e-8
        tx = (((v[:, :, 1:] - v[:, :, :-1]) ** 2) * mx).sum() / den
        ty = (((v[:, :, :, 1:] - v[:, :, :, :-1]) ** 2) * my).sum() / den
        tz = (((v[..., 1:] - v[..., :-1]) ** 2) * mz).sum() / den
        tv_l = torch.sqrt(tx + ty + tz)
        per_level.append(tv_l)
        total = total + tv_l * 0.5 ** lvl
    return total, per_level


def tv_reference(vols, masks, cot=1.0):
    """-> dict(total, levels [float], grads [float64 (1, 4, X, Y, Z)], bounds [the per-element gradient bound 128 u coef64 A])."""
    vs = [v.double().requires_grad_(True) for v in vols]
    total, per_level = tv64(vs, masks)
    grads = torch.autograd.grad(total * cot, vs)
    bounds = []
    for lvl, (v, m, tv_l) in enumerate(zip(vols, masks, per_level)):
        v, m = v.double(), m.double()
        a = torch.zeros_like(v)
        for dim in (2, 3, 4):
            n = v.shape[dim]
            lo, hi = [slice(None)] * 5, [slice(None)] * 5
            lo[dim], hi[dim] = slice(0, n - 1), slice(1, n)
            lo, hi = tuple(lo), tuple(hi)
            t = 2 * (v[hi] - v[lo]).abs() * ((m[hi] * m[lo]) > 0)
            a[lo] += t
            a[hi] += t
        den = ((m[:, :, 1:] * m[:, :, :-1]) > 0).sum().double() + 1e-8
        tv_l = tv_l.detach()
        coef = abs(cot) * 0.5 ** lvl / (2 * tv_l * den) if float(tv_l) > 0 else torch.tensor(float("inf"), dtype=F64)
        bounds.append(torch.where(a > 0, 128 * U * coef * a, torch.zeros_like(a)))
    return dict(total=float(total.detach()), levels=[float(t.detach()) for t in per_level], grads=[g.detach() for g in grads], bounds=bounds)


def tv_value_use(got, want):
    """|got - want| in units of 64 u |want| (want = 0: 0 when got is 0, else inf)."""
    got, want = float(got), float(want)
    if want == 0.0:
        return 0.0 if got == 0.0 else float("inf")
    return abs(got - want) / (64 * U * abs(want))


def tv_grad_use(got, want, bound):
    """-> (worst |got - want| / bound over the finite reference elements (0 / 0 = 0, x / 0 = inf), NaN patterns equal)."""
    got = got.detach().cpu().double()
    nan = torch.isnan(want)
    d = torch.where(nan, torch.zeros_like(want), (got - want).abs())
    b = torch.where(nan, torch.ones_like(want), bound)
    use = torch.where(d == 0, torch.zeros_like(d), d / b)                 # d > 0, b = 0 -> inf
    return float(use.max()), bool(torch.equal(torch.isnan(got), nan))


def tv_f32(vols, masks, cot=1.0, defect=None):
    """The scalar kernels voxel by voxel in float32 (flat index i -> (ix, jy, kz), neighbours at i + Y Z, i + Z, i + 1), 256-voxel block sums in
    float32, the partials in float64, the epilogue of ops._TVLevel.  -> (total float32, [tv_l], [g_vol float32 tensors]).
        own_count     each axis divided by its own pair count               z_seam   forward: the z + 1 neighbour dropped where z % 4 == 3
        xy_swap       X and Y exchanged in the split of the flat index      weight_shift   level weight 0.5^(l + 1)
        bwd_seam      backward: the z - 1 term dropped where z % 4 == 0"""
    assert defect is None or defect in TV_DEFECTS
    total, per_level, grads = f32(0), [], []
    for lvl, (v, m) in enumerate(zip(vols, masks)):
        _, _, x, y, z = v.shape
        n = x * y * z
        v, m = v.numpy().astype(f32).reshape(4, n), m.numpy().astype(f32).reshape(n)
        i = np.arange(n)
        ex, ey = (y, x) if defect == "xy_swap" else (x, y)
        kz, jy, ix = i % z, (i // z) % ey, i // (z * ey)
        sx, sy = y * z, z

        def pair(step, has):
            j = i + step
            ok = has & (j >= 0) & (j < n)                                 # (a swapped split may point past the level: no pair there)
            j = np.clip(j, 0, n - 1)
            return ok & (m * m[j] > 0), j
        px, jxp = pair(sx, ix + 1 < x)
        py, jyp = pair(sy, jy + 1 < y)
        pz, jzp = pair(1, kz + 1 < z)
        nx, jxn = pair(-sx, ix > 0)
        ny, jyn = pair(-sy, jy > 0)
        nz, jzn = pair(-1, kz > 0)
        fz = pz & (kz % 4 != 3) if defect == "z_seam" else pz
        acc = np.zeros((3, n), f32)
        for c in range(4):
            for k, (on, j) in enumerate(((px, jxp), (py, jyp), (fz, jzp))):
                d = v[c, j] - v[c]
                acc[k] = acc[k] + np.where(on, d * d, f32(0))
        pad = (-n) % 256
        blocks = np.pad(acc, ((0, 0), (0, pad))).reshape(3, -1, 256).sum(-1, dtype=f32).astype(np.float64).sum(-1)
        counts = [float(px.sum()), float(py.sum()), float(fz.sum())]
        if defect == "own_count":
            t = sum(blocks[k] / (counts[k] + 1e-8) for k in range(3))
            den = counts[0] + 1e-8
        else:
            den = counts[0] + 1e-8
            t = (blocks[0] + blocks[1] + blocks[2]) / den
        tv_l = f32(math.sqrt(t))
        weight = 0.5 ** (lvl + 1 if defect == "weight_shift" else lvl)
        per_level.append(float(tv_l))
        total = f32(total + tv_l * f32(weight))
        with np.errstate(all="ignore"):
            coef = f32(f32(cot) * f32(weight)) / (f32(2) * tv_l * f32(den))
            if defect == "bwd_seam":
                nz = nz & (kz % 4 != 0)
            g = np.zeros((4, n), f32)
            for c in range(4):
                s = np.zeros(n, f32)
                for on, j, sign in ((px, jxp, -1), (nx, jxn, 1), (py, jyp, -1), (ny, jyn, 1), (pz, jzp, -1), (nz, jzn, 1)):
                    term = f32(2) * (v[c, j] - v[c]) if sign < 0 else f32(2) * (v[c] - v[c, j])
                    s = np.where(on, s - term if sign < 0 else s + term, s)
                g[c] = coef * s
        grads.append(torch.from_numpy(g.reshape(1, 4, x, y, z)))
    return float(total), per_level, grads


def tv_check(ref, total, levels, grads):
    """The TV criteria on one evaluation (levels / grads may be None).  -> (worst value use, worst gradient use, NaN patterns equal)."""
    use_v = tv_value_use(total, ref["total"]) if total is not None else 0.0
    if levels is not None:
        use_v = max([use_v] + [tv_value_use(a, b) for a, b in zip(levels, ref["levels"])])
    use_g, nan_ok = 0.0, True
    if grads is not None:
        for g, w, bnd in zip(grads, ref["grads"], ref["bounds"]):
            u_, ok = tv_grad_use(g, w, bnd)
            use_g, nan_ok = max(use_g, u_), nan_ok and ok
    return use_v, use_g, nan_ok


# ================================================================================================================== fused loss
LOSS_KEYS = ("loss", "color_loss", "eikonal_loss", "sparse_loss", "mfc_loss", "smooth_loss", "tv_loss", "depth_loss", "pseudo_sdf_loss",
             "pseudo_depth_loss")
LOSS_DEFECTS = ("first_stride", "no_mid", "ge_zero", "grid_b", "wrong_den", "sign_one")
LOSS_GRADS = ("color_fine", "sparse_sdf", "pseudo_sdf", "ncc", "render_depth", "gradient_error", "smooth_error", "tv_reg")
SHIPPED_WEIGHTS = (1.0, 0.1, 0.02, 1.0, 0.0005, 0.1, 0.05, 0.05)        # colour, igr, sparse, mfc, smooth, tv, pseudo_sdf, pseudo_depth
DISTINCT_WEIGHTS = (1.3, 0.11, 0.023, 0.9, 0.0007, 0.17, 0.31, 0.057)
SPARSE_SCALE = 100.0
# name -> b, n_sparse, n_pseudo (None: absent), targets, valid, and what else differs from the defaults
LOSS_CASES = {
    "b1-s1-p3000-all": dict(b=1, ns=1, npz=3000, targets="all", valid="all"),                    # n_pseudo alone sizes the backward's grid
    "b63-s1025-none": dict(b=63, ns=1025, npz=None, targets="none", valid="random"),
    "b65-s1-p1-depth-only": dict(b=65, ns=1, npz=1, targets="depth", valid="random"),
    "b1023-s1025-p300-all": dict(b=1023, ns=1025, npz=300, targets="all", valid="random", cot=1.7),
    "b1024-s1-none-allvalid": dict(b=1024, ns=1, npz=None, targets="none", valid="all", weights=SHIPPED_WEIGHTS),
    "b1025-s16000-p300-all": dict(b=1025, ns=16000, npz=300, targets="all", valid="random", cot=1.7),
    "b2500-s1025-p3000-all": dict(b=2500, ns=1025, npz=3000, targets="all", valid="random", slice_color=True),
    "b2500-s1-p1-invalid": dict(b=2500, ns=1, npz=1, targets="all", valid="none"),
    "b1025-s1025-p1-gated": dict(b=1025, ns=1025, npz=1, targets="all", valid="random", depth_targets="nonpositive"),
    "b65-s16000-pseudo-depth-float-valid": dict(b=65, ns=16000, npz=None, targets="pseudo_depth", valid="random", float_valid=True),
}


@functools.lru_cache(maxsize=None)
def loss_case(name):
    """-> dict(preds, targets, weights, scale, cot).  float32 CPU tensors; valid_mask bool (b, 1) (float with float_valid).  Every case holds
    entries with color == target, sparse_sdf == 0, pseudo_sdf == 0 and render_depth == target exactly where its sizes leave room, depth targets
    with exact zeros and negatives, and |sparse_sdf| scale up to 120."""
    spec = LOSS_CASES[name]
    b, ns, npz = spec["b"], spec["ns"], spec["npz"]
    g = _rng(sum(ord(ch) for ch in name))
    rand = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    store = rand(b, 4)
    color = store[:, :3] if spec.get("slice_color") else store[:, :3].contiguous()
    target = rand(b, 3)
    target[::7] = color[::7]
    target[1::5, 1] = color[1::5, 1]
    valid = {"all": torch.ones(b, 1, dtype=torch.bool), "none": torch.zeros(b, 1, dtype=torch.bool), "random": rand(b, 1) > 0.3}[spec["valid"]]
    if spec.get("float_valid"):
        valid = valid.float()
    sparse = torch.randn(ns, 1, generator=g) * 0.05
    sparse[3::5] = 0.0
    sparse[1::11] = torch.sign(sparse[1::11]) * (0.3 + 0.9 * rand(sparse[1::11].shape))          # |x| scale = 30 .. 120: expf underflows
    preds = dict(color_fine=color, valid_mask=valid, mid_inside_sphere=(rand(b, 1) > 0.3).float(), ncc=2.0 * rand(b, 1),
                 gradient_error=rand(()), smooth_error=rand(()), tv_reg=rand(()), sparse_sdf=sparse, render_depth=0.5 + 3.0 * rand(b))
    if npz is not None:
        pseudo = torch.randn(npz, 1, generator=g) * 0.1
        pseudo[2::9] = 0.0
        preds["pseudo_sdf"] = pseudo
    targets = dict(color=target)

    def depth_target(zero_frac):
        t = 0.5 + 3.0 * rand(b)
        gate = rand(b)
        t = torch.where(gate < zero_frac, torch.zeros(b), t)
        t = torch.where((gate >= zero_frac) & (gate < zero_frac + 0.1), -t, t)
        t[4::6] = torch.where(t[4::6] > 0, preds["render_depth"][4::6], t[4::6])
        if spec.get("depth_targets") == "nonpositive":
            t = -t.abs()
        return t
    if spec["targets"] in ("all", "pseudo_depth"):
        targets["pseudo_depth"] = depth_target(0.3)
    if spec["targets"] in ("all", "depth"):
        targets["depth"] = depth_target(0.5)
    return dict(preds=preds, targets=targets, weights=spec.get("weights", DISTINCT_WEIGHTS), scale=SPARSE_SCALE, cot=spec.get("cot", 1.0))


def _as_f32(x):
    return float(f32(x))


def loss64(preds, targets, weights, scale):
    """loss.py:24-93 of the reference project on float64 tensors, with preds["ncc"] in the place of compute_LNCC(...).  weights in the kernel's
    order (SHIPPED_WEIGHTS); they and scale are taken at their float32 values.  -> dict over LOSS_KEYS."""
    w = [_as_f32(x) for x in weights]
    scale = _as_f32(scale)
    valid = preds["valid_mask"].to(F64)
    color_loss = ((preds["color_fine"] - targets["color"]).abs() * valid).sum() / (valid.sum() + 1e-5)
    eikonal_loss = preds["gradient_error"].mean()
    sparse_loss = torch.exp(-torch.abs(preds["sparse_sdf"]) * scale).mean()
    smooth_loss = preds["smooth_error"].mean()
    tv_loss = preds["tv_reg"].mean()
    ncc_mask = valid * preds["mid_inside_sphere"]
    mfc_loss = 0.5 * ((preds["ncc"] * ncc_mask).sum(dim=0) / (ncc_mask.sum(dim=0) + 1e-8)).squeeze(-1)
    zero = torch.zeros((), dtype=F64)
    pseudo_sdf_loss = torch.abs(preds["pseudo_sdf"]).mean() if "pseudo_sdf" in preds else zero

    def masked_l1(t):
        on = (t > 0).to(F64)
        return ((preds["render_depth"] - t).abs() * on).sum() / (on.sum() + 1e-8)
    pseudo_depth_loss = masked_l1(targets["pseudo_depth"]) if "pseudo_depth" in targets else zero
    depth_loss = masked_l1(targets["depth"]) if "depth" in targets else zero
    loss = (color_loss * w[0] + eikonal_loss * w[1] + sparse_loss * w[2] + mfc_loss * w[3] + smooth_loss * w[4] + tv_loss * w[5]
            + pseudo_sdf_loss * w[6] + pseudo_depth_loss * w[7])
    return {"loss": loss, "color_loss": color_loss, "eikonal_loss": eikonal_loss, "sparse_loss": sparse_loss, "mfc_loss": mfc_loss,
            "smooth_loss": smooth_loss, "tv_loss": tv_loss, "depth_loss": depth_loss, "pseudo_sdf_loss": pseudo_sdf_loss,
            "pseudo_depth_loss": pseudo_depth_loss}


def loss_reference(case):
    """-> dict(out {key: float}, grads {name: float64 tensor of d (cot loss) / d preds[name]; zeros where loss does not depend on it},
    out_bound {key: absolute bound}, grad_bound {name: element-wise bound})."""
    preds = {k: (v.double() if v.dtype != torch.bool else v) for k, v in case["preds"].items()}
    targets = {k: v.double() for k, v in case["targets"].items()}
    names = [k for k in LOSS_GRADS if k in preds]
    for k in names:
        preds[k] = preds[k].clone().requires_grad_(True)
    out = loss64(preds, targets, case["weights"], case["scale"])
    grads = torch.autograd.grad(out["loss"] * case["cot"], [preds[k] for k in names], allow_unused=True)
    grads = {k: (torch.zeros_like(preds[k]) if gr is None else gr).detach() for k, gr in zip(names, grads)}
    w = [_as_f32(x) for x in case["weights"]]
    scale = _as_f32(case["scale"])
    b = preds["color_fine"].shape[0]
    x = preds["sparse_sdf"].detach().abs() * scale
    ns = x.numel()
    expf_extra = float((U * x * torch.exp(-x)).mean()) + FLT_MIN
    rel = lambda n: 2 * (math.ceil(n / 1024) + 30) * U  # noqa: E731
    val = {k: float(v.detach()) for k, v in out.items()}
    length = {"color_loss": b, "mfc_loss": b, "depth_loss": b, "pseudo_depth_loss": b, "sparse_loss": ns,
              "pseudo_sdf_loss": preds["pseudo_sdf"].numel() if "pseudo_sdf" in preds else 1}
    out_bound = {k: rel(n) * abs(val[k]) for k, n in length.items()}
    out_bound["sparse_loss"] += expf_extra
    for k in ("eikonal_loss", "smooth_loss", "tv_loss"):
        out_bound[k] = 0.0
    order = ("color_loss", "eikonal_loss", "sparse_loss", "mfc_loss", "smooth_loss", "tv_loss", "pseudo_sdf_loss", "pseudo_depth_loss")
    out_bound["loss"] = rel(max(length.values())) * sum(abs(wk * val[k]) for wk, k in zip(w, order)) + abs(w[2]) * expf_extra
    grad_bound = {k: 32 * U * gr.abs() for k, gr in grads.items()}
    flush = FLT_MIN * (1 + abs(case["cot"] * w[2] * scale / ns))
    grad_bound["sparse_sdf"] = torch.where(grads["sparse_sdf"] != 0, grad_bound["sparse_sdf"] + U * x * grads["sparse_sdf"].abs() + flush,
                                           torch.zeros_like(x))
    return dict(out=val, grads=grads, out_bound=out_bound, grad_bound=grad_bound)


def _use(d, bound):
    """d / bound element-wise with 0 / 0 = 0 and x / 0 = inf.  -> the largest."""
    d, bound = torch.as_tensor(d, dtype=F64), torch.as_tensor(bound, dtype=F64)
    use = torch.where(d == 0, torch.zeros_like(d), d / bound)
    return float(use.max()) if use.numel() else 0.0


def loss_check(ref, out, grads):
    """out {key: number}, grads {name: tensor or None (= zeros)}.  -> (worst term use, worst gradient use, text of the worst of each)."""
    uses = {k: _use(abs(float(out[k]) - ref["out"][k]), ref["out_bound"][k]) for k in LOSS_KEYS}
    g_uses = {}
    for k, want in ref["grads"].items():
        got = grads.get(k)
        got = torch.zeros_like(want) if got is None else got.detach().cpu().double().reshape(want.shape)
        g_uses[k] = _use((got - want).abs(), ref["grad_bound"][k])
    kv, kg = max(uses, key=uses.get), max(g_uses, key=g_uses.get)
    return uses[kv], g_uses[kg], f"worst term use {uses[kv]:.3f} ({kv}), worst gradient use {g_uses[kg]:.3f} ({kg})"


def _wave_tree(x):
    """(..., 64) float32 -> (...,): a balanced tree, six steps."""
    while x.shape[-1] > 1:
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def _strided_sum32(terms, first_stride=False):
    """loss_fwd_k's sum of a float32 vector: thread t adds elements t, t + 1024, ... in turn, the wave sums, then the 16 wave totals in turn."""
    terms = terms.astype(f32).reshape(-1)
    rows = np.pad(terms, (0, (-terms.size) % 1024)).reshape(-1, 1024)
    acc = np.zeros(1024, f32)
    for row in (rows[:1] if first_stride else rows):
        acc = acc + row
    waves = _wave_tree(acc.reshape(16, 64))
    tot = f32(0)
    for wv in waves:
        tot = f32(tot + wv)
    return tot


def loss_f32(case, defect=None):
    """loss_fwd_k / loss_bwd_k in float32.  -> (out {key: float32}, grads {name: float32 tensor}).
        first_stride   only rays < 1024 are summed                       no_mid     the mfc mask ignores mid_inside_sphere
        ge_zero        the depth gate is t >= 0                           grid_b     the backward writes g_pseudo / g_sparse only for i < b
        wrong_den      the pseudo-depth gradient divides by the depth target's count            sign_one   sign(0) = +1"""
    assert defect is None or defect in LOSS_DEFECTS
    p, t = case["preds"], case["targets"]
    a = lambda x: x.detach().numpy().astype(f32).reshape(-1)  # noqa: E731
    w = [f32(x) for x in case["weights"]]
    scale, g_up = f32(case["scale"]), f32(case["cot"])
    color, target = p["color_fine"].detach().numpy().astype(f32), t["color"].numpy().astype(f32)
    b = color.shape[0]
    v = (a(p["valid_mask"]) != 0).astype(f32)
    mid = np.ones(b, f32) if defect == "no_mid" else a(p["mid_inside_sphere"])
    ncc, depth = a(p["ncc"]), a(p["render_depth"])
    fs = defect == "first_stride"
    sgn = (lambda x: np.where(x >= 0, f32(1), f32(-1))) if defect == "sign_one" else (lambda x: np.sign(x).astype(f32))
    gate = (lambda x: x >= 0) if defect == "ge_zero" else (lambda x: x > 0)
    diff = color - target
    tot0 = _strided_sum32((np.abs(diff[:, 0]) + np.abs(diff[:, 1]) + np.abs(diff[:, 2])) * v, fs)
    tot1 = _strided_sum32(v, fs)
    m = v * mid
    tot2, tot3 = _strided_sum32(ncc * m, fs), _strided_sum32(m, fs)
    out = {}
    out["color_loss"] = tot0 / f32(tot1 + f32(1e-5))
    out["mfc_loss"] = f32(0.5) * (tot2 / f32(tot3 + f32(1e-8)))
    dens = {}
    for key, name in (("pseudo_depth_loss", "pseudo_depth"), ("depth_loss", "depth")):
        if name in t:
            tt = a(t[name])
            on = gate(tt).astype(f32)
            dens[name] = f32(_strided_sum32(on, fs) + f32(1e-8))
            out[key] = _strided_sum32(np.abs(depth - tt) * on, fs) / dens[name]
        else:
            out[key] = f32(0)
    sp = a(p["sparse_sdf"])
    with np.errstate(under="ignore"):
        e = np.exp(-np.abs(sp) * scale).astype(f32)
    out["sparse_loss"] = _strided_sum32(e) / f32(sp.size)
    ps = a(p["pseudo_sdf"]) if "pseudo_sdf" in p else None
    out["pseudo_sdf_loss"] = _strided_sum32(np.abs(ps)) / f32(ps.size) if ps is not None else f32(0)
    out["eikonal_loss"], out["smooth_loss"], out["tv_loss"] = (f32(float(p[k])) for k in ("gradient_error", "smooth_error", "tv_reg"))
    loss = f32(out["color_loss"] * w[0])
    for k, wk in zip(("eikonal_loss", "sparse_loss", "mfc_loss", "smooth_loss", "tv_loss", "pseudo_sdf_loss", "pseudo_depth_loss"), w[1:]):
        loss = f32(loss + f32(out[k] * wk))
    out["loss"] = loss
    grads = {"gradient_error": torch.tensor(g_up * w[1]), "smooth_error": torch.tensor(g_up * w[4]), "tv_reg": torch.tensor(g_up * w[5])}
    with np.errstate(all="ignore"):
        k_col = g_up * w[0] * v / f32(tot1 + f32(1e-5))
        grads["color_fine"] = torch.from_numpy((k_col[:, None] * sgn(diff)).astype(f32))
        grads["ncc"] = torch.from_numpy((g_up * w[3] * f32(0.5) * v * mid / f32(tot3 + f32(1e-8))).astype(f32)[:, None])
        gd = np.zeros(b, f32)
        if "pseudo_depth" in t:
            tt = a(t["pseudo_depth"])
            den = dens["depth"] if (defect == "wrong_den" and "depth" in dens) else dens["pseudo_depth"]
            gd = np.where(gate(tt), g_up * w[7] * sgn(depth - tt) / den, f32(0)).astype(f32)
        grads["render_depth"] = torch.from_numpy(gd)
        gs = (g_up * w[2] * (-scale * sgn(sp) * e) / f32(sp.size)).astype(f32)
        if defect == "grid_b":
            gs[b:] = 0
        grads["sparse_sdf"] = torch.from_numpy(gs)[:, None]
        if ps is not None:
            gp = (g_up * w[6] * sgn(ps) / f32(ps.size)).astype(f32)
            if defect == "grid_b":
                gp[b:] = 0
            grads["pseudo_sdf"] = torch.from_numpy(gp)[:, None]
    return {k: float(x) for k, x in out.items()}, grads
