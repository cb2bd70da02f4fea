"""A float64 restatement of one importance-sampling round, up_sample + sample_pdf(det=True) (implicit_surface.py:60-109, 14-44; K5/K6,
upsample_core in k5_rays.hip), with a running error bound, for the ray-sampling tests.

The operation is ill-conditioned in float32: c_prev - c_next + 1e-5 cancels, and on rays that miss the surface the sum of the weights is about
n 1e-5, so the division by it magnifies the cancellation error (two correct float32 evaluations differ by 1e-3 in z_new on such rays).  No flat
tolerance on z_new is both safe and sharp.  What a correct float32 evaluation CAN be held to is a bracket in the CDF domain:

    reference   cdf64[0..n-1], the float64 CDF knots of a ray, and e_cdf[j], a first-order running error bound on each knot that covers any float32
                evaluation in any association order (u = 2^-24): every operation contributes the propagated input error plus u |result|, the sigmoid
                max sigma' over [x - e_x, x + e_x] e_x + 4u sigma, the prefix product the absolute recursion
                e_T[j+1] = e_T[j] |fac_j| + |T_j| e_fac[j] + u |T_{j+1}|, sums (number of terms) u |sum|.  The discrete decisions -- per-sample
                validity vm and the per-sample rad < 1 flags -- are INPUTS, so kernel and reference cannot disagree on a mask voxel or on the unit
                sphere.  delta = max_j e_cdf[j] + 4u (the 4u: the float32 quantile grid against the exact (k + 1/2) / n_new).
    inverse     Z(v): the float64 map CDF value -> z with the same searchsorted(right=True), the same lo / hi clamps and the same den < 1e-5 -> 1
                rule.  Z-(v) / Z+(v): in bins whose float64 width satisfies |den - 1e-5| <= e_cdf[lo] + e_cdf[hi] a float32 evaluation may take
                either side of the rule; there Z- takes the smaller of the two branch values and Z+ the larger.
    bracket     kernel and reference interpolate over the same abscissae z_j and their knots differ by at most delta, so a correct z_new satisfies
                    Z-(u - delta) - 4 ulp(z)  <=  z_new  <=  Z+(u + delta) + 4 ulp(z),          u +- delta clamped to [0, 1].
                Why: let c' be the evaluation's knots, (lo', hi') its bin for its quantile u' (so c'[lo'] <= u' < c'[hi'] unless lo' = n - 1).
                c[lo'] <= c'[lo'] + e <= u + delta, so the reference's bin for u + delta starts at lo >= lo'.  If lo > lo': z_new <= z[hi'] <= z[lo]
                <= Z+.  If lo = lo', same bin: with both on the linear branch the two piecewise-linear CDFs differ by at most delta on the bin, so
                F(z_new) <= u + delta and z_new <= F^-1(u + delta); with the evaluation on the den -> 1 branch its t = u' - c'[lo'] is at most
                (u + delta - c[lo]) / den for den <= 1; an evaluation on the linear branch while the reference is on the other one happens only in
                the ambiguous bins, where Z+ takes the larger value.  The lower side mirrors this.  The only slack is inside bins of negligible
                probability and is at most one sample gap; no sample is excluded.
    generator   three ray classes (make_case): `hit` aimed at a noisy sphere SDF of radius 0.55 with the first sign change of ray r PLACED at
                segment r mod (n - 1) (so segments 62..65, the hand-over between a lane's two register slots, each carry a surface whenever they
                exist), `holes` = hit with 15 % of the mask voxels cleared plus one ray with no valid sample at all, `miss` tangent to radius 1.05.
    upsample_f32   the same formulas in float32 (numpy; sequential cumprod / cumsum) with four seeded defects of the kind a two-slot kernel can
                have, to show that the bracket notices them.
"""
import functools

import numpy as np
import torch

from oracle import gens_oracle as K

U = 2.0 ** -24
F64 = torch.float64
C5 = float(np.float32(1e-5))          # the constants as float32 holds them (torch and the kernels add float32 scalars)
C7 = float(np.float32(1e-7))

# (n, n_new, inv_s): below, at and above the 64-sample slot boundary, both ends of n and n_new, sharp and soft sigmoids
SHAPES = ((2, 1, 64.0), (3, 2, 64.0), (63, 16, 64.0), (64, 16, 64.0), (65, 16, 64.0), (66, 17, 128.0), (96, 33, 256.0), (127, 63, 512.0),
          (128, 64, 1024.0), (128, 16, 1e4), (65, 64, 3000.0))
CLASSES = ("hit", "holes", "miss")
DEFECTS = ("prev_cos_64", "trans_upper", "cdf_upper", "bin_off_by_one")


def defect_applies(defect, n):
    """(a) to (c) need a segment in the upper slots (n >= 66); (d) applies everywhere."""
    return n >= 66 or defect == "bin_off_by_one"


# ---------------------------------------------------------------------------------------------------------------- float64 reference + bound
def _sigmoid_err(x, e_x):
    s = torch.sigmoid(x)
    m = (x.abs() - e_x).clamp_min(0.0)                 # sigma' = sigma (1 - sigma) falls with |x|: its maximum over [x - e_x, x + e_x]
    sm = torch.sigmoid(m)
    return s, sm * (1.0 - sm) * e_x + 4.0 * U * s


def reference(z, sdf, vm, rad_lt1, inv_s):
    """z, sdf (B, n) float32 values; vm (B, n) validity, rad_lt1 (B, n) bool, the decisions of the evaluation under test.
    -> dict(z (B, n) float64, cdf (B, n), e_cdf (B, n), delta (B,))."""
    z, sdf, vm = z.to(F64), sdf.to(F64), (vm.to(F64) > 0)
    rad_lt1 = rad_lt1.bool()
    b, n = z.shape
    inv_s = float(np.float32(inv_s))
    ins = ((rad_lt1[:, :-1] | rad_lt1[:, 1:]) & vm[:, :-1] & vm[:, 1:]).to(F64)
    dz = z[:, 1:] - z[:, :-1]
    e_dz = U * dz.abs()
    ssum = sdf[:, :-1] + sdf[:, 1:]
    mid = ssum * 0.5
    e_mid = U * mid.abs()
    num = sdf[:, 1:] - sdf[:, :-1]
    e_num = U * num.abs()
    den = dz + C5
    e_den = e_dz + U * den.abs()
    cos = num / den
    e_cos = e_num / den.abs() + num.abs() * e_den / den ** 2 + U * cos.abs()
    zero = torch.zeros(b, 1, dtype=F64)
    prev, e_prev = torch.cat([zero, cos[:, :-1]], -1), torch.cat([zero, e_cos[:, :-1]], -1)
    c = torch.minimum(prev, cos)
    e_c = torch.maximum(e_prev, e_cos)                 # min and clamp are 1-Lipschitz in the sup norm
    settled = (c - e_c > 0.0) | (c + e_c < -1e3)       # wholly inside a clamped range: the clamp's value, exactly
    c = c.clamp(-1e3, 0.0) * ins
    e_c = torch.where(settled, torch.zeros_like(e_c), e_c) * ins
    half = c * dz * 0.5
    e_half = e_c * dz.abs() * 0.5 + c.abs() * e_dz * 0.5 + U * half.abs()
    cs, e_cs = [], []
    for sign in (-1.0, 1.0):                           # e_prev = mid - c dz / 2, e_next = mid + c dz / 2
        est = mid + sign * half
        e_est = e_mid + e_half + U * est.abs()
        x = est * inv_s
        e_x = e_est * inv_s + U * x.abs()
        s, e_s = _sigmoid_err(x, e_x)
        cs.append(s)
        e_cs.append(e_s)
    (c_prev, c_next), (e_cp, e_cn) = cs, e_cs
    d = c_prev - c_next
    e_d = e_cp + e_cn + U * d.abs()
    q = d + C5
    e_q = e_d + U * q.abs()
    p = c_prev + C5
    e_p = e_cp + U * p.abs()
    alpha = q / p
    e_alpha = e_q / p.abs() + q.abs() * e_p / p ** 2 + U * alpha.abs()
    one_m = 1.0 - alpha
    fac = one_m + C7
    e_fac = e_alpha + U * one_m.abs() + U * fac.abs()
    trans, e_trans = torch.ones(b, n - 1, dtype=F64), torch.zeros(b, n - 1, dtype=F64)
    for j in range(n - 2):                             # T_0 = 1; the absolute recursion is, to first order, independent of the scan order
        trans[:, j + 1] = trans[:, j] * fac[:, j]
        e_trans[:, j + 1] = e_trans[:, j] * fac[:, j].abs() + trans[:, j].abs() * e_fac[:, j] + U * trans[:, j + 1].abs()
    at = alpha * trans
    w = at + C5
    e_w = e_alpha * trans.abs() + alpha.abs() * e_trans + U * at.abs() + U * w.abs()
    total = w.sum(-1, keepdim=True)
    e_total = e_w.sum(-1, keepdim=True) + (n - 1) * U * total.abs()
    pdf = w / total
    e_pdf = e_w / total.abs() + w.abs() * e_total / total ** 2 + U * pdf.abs()
    cdf = torch.cat([zero, torch.cumsum(pdf, -1)], -1)
    terms = torch.arange(n, dtype=F64)[None]
    e_cdf = torch.cat([zero, torch.cumsum(e_pdf, -1)], -1) + terms * U * cdf.abs()
    return dict(z=z, cdf=cdf, e_cdf=e_cdf, delta=e_cdf.max(-1)[0] + 4.0 * U)


def quantiles(n_new):
    return (torch.arange(n_new, dtype=F64) + 0.5) / n_new


def inverse(ref, v, side=0):
    """v (B, m) CDF values -> z (B, m): Z (side 0), Z- (side -1) or Z+ (side +1)."""
    z, cdf, e_cdf = ref["z"], ref["cdf"], ref["e_cdf"]
    n = z.shape[1]
    v = v.clamp(0.0, 1.0)
    cnt = torch.searchsorted(cdf, v.contiguous(), right=True)
    lo, hi = (cnt - 1).clamp_min(0), cnt.clamp_max(n - 1)
    c_lo, c_hi = cdf.gather(1, lo), cdf.gather(1, hi)
    b_lo, b_hi = z.gather(1, lo), z.gather(1, hi)
    den = c_hi - c_lo
    t_rule = v - c_lo                                                     # den < 1e-5 -> den = 1
    t_lin = (v - c_lo) / torch.where(den > 0, den, torch.ones_like(den))
    rule = den < C5
    t = torch.where(rule, t_rule, t_lin)
    if side:
        amb = (den - C5).abs() <= e_cdf.gather(1, lo) + e_cdf.gather(1, hi) + 1e-12
        both = torch.maximum(t_rule, t_lin) if side > 0 else torch.minimum(t_rule, t_lin)
        t = torch.where(amb, both, t)
    out = b_lo + t * (b_hi - b_lo)
    if side > 0:
        out = torch.where(v >= 1.0, z[:, -1:].expand_as(out), out)
    if side < 0:
        out = torch.where(v <= 0.0, z[:, :1].expand_as(out), out)
    return out


def bracket(ref, n_new):
    """-> (lower, centre, upper), each (B, n_new): a correct float32 z_new lies in [lower, upper]; centre = Z(u)."""
    u = quantiles(n_new)[None].expand(ref["z"].shape[0], -1)
    d = ref["delta"][:, None]
    slack = 4.0 * torch.from_numpy(np.spacing(ref["z"].abs().max(-1)[0].numpy().astype(np.float32)).astype(np.float64))[:, None]
    return inverse(ref, u - d, -1) - slack, inverse(ref, u, 0), inverse(ref, u + d, +1) + slack


def bracket_use(ref, z_new):
    """z_new (B, n_new) -> (B, n_new): the distance past Z(u) in units of the bracket's half-width on that side; > 1 is outside."""
    z_new = z_new.detach().cpu().to(F64)
    lower, centre, upper = bracket(ref, z_new.shape[1])
    above = z_new >= centre
    width = torch.where(above, upper - centre, centre - lower)
    return (z_new - centre).abs() / width


# ---------------------------------------------------------------------------------------------------------------- inputs
def _unit(v):
    return v / torch.linalg.norm(v, dim=-1, keepdim=True)


def make_case(cls, n_rays, n, seed, inv_s=64.0):
    """inv_s: the sharpness the case will be sampled at; in every second pass of the placed crossing over the segments (rays with
    (r // (n - 1)) odd) the SDF is scaled by 64 / inv_s, so that at sharp sigmoids too some rays spread their weight over the segments around
    the surface (as the samples of a late round do, which lie that much closer together) instead of putting all of it on one.
    -> dict(ro, rd (B, 3), z, sdf (B, n) float32, masks [(1, 1, X, X, X) float32], vm (B, n) bool = K.point_valid(masks, o + d z) in float32,
    rad_lt1 (B, n) bool, cross (B,) the placed segment, or None for `miss`)."""
    assert cls in CLASSES and n >= 2
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=F64)  # noqa: E731
    b = n_rays
    z = torch.sort(rnd(b, n) * 2.2 + 1.1, -1)[0].float()
    pair_ray, pair_at = min(2, b - 1), min(63, n - 2)                    # one pair of equal neighbours per case, across the slots where it can be
    z[pair_ray, pair_at + 1] = z[pair_ray, pair_at]
    rows = torch.arange(b)
    cross = rows % (n - 1)
    zc = 0.5 * (z[rows, cross].double() + z[rows, cross + 1].double())
    if cls == "miss":
        off = torch.full((b,), 1.05, dtype=F64)
        zm = 2.2 + (rnd(b) - 0.5)
    else:
        off = 0.4 * rnd(b)                                                # the sphere of radius 0.55 is entered at z = zc
        zm = zc + torch.sqrt(0.55 ** 2 - off ** 2)
    d = _unit(torch.randn(b, 3, generator=g, dtype=F64))
    e = _unit(torch.linalg.cross(d, torch.randn(b, 3, generator=g, dtype=F64)))
    ro, rd = (-zm[:, None] * d + off[:, None] * e).float(), d.float()

    def radius(zz):
        return torch.linalg.norm(ro.double()[:, None] + rd.double()[:, None] * zz.double()[..., None], dim=-1)

    for _ in range(50):                                                   # no sample within 1e-5 of the unit sphere: redraw between its neighbours
        near = (radius(z) - 1.0).abs() < 1e-5
        if not bool(near.any()):
            break
        left = torch.cat([torch.full((b, 1), 1.1), z[:, :-1]], -1)
        right = torch.cat([z[:, 1:], torch.full((b, 1), 3.3)], -1)
        z = torch.where(near, (left.double() + (right - left).double() * rnd(b, n)).float(), z)
        z[pair_ray, pair_at + 1] = z[pair_ray, pair_at]
    rad = radius(z)
    assert not bool(((rad - 1.0).abs() < 1e-5).any()) and bool((z[:, 1:] >= z[:, :-1]).all())
    noise = 1.0 + 0.25 * torch.randn(b, n, generator=g, dtype=F64).clamp(-2.0, 2.0)
    sdf = (rad - 0.55) * noise
    soft = ((rows // (n - 1)) % 2 == 1).to(F64) * (min(1.0, 64.0 / inv_s) - 1.0) + 1.0
    sdf = sdf * soft[:, None]
    if cls != "miss":                                                     # the first sign change, placed: + up to sample `cross`, - right behind it
        j = torch.arange(n)[None]
        mag = sdf.abs().clamp_min(1e-4)
        sdf = torch.where(j <= cross[:, None], mag, torch.where(j == cross[:, None] + 1, -mag, sdf))
    sdf = sdf.float()
    pts = (ro[:, None] + rd[:, None] * z[..., None]).reshape(-1, 3)       # float32, as the oracle forms them
    if cls == "holes":
        fine = (torch.rand(1, 1, 32, 32, 32, generator=g) > 0.15).float()
        size = torch.tensor([32.0, 32.0, 32.0])
        dead = pts.reshape(b, n, 3)[b - 1]
        idx = torch.round(((dead + 1) * size - 1) / 2)
        idx = idx[((idx >= 0) & (idx < size)).all(-1)].long()
        fine[0, 0, idx[:, 0], idx[:, 1], idx[:, 2]] = 0.0                 # the last ray: no valid sample at all
        masks = [fine, torch.zeros(1, 1, 8, 8, 8)]
    else:
        masks = [torch.ones(1, 1, 16, 16, 16), torch.ones(1, 1, 8, 8, 8)]
    vm = K.point_valid(masks, pts).reshape(b, n)
    if cls == "holes":
        assert not bool(vm[b - 1].any())
    return dict(ro=ro, rd=rd, z=z, sdf=sdf, masks=masks, vm=vm, rad_lt1=rad < 1.0, cross=None if cls == "miss" else cross)


def case_reference(c, inv_s):
    return reference(c["z"], c["sdf"], c["vm"], c["rad_lt1"], inv_s)


@functools.lru_cache(maxsize=None)
def shape_case(shape, cls, n_rays=None):
    """The case of SHAPES[shape] and ray class cls that the CPU and the GPU tests share (computed once, never modified): 255 or 257 rays, so
    that the last workgroup of four waves has idle ones.  -> (case, reference)."""
    n, _, inv_s = SHAPES[shape]
    c = make_case(cls, n_rays or (255, 257)[shape % 2], n, seed=100 * shape + CLASSES.index(cls), inv_s=inv_s)
    return c, case_reference(c, inv_s)


# ---------------------------------------------------------------------------------------------------------------- float32 restatement
def upsample_f32(z, sdf, vm, rad_lt1, n_new, inv_s, defect=None):
    """The same formulas in float32, sequential cumprod / cumsum.  -> (z_new (B, n_new), cdf (B, n)) float32 tensors.  defect: one of DEFECTS:
        prev_cos_64      the previous cosine of segment 64 taken as 0            (next2 / prev2 across lanes 63 and 64)
        trans_upper      the transmittance of slots >= 64 without factor 63      (excl_cumprod2's carry)
        cdf_upper        the CDF of slots >= 64 without the lower half's total   (the scan's carry, the LDS writes at lane + 65)
        bin_off_by_one   the bin index off by one                                (the search)"""
    assert defect is None or defect in DEFECTS
    f = np.float32
    z, sdf = z.numpy().astype(f), sdf.numpy().astype(f)
    vm, rad_lt1 = vm.numpy() > 0, rad_lt1.numpy().astype(bool)
    b, n = z.shape
    inv_s, c5, c7 = f(inv_s), f(1e-5), f(1e-7)
    ins = ((rad_lt1[:, :-1] | rad_lt1[:, 1:]) & vm[:, :-1] & vm[:, 1:]).astype(f)
    dz = z[:, 1:] - z[:, :-1]
    mid = (sdf[:, :-1] + sdf[:, 1:]) * f(0.5)
    cos = (sdf[:, 1:] - sdf[:, :-1]) / (dz + c5)
    prev = np.concatenate([np.zeros((b, 1), f), cos[:, :-1]], -1)
    if defect == "prev_cos_64" and n - 1 > 64:
        prev[:, 64] = 0
    c = np.clip(np.minimum(prev, cos), f(-1e3), f(0)) * ins
    with np.errstate(over="ignore"):
        sig = lambda x: f(1) / (f(1) + np.exp(-x))  # noqa: E731
        c_prev, c_next = sig((mid - c * dz * f(0.5)) * inv_s), sig((mid + c * dz * f(0.5)) * inv_s)
    alpha = (c_prev - c_next + c5) / (c_prev + c5)
    fac = f(1) - alpha + c7
    trans = np.ones((b, n - 1), f)
    for j in range(n - 2):
        trans[:, j + 1] = trans[:, j] * fac[:, j]
    if defect == "trans_upper" and n - 1 > 64:
        upper = np.ones((b, n - 1 - 64), f)                               # slots 64..: the product of factors 0..62 and 64..j-1
        upper[:, 0] = trans[:, 63]
        for j in range(64, n - 2):
            upper[:, j - 63] = upper[:, j - 64] * fac[:, j]
        trans[:, 64:] = upper
    w = alpha * trans + c5
    total = np.zeros(b, f)
    for j in range(n - 1):
        total = total + w[:, j]
    pdf = w / total[:, None]
    cdf = np.zeros((b, n), f)
    for j in range(n - 1):
        cdf[:, j + 1] = cdf[:, j] + pdf[:, j]
    if defect == "cdf_upper" and n - 1 > 64:
        cdf[:, 65:] = cdf[:, 65:] - cdf[:, 64:65]
    if n_new == 1:
        u = np.full(1, 0.5, f)
    else:
        u = np.linspace(0.5 / n_new, 1 - 0.5 / n_new, n_new).astype(f)
    cnt = (cdf[:, None, :] <= u[None, :, None]).sum(-1)                   # searchsorted(right=True); counts, so an unsorted row cannot derail it
    if defect == "bin_off_by_one":
        cnt = cnt + 1
    lo, hi = np.maximum(cnt - 1, 0), np.minimum(cnt, n - 1)
    lo = np.minimum(lo, n - 1)
    take = lambda a, i: np.take_along_axis(a, i, -1)  # noqa: E731
    den = take(cdf, hi) - take(cdf, lo)
    den = np.where(den < c5, f(1), den)
    t = (u[None] - take(cdf, lo)) / den
    z_new = take(z, lo) + t * (take(z, hi) - take(z, lo))
    return torch.from_numpy(z_new.astype(f)), torch.from_numpy(cdf)
