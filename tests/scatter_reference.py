"""A float64 restatement of the volume-gradient scatters, for the scatter tests.

    axis_cell   a point's cell and weights on one axis, formed in float32 exactly as the kernels form them (axis_cell in k2_lookup.hip, its copy
                in sdf_train_scatter_k): pos = (x + 1) / 2 * (size - 1), f = floor(pos) clamped to [-2, size + 1], w0 = (f + 1) - pos, w1 = pos - f
    scatter     every touched entry of every level's gradient with its float64 sum S, its absolute sum A (every product term counted on its own)
                and its contribution count k, for
                    K2 first order       f = g_out                       dV[c] += w g_out[c]
                    K2 second order      s_bar = gg_pts, mu = g_out      dV[c] += (grad_p w . gg_pts) g_out[c]
                    K17                  f, s_bar, mu, g_bar, lam        dV[c] += w f[c] + (grad_p w . s_bar) mu[c] + (grad_p w . g_bar) lam[c]
                in the planar (4, X, Y, Z) or packed (X, Y, Z, 4) layout, with an optional index map (row -> point) and live-row count
    bound       (k + 8) 2^-24 A: the worst case of summing k float32 terms of a few roundings each, in any order

Weights are the kernels' float32 values (at 256 cells float64 un-normalisation would move them by up to 255 * 2^-24); everything after them is
float64.  At an integer position the floor cell is taken and an out-of-range corner dropped (ATen's convention); a NaN point, or one beyond the
clamp, adds nothing.  The work is sparse: flat entry indices, torch.unique and index_add_ -- no dense float64 copy of a level.
"""
import torch

U = 2.0 ** -24
PLANAR, PACKED = 0, 1


def axis_cell(x, size):
    """x (n,) -> (i0 int64, w0 float64, w1 float64, live bool): the kernels' float32 cell on an axis of `size` voxels; live is False for NaN."""
    x = x.to(torch.float32)
    pos = (x + 1.0) / 2.0 * float(size - 1)
    live = ~torch.isnan(pos)
    f = torch.floor(torch.where(live, pos, torch.zeros_like(pos))).clamp(-2.0, float(size + 1))
    w0 = (f + 1.0) - pos
    w1 = pos - f
    return f.to(torch.int64), w0.double(), w1.double(), live


def _corner_terms(pts, size, f, s_bar, mu, g_bar, lam):
    """One level: -> (lin (m,), channel-free coefficient rows) of every (point, corner) inside the volume; terms (m, 4) and |terms| (m, 4)."""
    cells = [axis_cell(pts[:, ax], size[ax]) for ax in range(3)]
    half = [(s - 1) / 2.0 for s in size]                                    # d pos / d x, exact in float64
    lins, terms, absol = [], [], []
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                corner = (a, b, c)
                idx = [cells[ax][0] + corner[ax] for ax in range(3)]
                ok = cells[0][3] & cells[1][3] & cells[2][3]
                for ax in range(3):
                    ok = ok & (idx[ax] >= 0) & (idx[ax] < size[ax])
                rows = torch.nonzero(ok)[:, 0]
                w = [(cells[ax][2] if corner[ax] else cells[ax][1])[rows] for ax in range(3)]
                lin = (idx[0][rows] * size[1] + idx[1][rows]) * size[2] + idx[2][rows]
                sign = [1.0 if corner[ax] else -1.0 for ax in range(3)]
                dw = [sign[0] * half[0] * w[1] * w[2], w[0] * sign[1] * half[1] * w[2], w[0] * w[1] * sign[2] * half[2]]
                t = torch.zeros(rows.numel(), 4, dtype=torch.float64, device=pts.device)
                ab = torch.zeros_like(t)
                if f is not None:
                    p = (w[0] * w[1] * w[2])[:, None] * f[rows]
                    t, ab = t + p, ab + p.abs()
                for vec, cot in ((s_bar, mu), (g_bar, lam)):
                    if vec is None or cot is None:
                        continue
                    v = vec[rows]
                    parts = [dw[ax] * v[:, ax] for ax in range(3)]
                    # the coefficient first, then the cotangent: an infinite cotangent on a zero coefficient is NaN, as in the kernels
                    t = t + (parts[0] + parts[1] + parts[2])[:, None] * cot[rows]
                    ab = ab + sum(p_.abs() for p_ in parts)[:, None] * cot[rows].abs()
                lins.append(lin)
                terms.append(t)
                absol.append(ab)
    return torch.cat(lins), torch.cat(terms), torch.cat(absol)


def scatter(pts, dims, layout=PLANAR, f=None, s_bar=None, mu=None, g_bar=None, lam=None, index=None, count=None):
    """pts (P, 3); dims [(X, Y, Z)] per level; f / mu / lam (R, L, 4) per row and level; s_bar / g_bar (P, 3) per point; index (R,) row -> point
    (None: row i is point i); count: rows at and past it add nothing.  -> per level (entries int64, S float64, A float64, k int64), entries being
    flat indices into the level's contiguous gradient (planar: c * XYZ + voxel, packed: voxel * 4 + c), sorted and unique."""
    dev = pts.device
    rows = f.shape[0] if f is not None else mu.shape[0]
    live = rows if count is None else max(0, min(int(count), rows))
    src = torch.arange(live, device=dev) if index is None else index[:live].to(dev).long()
    p = pts[src]

    def per_row(t):
        return None if t is None else t[:live].double()

    def per_point(t):
        return None if t is None else t[src].double()
    out = []
    for l, size in enumerate(dims):
        size = tuple(int(s) for s in size)
        nvox = size[0] * size[1] * size[2]
        lvl = (lambda t: None if t is None else t[:, l])                   # noqa: E731
        lin, t, ab = _corner_terms(p, size, lvl(per_row(f)), per_point(s_bar), lvl(per_row(mu)), per_point(g_bar), lvl(per_row(lam)))
        ch = torch.arange(4, device=dev)
        ent = (ch[None, :] * nvox + lin[:, None]) if layout == PLANAR else (lin[:, None] * 4 + ch[None, :])
        ent, t, ab = ent.reshape(-1), t.reshape(-1), ab.reshape(-1)
        uniq, inv = torch.unique(ent, return_inverse=True)
        S = torch.zeros(uniq.numel(), dtype=torch.float64, device=dev).index_add_(0, inv, t)
        A = torch.zeros_like(S).index_add_(0, inv, ab)
        k = torch.zeros(uniq.numel(), dtype=torch.int64, device=dev).index_add_(0, inv, torch.ones_like(inv))
        out.append((uniq, S, A, k))
    return out


def bound(k, A):
    """The largest |float32 result - S| a correct scatter may leave: (k + 8) 2^-24 A."""
    return (k.double() + 8.0) * U * A
