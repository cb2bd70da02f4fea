"""A torch restatement of the two-level lattice (K28, ops.sparse_lattice) for the tests: coarse indices, deciding and point bricks, the active
rule, the fill, the leak count and the filled lattice, all on dense (R, R, R) arrays with no kernel.  Written from the method's definition
(DESIGN.md, section 5e), not from the kernels."""
import math

import numpy as np
import torch


def dims(r, b):
    """-> (C coarse points, C - 1 deciding bricks, P point bricks) per axis."""
    c = -(-(r - 1) // b) + 1
    return c, c - 1, -(-r // b)


def coarse_index(r, b):
    c, _, _ = dims(r, b)
    return torch.clamp(torch.arange(c) * b, max=r - 1)


def deciding_brick(r, b):
    """(R,) the brick that decides for each fine index: the last brick also takes the index R - 1."""
    _, nb, _ = dims(r, b)
    return torch.clamp(torch.arange(r) // b, max=nb - 1)


def margin(lo, hi, r, b, lipschitz):
    """lipschitz * ||(B + 1) h||_2, rounded UP to float32."""
    h = [(float(y) - float(x)) / (r - 1) for x, y in zip(lo, hi)]
    m = float(lipschitz) * math.sqrt(sum(((b + 1) * v) ** 2 for v in h))
    m32 = np.float32(m)
    return float(m32 if float(m32) >= m else np.nextafter(m32, np.float32(np.inf)))


def active(uc, t, mrg):
    """uc (C, C, C) float32 -> (C - 1)^3 bool: a corner non-finite, or |u - t| <= margin in float32, or the corners disagree on u < t."""
    uc = uc.to(torch.float32)
    t32, m32 = torch.tensor(t, dtype=torch.float32), torch.tensor(mrg, dtype=torch.float32)
    near = ~torch.isfinite(uc) | ((uc - t32).abs() <= m32)
    below = uc < t32
    nb = uc.shape[0] - 1
    act = torch.zeros(nb, nb, nb, dtype=torch.bool)
    any_b, all_b = torch.zeros_like(act), torch.ones_like(act)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                s = (slice(dx, dx + nb), slice(dy, dy + nb), slice(dz, dz + nb))
                act |= near[s]
                any_b |= below[s]
                all_b &= below[s]
    return act | (any_b & ~all_b)


def per_point(grid, r, b):
    """A (C - 1)^3 (or C^3: its lowest-corner part) array of the deciding bricks spread over the (R, R, R) lattice points."""
    at = deciding_brick(r, b)
    return grid[at][:, at][:, :, at]


def fill(uc, r, b):
    return per_point(uc, r, b)


def point_brick_flags(act, r, b):
    """(C - 1)^3 deciding-brick flags -> P^3 point-brick flags (the plane R - 1 as a brick of its own when (R - 1) % B == 0)."""
    _, nb, p = dims(r, b)
    at = torch.clamp(torch.arange(p), max=nb - 1)
    return act[at][:, at][:, :, at]


def filled(u, r, b, t, mrg):
    """The lattice the method returns for the dense lattice u -> (filled (R, R, R), active (C - 1)^3 bool, evaluated owned points)."""
    ci = coarse_index(r, b)
    uc = u[ci][:, ci][:, :, ci]
    act = active(uc, t, mrg)
    a = per_point(act, r, b)
    return torch.where(a, u, fill(uc, r, b)), act, int(a.sum())


def crossing_edges(u, t):
    """For each axis the bool array of edges (p, p + e_axis) with (u[p] < t) != (u[q] < t)."""
    s = u < torch.tensor(t, dtype=torch.float32)
    out = []
    for ax in range(3):
        n = u.shape[ax] - 1
        out.append(s.narrow(ax, 0, n) != s.narrow(ax, 1, n))
    return out


def leaks(u, act, r, b, t):
    """Crossing edges with at least one endpoint decided by an inactive brick."""
    a = per_point(act, r, b)
    total = 0
    for ax, cross in enumerate(crossing_edges(u, t)):
        n = r - 1
        total += int((cross & ~(a.narrow(ax, 0, n) & a.narrow(ax, 1, n))).sum())
    return total


def crossing_endpoints(u, t):
    """(R, R, R) bool: the points marching cubes interpolates between."""
    need = torch.zeros(u.shape, dtype=torch.bool)
    for ax, cross in enumerate(crossing_edges(u, t)):
        n = u.shape[ax] - 1
        need.narrow(ax, 0, n).logical_or_(cross)
        need.narrow(ax, 1, n).logical_or_(cross)
    return need


def brick_rows(r, b, entries):
    """Point-brick numbers (C order of the P^3 grid) -> (len * B^3, 3) int64 UNCLAMPED fine indices in brick-local C order."""
    _, _, p = dims(r, b)
    e = torch.as_tensor(entries, dtype=torch.int64)
    ex, ey, ez = e // (p * p), (e // p) % p, e % p
    l = torch.arange(b ** 3)
    lx, ly, lz = l // (b * b), (l // b) % b, l % b
    return torch.stack([(ex[:, None] * b + lx[None]).reshape(-1), (ey[:, None] * b + ly[None]).reshape(-1), (ez[:, None] * b + lz[None]).reshape(-1)], 1)


# ---- analytic fields (signed distances) on the lattice of torch.linspace(-1, 1, R)^3 -----------------------------------------------
def sphere(radius, centre=(0.0, 0.0, 0.0)):
    def f(p):
        c = torch.tensor(centre, dtype=p.dtype, device=p.device)
        return ((p - c) ** 2).sum(-1, keepdim=True).sqrt() - radius
    return f


def two_spheres(p):
    return torch.minimum(sphere(0.25, (0.4, 0.0, 0.0))(p), sphere(0.3, (-0.4, 0.0, 0.1))(p))


def plane(p):
    return p[..., :1].clone()


def planted(r, b):
    """A field that breaks lipschitz = 1 where no brick corner can see it: the sphere of radius 0.5 everywhere, except inside a sphere of
    radius 0.6 h around the lattice point (B // 2,) * 3 -- the middle of the corner brick, far from the big sphere -- where the value is that
    small sphere's negative distance.  Only the centre is a lattice point inside it: one point of the other sign, six crossing edges, in a
    brick whose corners are all far from the threshold.  -> (field, centre index)."""
    h = 2.0 / (r - 1)
    i = b // 2
    x = float(torch.linspace(-1.0, 1.0, r)[i])

    def f(p):
        c = torch.tensor((x, x, x), dtype=p.dtype, device=p.device)
        small = ((p - c) ** 2).sum(-1, keepdim=True).sqrt() - 0.6 * h
        return torch.where(small < 0.0, small, sphere(0.5)(p))
    return f, i


def lattice(r, device="cpu"):
    xs = torch.linspace(-1.0, 1.0, r)
    return torch.stack(torch.meshgrid(xs, xs, xs, indexing="ij"), -1).reshape(-1, 3).to(device)


def dense_u(field, r):
    return (-field(lattice(r))).reshape(r, r, r).to(torch.float32)
