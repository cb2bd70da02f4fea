"""A torch restatement of the emitting-set rule of the brick-sparse marching cubes (K29, ops.brick_marching_cubes) on dense (R, R, R) arrays,
on top of tests/sparse_lattice_reference.py.  Written from the definition, not from the kernels: a deciding brick X
EMITS if a brick of X + {0,1}^3, clipped to the brick grid, is active; marching cubes runs on the points decided by emitting bricks."""
import torch

from . import sparse_lattice_reference as SR


def emitting(act):
    """(C - 1)^3 bool active flags -> (C - 1)^3 bool: a brick of X + {0,1}^3 (clipped) is active."""
    nb = act.shape[0]
    out = torch.zeros_like(act)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                at = [torch.clamp(torch.arange(nb) + d, max=nb - 1) for d in (dx, dy, dz)]
                out |= act[at[0]][:, at[1]][:, :, at[2]]
    return out


def mixed_cells(u, t):
    """(R - 1)^3 bool: the cells whose eight corners disagree on u < t -- the cells marching cubes gives triangles."""
    s = u < torch.tensor(t, dtype=torch.float32)
    n = u.shape[0] - 1
    any_b, all_b = torch.zeros(n, n, n, dtype=torch.bool), torch.ones(n, n, n, dtype=torch.bool)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                c = s[dx:dx + n, dy:dy + n, dz:dz + n]
                any_b |= c
                all_b &= c
    return any_b & ~all_b


def outside_the_emitting_set(u, r, b, t, mrg):
    """For the dense lattice u: the lattice us the two-level method builds, its active and emitting bricks, and what marching cubes on us needs
    from points NOT decided by an emitting brick -> (us, act, emit, mixed-sign cells with such an origin, crossing edges with such an owner)."""
    us, act, _ = SR.filled(u, r, b, t, mrg)
    emit = emitting(act)
    e = SR.per_point(emit, r, b)
    n = r - 1
    cells = int((mixed_cells(us, t) & ~e[:n, :n, :n]).sum())
    edges = sum(int((cross & ~e.narrow(ax, 0, n)).sum()) for ax, cross in enumerate(SR.crossing_edges(us, t)))
    return us, act, emit, cells, edges


def noise_lattice(r, seed):
    """White noise on the lattice: a fixed (R, R, R) float32 tensor of signed distances."""
    return torch.randn(r, r, r, generator=torch.Generator().manual_seed(seed))


def lookup_field(values):
    """values (R, R, R) float32 -> a field on [-1, 1]^3 that returns the value at the nearest lattice index: its lattice values are `values`
    whatever the batch, non-finite ones included."""
    r = values.shape[0]

    def f(p):
        i = torch.round((p.double() + 1.0) * 0.5 * (r - 1)).long().clamp_(0, r - 1)
        return values.to(p.device)[i[:, 0], i[:, 1], i[:, 2]].reshape(-1, 1)
    return f
