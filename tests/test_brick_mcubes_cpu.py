"""The two covering claims behind the brick-sparse marching cubes (K29), checked on the torch restatement with no kernel:
on the lattice the two-level method builds, no mixed-sign cell has its origin outside the emitting bricks, and no crossing edge has its owner
outside them -- with or without the Lipschitz bound holding.  And the operator's own argument checks, which need no device."""
import pytest
import torch

from . import brick_mcubes_reference as BR
from . import sparse_lattice_reference as SR

LO, HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
SIZES = [(r, b) for r in (9, 10, 33, 64, 65, 100) for b in (4, 8)]


def _cases(r, b):
    """(name, dense u, threshold, lipschitz) of the fields of DESIGN.md 5f at one size."""
    noise = BR.noise_lattice(r, r)                                        # (R = 33: the field of the device test, 77 leaks at B = 4 and 281 at B = 8)
    return [("sphere", SR.dense_u(SR.sphere(0.5), r), 0.0, 1.0),
            ("two_spheres", SR.dense_u(SR.two_spheres, r), 0.0, 1.0),
            ("two_spheres at 0.05", SR.dense_u(SR.two_spheres, r), 0.05, 1.0),
            ("plane", SR.dense_u(SR.plane, r), 0.0, 1.0),
            ("planted", SR.dense_u(SR.planted(r, b)[0], r), 0.0, 1.0),
            ("sphere under 0.1", SR.dense_u(SR.sphere(0.5), r), 0.0, 0.1),
            ("noise under 0.05", -noise, 0.0, 0.05)]


@pytest.mark.parametrize("r,b", SIZES)
def test_the_emitting_bricks_hold_every_cell_and_every_crossing_edge(r, b):
    leaky, surfaces = 0, 0
    for name, u, t, lipschitz in _cases(r, b):
        us, act, emit, cells, edges = BR.outside_the_emitting_set(u, r, b, t, SR.margin(LO, HI, r, b, lipschitz))
        assert cells == 0 and edges == 0, (name, cells, edges)
        assert bool((emit | ~act).all())                                  # an active brick emits
        surfaces += int(BR.mixed_cells(us, t).sum()) > 0                  # (a field that breaks its bound may lose its surface: R = 9, B = 8)
        leaky += SR.leaks(us, act, r, b, t) > 0
        if name == "sphere" and r >= 64:
            print(f"R = {r}, B = {b}: {int(act.sum())} active, {int(emit.sum())} emitting of {emit.numel()} bricks")
            assert int(emit.sum()) <= 2 * int(act.sum())                  # (measured: 1.17 to 1.42 times the active set on the sphere at these sizes)
    assert surfaces >= 5                                                  # the claims are not vacuous
    assert leaky > 0 or r < 33                                            # the claims were met where the bound fails, too: the noise leaks from R = 33 on


def test_emitting_is_the_clipped_union():
    act = torch.zeros(4, 4, 4, dtype=torch.bool)
    act[2, 3, 1] = True
    want = torch.zeros_like(act)
    want[1:3, 2:4, 0:2] = True                                            # X + {0,1}^3 reaches (2, 3, 1) from these, and the grid ends at 3
    assert torch.equal(BR.emitting(act), want)
    assert not BR.emitting(torch.zeros(3, 3, 3, dtype=torch.bool)).any() and BR.emitting(torch.ones(1, 1, 1, dtype=torch.bool)).all()


def test_operator_refuses_bad_arguments_before_any_launch():
    from gens_amd import ops
    field = lambda p: p[:, :1]  # noqa: E731
    for bad in [dict(resolution=1, brick=4), dict(resolution=64, brick=1), dict(resolution=64, brick=9), dict(resolution=64, brick=16),
                dict(resolution=10400, brick=8)]:                         # C = 1301: C^3 >= 2^31
        with pytest.raises(ValueError):
            ops.brick_mc_dims(**bad)
        with pytest.raises(ValueError):
            ops.brick_marching_cubes(field, LO, HI, bad["resolution"], 0.0, bad["brick"], 1.0, device="cpu")
    with pytest.raises(ValueError, match="lipschitz"):
        ops.brick_marching_cubes(field, LO, HI, 64, 0.0, 4, 0.0, device="cpu")
    with pytest.raises(ValueError, match="chunk"):
        ops.brick_marching_cubes(field, LO, HI, 64, 0.0, 4, 1.0, chunk=0, device="cpu")
    with pytest.raises(ValueError, match="three values"):
        ops.brick_marching_cubes(field, (0.0, 0.0), HI, 64, 0.0, 4, 1.0, device="cpu")
    assert ops.brick_mc_dims(2049, 8) == (257, 257) and ops.brick_mc_dims(5000, 4) == (1251, 1250) and ops.brick_mc_dims(10, 8) == (3, 2)
    assert ops.BRICK_MC_MAX == 8
