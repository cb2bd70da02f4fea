"""CPU checks of the two-level lattice's METHOD on analytic fields (tests/sparse_lattice_reference.py, no kernel): under the Lipschitz bound
the filled lattice has the dense lattice's signs everywhere and its values on every crossing edge, so marching cubes cannot tell them apart;
a field that breaks the bound out of the corners' sight is reported by the leak count."""
import pytest
import torch

from . import sparse_lattice_reference as SR

LO, HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
FIELDS = {"sphere": SR.sphere(0.5), "two_spheres": SR.two_spheres, "plane": SR.plane}


@pytest.fixture(scope="module")
def dense():
    cache = {}

    def get(name, r):
        if (name, r) not in cache:
            cache[name, r] = SR.dense_u(FIELDS[name], r)
        return cache[name, r]
    return get


@pytest.mark.parametrize("b", [4, 8])
@pytest.mark.parametrize("r", [9, 10, 33, 64, 65, 100, 128])
@pytest.mark.parametrize("name", sorted(FIELDS))
def test_filled_lattice_has_the_dense_signs_and_crossing_values(dense, name, r, b):
    u = dense(name, r)
    for t in (0.0, 0.05):
        us, act, evaluated = SR.filled(u, r, b, t, SR.margin(LO, HI, r, b, 1.0))
        t32 = torch.tensor(t, dtype=torch.float32)
        assert torch.equal(us < t32, u < t32)
        need = SR.crossing_endpoints(u, t)
        assert bool(need.any())                                       # every field crosses both thresholds
        assert torch.equal(us[need], u[need])
        assert SR.leaks(us, act, r, b, t) == 0 and SR.leaks(u, act, r, b, t) == 0
    if name == "plane" and r % 2 == 1:
        assert int((u == 0).sum()) == r * r                           # exact zeros ON lattice points


def test_evaluated_share_of_the_half_sphere_at_128():
    u = SR.dense_u(FIELDS["sphere"], 128)
    _, act, evaluated = SR.filled(u, 128, 4, 0.0, SR.margin(LO, HI, 128, 4, 1.0))
    assert 0.10 < evaluated / 128 ** 3 < 0.20                         # 0.147: the shell of active bricks, not the volume


@pytest.mark.parametrize("b", [4, 8])
@pytest.mark.parametrize("r", [9, 10, 33])
@pytest.mark.parametrize("name", sorted(FIELDS))
def test_marching_cubes_cannot_tell_the_lattices_apart(dense, name, r, b):
    import numpy as np
    from gens_amd import mc_tables
    from oracle import mc_oracle
    u = dense(name, r)
    for t in (0.0, 0.05):
        us, _, _ = SR.filled(u, r, b, t, SR.margin(LO, HI, r, b, 1.0))
        v0, t0 = mc_oracle.marching_cubes(u.numpy(), t, mc_tables.TRI_TABLE, mc_tables.TRI_COUNT)
        v1, t1 = mc_oracle.marching_cubes(us.numpy(), t, mc_tables.TRI_TABLE, mc_tables.TRI_COUNT)
        assert len(t0) > 0 and np.array_equal(v0, v1) and np.array_equal(t0, t1)


@pytest.mark.parametrize("r,b", [(65, 4), (65, 8), (100, 8), (128, 4)])
def test_a_planted_violation_is_counted(r, b):
    field, i = SR.planted(r, b)
    u = SR.dense_u(field, r)
    us, act, _ = SR.filled(u, r, b, 0.0, SR.margin(LO, HI, r, b, 1.0))
    assert not bool(act[0, 0, 0]) and i < b                           # the planted point sits in a brick no corner of which saw it
    assert float(u[i, i, i]) > 0.0 and float(us[i, i, i]) < 0.0       # ... and the fill lost it
    assert SR.leaks(u, act, r, b, 0.0) == 6                           # counted on the lattice that has it: its six edges
    assert SR.leaks(us, act, r, b, 0.0) == 0                          # the filled lattice alone cannot know


def test_brick_geometry():
    assert SR.dims(9, 8) == (2, 1, 2) and SR.dims(10, 8) == (3, 2, 2) and SR.dims(100, 8) == (14, 13, 13) and SR.dims(128, 4) == (33, 32, 32)
    assert SR.coarse_index(10, 8).tolist() == [0, 8, 9] and SR.coarse_index(9, 4).tolist() == [0, 4, 8]
    assert SR.deciding_brick(10, 8).tolist() == [0] * 8 + [1, 1] and SR.deciding_brick(9, 8).tolist() == [0] * 9
    for r, b in [(9, 8), (10, 8), (33, 4), (100, 8), (100, 4)]:
        _, nb, p = SR.dims(r, b)
        rows = SR.brick_rows(r, b, list(range(p ** 3)))
        own = rows[(rows < r).all(1)]
        flat = (own[:, 0] * r + own[:, 1]) * r + own[:, 2]
        assert torch.equal(flat.sort().values, torch.arange(r ** 3))  # every fine point has exactly one owner
