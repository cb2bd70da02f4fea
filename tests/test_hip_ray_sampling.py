"""The per-ray sampling kernels of k5_rays.hip (upsample_k, merge_k, merge_upsample_k<0 / 1>) at the shapes where a two-slot kernel goes wrong:
n below, at and right above 64 samples, surfaces in segments 62..65, n_new from 1 to 64, ray counts off a multiple of the four waves of a block.

    ops.upsample        against the float64 bracket of tests/ray_sampling_reference.py (pinned on the CPU by test_ray_sampling_reference_cpu.py):
                        a per-ray bound derived from the inputs, which a correct float32 evaluation cannot leave and which each of the seeded
                        hand-over defects does leave.  The mask decisions are the generator's (valid_in), so kernel and reference cannot differ
                        on a voxel; the look-up path (valid_in=None) is then held to the carried path bit for bit.
    ops.merge_upsample, ops.merge_mid_points   bit for bit against the separate operators, with ties at the slot boundary.

Run with -s for the worst bracket use per case."""
import pytest
import torch

from oracle import gens_oracle as K
from tests import ray_sampling_reference as R

pytestmark = pytest.mark.gpu

SHAPE_IDS = [f"n{n}-new{m}-s{s:g}" for n, m, s in R.SHAPES]


@pytest.fixture(scope="module")
def ops():
    from gens_amd import ops
    return ops


def dev(t):
    if isinstance(t, (list, tuple)):
        return [dev(x) for x in t]
    return t.cuda()


def _upsample_in_bracket(ops, c, ref, n_new, inv_s, what):
    z_new, pts_new, valid_new = ops.upsample(dev(c["ro"]), dev(c["rd"]), dev(c["z"]), dev(c["sdf"]), n_new, dev(c["masks"]), inv_s, valid_in=dev(c["vm"]))
    z_new, pts_new, valid_new = z_new.cpu(), pts_new.cpu(), valid_new.cpu()
    b = c["z"].shape[0]
    assert z_new.shape == (b, n_new) and bool(torch.isfinite(z_new).all())
    lower, _, upper = R.bracket(ref, n_new)
    use = R.bracket_use(ref, z_new)
    print(f"{what}: worst bracket use {float(use.max()):.3f}, delta {float(ref['delta'].min()):.2e} .. {float(ref['delta'].max()):.2e}")
    bad = (z_new.double() < lower) | (z_new.double() > upper)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} samples of {int(bad.any(-1).sum())} rays outside the bracket, worst use {float(use.max()):.3g}"
    assert bool((z_new >= c["z"][:, :1]).all()) and bool((z_new <= c["z"][:, -1:]).all()), f"{what}: z_new outside [z[0], z[-1]]"
    own = (c["ro"][:, None] + c["rd"][:, None] * z_new[..., None]).reshape(-1, 3)
    assert float((pts_new - own).abs().max()) <= 1e-6, f"{what}: pts_new"
    assert torch.equal(valid_new, K.point_valid(c["masks"], pts_new)), f"{what}: valid_new"
    return float(use.max())


@pytest.mark.parametrize("cls", R.CLASSES)
@pytest.mark.parametrize("shape", range(len(R.SHAPES)), ids=SHAPE_IDS)
def test_upsample_lies_inside_the_float64_bracket(ops, shape, cls):
    n, n_new, inv_s = R.SHAPES[shape]
    c, ref = R.shape_case(shape, cls)
    _upsample_in_bracket(ops, c, ref, n_new, inv_s, f"{cls} {R.SHAPES[shape]}")


@pytest.mark.parametrize("n_rays", [1, 3, 5])
def test_upsample_with_idle_waves_in_the_only_or_last_block(ops, n_rays):
    """1, 3 and 5 rays: idle waves must still reach the barrier between the CDF and the search.  holes: the last ray has no valid sample."""
    shape = 4
    n, n_new, inv_s = R.SHAPES[shape]
    c, ref = R.shape_case(shape, "holes", n_rays)
    _upsample_in_bracket(ops, c, ref, n_new, inv_s, f"holes {R.SHAPES[shape]} {n_rays} rays")


@pytest.mark.parametrize("shape", [0, 2, 4, 8], ids=[SHAPE_IDS[i] for i in (0, 2, 4, 8)])
def test_upsample_looking_the_masks_up_equals_the_carried_decisions(ops, shape):
    """valid_in=None looks all n samples up again; fed with ops.ray_points' decisions the carried path must give the same bits, with float masks
    and with the scene's bit masks -- and those decisions are the generator's, which the bracket test carried."""
    n, n_new, inv_s = R.SHAPES[shape]
    c, _ = R.shape_case(shape, "holes")
    ro, rd, z, sdf = dev(c["ro"]), dev(c["rd"]), dev(c["z"]), dev(c["sdf"])
    mask_list = dev(c["masks"])
    results = []
    for masks in (mask_list, ops.VolumeSet.masks(mask_list)):
        _, valid = ops.ray_points(ro, rd, z, masks)
        valid = valid.reshape(z.shape)
        assert torch.equal(valid.cpu(), c["vm"]) and 0 < int(valid.sum()) < valid.numel()
        looked = ops.upsample(ro, rd, z, sdf, n_new, masks, inv_s)
        carried = ops.upsample(ro, rd, z, sdf, n_new, masks, inv_s, valid_in=valid)
        for a, b_ in zip(looked, carried):
            assert torch.equal(a, b_)
        results.append(looked)
    for a, b_ in zip(*results):
        assert torch.equal(a, b_)


def _merge_case(n, n_add, seed):
    """A holes case of n + n_add samples per ray, split at random into n old and n_add new samples (both stay sorted), with
        ray 0   a new sample equal to an old one                 ray 1   two equal new samples (n_add >= 2)
        ray 3   an old sample at merged position min(63, m - 2) and an equal new one right behind it: a tie across a lane's two register slots
        the last two rays   no valid sample at all."""
    m = n + n_add
    b = 257
    c = R.make_case("holes", b, m, seed)
    g = torch.Generator().manual_seed(seed + 1)
    tie = min(63, m - 2)
    z_all = c["z"].clone()
    z_all[3, tie + 1] = z_all[3, tie]
    vm = c["vm"].clone()
    vm[b - 2] = False
    is_new = torch.zeros(b, m, dtype=torch.bool)
    for r in range(b):
        if r == 3:
            rest = torch.tensor([j for j in range(m) if j not in (tie, tie + 1)], dtype=torch.long)
            pick = rest[torch.randperm(m - 2, generator=g)[:n_add - 1]]
            is_new[r, tie + 1] = True
        else:
            pick = torch.randperm(m, generator=g)[:n_add]
        is_new[r, pick] = True
    split = lambda t, new: t[is_new if new else ~is_new].reshape(b, n_add if new else n)  # noqa: E731
    z, z_add = split(z_all, False).clone(), split(z_all, True).clone()
    z_add[0, 0] = z[0, min(n - 1, 5)]
    z_add[0] = torch.sort(z_add[0])[0]
    if n_add >= 2:
        z_add[1, 1] = z_add[1, 0]
    return dict(ro=c["ro"], rd=c["rd"], masks=c["masks"], z=z, z_add=z_add, sdf=split(c["sdf"], False), sdf_add=split(c["sdf"], True),
                valid=split(vm, False), valid_add=split(vm, True), tie=tie)


@pytest.mark.parametrize("n,n_add", [(1, 1), (63, 1), (64, 1), (63, 2), (64, 64), (127, 1), (100, 28)])
def test_fused_merge_launches_equal_the_separate_operators(ops, n, n_add):
    c = _merge_case(n, n_add, seed=500 + 3 * n + n_add)
    m = n + n_add
    ro, rd, z, z_add, sdf, sdf_add = (dev(c[k]) for k in ("ro", "rd", "z", "z_add", "sdf", "sdf_add"))
    valid, valid_add = dev(c["valid"]), dev(c["valid_add"])
    mask_list = dev(c["masks"])
    # the merge itself: the stable sort of the oracle, and the tie across the slots where it was put
    ref_z, ref_s = K.merge_samples(c["z"], c["z_add"], c["sdf"], c["sdf_add"])
    ref_v = torch.gather(torch.cat([c["valid"], c["valid_add"]], -1), 1, torch.sort(torch.cat([c["z"], c["z_add"]], -1), dim=-1, stable=True)[1])
    assert ref_z[3, c["tie"]] == ref_z[3, c["tie"] + 1] and not bool(ref_v[-2:].any())
    mz, ms, mv = ops.merge_samples(z, z_add, sdf, sdf_add, valid, valid_add)
    assert torch.equal(mz.cpu(), ref_z) and torch.equal(ms.cpu(), ref_s) and torch.equal(mv.cpu(), ref_v)
    for masks in (mask_list, ops.VolumeSet.masks(mask_list)):
        for n_new in (1, 16, 64):
            sep = (mz, ms, mv) + tuple(ops.upsample(ro, rd, mz, ms, n_new, masks, 64.0, valid_in=mv))
            fused = ops.merge_upsample(ro, rd, z, sdf, valid, z_add, sdf_add, valid_add, n_new, masks, 64.0)
            assert len(fused) == 6 and fused[3].shape == (z.shape[0], n_new)
            for k, (a, b_) in enumerate(zip(fused, sep)):
                assert torch.equal(a, b_), f"merge_upsample ({n} + {n_add} -> {n_new}) output {k}"
        mz_only, _ = ops.merge_samples(z, z_add)
        assert torch.equal(mz_only, mz)
        sep = (mz_only,) + tuple(ops.ray_points(ro, rd, mz_only, masks, mid=True, sample_dist=1 / 32))
        fused = ops.merge_mid_points(ro, rd, z, z_add, masks, 1 / 32)
        assert fused[1].shape == (z.shape[0] * m, 3)
        for k, (a, b_) in enumerate(zip(fused, sep)):
            assert torch.equal(a, b_), f"merge_mid_points ({n} + {n_add}) output {k}"
