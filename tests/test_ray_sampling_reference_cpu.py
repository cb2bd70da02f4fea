"""tests/ray_sampling_reference.py pinned on the CPU: the float64 bracket holds the reference project's recorded samples and the oracle's
float32 up_sample, is far wider than a float32 evaluation needs, notices each seeded defect, and is not vacuous on rays that hit the surface.
Run with -s for the figures."""
import pytest
import torch

from oracle import gens_oracle as K
from tests import ray_sampling_reference as R

SHAPE_IDS = [f"n{n}-new{m}-s{s:g}" for n, m, s in R.SHAPES]
ALL_SHAPES = range(len(R.SHAPES))


def _outside(ref, z_new):
    lower, _, upper = R.bracket(ref, z_new.shape[1])
    z_new = z_new.double()
    return (z_new < lower) | (z_new > upper)


def test_recorded_samples_of_the_golden_lie_inside_the_bracket(golden):
    g = golden("g5_upsample")
    masks = [g[f"mask{i}"] for i in range(3)]
    ro, rd = g["rays_o"], g["rays_d"]
    for r in range(4):
        z, sdf, z_new = g[f"z{r}"], g[f"sdf{r}"], g[f"znew{r}"]
        b, n = z.shape
        vm = K.point_valid(masks, (ro[:, None] + rd[:, None] * z[..., None]).reshape(-1, 3)).reshape(b, n)
        rad = torch.linalg.norm(ro.double()[:, None] + rd.double()[:, None] * z.double()[..., None], dim=-1)
        assert float((rad - 1.0).abs().min()) > 1e-4             # no decision about the unit sphere hangs on a rounding
        ref = R.reference(z, sdf, vm, rad < 1.0, 64 * 2 ** r)
        use = R.bracket_use(ref, z_new)
        print(f"golden round {r}: n {n}, delta {float(ref['delta'].min()):.2e} .. {float(ref['delta'].max()):.2e}, worst bracket use {float(use.max()):.3f}")
        assert not bool(_outside(ref, z_new).any())


@pytest.mark.parametrize("cls", R.CLASSES)
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=SHAPE_IDS)
def test_oracle_up_sample_lies_inside_the_bracket(shape, cls):
    """K.up_sample makes its own decisions from the masks and from float32 radii: they are the generator's (no sample within 1e-5 of the sphere).
    Its per-quantile Python loop is slow, so it runs the rays that place a surface in segments 0..67 and the last two (holes: the dead ray)."""
    n, n_new, inv_s = R.SHAPES[shape]
    c, ref = R.shape_case(shape, cls)
    b = c["z"].shape[0]
    rows = torch.cat([torch.arange(min(68, b - 2)), torch.arange(b - 2, b)])
    z_new = K.up_sample(c["ro"][rows], c["rd"][rows], c["z"][rows], c["sdf"][rows], n_new, c["masks"], torch.tensor(inv_s))
    sub = {k: v[rows] for k, v in ref.items()}
    use = R.bracket_use(sub, z_new)
    print(f"oracle {cls} {R.SHAPES[shape]}: worst bracket use {float(use.max()):.3f}")
    assert not bool(_outside(sub, z_new).any())


@pytest.mark.parametrize("cls", R.CLASSES)
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=SHAPE_IDS)
def test_float32_restatement_uses_a_fraction_of_the_bound(shape, cls):
    n, n_new, inv_s = R.SHAPES[shape]
    c, ref = R.shape_case(shape, cls)
    z_new, cdf32 = R.upsample_f32(c["z"], c["sdf"], c["vm"], c["rad_lt1"], n_new, inv_s)
    head = float(((cdf32.double() - ref["cdf"]).abs().max(-1)[0] / ref["delta"]).max())
    use = R.bracket_use(ref, z_new)
    print(f"float32 {cls} {R.SHAPES[shape]}: worst |cdf32 - cdf64| / delta {head:.3f}, worst bracket use {float(use.max()):.3f}, "
          f"delta {float(ref['delta'].min()):.2e} .. {float(ref['delta'].max()):.2e}")
    assert head <= 1.0
    assert not bool(_outside(ref, z_new).any())
    assert bool((z_new >= c["z"][:, :1]).all()) and bool((z_new <= c["z"][:, -1:]).all())


APPLICABLE = [(i, d) for i in ALL_SHAPES for d in R.DEFECTS if R.defect_applies(d, R.SHAPES[i][0])]


@pytest.mark.parametrize("shape,defect", APPLICABLE, ids=[f"{SHAPE_IDS[i]}-{d}" for i, d in APPLICABLE])
def test_each_seeded_defect_leaves_the_bracket(shape, defect):
    """Every hit case where the defect applies (below 66 samples no segment lies in the upper slots and (a) to (c) change nothing)."""
    n, n_new, inv_s = R.SHAPES[shape]
    c, ref = R.shape_case(shape, "hit")
    z_new, _ = R.upsample_f32(c["z"], c["sdf"], c["vm"], c["rad_lt1"], n_new, inv_s, defect=defect)
    out = _outside(ref, z_new)
    rays = out.any(-1)
    print(f"{defect} {R.SHAPES[shape]}: {int(out.sum())} samples of {int(rays.sum())} rays outside the bracket; surfaces at segments "
          f"{sorted(set(c['cross'][rays].tolist()))[:12]}")
    assert bool(out.any())


def test_upper_slot_defects_change_nothing_below_66_samples():
    for shape in ALL_SHAPES:
        n, n_new, inv_s = R.SHAPES[shape]
        if n >= 66:
            continue
        c, _ = R.shape_case(shape, "hit")
        args = (c["z"], c["sdf"], c["vm"], c["rad_lt1"], n_new, inv_s)
        clean = R.upsample_f32(*args)
        for defect in R.DEFECTS[:3]:
            assert all(torch.equal(a, b_) for a, b_ in zip(R.upsample_f32(*args, defect=defect), clean))


@pytest.mark.parametrize("cls", ("hit", "holes"))
@pytest.mark.parametrize("shape", [i for i in ALL_SHAPES if R.SHAPES[i][0] >= 63], ids=[s for s, sh in zip(SHAPE_IDS, R.SHAPES) if sh[0] >= 63])
def test_the_bound_is_not_vacuous_on_rays_that_hit(shape, cls):
    """At least half of the rays of every hit / holes case must be held to delta <= 2e-4 (miss rays legitimately reach 5e-2: the sum of their
    weights is n 1e-5; they stay in the suite to catch gross errors)."""
    _, ref = R.shape_case(shape, cls)
    frac = float((ref["delta"] <= 2e-4).double().mean())
    print(f"{cls} {R.SHAPES[shape]}: delta <= 2e-4 on {100 * frac:.0f} % of the rays, <= 1e-4 on {100 * float((ref['delta'] <= 1e-4).double().mean()):.0f} %, "
          f"median {float(ref['delta'].median()):.2e}")
    assert frac >= 0.5
