"""gens_blend_views_bf16x3's kernel at THREE resident waves per SIMD (k7b_blend_bf16x3.hip, the "diet" build: the colour, the ray
difference's rgb_fc.0 quads and the row mask are read a second time from the LDS tiles of phase 0 and not carried through the network).

gens_blend_bf16x3_residency states the occupancy claim on the device; every instantiation is held to gens_blend_views_t (k7t_blend.hip,
untouched code that shares phase 0) on the edges of a wave, and not-a-number inputs must poison the points they poison there."""
import ctypes as C

import pytest
import torch

from .test_hip_blend_bf16x3 import _setup

pytestmark = pytest.mark.gpu

# The largest |K7b - K7t| over a colour channel in the cases of test_every_instantiation_on_the_edges_of_a_wave, measured on an MI355X
# with the kernel bounded for two waves (-DGENS_K7B_OCC=2: the instructions before the diet): profiles/r26_blend_three_waves.txt.  The
# three-wave build is allowed twice that -- room for a legal change of instruction selection only; a value read back from a wrong row
# or column moves a colour by 1e-2 or more.
PARENT_MAX_DIFF = 2.0 ** -22      # 2.384e-07, at n_levels = 2, nv = 3, n = 33; the three-wave build measures the same figure in every case
COLOUR_BOUND = 2 * PARENT_MAX_DIFF

CASES = [(nl, nv, n) for nl in (1, 2, 3, 4, 5) for nv in (3, 4, 5) for n in ((1, 33) if nv == 3 else (1, 17))]


def _residency(n_levels, nv):
    from gens_amd import lib as L
    out = (C.c_int * 4)()
    rc = L.load().gens_blend_bf16x3_residency(n_levels, nv, out)
    assert rc == 0, L.load().gens_last_error()
    return {"regs": out[0], "scratch": out[1], "lds": out[2], "blocks": out[3]}


def test_residency_on_the_device():
    """All fifteen instantiations: no scratch, at most 168 registers, the 8 960 bytes of X, RD and R, and twelve one-wave workgroups per
    CU -- four SIMDs x three waves (the LDS alone would allow 18)."""
    from gens_amd import lib as L
    for nl in (1, 2, 3, 4, 5):
        for nv in (3, 4, 5):
            r = _residency(nl, nv)
            print("residency", nl, nv, r)
            assert r["scratch"] == 0 and 0 < r["regs"] <= 168 and r["lds"] == 8960 and r["blocks"] == 12, (nl, nv, r)
    out = (C.c_int * 4)()
    for nl in (0, 6):
        assert L.load().gens_blend_bf16x3_residency(nl, 5, out) == -2 and b"1 to 5 feature levels" in L.load().gens_last_error()
    for nv in (2, 6):
        assert L.load().gens_blend_bf16x3_residency(5, nv, out) == -2 and b"two to four source views" in L.load().gens_last_error()
    assert L.load().gens_blend_bf16x3_residency(5, 5, None) == -1


def _run(ops, plan, views, pts, kind, monkeypatch, idx=None, count=None):
    monkeypatch.setattr(ops.kernels, "blend", kind)
    n, nv = pts.shape[0], views.nv
    rgb = torch.full((n, 3), -7.0, device="cuda")
    vis = torch.full((n, nv - 1), 9, dtype=torch.uint8, device="cuda")
    ops.blend_views(plan, views, pts, index=idx, rgb_out=rgb, vis_out=vis, count=count)
    return rgb, vis


@pytest.mark.parametrize("n_levels,nv,n", CASES)
def test_every_instantiation_on_the_edges_of_a_wave(n_levels, nv, n, monkeypatch):
    """16 points per wave at S = 3, 4 and 32 at S = 2: one point, and one over a wave, on 48 x 64 maps, with a random index map and a
    device-side count of 3 n / 4.  The flags equal gens_blend_views_t's, the colours agree with its within twice what the two-wave build
    differs from it on these cases (PARENT_MAX_DIFF: 2.384e-07 measured on an MI355X, and 2.384e-07 with the three-wave build, case by
    case the same figures), rows beyond the count keep the caller's fill values."""
    from gens_amd import lib as L
    ops, net, views, pts = _setup(nv, n_levels, seed=40 + nv, n=n)
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(n)).cuda()
    count = torch.tensor([max(1, (3 * n) // 4)], dtype=torch.int32, device="cuda")
    plan = ops.BlendPlan(net)
    L.profile_begin()
    new = _run(ops, plan, views, pts, "bf16x3", monkeypatch, idx, count)
    old = _run(ops, plan, views, pts, "transposed", monkeypatch, idx, count)
    table = L.profile_end()
    assert len(table) == 2 and table["gens_blend_views_bf16x3"]["launches"] == 1, table      # (gens_blend_views_t has a label of its own)
    live, dead = idx[:int(count)], idx[int(count):]
    diff = float((new[0][live] - old[0][live]).abs().max())
    print(f"K7b-K7t n_levels={n_levels} nv={nv} n={n} max colour difference {diff:.3e}")
    assert torch.equal(new[1], old[1])
    assert torch.isfinite(new[0][live]).all()
    assert diff <= COLOUR_BOUND, (diff, COLOUR_BOUND)
    assert (new[0][dead] == -7).all() and (new[1][dead] == 9).all()


@pytest.mark.parametrize("where", ["image", "feature"])
def test_not_a_number_in_one_rows_texels_poisons_the_points_it_poisons_in_the_float32_kernel(where, monkeypatch):
    """S = 4, 17 points.  A not-a-number in the image texels that one (point, view) row reads and nowhere else, then in that row's
    level-0 feature texels and nowhere else: the colour channel and the mask are the values the diet reads a second time.  The bilinear
    taps of a row at pixel (px, py) lie in columns floor(px) - 1 .. floor(px) + 2 (read position px w / (w - 1) - 1 / 2), and so for py."""
    ops, net, views, pts = _setup(5, 5, seed=9, n=17)
    plan = ops.BlendPlan(net)
    clean, vis = _run(ops, plan, views, pts, "transposed", monkeypatch)
    assert torch.isfinite(clean).all()
    sv = 2                                                                  # the second source view (view 0 is the target)
    k = int(torch.nonzero(vis[:, sv - 1] == 1)[0])                          # a point that view sees
    h, w = views.imgs_tex.shape[1:3]
    p = views.w2c.reshape(-1, 4, 4)[sv].double().cpu() @ torch.cat([pts[k].double().cpu(), torch.ones(1, dtype=torch.float64)])
    uvd = views.intr.reshape(-1, 4, 4)[sv].double().cpu()[:3, :3] @ p[:3]
    px, py = int(uvd[0] / uvd[2]), int(uvd[1] / uvd[2])
    assert 0 <= px < w and 0 <= py < h, (px, py)
    tex = views.imgs_tex if where == "image" else views.feat_tex[0]
    assert tex.shape[1:3] == (h, w)
    tex[sv, max(py - 1, 0):py + 3, max(px - 1, 0):px + 3, 1] = float("nan")
    want, vis_t = _run(ops, plan, views, pts, "transposed", monkeypatch)
    got, vis_b = _run(ops, plan, views, pts, "bf16x3", monkeypatch)
    bad = torch.isnan(want).any(1)
    print(f"NaN in the {where} texels of point {k}, view {sv}: {int(bad.sum())} of 17 points poisoned")
    assert bool(bad[k]) and int(bad.sum()) < 17
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(vis_b, vis_t)
    assert torch.isfinite(got[~bad]).all()
