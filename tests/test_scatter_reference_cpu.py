"""The float64 scatter reference (tests/scatter_reference.py) against float64 autograd of F.grid_sample(align_corners=True, padding_mode="zeros")
on the CPU, so that the GPU scatter tests lean on no kernel.

    first order      the volume gradient of <grid_sample(V, p), g>
    grad_p w terms   the volume gradient of <d y / d p, c> (double backward; ATen has none for grid_sample, so: a one-sided difference of the
                     first-order volume gradient per axis, EXACT on a dyadic lattice -- the weights are linear in each coordinate inside a cell, and
                     the points and the step are exact in float32 and float64 with (size - 1) a power of two)
    K17              the sum of the three
Points: a dyadic lattice over and past the cube (faces, corners, integer positions of every level), far outside, NaN; random points on grids whose
(size - 1) is no power of two (there float32 and float64 weights differ in the last bits: a looser bound)."""
import pytest
import torch
import torch.nn.functional as F

from tests import scatter_reference as R

f64 = torch.float64


def _vol_grad(pts, size, cot):
    """d/dV <grid_sample(V, pts), cot> for one (1, 4, X, Y, Z) level, float64: -> (4, X, Y, Z)."""
    V = torch.zeros((1, 4) + tuple(size), dtype=f64, requires_grad=True)
    y = F.grid_sample(V, pts.double().flip(-1)[None, None, None], align_corners=True, padding_mode="zeros").reshape(4, -1).t()
    g, = torch.autograd.grad((y * cot.double()).sum(), V)
    return g[0]


def _vol_grad_dir(pts, size, vec, cot, h=2.0 ** -20):
    """d/dV <(d y / d p) vec, cot>: the per-axis forward difference of the first-order volume gradient (ATen's floor cell at integer positions)."""
    base = _vol_grad(pts, size, cot)
    out = torch.zeros_like(base)
    for ax in range(3):
        step = torch.zeros(3, dtype=f64)
        step[ax] = h
        moved = _vol_grad(pts.double() + step, size, cot * vec[:, ax:ax + 1].double())
        out += (moved - _vol_grad(pts, size, cot * vec[:, ax:ax + 1].double())) / h
    return out


def _dense(level, size, layout=R.PLANAR):
    ent, S, A, k = level
    n = 4 * size[0] * size[1] * size[2]
    d = torch.zeros(n, dtype=f64).index_add_(0, ent, S)
    if layout == R.PACKED:
        d = d.reshape(tuple(size) + (4,)).permute(3, 0, 1, 2)
    return d.reshape((4,) + tuple(size))


def _lattice(seed, n=400):
    g = torch.Generator().manual_seed(seed)
    m = torch.randint(-80, 209, (n, 3), generator=g)
    pts = m.double() / 64.0 - 1.0                                       # every 1/64: faces, integer positions of every level, past the cube
    pts[:8] = torch.tensor([[sx, sy, sz] for sx in (-1.0, 1.0) for sy in (-1.0, 1.0) for sz in (-1.0, 1.0)], dtype=f64)   # the corners
    pts[8:12] = torch.tensor([[1e6, 0.0, 0.0], [-1e6, 0.25, 0.5], [0.5, 3.0, -0.5], [-3.0, -3.0, -3.0]], dtype=f64)   # beyond the clamp
    pts[12, 1] = float("nan")
    pts[13] = float("nan")
    return pts.float()


DIMS = [(9, 5, 3), (5, 9, 2), (3, 3, 9)]           # (size - 1) a power of two; non-cubic; a coarser level finer on one axis


def _cots(n, L, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, L, 4, generator=g) for _ in range(3)] + [torch.randn(n, 3, generator=g) for _ in range(2)]


def test_first_order_is_the_grid_sample_volume_gradient():
    pts = _lattice(1)
    f, *_ = _cots(pts.shape[0], len(DIMS), 2)
    ref = R.scatter(pts, DIMS, R.PLANAR, f=f)
    for l, size in enumerate(DIMS):
        want = _vol_grad(pts, size, f[:, l])
        got = _dense(ref[l], size)
        assert torch.allclose(got, want, rtol=1e-13, atol=1e-13), (l, float((got - want).abs().max()))
        ent, S, A, k = ref[l]
        assert bool((A >= S.abs()).all()) and bool((k >= 1).all())
        assert torch.equal(_vol_grad(pts, size, f[:, l].abs()).reshape(-1)[ent], A)     # weights >= 0: A is the gradient of |g|


def test_second_order_is_the_double_backward_of_grid_sample():
    pts = _lattice(3)
    _, mu, _, s_bar, _ = _cots(pts.shape[0], len(DIMS), 4)
    ref = R.scatter(pts, DIMS, R.PLANAR, s_bar=s_bar, mu=mu)
    for l, size in enumerate(DIMS):
        want = _vol_grad_dir(pts, size, s_bar, mu[:, l])
        got = _dense(ref[l], size)
        scale = float(want.abs().max())
        assert scale > 1.0
        assert float((got - want).abs().max()) <= 1e-9 * scale, (l, float((got - want).abs().max()))


def test_the_k17_combination_with_an_index_map_a_live_count_and_both_layouts():
    pts = _lattice(5, n=500)
    n_rows = 450
    g = torch.Generator().manual_seed(6)
    index = torch.randperm(500, generator=g)[:n_rows]
    count = 300
    f, mu, lam, s_bar, g_bar = _cots(n_rows, len(DIMS), 7)
    s_bar, g_bar = torch.randn(500, 3, generator=g), torch.randn(500, 3, generator=g)
    planar = R.scatter(pts, DIMS, R.PLANAR, f=f, s_bar=s_bar, mu=mu, g_bar=g_bar, lam=lam, index=index, count=count)
    packed = R.scatter(pts, DIMS, R.PACKED, f=f, s_bar=s_bar, mu=mu, g_bar=g_bar, lam=lam, index=index, count=count)
    live = index[:count]
    p = pts[live]
    for l, size in enumerate(DIMS):
        want = (_vol_grad(p, size, f[:count, l]) + _vol_grad_dir(p, size, s_bar[live], mu[:count, l])
                + _vol_grad_dir(p, size, g_bar[live], lam[:count, l]))
        scale = float(want.abs().max())
        for lay, ref in ((R.PLANAR, planar), (R.PACKED, packed)):
            got = _dense(ref[l], size, lay)
            assert float((got - want).abs().max()) <= 1e-9 * scale, (l, lay, float((got - want).abs().max()))
        # the same entries, sums and counts in both layouts
        nvox = size[0] * size[1] * size[2]
        ent_p, S_p, A_p, k_p = planar[l]
        ent_k, S_k, A_k, k_k = packed[l]
        as_packed = (ent_p % nvox) * 4 + ent_p // nvox
        order = torch.argsort(as_packed)
        assert torch.equal(as_packed[order], ent_k)
        assert torch.equal(S_p[order], S_k) and torch.equal(A_p[order], A_k) and torch.equal(k_p[order], k_k)
    # rows past the count add nothing; no rows, no entries
    none = R.scatter(pts, DIMS, R.PLANAR, f=f, s_bar=s_bar, mu=mu, g_bar=g_bar, lam=lam, index=index, count=0)
    assert all(ent.numel() == 0 for ent, _, _, _ in none)


def test_sums_absolute_sums_and_counts_against_a_loop():
    """S, A and k of a few points, corner by corner in plain Python floats (the float32 weights taken from axis_cell)."""
    pts = torch.tensor([[0.0, 0.5, -1.0], [0.25, 0.5, 1.0], [1.0, 1.0, 1.0], [-1.0078125, 0.3, 0.7], [0.1, 0.2, 0.3], [0.1, 0.2, 0.3],
                        [float("nan"), 0.0, 0.0], [5.0, 0.0, 0.0]])
    size = (7, 6, 5)
    f, mu, lam, s_bar, g_bar = _cots(pts.shape[0], 1, 9)
    ref = R.scatter(pts, [size], R.PACKED, f=f, s_bar=s_bar, mu=mu, g_bar=g_bar, lam=lam)[0]
    cells = [R.axis_cell(pts[:, ax], size[ax]) for ax in range(3)]
    S, A, K = {}, {}, {}
    for i in range(pts.shape[0]):
        for corner in [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]:
            ix = [int(cells[ax][0][i]) + corner[ax] for ax in range(3)]
            if not all(bool(cells[ax][3][i]) and 0 <= ix[ax] < size[ax] for ax in range(3)):
                continue
            w = [float(cells[ax][2 if corner[ax] else 1][i]) for ax in range(3)]
            dw = [(1 if corner[ax] else -1) * (size[ax] - 1) / 2 * w[(ax + 1) % 3] * w[(ax + 2) % 3] for ax in range(3)]
            for ch in range(4):
                e = ((ix[0] * size[1] + ix[1]) * size[2] + ix[2]) * 4 + ch
                parts_s = [dw[ax] * float(s_bar[i, ax]) for ax in range(3)]
                parts_g = [dw[ax] * float(g_bar[i, ax]) for ax in range(3)]
                wt = w[0] * w[1] * w[2]
                S[e] = S.get(e, 0.0) + wt * float(f[i, 0, ch]) + sum(parts_s) * float(mu[i, 0, ch]) + sum(parts_g) * float(lam[i, 0, ch])
                A[e] = A.get(e, 0.0) + abs(wt * float(f[i, 0, ch])) + sum(map(abs, parts_s)) * abs(float(mu[i, 0, ch])) \
                    + sum(map(abs, parts_g)) * abs(float(lam[i, 0, ch]))
                K[e] = K.get(e, 0) + 1
    ent, s, a, k = ref
    assert ent.tolist() == sorted(S)
    assert torch.allclose(s, torch.tensor([S[e] for e in sorted(S)], dtype=f64), rtol=1e-12, atol=1e-12)
    assert torch.allclose(a, torch.tensor([A[e] for e in sorted(S)], dtype=f64), rtol=1e-12, atol=1e-12)
    assert k.tolist() == [K[e] for e in sorted(S)]
    assert max(K.values()) == 2                                          # the repeated point


@pytest.mark.parametrize("size", [(7, 6, 11), (12, 7, 7)])
def test_random_points_on_other_grids(size):
    """(size - 1) no power of two: the reference's float32 weights and grid_sample's float64 ones differ by a few 2^-24 * size."""
    g = torch.Generator().manual_seed(size[0])
    pts = torch.rand(300, 3, generator=g) * 2.3 - 1.15
    f = torch.randn(300, 1, 4, generator=g)
    ent, S, A, k = R.scatter(pts, [size], R.PLANAR, f=f)[0]
    want = _vol_grad(pts, size, f[:, 0])
    got = _dense((ent, S, A, k), size)
    assert float((got - want).abs().max()) <= 64 * max(size) * R.U * float(A.max())


def test_weights_are_formed_in_float32():
    """At 256 voxels a float64 un-normalisation moves the weights by up to ~255 * 2^-24; the reference takes the kernels' float32 values."""
    x = torch.tensor([0.123456789, -0.87654321, 0.999999], dtype=torch.float32)
    i0, w0, w1, live = R.axis_cell(x, 256)
    pos32 = (x + 1.0) / 2.0 * 255.0
    assert pos32.dtype == torch.float32
    assert torch.equal(w1, (pos32 - torch.floor(pos32)).double()) and torch.equal(w0, ((torch.floor(pos32) + 1.0) - pos32).double())
    pos64 = (x.double() + 1.0) / 2.0 * 255.0
    assert float((w1 - (pos64 - torch.floor(pos64))).abs().max()) > 2.0 ** -24     # the two conventions do differ here
