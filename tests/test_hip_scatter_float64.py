"""The volume-gradient scatters against the float64 reference (tests/scatter_reference.py, itself pinned to F.grid_sample on the CPU by
tests/test_scatter_reference_cpu.py), entry by entry, at the sizes where they run.

    K17   gens_sdf_train_scatter (the fused training step's dV += w f + (grad w . s_bar) mu + (grad w . g_bar) lam), called as ops/sdf.py calls it
    K2    gens_lookup_volume_bwd / _bwd2 (a lane per float, or GENS_K2_SCATTER_PER_POINT) and _bwd_bricks / _bwd2_bricks, both layouts, both orders

The bound: every touched entry within (k + 8) 2^-24 A of the float64 sum S (k contributions, A the sum of |term|: the worst case of float32
sums in any order, plus a few roundings per term), so a correct kernel cannot fail it; every untouched entry exactly 0.  Into prefilled buffers:
untouched entries keep their bits, touched ones meet the bound with |prefill| added to A.  Each check prints its worst err / bound and the median
A / |S| per level (pytest -s)."""
import pytest
import torch

from tests import scatter_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from gens_amd import lib
    return lib


def check(what, grads, ref, prefill=None):
    """grads: the kernel's per-level gradient tensors; ref: R.scatter(...) in the same layout; prefill: what the buffers held before the call.
    -> the worst err / bound over the levels."""
    worst_all = 0.0
    for l, (g, (ent, S, A, k)) in enumerate(zip(grads, ref)):
        flat = g.reshape(-1)
        got = flat[ent].double()
        if prefill is not None:
            pf = prefill[l].reshape(-1)
            S, A = S + pf[ent].double(), A + pf[ent].double().abs()
        fin = torch.isfinite(S)
        err, b = (got - S).abs(), R.bound(k, A)
        bad = fin & ~(err <= b)
        ratio = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0))[fin]
        worst = float(ratio.max()) if ratio.numel() else 0.0
        nz = fin & (S != 0)
        med = float((A[nz] / S[nz].abs()).median()) if bool(nz.any()) else float("nan")
        print(f"{what} level {l}: {ent.numel()} entries, worst err/bound {worst:.3g}, median A/|S| {med:.3g}, most contributions {int(k.max()) if k.numel() else 0}")
        assert not bool(bad.any()), f"{what} level {l}: {int(bad.sum())} of {ent.numel()} entries past the bound, worst err/bound {worst:.3g}"
        inf = ~fin
        assert torch.equal(torch.isnan(got[inf]), torch.isnan(S[inf])), f"{what} level {l}: NaN pattern"
        assert torch.equal(got[inf & ~torch.isnan(S)], S[inf & ~torch.isnan(S)]), f"{what} level {l}: infinities"
        untouched = torch.ones(flat.numel(), dtype=torch.bool, device=flat.device)
        untouched[ent] = False
        rest = flat[untouched].view(torch.int32)
        want = torch.zeros_like(rest) if prefill is None else prefill[l].reshape(-1)[untouched].view(torch.int32)
        assert torch.equal(rest, want), f"{what} level {l}: {int((rest != want).sum())} untouched entries changed"
        worst_all = max(worst_all, worst)
    return worst_all


def _specials(dev):
    """Faces, corners, the centre, just outside, beyond the clamp, far away, NaN."""
    c = [[sx, sy, sz] for sx in (-1.0, 1.0) for sy in (-1.0, 1.0) for sz in (-1.0, 1.0)]
    faces = [[1.0, 0.3, -0.2], [-1.0, -0.7, 0.1], [0.4, 1.0, 0.5], [0.2, -1.0, -0.9], [-0.3, 0.6, 1.0], [0.8, 0.1, -1.0], [0.0, 0.0, 0.0],
             [-0.5, 0.0, 0.5], [-1.0 + 1 / 128, 1.0 - 3 / 64, 0.25]]
    out = [[1.003, 0.2, 0.1], [-1.004, -1.002, 0.5], [0.3, 1.0005, -1.0007], [2.5, 0.0, 0.0], [-3.0, -3.0, -3.0], [1e12, 0.0, 0.0], [0.0, -1e12, 0.0],
           [float("nan"), 0.1, 0.2], [float("nan")] * 3, [0.1, float("inf"), 0.2]]
    return torch.tensor(c + faces + out, dtype=torch.float32, device=dev)


def _points(n, seed, crowd=0, at=(0.31, -0.47, 0.12), spread=2e-3):
    """n points: uniform in and a little past the cube, `crowd` of them around `at`, the specials first."""
    g = torch.Generator().manual_seed(seed)
    pts = (torch.rand(n, 3, generator=g) * 2.2 - 1.1).cuda()
    sp = _specials("cuda")
    pts[:sp.shape[0]] = sp
    if crowd:
        pts[sp.shape[0]:sp.shape[0] + crowd] = (torch.randn(crowd, 3, generator=g) * spread + torch.tensor(at)).cuda()
    return pts


# ---------------------------------------------------------------------------------------------------------------------------------------- K17
def _k17(L, dims, pts, f, mu, lam, s_bar, g_bar, index, count, grads):
    n = f.shape[0]
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device="cuda")
    L.call("gens_sdf_train_scatter", L.int_table([x for d in dims for x in d]), len(dims), L.ptr(pts), L.ptr(g_bar), L.ptr(s_bar), L.ptr(f), L.ptr(mu),
           L.ptr(lam), L.ptr(index, torch.int64), n, L.ptr(cnt, torch.int32), L.ptr_table(grads), L.stream())
    torch.cuda.synchronize()


def _k17_rows(seed, n_pts=512 * 128 + 1024 + 2048, crowd=3000):
    """The fused step's rows: 512 rays x 128 samples (points along lines through the cube), 1 024 + 2 048 more, a crowded voxel, the specials."""
    g = torch.Generator().manual_seed(seed)
    o = torch.rand(512, 1, 3, generator=g) * 2 - 1
    d = torch.nn.functional.normalize(torch.randn(512, 1, 3, generator=g), dim=-1)
    t = torch.linspace(-1.2, 1.2, 128)[None, :, None]
    pts = torch.cat([(o + d * t).reshape(-1, 3), torch.rand(n_pts - 512 * 128, 3, generator=g) * 2 - 1]).cuda()
    sp = _specials("cuda")
    pts[:sp.shape[0]] = sp
    pts[sp.shape[0]:sp.shape[0] + crowd] = (torch.randn(crowd, 3, generator=g) * 1e-4 + torch.tensor([-0.2, 0.4, 0.6])).cuda()   # one voxel of 256^3
    return pts


@pytest.mark.parametrize("sizes", [[256, 128, 64, 32, 16], [256, 128, 64]])
def test_k17_scatter_at_step_size(L, sizes):
    dims = [(s, s, s) for s in sizes]
    nl = len(dims)
    pts = _k17_rows(1)
    n_pts = pts.shape[0]
    g = torch.Generator().manual_seed(2)
    index = torch.randperm(n_pts, generator=g).cuda()                  # compact row -> dense row, permuted
    count = n_pts - 4321                                                # the device count: rows past it add nothing
    f, mu, lam = [torch.randn(n_pts, nl, 4, generator=g).cuda() for _ in range(3)]
    s_bar, g_bar = [torch.randn(n_pts, 3, generator=g).cuda() for _ in range(2)]
    grads = [torch.zeros(4, *d, device="cuda") for d in dims]
    _k17(L, dims, pts, f, mu, lam, s_bar, g_bar, index, count, grads)
    ref = R.scatter(pts, dims, R.PLANAR, f=f, s_bar=s_bar, mu=mu, g_bar=g_bar, lam=lam, index=index, count=count)
    check(f"K17 {sizes}", grads, ref)
    assert max(int(k.max()) for _, _, _, k in ref) >= 1000                # the crowded voxel
    # g_bar = s_bar = NULL: the first term alone; no index map, no device count
    grads = [torch.zeros(4, *d, device="cuda") for d in dims]
    _k17(L, dims, pts, f, mu, lam, None, None, None, None, grads)
    check(f"K17 {sizes} w f only", grads, R.scatter(pts, dims, R.PLANAR, f=f))


def test_k17_scatter_adds_into_prefilled_buffers_and_small_calls(L):
    dims = [(48, 40, 36), (24, 20, 18), (12, 10, 9)]
    nl = len(dims)
    pts = _points(20000, 3, crowd=2000)
    g = torch.Generator().manual_seed(4)
    f, mu, lam = [torch.randn(20000, nl, 4, generator=g).cuda() for _ in range(3)]
    s_bar, g_bar = [torch.randn(20000, 3, generator=g).cuda() for _ in range(2)]
    pre = [torch.randn(4, *d, generator=g).cuda() for d in dims]
    grads = [p.clone() for p in pre]
    _k17(L, dims, pts, f, mu, lam, s_bar, g_bar, None, None, grads)
    check("K17 prefilled", grads, R.scatter(pts, dims, R.PLANAR, f=f, s_bar=s_bar, mu=mu, g_bar=g_bar, lam=lam), prefill=pre)
    # one point (a dense row picked by the index map), then none: a 0-point call and a device count of 0 leave the buffers alone
    one = torch.tensor([777], dtype=torch.int64, device="cuda")
    grads = [torch.zeros(4, *d, device="cuda") for d in dims]
    _k17(L, dims, pts, f[:1], mu[:1], lam[:1], s_bar, g_bar, one, None, grads)
    check("K17 one point", grads, R.scatter(pts, dims, R.PLANAR, f=f[:1], s_bar=s_bar, mu=mu[:1], g_bar=g_bar, lam=lam[:1], index=one))
    assert all(int((gr != 0).sum()) == 32 for gr in grads)
    for n, count in ((0, None), (100, 0)):
        grads = [p.clone() for p in pre]
        _k17(L, dims, pts, f[:n], mu[:n], lam[:n], s_bar, g_bar, None, count, grads)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(grads, pre))


# ---------------------------------------------------------------------------------------------------------------------------------------- K2
VARIANTS = ("lanes", "per_point", "bricks")


def _k2(L, monkeypatch, variant, layout, second, shapes, pts, g_out, gg_pts, grads):
    """One volume-gradient scatter of K2 into `grads` (the point outputs go to scratch)."""
    n, nl = pts.shape[0], len(shapes)
    vols = [torch.zeros(g.shape, device="cuda") for g in grads]          # (the values do not reach the volume gradient)
    dim_table = L.int_table([x for s in shapes for x in s])
    gp = torch.empty(n, 3, device="cuda")
    if variant == "per_point":
        monkeypatch.setenv("GENS_K2_SCATTER_PER_POINT", "1")
    else:
        monkeypatch.delenv("GENS_K2_SCATTER_PER_POINT", raising=False)
    scratch = torch.empty(max(L.load().gens_lookup_scatter_bricks_scratch_bytes(n), 16), device="cuda", dtype=torch.uint8)
    sc = (L.ptr(scratch, torch.uint8), scratch.numel())
    if not second:
        if variant == "bricks":
            L.call("gens_lookup_volume_bwd_bricks", L.ptr_table(vols), dim_table, nl, layout, L.ptr(pts), L.ptr(g_out), n, L.ptr_table(grads), L.ptr(gp), *sc,
                   L.stream())
        else:
            L.call("gens_lookup_volume_bwd", L.ptr_table(vols), dim_table, nl, layout, L.ptr(pts), L.ptr(g_out), n, L.ptr_table(grads), L.ptr(gp), L.stream())
    else:
        ggo = torch.empty(n, nl, 4, device="cuda")
        if variant == "bricks":
            L.call("gens_lookup_volume_bwd2_bricks", L.ptr_table(vols), dim_table, nl, layout, L.ptr(pts), L.ptr(g_out), L.ptr(gg_pts), None, n, L.ptr(ggo),
                   L.ptr_table(grads), L.ptr(gp), *sc, L.stream())
        else:
            L.call("gens_lookup_volume_bwd2", L.ptr_table(vols), dim_table, nl, layout, L.ptr(pts), L.ptr(g_out), L.ptr(gg_pts), None, n, L.ptr(ggo),
                   L.ptr_table(grads), L.ptr(gp), L.stream())
    monkeypatch.delenv("GENS_K2_SCATTER_PER_POINT", raising=False)
    torch.cuda.synchronize()


def _k2_all(L, monkeypatch, what, dims, pts, g_out, gg_pts, prefill_seed=None):
    """Every variant, both layouts, both orders, against the reference."""
    worst = 0.0
    for layout in (R.PLANAR, R.PACKED):
        shape = (lambda d: (4,) + tuple(d)) if layout == R.PLANAR else (lambda d: tuple(d) + (4,))    # noqa: E731
        for second in (False, True):
            ref = R.scatter(pts, dims, layout, s_bar=gg_pts, mu=g_out) if second else R.scatter(pts, dims, layout, f=g_out)
            for variant in VARIANTS:
                pre = None
                if prefill_seed is not None:
                    g = torch.Generator().manual_seed(prefill_seed)
                    pre = [torch.randn(shape(d), generator=g).cuda() for d in dims]
                grads = [p.clone() for p in pre] if pre is not None else [torch.zeros(shape(d), device="cuda") for d in dims]
                _k2(L, monkeypatch, variant, layout, second, dims, pts, g_out, gg_pts, grads)
                tag = f"K2 {what} {'packed' if layout else 'planar'} {'second' if second else 'first'} {variant}"
                worst = max(worst, check(tag, grads, ref, prefill=pre))
    return worst


def _cots(n, nl, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, nl, 4, generator=g).cuda(), torch.randn(n, 3, generator=g).cuda()


def test_k2_scatters_with_the_finest_level_at_the_brick_limit(L, monkeypatch):
    """256^3: 32 bricks per axis (BR_NB), every tile 9 wide; one brick holds ~3 000 points (several work items of BR_SEG, several BR_STAGE chunks)."""
    dims = [(256, 256, 256), (96, 96, 96)]
    pts = _points(60000, 5, crowd=3000)
    g_out, gg = _cots(pts.shape[0], len(dims), 6)
    _k2_all(L, monkeypatch, "256^3", dims, pts, g_out, gg)


def test_k2_scatters_past_the_brick_limit(L, monkeypatch):
    """264^3: 33 bricks per axis would be needed, bricks_fit refuses and the brick entries take the direct scatter; still right."""
    dims = [(264, 264, 264), (64, 64, 64)]
    pts = _points(40000, 7, crowd=1000)
    g_out, gg = _cots(pts.shape[0], len(dims), 8)
    _k2_all(L, monkeypatch, "264^3", dims, pts, g_out, gg)


def test_k2_scatters_with_a_coarser_level_finer_on_one_axis(L, monkeypatch):
    """The bricks are cut from the level with the most voxels; a level that is finer on z than that one has tiles wider than BR_EXT (clamped),
    so corners take the out-of-tile atomic.  Non-cubic dims; prefilled buffers too (the kernels add, they do not overwrite)."""
    dims = [(64, 64, 24), (24, 20, 96), (16, 12, 8)]
    assert 64 * 64 * 24 > 24 * 20 * 96
    pts = _points(50000, 9, crowd=2000, at=(0.1, -0.2, 0.3), spread=0.02)
    g_out, gg = _cots(pts.shape[0], len(dims), 10)
    _k2_all(L, monkeypatch, "finer on z", dims, pts, g_out, gg)
    _k2_all(L, monkeypatch, "finer on z, prefilled", dims, pts, g_out, gg, prefill_seed=11)


def test_k2_scatters_with_an_infinite_cotangent(L, monkeypatch):
    """+inf on a point that sits on a node of both levels (its zero-weight taps give inf * 0 = NaN), -inf on a point inside a cell: where the
    sums are infinite or NaN must match the reference's IEEE products."""
    dims = [(41, 41, 41), (21, 21, 21)]
    pts = _points(20000, 12)
    pts[100] = torch.tensor([-0.5, 0.0, 0.5])                         # pos 10 / 20 / 30 of 40 and 5 / 10 / 15 of 20: exact nodes
    pts[101] = torch.tensor([0.123, -0.456, 0.789])
    g_out, gg = _cots(pts.shape[0], len(dims), 13)
    g_out[100, :, 1] = float("inf")
    g_out[101, :, 2] = float("-inf")
    ref = R.scatter(pts, dims, R.PLANAR, f=g_out)
    assert all(bool(torch.isnan(S).any()) and bool(torch.isinf(S).any()) for _, S, _, _ in ref)
    _k2_all(L, monkeypatch, "inf cotangent", dims, pts, g_out, gg)


def test_k2_empty_call_leaves_the_buffers(L, monkeypatch):
    dims = [(20, 20, 20)]
    pre = [torch.randn(4, 20, 20, 20).cuda()]
    for variant in VARIANTS:
        for second in (False, True):
            grads = [p.clone() for p in pre]
            _k2(L, monkeypatch, variant, R.PLANAR, second, dims, torch.empty(0, 3, device="cuda"), torch.empty(0, 1, 4, device="cuda"),
                torch.empty(0, 3, device="cuda"), grads)
            assert torch.equal(grads[0].view(torch.int32), pre[0].view(torch.int32))


def test_k2_shipped_levels_take_the_bricks_through_autograd(L, monkeypatch):
    """The shipped five levels, 262 144 points: ops.lookup_volume's backward and double backward pick the brick entries by themselves (the default
    kernels.k2_bricks_min), and their volume gradients meet the bound."""
    from gens_amd import ops
    sizes = [256, 128, 64, 32, 16]
    dims = [(s, s, s) for s in sizes]
    n = 262144
    assert n >= ops.kernels.k2_bricks_min
    pts = _points(n, 14, crowd=4000)
    g_out, gg = _cots(n, len(dims), 15)
    calls = []
    real = L.call
    monkeypatch.setattr(L, "call", lambda nm, *a, **k: (calls.append(nm), real(nm, *a, **k))[1])
    vols = [torch.zeros(1, 4, s, s, s, device="cuda", requires_grad=True) for s in sizes]
    p = pts.clone().requires_grad_(True)
    y = ops.lookup_volume(p, vols)
    first = torch.autograd.grad(y, vols, g_out.reshape(n, -1), retain_graph=True)
    gp, = torch.autograd.grad(y, p, g_out.reshape(n, -1), create_graph=True)
    second = torch.autograd.grad(gp, vols, gg)
    monkeypatch.setattr(L, "call", real)
    assert "gens_lookup_volume_bwd_bricks" in calls and "gens_lookup_volume_bwd2_bricks" in calls, calls
    assert "gens_lookup_volume_bwd" not in calls and "gens_lookup_volume_bwd2" not in calls, calls
    check("K2 shipped first (autograd)", list(first), R.scatter(pts, dims, R.PLANAR, f=g_out))
    check("K2 shipped second (autograd)", list(second), R.scatter(pts, dims, R.PLANAR, s_bar=gg, mu=g_out))
