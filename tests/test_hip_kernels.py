"""GPU parity: every HIP kernel (through the C ABI, via gens_amd.ops) against the reference's golden vectors and
against the CPU oracle on seeded inputs.  Tolerances: float32 round-off (1e-5 abs/rel unless a comment says why)."""
import pytest
import torch

from oracle import gens_oracle as K

pytestmark = pytest.mark.gpu


def dev(t):
    if isinstance(t, (list, tuple)):
        return [dev(x) for x in t]
    return t.cuda()


def close(a, b, atol=1e-5, rtol=1e-5, what="", frac=0.0):
    a, b = torch.as_tensor(a).detach().float().cpu(), torch.as_tensor(b).detach().float().cpu()
    assert a.shape == b.shape, f"{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    if a.numel() == 0:
        return
    bad = (a - b).abs() > atol + rtol * b.abs()
    assert bad.float().mean().item() <= frac, f"{what}: {int(bad.sum())}/{bad.numel()} off, max err {(a - b).abs().max().item():.3e}"


@pytest.fixture(scope="module")
def ops():
    from gens_amd import ops
    return ops


# --------------------------------------------------------------------------------------------------- K1
@pytest.mark.parametrize("bwd", ["window", "auto"])
def test_k1_volume_golden_c1(ops, golden, bwd, monkeypatch):
    monkeypatch.setattr(ops.kernels, "k1_bwd", bwd)      # both backward kernels against the reference
    g = golden("g1a_volume_c1")
    feat = dev(g["feat"]).requires_grad_(True)
    v, m = ops.volume_build([feat], dev(g["intrs"]), dev(g["c2ws"]), [16])
    close(v[0], g["volume"], atol=5e-5, rtol=1e-4, what="volume")  # var = E[x^2]-E[x]^2 cancels
    close(m[0], g["mask"], atol=0, rtol=0, what="mask")
    (v[0] * dev(g["cot"])).sum().backward()
    close(feat.grad, g["gfeat"], atol=2e-5, what="d/dfeat")


@pytest.mark.parametrize("bwd", ["window", "auto"])
def test_k1_volume_golden_backward_over_image_tiles(ops, golden, bwd, monkeypatch):
    """4 views 96 x 160, one 32^3 volume: the image-tile backward spreads every view over 2 x 3 tiles (and the 4 x 16 voxel wave tiles over up to
    2 x 2 of them); the reference's own gradient."""
    monkeypatch.setattr(ops.kernels, "k1_bwd", bwd)
    g = golden("g1c_volume_tiles")
    feat = dev(g["feat"]).requires_grad_(True)
    v, m = ops.volume_build([feat], dev(g["intrs"]), dev(g["c2ws"]), [32])
    close(m[0], g["mask"], atol=0, rtol=0, what="mask")
    (v[0] * dev(g["cot"])).sum().backward()
    # a voxel projecting within an ulp of an image border may flip visibility in one view (count 3 <-> 4: the mask stays, its taps move by 1e-4).
    # Which voxels do depends on the last bit of inverse(c2ws): the golden's came from LAPACK's float32 LU on the CPU, the device's is the
    # correctly rounded inverse (gens_scene_setup; rocSOLVER's LU, used until round 2, flipped 0.2 % of the texels, this one 0.3 %)
    close(feat.grad, g["gfeat"], atol=2e-5, what="d/dfeat", frac=5e-3)
    close(feat.grad, g["gfeat"], atol=2e-4, what="d/dfeat")


def test_k1_volume_golden_multiscale(ops, golden):
    g = golden("g1b_volume_ms")
    dims = [int(d) for d in g["dims"]]
    feats = [dev(g[f"feat{i}"]).requires_grad_(True) for i in range(3)]
    v, m = ops.volume_build(feats, dev(g["intrs"]), dev(g["c2ws"]), dims)
    for i in range(3):
        close(v[i], g[f"volume{i}"], atol=5e-5, rtol=1e-4, what=f"volume{i}")
        close(m[i], g[f"mask{i}"], atol=0, rtol=0, what=f"mask{i}")
    sum((a * dev(g[f"cot{i}"])).sum() for i, a in enumerate(v)).backward()
    for i in range(3):
        close(feats[i].grad, g[f"gfeat{i}"], atol=5e-5, what=f"gfeat{i}")


def test_k1_volume_vs_oracle_480x640(ops):
    from gens_amd import synthetic
    sc = synthetic.make_scene(nv=5, h=480, w=640, n_levels=5, seed=3)
    # band-limited features (period >= 40 px): white noise has O(1)/px gradients, which turns the 1e-4 px float32
    # uncertainty of a projected coordinate near x=640 into 1e-3 value differences between ANY two implementations
    for i, f in enumerate(sc["features"]):
        nv, c, h, w = f.shape
        yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
        ph = torch.arange(nv * c, dtype=torch.float32).reshape(nv, c, 1, 1)
        sc["features"][i] = torch.sin(xx * (0.15 * 2 ** i / (1 + ph % 3)) + yy * (0.11 * 2 ** i) + ph) * (1 + 0.1 * ph)
    dims = [48, 32, 24, 16, 8]
    ref_v, ref_m = K.volume_build(sc["features"], sc["intrs"], sc["c2ws"], dims)
    v, m = ops.volume_build(dev(sc["features"]), dev(sc["intrs"]), dev(sc["c2ws"]), dims)
    for i in range(5):
        # a voxel projecting within an ulp of the image border may flip visibility in one view
        close(m[i], ref_m[i], atol=0, rtol=0, what=f"mask{i}", frac=1e-4)
        close(v[i], ref_v[i], atol=5e-5, rtol=1e-4, what=f"volume{i}", frac=1e-4)


# --------------------------------------------------------------------------------------------------- K2
@pytest.mark.parametrize("packed", [False, True])
def test_k2_lookup_golden(ops, golden, packed):
    g = golden("g2_lookup")
    vols = [dev(g[f"vol{i}"]) for i in range(3)]
    pts = dev(g["pts"]).requires_grad_(True)
    if packed:
        vol_arg = ops.VolumeSet.packed(vols)
    else:
        vols = [v.requires_grad_(True) for v in vols]
        vol_arg = vols
    y = ops.lookup_volume(pts, vol_arg)
    close(y, g["feats"], what="fwd")
    go = dev(g["gO"]).requires_grad_(True)
    targets = [pts] if packed else [pts] + vols
    grads = torch.autograd.grad(y, targets, go, create_graph=True)
    close(grads[0], g["gP"], atol=2e-5, what="gP")
    if not packed:
        for i in range(3):
            close(grads[1 + i], g[f"gV{i}"], atol=2e-5, what=f"gV{i}")
    outs = torch.autograd.grad(grads[0], [go, pts] + ([] if packed else vols), dev(g["ggG"]))
    close(outs[0], g["ggO"], atol=5e-5, what="ggO")
    close(outs[1], g["gP2"], atol=2e-4, rtol=1e-4, what="gP2")
    if not packed:
        for i in range(3):
            close(outs[2 + i], g[f"gV2_{i}"], atol=5e-5, what=f"gV2_{i}")


def test_k2_second_order_with_volume_cotangent_vs_oracle(ops):
    """grad2_3d's `grad2_grad_input` branch (gridsample_cuda.cu:345, 449-452): cotangent on the volume gradient."""
    g = torch.Generator().manual_seed(7)
    dims = [9, 6]
    vols = [torch.randn(1, 4, d, d, d, generator=g) for d in dims]
    pts = torch.rand(500, 3, generator=g) * 2.4 - 1.2
    go = torch.randn(500, 8, generator=g)
    ggp = torch.randn(500, 3, generator=g)
    ggv = [torch.randn(1, 4, d, d, d, generator=g) for d in dims]
    ref = K.lookup_volume_bwd2(ggv, ggp, go, vols, pts)
    dv = [dev(v).requires_grad_(True) for v in vols]
    dp = dev(pts).requires_grad_(True)
    dgo = dev(go).requires_grad_(True)
    grads = torch.autograd.grad(ops.lookup_volume(dp, dv), [dp] + dv, dgo, create_graph=True)
    phi = (grads[0] * dev(ggp)).sum() + sum((a * dev(b)).sum() for a, b in zip(grads[1:], ggv))
    outs = torch.autograd.grad(phi, [dgo, dp] + dv)
    close(outs[0], ref[0], atol=5e-5, what="ggO")
    close(outs[1], ref[2], atol=3e-4, rtol=1e-4, what="gP2")
    for i in range(2):
        close(outs[2 + i], ref[1][i], atol=5e-5, what=f"gV2_{i}")


def test_k2_lookup_large_vs_oracle(ops):
    g = torch.Generator().manual_seed(8)
    dims = [64, 32, 16, 8, 4]
    vols = [0.1 * torch.randn(1, 4, d, d, d, generator=g) for d in dims]
    pts = torch.rand(20000, 3, generator=g) * 2.2 - 1.1
    ref = K.lookup_volume(vols, pts)
    close(ops.lookup_volume(dev(pts), dev(vols)), ref, what="planar")
    close(ops.lookup_volume(dev(pts), ops.VolumeSet.packed(dev(vols))), ref, what="packed")
    assert ops.lookup_volume(dev(pts[:0]), dev(vols)).shape == (0, 20)   # empty input


# --------------------------------------------------------------------------------------------------- K3
def test_k3_nearest_golden(ops, golden):
    g = golden("g3_nearest")
    masks = [dev(g[f"mask{i}"]) for i in range(3)]
    valid, vals = ops.lookup_mask(dev(g["pts"]), masks, return_values=True)
    close(vals, g["val"], atol=0, rtol=0, what="values")
    assert torch.equal(valid.cpu(), g["any"])


def test_k3_ray_points_vs_oracle(ops):
    from gens_amd import synthetic
    g = torch.Generator().manual_seed(9)
    sc = synthetic.make_scene(nv=3, h=48, w=64, n_levels=1, seed=4)
    ro, rd = synthetic.make_rays(sc["intrs"], sc["c2ws"], 48, 64, step=4)
    masks = [(torch.rand(1, 1, d, d, d, generator=g) > 0.4).float() for d in (32, 16, 8)]
    for n in (37, 64, 128):            # 37: ray and sample index by division; 64 and 128: by shift and mask
        z = torch.sort(torch.rand(ro.shape[0], n, generator=g) * 2.2 + 1.1, -1)[0]
        for mid in (False, True):
            if mid:
                dist = torch.cat([z[:, 1:] - z[:, :-1], torch.full((z.shape[0], 1), 1 / 32)], -1)
                zz = z + dist * 0.5
            else:
                zz = z
            ref_pts = (ro[:, None] + rd[:, None] * zz[..., None]).reshape(-1, 3)
            pts, valid = ops.ray_points(dev(ro), dev(rd), dev(z), dev(masks), mid=mid, sample_dist=1 / 32)
            close(pts, ref_pts, atol=1e-6, what=f"pts n={n}")
            ref_valid = K.point_valid(masks, pts.cpu())
            assert torch.equal(valid.cpu(), ref_valid)


# --------------------------------------------------------------------------------------------------- K4
def test_k4_lookup_feature_golden(ops, golden):
    g = golden("g4_feature")
    feats = [dev(g[f"feat{i}"]).requires_grad_(True) for i in range(5)]
    imgs = dev(g["imgs"]).requires_grad_(True)
    views = ops.SceneViews(imgs, dev(g["intrs"]), dev(g["c2ws"]), feats)
    fv, rd, mk = ops.lookup_feature(dev(g["pts"]), views)
    assert torch.equal(mk.cpu(), g["mask"])
    close(rd, g["ray_diff"], atol=2e-5, what="ray_diff")
    close(fv, g["feat_views"], atol=2e-5, rtol=1e-4, what="feat_views")
    grads = torch.autograd.grad((fv * dev(g["cot"])).sum(), feats + [imgs])
    for i in range(5):
        close(grads[i], g[f"gfeat{i}"], atol=1e-4, what=f"gfeat{i}")
    close(grads[5], g["gimgs"], atol=1e-4, what="gimgs")


def test_k4_ragged_and_empty(ops, golden):
    g = golden("g4_feature")
    feats = [dev(g[f"feat{i}"]) for i in range(5)]
    views = ops.SceneViews(dev(g["imgs"]), dev(g["intrs"]), dev(g["c2ws"]), feats)
    for n in (0, 1, 85, 256):     # 85*3 rows is not a multiple of the 256-row block
        fv, rd, mk = ops.lookup_feature(dev(g["pts"][:n]), views)
        close(fv, g["feat_views"][:n], atol=2e-5, rtol=1e-4, what=f"n={n}")
        assert torch.equal(mk.cpu(), g["mask"][:n])


# --------------------------------------------------------------------------------------------------- K5-K7
def test_k5_k7_golden(ops, golden):
    g = golden("g5_upsample")
    masks = [dev(g[f"mask{i}"]) for i in range(3)]
    ro, rd = dev(g["rays_o"]), dev(g["rays_d"])
    for r in range(4):
        zn, pts_new, valid_new = ops.upsample(ro, rd, dev(g[f"z{r}"]), dev(g[f"sdf{r}"]), 16, masks, 64 * 2 ** r)
        close(zn, g[f"znew{r}"], atol=5e-5, what=f"z_new round {r}")
        ref_pts = (g["rays_o"][:, None] + g["rays_d"][:, None] * zn.cpu()[..., None]).reshape(-1, 3)
        close(pts_new, ref_pts, atol=1e-6, what="pts_new")
        assert torch.equal(valid_new.cpu(), K.point_valid([g[f"mask{i}"] for i in range(3)], pts_new.cpu()))
        zc, _ = ops.merge_samples(dev(g[f"z{r}"]), dev(g[f"znew{r}"]))
        close(zc, g[f"zcat{r}"], atol=0, rtol=0, what="merged z")


def test_k7_merge_with_sdf_and_ties_vs_oracle(ops):
    g = torch.Generator().manual_seed(11)
    for n, n_new in ((64, 16), (112, 16), (5, 3), (100, 28), (64, 64), (127, 1), (1, 64), (63, 2)):
        z = torch.sort(torch.rand(9, n, generator=g), -1)[0]
        zn = torch.sort(torch.rand(9, n_new, generator=g), -1)[0]
        zn[0, :2] = z[0, min(3, n - 1)]   # ties between old and new, and among new
        zn[1] = z[1, -1] + 1.0         # all new samples after the last old one
        zn[2] = z[2, 0] - 1.0          # all before
        zn[0] = torch.sort(zn[0])[0]
        if (n, n_new) == (63, 2):      # a tie across the two register slots of a lane: the last old sample (merged index 62) and a new one (63)
            zn[3, 0], zn[3, 1] = z[3, 62], z[3, 62] + 0.1
        if n >= 64:                    # and one between old sample 63 and a new one, which lands on merged index 64 or later
            zn[4, 0] = z[4, 63]
            zn[4] = torch.sort(zn[4])[0]
        s, sn = torch.randn(9, n, generator=g), torch.randn(9, n_new, generator=g)
        rz, rs = K.merge_samples(z, zn, s, sn)
        oz, os_ = ops.merge_samples(dev(z), dev(zn), dev(s), dev(sn))
        close(oz, rz, atol=0, rtol=0, what="z")
        close(os_, rs, atol=0, rtol=0, what="sdf")


def test_bit_packed_masks_and_carried_validity_change_nothing(ops, golden):
    """The scene path reads masks as 1 bit per voxel and carries each sample's mask decision through the merges instead of
    looking all n samples up again every round (implicit_surface.py:66-67): decisions and samples must be identical."""
    g = golden("g5_upsample")
    mask_list = [dev(g[f"mask{i}"]) for i in range(3)]
    mset = ops.VolumeSet.masks(mask_list)
    ro, rd = dev(g["rays_o"]), dev(g["rays_d"])
    # K3: float masks vs bit masks, incl. points outside the cube and half-integer ties (scaled rays leave [-1, 1]^3)
    for scale in (1.0, 1.7):
        z = dev(g["z0"]) * scale
        p0, v0 = ops.ray_points(ro, rd, z, mask_list, mid=True, sample_dist=1 / 32)
        p1, v1 = ops.ray_points(ro, rd, z, mset, mid=True, sample_dist=1 / 32)
        assert torch.equal(p0, p1) and torch.equal(v0, v1) and 0 < int(v0.sum()) < v0.numel()
    # K5-K7: four rounds, once as the reference does it and once with bits + carried validity
    z_a = z_b = dev(g["z0"])
    s_a = s_b = dev(g["sdf0"])
    _, valid = ops.ray_points(ro, rd, z_b, mset)
    valid = valid.reshape(z_b.shape)
    gen = torch.Generator().manual_seed(3)
    for r in range(4):
        za, pa, va = ops.upsample(ro, rd, z_a, s_a, 16, mask_list, 64 * 2 ** r)
        zb, pb, vb = ops.upsample(ro, rd, z_b, s_b, 16, mset, 64 * 2 ** r, valid_in=valid)
        assert torch.equal(za, zb) and torch.equal(pa, pb) and torch.equal(va, vb)
        s_new = dev(torch.randn(za.shape, generator=gen) * 0.1)
        z_a, s_a = ops.merge_samples(z_a, za, s_a, s_new)
        z_b, s_b, valid = ops.merge_samples(z_b, zb, s_b, s_new, valid, vb)
        assert torch.equal(z_a, z_b) and torch.equal(s_a, s_b)
        _, again = ops.ray_points(ro, rd, z_b, mask_list)
        assert torch.equal(valid.reshape(-1), again)            # the carried flags ARE the look-up of the merged samples


# --------------------------------------------------------------------------------------------------- K8
def _composite_case(b, n, s, seed, smooth=True, placed=False):
    """placed: the first valid sign change of ray r (r >= 2) sits at segment r mod (n - 1): both of its samples valid, the SDF positive up to
    it (an invalid sample's 100 is positive too) and negative right behind it."""
    from gens_amd import synthetic
    g = torch.Generator().manual_seed(seed)
    sc = synthetic.make_scene(nv=s + 1, h=48, w=64, n_levels=1, seed=seed)
    pix = torch.stack([torch.randint(0, 64, (b,), generator=g), torch.randint(0, 48, (b,), generator=g)], -1)
    ro, rd = synthetic.make_rays(sc["intrs"], sc["c2ws"], 48, 64, pixels=pix)
    z = torch.sort(torch.rand(b, n, generator=g) * 2.3 + 1.1, -1)[0]
    mid = (ro[:, None] + rd[:, None] * z[..., None])
    vm = (torch.rand(b, n, generator=g) > 0.25).float()
    vm[0] = 0                       # a ray with no valid sample at all
    vm[1] = 1
    sdf = torch.linalg.norm(mid, dim=-1) - 0.55 + 0.03 * torch.randn(b, n, generator=g)
    if placed:
        rows, j = torch.arange(2, b), torch.arange(n)[None]
        k = rows % (n - 1)
        vm[rows, k] = 1
        vm[rows, k + 1] = 1
        mag = sdf[2:].abs().clamp_min(1e-3)
        sdf[2:] = torch.where(j <= k[:, None], mag, torch.where(j == k[:, None] + 1, -mag, sdf[2:]))
    sdf = torch.where(vm > 0, sdf, torch.full_like(sdf, 100.0))
    grad = torch.nn.functional.normalize(mid, dim=-1) + 0.2 * torch.randn(b, n, 3, generator=g)
    grad = grad * vm[..., None]
    col = torch.rand(b, n, 3, generator=g) * vm[..., None]
    sm = torch.randn(b, n, 3, generator=g) * vm[..., None] if smooth else None
    vis = (torch.rand(b, n, s, generator=g) > 0.3) & (vm[..., None] > 0)
    return dict(ro=ro, rd=rd, z=z, sdf=sdf, grad=grad, col=col, sm=sm, vm=vm, vis=vis, c2w=sc["c2ws"][0])


@pytest.mark.parametrize("n,cos_anneal,inv_s", [(128, 0.5, 20.0), (128, 1.0, 300.0), (70, 0.0, 64.0), (2, 0.5, 20.0), (64, 1.0, 64.0), (65, 0.5, 64.0)])
def test_k8_composite_fwd_bwd_vs_oracle(ops, n, cos_anneal, inv_s):
    """n = 2, 64, 65: the smallest ray, a ray that fills the lower register slots exactly, and one sample more; 70 rays with the first valid sign
    change of ray r placed at segment r mod (n - 1), so that at n = 65 ray 63 crosses between samples 63 and 64 -- pick2 across a lane's two
    slots and the crossing index taken from the upper slots' ballot, forward and backward."""
    if n in (2, 64, 65):
        c = _composite_case(b=70, n=n, s=3, seed=20 + n, placed=True)
        assert n < 65 or int(torch.argmax((c["sdf"][63, :-1] * c["sdf"][63, 1:] <= 0).float())) == 63
    else:
        c = _composite_case(b=37, n=n, s=3, seed=20 + n)
    leaf = lambda t: t.clone().requires_grad_(True)  # noqa: E731
    # oracle
    o_in = [leaf(c["sdf"]), leaf(c["grad"]), leaf(c["sm"]), leaf(c["col"]), torch.tensor(inv_s, requires_grad=True)]
    ref = K.composite(c["ro"], c["rd"], c["z"], 1 / 32, o_in[0], o_in[1], o_in[2], o_in[3], c["vm"], c["vis"], o_in[4], cos_anneal, c["c2w"])
    # HIP
    d_in = [leaf(dev(c["sdf"])), leaf(dev(c["grad"])), leaf(dev(c["sm"])), leaf(dev(c["col"])), torch.tensor([inv_s], device="cuda", requires_grad=True)]
    out = ops.composite(dev(c["ro"]), dev(c["rd"]), dev(c["z"]), 1 / 32, d_in[0], d_in[1], d_in[2], d_in[3], dev(c["vm"]) > 0,
                        dev(c["vis"]), d_in[4], cos_anneal, dev(c["c2w"]))
    b = c["z"].shape[0]
    if n in (2, 64, 65):
        assert torch.equal(out["cross_idx"][2:].cpu().long(), torch.arange(2, b) % (n - 1))      # the placed crossings, 63 among them at n = 65
    close(out["color"], ref["color_fine"], atol=2e-5, rtol=1e-4, what="color")
    close(out["normal"], ref["normal"], atol=2e-5, rtol=1e-4, what="normal")
    close(out["depth"], ref["render_depth"], atol=2e-5, rtol=1e-4, what="depth")
    close(out["weights"], ref["weights"], atol=1e-5, rtol=1e-4, what="weights")
    close(out["wsum"], ref["weight_sum"][:, 0], atol=2e-5, rtol=1e-4, what="wsum")
    close(out["wmax"], ref["weight_max"][:, 0], atol=1e-5, rtol=1e-4, what="wmax")
    close(out["inside"], ref["inside_sphere"], atol=0, rtol=0, what="inside")
    assert torch.equal(out["valid"].cpu().bool(), ref["valid_mask"][:, 0])
    close(out["mid_in"], ref["mid_inside_sphere"][:, 0], atol=0, rtol=0, what="mid_inside_sphere")
    close(out["sdf_depth"], ref["sdf_depth"][:, 0], atol=2e-5, rtol=1e-4, what="sdf_depth")
    ge = out["eik_num"].sum() / (out["eik_den"].sum() + 1e-5)
    close(ge, ref["gradient_error"], atol=1e-5, rtol=1e-4, what="gradient_error")
    se = torch.linalg.norm(out["smooth_vec"], dim=-1).abs().mean()
    close(se, ref["smooth_error"], atol=1e-5, rtol=1e-4, what="smooth_error")
    ref_zc = ((ref["pts_sdf0"][:, 0] - c["ro"]) * c["rd"]).sum(-1)
    close(out["z_cross"], ref_zc, atol=1e-4, rtol=1e-4, what="z_cross")

    # backward: one scalar made of every differentiable output
    g = torch.Generator().manual_seed(5)
    wc, wn, wd, ww, wz = (torch.randn(b, 3, generator=g), torch.randn(b, 3, generator=g), torch.randn(b, generator=g),
                          torch.randn(b, n, generator=g), torch.randn(b, generator=g))
    loss_ref = ((ref["color_fine"] * wc).sum() + (ref["normal"] * wn).sum() + (ref["render_depth"] * wd).sum() + (ref["weights"] * ww).sum()
                + 0.3 * ref["weight_sum"].sum() + 2.0 * ref["gradient_error"] + 1.5 * ref["smooth_error"]
                + (((ref["pts_sdf0"][:, 0] - c["ro"]) * c["rd"]).sum(-1) * wz).sum())
    loss_hip = ((out["color"] * dev(wc)).sum() + (out["normal"] * dev(wn)).sum() + (out["depth"] * dev(wd)).sum()
                + (out["weights"] * dev(ww)).sum() + 0.3 * out["wsum"].sum() + 2.0 * ge + 1.5 * se + (out["z_cross"] * dev(wz)).sum())
    g_ref = torch.autograd.grad(loss_ref, o_in)
    g_hip = torch.autograd.grad(loss_hip, d_in)
    names = ["d/dsdf", "d/dgradients", "d/dsmooth", "d/dcolor", "d/dinv_s"]
    for a, r_, nm in zip(g_hip, g_ref, names):
        scale = float(r_.abs().max()) + 1e-12
        # the cumprod backward divides by (1 - alpha + 1e-7): error grows where alpha ~ 1, so compare relative to the tensor's scale
        close(a.reshape(r_.shape) / scale, r_ / scale, atol=2e-4, rtol=2e-3, what=nm)


def test_k8_inference_without_smooth_or_visibility(ops):
    c = _composite_case(b=9, n=128, s=2, seed=77, smooth=False)
    ref = K.composite(c["ro"], c["rd"], c["z"], 1 / 32, c["sdf"], c["grad"], torch.zeros_like(c["grad"]), c["col"], c["vm"], c["vis"],
                      torch.tensor(50.0), 1.0, c["c2w"])
    out = ops.composite(dev(c["ro"]), dev(c["rd"]), dev(c["z"]), 1 / 32, dev(c["sdf"]), dev(c["grad"]), None, dev(c["col"]), dev(c["vm"]) > 0,
                        None, torch.tensor([50.0], device="cuda"), 1.0, dev(c["c2w"]))
    close(out["color"], ref["color_fine"], atol=2e-5, rtol=1e-4, what="color")
    close(out["depth"], ref["render_depth"], atol=2e-5, rtol=1e-4, what="depth")
    assert not out["valid"].any()


# --------------------------------------------------------------------------------------------------- K9
def test_k9_patch_sample_golden(ops, golden):
    """The sampling half of surface_patch_warp: feed the oracle's homography coordinates, compare with the reference patches."""
    g = golden("g7_patchwarp")
    imgs = g["images"]
    nv, c, h, w = imgs.shape
    tex = ops.pack_nchw(dev(imgs))
    ref, src = g["ref_val"], g["src_val"]
    # coordinates of the reference patch: the pixel of each surface point + the 11x11 offsets
    from oracle.gens_oracle import patch_warp
    pts = g["pts"].clone().requires_grad_(True)
    r_or, s_or = patch_warp(pts, g["normals"], imgs, g["intrs"], g["c2ws"])
    close(r_or, ref, atol=2e-4, rtol=1e-4, what="oracle sanity")
    from gens_amd.models.modules import projector
    r_hip, s_hip = projector.surface_patch_warp(dev(g["pts"]).requires_grad_(True), dev(g["normals"]), (tex, c), dev(g["intrs"]), dev(g["c2ws"]))
    close(r_hip, ref, atol=2e-4, rtol=1e-4, what="ref patch")
    close(s_hip[:, 1:], src[:, 1:], atol=2e-3, rtol=1e-3, what="src patch")


def test_k9_patch_warp_gradient_golden(ops, golden):
    g = golden("g7_patchwarp")
    from gens_amd.models.modules import projector
    tex = ops.pack_nchw(dev(g["images"]))
    pts = dev(g["pts"]).requires_grad_(True)
    _, s_hip = projector.surface_patch_warp(pts, dev(g["normals"]), (tex, 12), dev(g["intrs"]), dev(g["c2ws"]))
    gp = torch.autograd.grad((s_hip[:, 1:] * dev(g["cot"])[:, 1:]).sum(), pts)[0]
    close(gp, g["gpts"], atol=2e-2, rtol=2e-3, what="d/dpts")


def test_k9_warp_feature_upsampling_vs_oracle(ops):
    g = torch.Generator().manual_seed(13)
    lv = [torch.randn(3, 4, 48 >> i, 64 >> i, generator=g) for i in range(3)]
    tex, c = ops.build_warp_features(dev(lv))
    ref = torch.cat([lv[0], K.upsample_bilinear_half_pixel(lv[1], 48, 64), K.upsample_bilinear_half_pixel(lv[2], 48, 64)], 1)
    close(tex.permute(0, 3, 1, 2)[:, :c], ref, atol=1e-6, what="warp feats")
    torch_ref = torch.nn.functional.interpolate(lv[2], size=(48, 64), mode="bilinear")
    close(tex.permute(0, 3, 1, 2)[:, 8:12], torch_ref, atol=1e-6, what="vs F.interpolate")


@pytest.mark.parametrize("layout", ["planar", "packed"])
@pytest.mark.parametrize("dims", [[64, 32, 16], [40, 24], [20]])
def test_k2_brick_scatter_equals_the_direct_scatter(ops, dims, layout):
    """gens_lookup_volume_bwd_bricks / _bwd2_bricks against the direct scatter of gens_lookup_volume_bwd / _bwd2: volume gradients (first and second
    order) equal up to the order of the float sums; the point gradients are the same kernels'.  Points: uniform in the cube, a cluster that fills a
    few bricks, points on the faces, outside the cube, far outside and a NaN -- every path of the brick kernel (tile, out-of-tile fallback, bounds)."""
    from gens_amd import lib as L
    g = torch.Generator().manual_seed(31)
    n = 6000
    pts = torch.rand(n, 3, generator=g) * 2 - 1
    pts[1000:3000] = torch.randn(2000, 3, generator=g) * 0.03 + torch.tensor([0.31, -0.4, 0.77])
    pts[4000:5500] = torch.randn(1500, 3, generator=g) * 0.004 + torch.tensor([-0.52, 0.13, -0.2])      # one crowded brick: several work items, several chunks each
    pts[3000:3200] = pts[3000:3200].sign()
    pts[3200:3400] = pts[3200:3400] * 1.2
    pts[3400:3410] = 1e12
    pts[3410] = float("nan")
    pts = pts.cuda()
    nl = len(dims)
    if layout == "planar":
        vols = [torch.randn(4, d, d + 2 * (d > 20), d, generator=g).cuda() for d in dims]
        shapes = [v.shape[1:] for v in vols]
    else:
        vols = [torch.randn(d, d + 2 * (d > 20), d, 4, generator=g).cuda() for d in dims]
        shapes = [v.shape[:3] for v in vols]
    lay = 0 if layout == "planar" else 1
    dim_table = L.int_table([x for s_ in shapes for x in s_])
    g_out = torch.randn(n, nl, 4, generator=g).cuda()
    gg_pts = torch.randn(n, 3, generator=g).cuda()
    scratch = torch.empty(L.load().gens_lookup_scatter_bricks_scratch_bytes(n), device="cuda", dtype=torch.uint8)

    def run(bricks, second):
        gv = [torch.zeros_like(v) for v in vols]
        gp = torch.empty(n, 3, device="cuda")
        if not second:
            if bricks:
                L.call("gens_lookup_volume_bwd_bricks", L.ptr_table(vols), dim_table, nl, lay, L.ptr(pts), L.ptr(g_out), n, L.ptr_table(gv), L.ptr(gp),
                       L.ptr(scratch, torch.uint8), scratch.numel(), L.stream())
            else:
                L.call("gens_lookup_volume_bwd", L.ptr_table(vols), dim_table, nl, lay, L.ptr(pts), L.ptr(g_out), n, L.ptr_table(gv), L.ptr(gp), L.stream())
            return gv, gp
        ggo = torch.empty_like(g_out)
        if bricks:
            L.call("gens_lookup_volume_bwd2_bricks", L.ptr_table(vols), dim_table, nl, lay, L.ptr(pts), L.ptr(g_out), L.ptr(gg_pts), None, n, L.ptr(ggo),
                   L.ptr_table(gv), L.ptr(gp), L.ptr(scratch, torch.uint8), scratch.numel(), L.stream())
        else:
            L.call("gens_lookup_volume_bwd2", L.ptr_table(vols), dim_table, nl, lay, L.ptr(pts), L.ptr(g_out), L.ptr(gg_pts), None, n, L.ptr(ggo),
                   L.ptr_table(gv), L.ptr(gp), L.stream())
        return gv, torch.cat([gp.reshape(-1), ggo.reshape(-1)])

    for second in (False, True):
        ref_v, ref_p = run(False, second)
        got_v, got_p = run(True, second)
        assert torch.equal(torch.nan_to_num(got_p, nan=7.0), torch.nan_to_num(ref_p, nan=7.0))
        for a_, b_ in zip(got_v, ref_v):
            assert torch.equal(torch.isnan(a_), torch.isnan(b_))
            a0, b0 = torch.nan_to_num(a_), torch.nan_to_num(b_)
            assert float(b0.abs().max()) > 0.1
            assert float((a0 - b0).abs().max()) <= 2e-5 * float(b0.abs().max()), (second, float((a0 - b0).abs().max()), float(b0.abs().max()))


def test_k2_large_point_sets_take_the_brick_scatter_through_autograd(ops, monkeypatch):
    """ops.lookup_volume's backward and double backward above kernels.k2_bricks_min points run the brick entries (asserted through the launch labels'
    timing table: the direct entries are not called) and give the direct scatter's volume gradients."""
    from gens_amd import lib as L
    g = torch.Generator().manual_seed(5)
    n = 40000
    pts0 = (torch.rand(n, 3, generator=g) * 2 - 1)
    pts0[:15000] = torch.randn(15000, 3, generator=g) * 0.05 + torch.tensor([0.2, 0.1, -0.3])
    vols0 = [0.5 * torch.randn(1, 4, d, d, d, generator=g) for d in (48, 24)]
    cot = torch.randn(n, 8, generator=g).cuda()
    res = {}
    for name, least in (("bricks", 1000), ("direct", 10 ** 9)):
        monkeypatch.setattr(ops.kernels, "k2_bricks_min", least)
        p = pts0.clone().cuda().requires_grad_(True)
        vs = [v.clone().cuda().requires_grad_(True) for v in vols0]
        calls = []
        real = L.call
        monkeypatch.setattr(L, "call", lambda nm, *a, **k: (calls.append(nm), real(nm, *a, **k))[1])
        f = ops.lookup_volume(p, vs)
        gp, = torch.autograd.grad((f * cot).sum(), p, create_graph=True)
        ((gp * gp).sum() + (f * cot).sum()).backward()
        monkeypatch.setattr(L, "call", real)
        res[name] = [v.grad.clone() for v in vs]
        if name == "bricks":
            assert "gens_lookup_volume_bwd_bricks" in calls and "gens_lookup_volume_bwd2_bricks" in calls
            assert "gens_lookup_volume_bwd" not in calls and "gens_lookup_volume_bwd2" not in calls
        else:
            assert "gens_lookup_volume_bwd_bricks" not in calls
    for a_, b_ in zip(res["bricks"], res["direct"]):
        assert float(b_.abs().max()) > 0.1
        assert float((a_ - b_).abs().max()) <= 2e-5 * float(b_.abs().max())


@pytest.mark.parametrize("chans", [(4, 4, 4), (3, 5, 2), (4, 4)])
def test_k9_one_launch_upsampling_equals_the_launch_per_level(ops, chans):
    """gens_upsample2d_cat against gens_upsample2d_into level by level, bit for bit; the pad channels are written (zeros), not left to a fill."""
    from gens_amd import lib as L
    g = torch.Generator().manual_seed(21)
    nv, h, w = 2, 44, 60
    maps = [torch.randn(nv, c, max(h >> i, 1), max(w >> i, 1), generator=g).cuda() for i, c in enumerate(chans)]
    ctot = sum(chans)
    cpad = 4 * ((ctot + 3) // 4)
    ref = torch.zeros(nv, h, w, cpad, device="cuda")
    off = 0
    for f in maps:
        L.call("gens_upsample2d_into", L.ptr(f), nv, f.shape[1], f.shape[2], f.shape[3], L.ptr(ref), h, w, cpad, off, L.stream())
        off += f.shape[1]
    out = torch.full((nv, h, w, cpad), float("nan"), device="cuda")
    chw = [d for f in maps for d in f.shape[1:]]
    L.call("gens_upsample2d_cat", L.ptr_table(maps), L.int_table(chw), len(maps), nv, L.ptr(out), h, w, cpad, L.stream())
    assert torch.equal(out, ref)
    tex, c = ops.build_warp_features(maps)
    assert c == ctot and torch.equal(tex, ref)


# --------------------------------------------------------------------------------------------------- K10 / K11
def test_k10_tv_golden(ops, golden):
    g = golden("g8_tv")
    vols = [dev(g["vol0"]).requires_grad_(True), dev(g["vol1"]).requires_grad_(True)]
    tv = ops.tv_regularization(vols, [dev(g["mask0"]), dev(g["mask1"])])
    close(tv, g["tv"], what="tv")
    gv = torch.autograd.grad(tv, vols)
    close(gv[0], g["gvol0"], atol=1e-6, what="gvol0")
    close(gv[1], g["gvol1"], atol=1e-6, what="gvol1")


def test_k11_lattice_vs_oracle(ops):
    res = 37
    ref = K.lattice_points([-1, -0.5, -1], [1, 1, 0.75], res)
    pts = ops.lattice_points([-1, -0.5, -1], [1, 1, 0.75], res, 0, res ** 3, "cuda")
    # torch.linspace on CPU is vectorised (base + step*lane), so its last bit depends on the host's SIMD width; 1 ulp
    close(pts, ref, atol=1.2e-7, rtol=0, what="lattice")
    part = ops.lattice_points([-1, -0.5, -1], [1, 1, 0.75], res, 1000, 4321, "cuda")
    close(part, ref[1000:5321], atol=1.2e-7, rtol=0, what="lattice slice")


# --------------------------------------------------------------------------------------------------- compaction
@pytest.mark.parametrize("n,frac", [(1, 1.0), (7, 0.0), (1000, 0.5), (1024, 1.0), (123457, 0.94), (3_000_001, 0.3), (5000, 0.0)])
def test_device_compaction_matches_nonzero_and_rescue(ops, n, frac):
    g = torch.Generator().manual_seed(n)
    valid = (torch.rand(n, generator=g) < frac).cuda()
    idx, count = ops.compact_valid(valid)
    ref = torch.nonzero(valid)[:, 0]
    if ref.numel() < 1:
        ref = torch.arange(min(10, n), device="cuda")          # implicit_surface.py:123-124
    assert int(count) == ref.numel()
    assert torch.equal(idx[:ref.numel()], ref)


def test_k2_second_order_outside_the_cube_vs_fd64_of_aten(ops):
    """K2'' at and beyond the border of the volume (rays without a crossing are sampled at the camera centre, outside the cube:
    implicit_surface.py:301-305).  The reference's CUDA kernel cannot run here and its pure-torch sampler clamps instead of zero-padding,
    so golden g2 pins second order only inside the cube.  Ground truth for the rest: central differences, in float64, of ATen's OWN
    first-order backward (aten::grid_sampler_3d_backward, the op cuda_gridsample.py:97 calls) -- gG'(p) . e_k = d/dp_k <gG(p), ggG>,
    ggO = d/d gO <gG, ggG>, gI' = d/dV <gG, ggG> -- compared with the HIP kernel's outputs.  Points are kept 1e-3 away from the
    kinks of the piecewise-trilinear interpolant (integer voxel positions), where no second derivative exists."""
    vols, pts, go, ggp, gp2, ggo_ref, gv_ref = second_order_fd64_case()
    dv = [v.float().cuda().requires_grad_(True) for v in vols]
    dp = pts.float().cuda().requires_grad_(True)
    dgo = go.float().cuda().requires_grad_(True)
    grads = torch.autograd.grad(ops.lookup_volume(dp, dv), [dp], dgo, create_graph=True)
    outs = torch.autograd.grad((grads[0] * ggp.float().cuda()).sum(), [dgo, dp] + dv)
    close(outs[1], gp2, atol=2e-3, rtol=2e-4, what="gP2 (fd64 of aten backward)")
    close(outs[0], ggo_ref, atol=1e-4, rtol=1e-4, what="ggO")
    for i in range(2):
        close(outs[2 + i], gv_ref[i], atol=1e-4, rtol=1e-4, what=f"gV2_{i}")
    assert ((pts.abs() > 1).any(-1)).float().mean() > 0.5


# the three K2 tests above once more with kernels.k2_bricks_min = 1: every volume gradient (first and second order) through the brick entries,
# which their small point sets never reach at the default threshold
def _through_the_bricks(ops, monkeypatch, run):
    """-> the entry points `run` called with k2_bricks_min = 1."""
    from gens_amd import lib as L
    monkeypatch.setattr(ops.kernels, "k2_bricks_min", 1)
    calls, real = [], L.call
    monkeypatch.setattr(L, "call", lambda nm, *a, **k: (calls.append(nm), real(nm, *a, **k))[1])
    try:
        run()
    finally:
        monkeypatch.setattr(L, "call", real)
    return calls


def _bricks_only(calls):
    assert "gens_lookup_volume_bwd_bricks" in calls and "gens_lookup_volume_bwd2_bricks" in calls, calls
    assert "gens_lookup_volume_bwd" not in calls and "gens_lookup_volume_bwd2" not in calls, calls


@pytest.mark.parametrize("packed", [False, True])
def test_k2_lookup_golden_through_the_bricks(ops, golden, packed, monkeypatch):
    calls = _through_the_bricks(ops, monkeypatch, lambda: test_k2_lookup_golden(ops, golden, packed))
    if not packed:                                                   # (packed: no volume gradient is asked for, nothing to scatter)
        _bricks_only(calls)


def test_k2_second_order_with_volume_cotangent_vs_oracle_through_the_bricks(ops, monkeypatch):
    _bricks_only(_through_the_bricks(ops, monkeypatch, lambda: test_k2_second_order_with_volume_cotangent_vs_oracle(ops)))


def test_k2_second_order_outside_the_cube_vs_fd64_of_aten_through_the_bricks(ops, monkeypatch):
    _bricks_only(_through_the_bricks(ops, monkeypatch, lambda: test_k2_second_order_outside_the_cube_vs_fd64_of_aten(ops)))


def second_order_fd64_case():
    """-> (vols, pts, gO, ggG, gP2_fd, ggO_fd, gV2_fd), all float64 (see test_k2_second_order_outside_the_cube_vs_fd64_of_aten)."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(17)
    dims = [7, 5]
    vols = [torch.randn(1, 4, d, d, d, generator=g, dtype=torch.float64) for d in dims]
    n = 600
    pts = torch.rand(n, 3, generator=g, dtype=torch.float64) * 3.0 - 1.5               # a third of the points lie outside [-1, 1]^3
    pts[:40] = torch.sign(pts[:40]) * (1.0 + 0.02 * torch.rand(40, 3, generator=g, dtype=torch.float64))   # just over the border
    for d in dims:                                                                         # off the kinks of every level
        pos = (pts + 1) * 0.5 * (d - 1)
        near = (pos - pos.round()).abs() < 2e-3
        pts = torch.where(near, pts + 8e-3 / (d - 1), pts)
    go = torch.randn(n, 8, generator=g, dtype=torch.float64)
    ggp = torch.randn(n, 3, generator=g, dtype=torch.float64)

    def first_order(p, vs, o):
        """<gG(p), ggG> summed per point, with gG from ATen's backward (float64)."""
        p = p.clone().requires_grad_(True)
        x = p.flip(-1)[None, None, None]
        y = torch.cat([F.grid_sample(v, x, padding_mode="zeros", align_corners=True).reshape(4, -1).t() for v in vs], -1)
        gp = torch.autograd.grad(y, p, o)[0]
        return (gp * ggp).sum(-1)

    eps = 1e-6
    gp2 = torch.stack([(first_order(pts + eps * e, vols, go) - first_order(pts - eps * e, vols, go)) / (2 * eps)
                       for e in torch.eye(3, dtype=torch.float64)], -1)
    ggo_ref, gv_ref = _second_order_linear_parts_fd(vols, pts, go, ggp)
    return vols, pts, go, ggp, gp2, ggo_ref, gv_ref


def _second_order_linear_parts_fd(vols, pts, go, ggp):
    """ggO[n, c] = d/d gO[n, c] <gG, ggG> and gI' = d/dV <gG, ggG>: <gG, ggG> is LINEAR in gO and in V, so one evaluation of ATen's
    backward per basis direction would do; cheaper: directional derivative of the forward, y(p + t ggG) in t, again through ATen in
    float64 (central difference, exact up to the O(eps^2) term, which vanishes for a trilinear polynomial away from the kinks)."""
    import torch.nn.functional as F
    eps = 1e-5

    def fwd(p, vs):
        x = p.flip(-1)[None, None, None]
        return torch.cat([F.grid_sample(v, x, padding_mode="zeros", align_corners=True).reshape(4, -1).t() for v in vs], -1)

    ggo = (fwd(pts + eps * ggp, vols) - fwd(pts - eps * ggp, vols)) / (2 * eps)            # J ggG
    vs = [v.clone().requires_grad_(True) for v in vols]
    phi = (((fwd(pts + eps * ggp, vs) - fwd(pts - eps * ggp, vs)) / (2 * eps)) * go).sum()
    return ggo, torch.autograd.grad(phi, vs)
