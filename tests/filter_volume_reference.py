"""GenS.filter_volume (reference models/gens.py:87-122) restated in plain torch, in this project's words: what a user would write without
the K26 kernel, and what tests/golden/g23*_filter_volume.npz (the reference's own run) is reproduced from.

The chain, on the level-0 lattice u[ix, iy, iz] = -sdf on linspace(-1, 1, D0)^3 (ImplicitSurface.sdf_grid's layout):
  * the reference lists its points with x fastest (gens.py:97), so its flat mask viewed as (D0, D0, D0) is indexed [iz, iy, ix]: the
    lattice transposed;
  * threshold |sdf| < thresh as floats (:106), times the unit-sphere test on the float32 norm of the points (:111-112) -> the band, whose
    mean is the first printed ratio (:113);
  * F.max_pool3d(band, 3, 1, 1) (:114), whose mean is the second ratio (:115);
  * permute (0, 1, 4, 3, 2) back to [x, y, z] (:116);
  * per level: mask_l * dil, then dil = F.interpolate(dil, scale_factor=0.5, mode="nearest") (:118-120): every second voxel, no pooling."""
import torch
import torch.nn.functional as F

LATTICE_ATOL, LATTICE_RTOL = 2e-5, 1e-4          # what tests/test_hip_render.py holds sdf_grid to against g10


def filter_chain(u, masks, thresh):
    """u (D0, D0, D0) float32 [ix, iy, iz]; masks: list of (1, 1, D_l, D_l, D_l) floats, on u's device.
    -> dict(band, dilated: (D0, D0, D0) floats [x, y, z]; masks: the filtered list; ratio, ratio_dilated: 0-dim float32 tensors)."""
    d0 = u.shape[0]
    dev = u.device
    axis = torch.linspace(-1, 1, d0)                                   # built on the host, as the reference builds it, then moved
    gz, gy, gx = torch.meshgrid([axis, axis, axis], indexing="ij")     # point (iz, iy, ix) = (x_ix, y_iy, z_iz)
    pts = torch.stack([gx, gy, gz], dim=-1).view(-1, 3).to(dev)
    sdf = (-u).permute(2, 1, 0).reshape(-1, 1)                         # the lattice in the reference's point order
    band = (sdf.abs() < thresh).float().view(1, 1, d0, d0, d0)
    norm = torch.linalg.norm(pts, ord=2, dim=-1, keepdim=False).reshape(1, 1, d0, d0, d0)
    band = band * (norm < 1).float()
    ratio = band.mean()
    dil = F.max_pool3d(band, 3, 1, 1)
    ratio_dil = dil.mean()
    band_xyz, cur = band.permute(0, 1, 4, 3, 2), dil.permute(0, 1, 4, 3, 2)
    dil_xyz = cur
    out = []
    for m in masks:
        out.append(m * cur)                                            # (a shape that does not fit dies here on a broadcasting error)
        cur = F.interpolate(cur, scale_factor=0.5, mode="nearest")
    return {"band": band_xyz[0, 0].contiguous(), "dilated": dil_xyz[0, 0].contiguous(), "masks": out, "ratio": ratio, "ratio_dilated": ratio_dil}


def printed_lines(ratio, ratio_dilated):
    """The three lines gens.py:89,113,115 print, the ratios as CPU float32 tensors."""
    return ["Filtering sdf volume...", "Survival ratio: " + str(ratio.detach().cpu().float()), "Survival ratio after dilation: " + str(ratio_dilated.detach().cpu().float())]


def ambiguous(u, thresh, factor=1.0):
    """Level-0 voxels whose band decision a lattice within the g10 tolerance of `u` may take the other way: | |u| - thresh | <=
    factor * (2e-5 + 1e-4 |u|).  (The sphere test has no such voxels at even D0: |p|^2 (D0 - 1)^2 is a sum of three odd squares, 3 mod 8,
    and (D0 - 1)^2 is 1 mod 8, so the nearest miss is 2 / (D0 - 1)^2, far above float32 rounding.)  -> bool (D0, D0, D0)."""
    a = u.abs().double()
    return (a - float(torch.tensor(thresh, dtype=torch.float32))).abs() <= factor * (LATTICE_ATOL + LATTICE_RTOL * a)


def near_ambiguous(amb):
    """Voxels whose 3 x 3 x 3 level-0 neighbourhood holds an ambiguous voxel (their dilated value may flip)."""
    return F.max_pool3d(amb.float()[None, None], 3, 1, 1)[0, 0] > 0


def pack_bits(t):
    """(> 0) of a tensor as numpy packbits of its C-order voxels (how g18 packs its large masks)."""
    import numpy as np
    return np.packbits((t.detach().cpu().reshape(-1) > 0).numpy().astype(np.uint8))


def unpack_bits(bits, shape):
    import numpy as np
    n = 1
    for s in shape:
        n *= int(s)
    return torch.from_numpy(np.unpackbits(bits)[:n].astype(np.float32)).reshape(tuple(shape))


def unpack_words(words, shape):
    """gens_pack_mask_bits' words (int32, bit i & 31 of word i >> 5 = voxel i in C order) -> float tensor of `shape` on the CPU."""
    n = 1
    for s in shape:
        n *= int(s)
    w = words.detach().cpu().to(torch.int64) & 0xFFFFFFFF
    bits = (w[:, None] >> torch.arange(32)[None, :]) & 1
    return bits.reshape(-1)[:n].float().reshape(tuple(shape))
