"""K26: GenS.filter_volume (models/gens.py:87-122) -- the mask pyramid restricted to a one-voxel dilation of the band |sdf| < thresh inside the
unit sphere, all levels in one call of gens_filter_masks.

Part of gens_amd.ops (see ops/__init__.py); citations are relative to /root/reference."""
from .base import *  # noqa: F401,F403


def filter_mask_dims(u_shape, mask_shapes):
    """The shapes gens_filter_masks accepts, checked before anything touches the device: u (D0, D0, D0); masks (1, 1, D_l, D_l, D_l) with
    D_l = D0 >> l, D0 a multiple of 2^(levels - 1), at most GENS_MAX_LEVELS levels.  (The reference's chain of nearest halvings dies on a
    broadcasting error in the same cases, gens.py:118-120.)  -> [D_0, ..., D_{L-1}]; ValueError otherwise."""
    u_shape = tuple(int(s) for s in u_shape)
    if len(u_shape) != 3 or len(set(u_shape)) != 1 or u_shape[0] < 1:
        raise ValueError(f"filter_masks: the lattice must be a cube (D0, D0, D0), got {u_shape}")
    d0, n = u_shape[0], len(mask_shapes)
    if not 1 <= n <= L.MAX_LEVELS:
        raise ValueError(f"filter_masks: {n} mask levels, 1 to GENS_MAX_LEVELS = {L.MAX_LEVELS} (GENS_ELIMIT)")
    if d0 > 1024:
        raise ValueError(f"filter_masks: D0 = {d0}, at most 1024 (32-bit voxel indices)")
    if d0 % (1 << (n - 1)) != 0:
        raise ValueError(f"filter_masks: D0 = {d0} is no multiple of 2^(levels - 1) = {1 << (n - 1)} (GENS_EINVAL)")
    for l, s in enumerate(mask_shapes):
        s = tuple(int(v) for v in s)
        want = d0 >> l
        if len(s) < 3 or s[-3:] != (want, want, want) or any(v != 1 for v in s[:-3]):
            raise ValueError(f"filter_masks: mask level {l} has shape {s}, expected (1, 1, {want}, {want}, {want}) = D0 >> {l} per axis (GENS_EINVAL)")
    return [d0 >> l for l in range(n)]


def filter_masks(u, masks, thresh, return_band=False):
    """u (D0, D0, D0) float32 on the device, indexed [ix, iy, iz] (ImplicitSurface.sdf_grid: -sdf on linspace(-1, 1, D0)^3); masks: the model's
    (1, 1, D_l, D_l, D_l) float pyramid -> (filtered masks, band count, dilated count): new tensors of the masks' shapes,
        out_l[x, y, z] = in_l[x, y, z] * max_pool3d(band, 3, 1, 1)[x << l, y << l, z << l],   band = (|u| < thresh) & (|p| < 1),
    and two 0-dim int64 device tensors (level-0 voxels in the band, and after the dilation; no read-back here).  The bit words of every
    result (gens_pack_mask_bits' format) come out of the same launch and are attached to the returned tensors where VolumeSet.bit_table and
    the captured steps look for them, for the tensors' current versions: a render after filtering packs nothing, and an in-place change of
    a returned mask drops its words like any other cached layout.  return_band=True: a fourth result, the band itself as ceil(D0^3 / 32) int32
    words in the same format (bit i & 31 of word i >> 5 = level-0 voxel i in C order), as the first launch leaves it."""
    masks = list(masks)
    dims = filter_mask_dims(u.shape, [m.shape for m in masks])
    thresh = float(thresh)
    dev = u.device
    if any(m.device != dev for m in masks):
        raise RuntimeError("filter_masks: the lattice and the masks live on different devices")
    if any(m.dtype != _f32 for m in masks) or u.dtype != _f32:
        raise RuntimeError("filter_masks: float32 lattice and masks")
    uc = _c(u.detach())
    ins = [_c(m.detach()) for m in masks]
    outs = [torch.empty(m.shape, device=dev, dtype=_f32) for m in masks]
    words = [torch.empty((d ** 3 + 31) // 32, device=dev, dtype=torch.int32) for d in dims]
    band = torch.empty((dims[0] ** 3 + 31) // 32, device=dev, dtype=torch.int32)
    counts = torch.empty(2, device=dev, dtype=torch.int64)
    n_all = sum(d ** 3 for d in dims)
    L.call("gens_filter_masks", L.ptr(uc), thresh, L.ptr_table(ins), L.ptr_table(outs), L.ptr_table(words, torch.int32), L.int_table(dims), len(dims),
           L.ptr(band, torch.int32), L.ptr(counts, torch.int64), L.stream(), nbytes=4 * dims[0] ** 3 + 8 * n_all + n_all // 8 + dims[0] ** 3 // 4)
    for o, w in zip(outs, words):
        o._gens_bits = (o._version, w)
    if return_band:
        return outs, counts[0], counts[1], band
    return outs, counts[0], counts[1]


__all__ = [n_ for n_ in dir() if not n_.startswith("__")]
