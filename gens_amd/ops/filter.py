"""K26: GenS.filter_volume (models/gens.py:87-122) -- the mask pyramid restricted to a one-voxel dilation of the band |sdf| < thresh inside the
unit sphere, all levels in one call of gens_filter_masks.  K27: the largest connected component of a mask volume (utils/tools.py:34-50,
clean_volume), alone or between K26's two launches.

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


def filter_masks(u, masks, thresh, return_band=False, keep_largest=False):
    """u (D0, D0, D0) float32 on the device, indexed [ix, iy, iz] (ImplicitSurface.sdf_grid: -sdf on linspace(-1, 1, D0)^3); masks: the model's
    (1, 1, D_l, D_l, D_l) float pyramid -> (filtered masks, band count, dilated count): new tensors of the masks' shapes,
        out_l[x, y, z] = in_l[x, y, z] * max_pool3d(band, 3, 1, 1)[x << l, y << l, z << l],   band = (|u| < thresh) & (|p| < 1),
    and two 0-dim int64 device tensors (level-0 voxels in the band, and after the dilation; no read-back here).  The bit words of every
    result (gens_pack_mask_bits' format) come out of the same launch and are attached to the returned tensors where VolumeSet.bit_table and
    the captured steps look for them, for the tensors' current versions: a render after filtering packs nothing, and an in-place change of
    a returned mask drops its words like any other cached layout.  return_band=True: a last result, the band itself as ceil(D0^3 / 32) int32
    words in the same format (bit i & 31 of word i >> 5 = level-0 voxel i in C order), as the first launch leaves it.
    keep_largest=True: the band of the first launch is reduced to its largest 26-connected component (K27, gens_largest_component) BEFORE
    the dilation -- the band is the mask volume clean_volume would be handed -- and the second launch runs on that.  Two more counts follow
    the other two: the band's components (clean_volume's `Num region`) and, fourth, the band voxels kept (band count >= kept; the dilated
    count is the kept band's); return_band gives the kept band.
    The default makes the one call of gens_filter_masks."""
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
    d0 = dims[0]
    band = torch.empty((d0 ** 3 + 31) // 32, device=dev, dtype=torch.int32)
    counts = torch.empty(2, device=dev, dtype=torch.int64)
    n_all = sum(d ** 3 for d in dims)
    tables = (L.ptr_table(ins), L.ptr_table(outs), L.ptr_table(words, torch.int32), L.int_table(dims), len(dims))
    if not keep_largest:
        L.call("gens_filter_masks", L.ptr(uc), thresh, *tables, L.ptr(band, torch.int32), L.ptr(counts, torch.int64), L.stream(),
               nbytes=4 * d0 ** 3 + 8 * n_all + n_all // 8 + d0 ** 3 // 4)
        kept = ()
    else:
        L.call("gens_filter_band", L.ptr(uc), thresh, d0, L.ptr(band, torch.int32), L.ptr(counts, torch.int64), L.stream(),
               nbytes=4 * d0 ** 3 + d0 ** 3 // 8)
        band, info = _largest_component_bits(band, (d0, d0, d0), 3)
        L.call("gens_filter_levels", *tables, L.ptr(band, torch.int32), L.ptr(counts, torch.int64), L.stream(),
               nbytes=8 * n_all + n_all // 8 + d0 ** 3 // 8)
        kept = (info[0], info[1])
    for o, w in zip(outs, words):
        o._gens_bits = (o._version, w)
    if return_band:
        return (outs, counts[0], counts[1]) + kept + (band,)
    return (outs, counts[0], counts[1]) + kept


def _largest_component_bits(words, shape, connectivity):
    """words: ceil(n / 32) int32 on the device, gens_pack_mask_bits' format, of an (nx, ny, nz) volume -> (the largest component's words, a
    new tensor; (4) int64 device tensor: components, winner's size, winner's root or -1, winner's label number)."""
    nx, ny, nz = shape
    n = nx * ny * nz
    nbytes = L.load().gens_components_scratch_bytes(nx, ny, nz)
    if nbytes <= 0:
        raise ValueError(f"largest_component: extents {tuple(shape)} must be positive with fewer than 2^31 voxels (GENS_ELIMIT)")
    out = torch.empty_like(words)
    scratch = torch.empty((nbytes + 7) // 8, device=words.device, dtype=torch.int64)
    info = torch.empty(4, device=words.device, dtype=torch.int64)
    # algorithmic bytes: the words once per launch (six in, one out), a parent written by init and read or rewritten by the five launches after it
    L.call("gens_largest_component", L.ptr(words, torch.int32), nx, ny, nz, int(connectivity), L.ptr(out, torch.int32), L.ptr(scratch, torch.int64),
           L.ptr(info, torch.int64), L.stream(), nbytes=7 * (n // 8) + 6 * 4 * n)
    return out, info


def _volume_shape(mask, who):
    s = tuple(int(v) for v in mask.shape)
    if len(s) == 5 and s[:2] == (1, 1):
        s = s[2:]
    if len(s) != 3 or min(s) < 1:
        raise ValueError(f"{who}: a volume of three positive extents, or (1, 1, X, Y, Z), got {tuple(mask.shape)}")
    if s[0] * s[1] * s[2] >= 1 << 31:
        raise ValueError(f"{who}: {s} has 2^31 voxels or more (GENS_ELIMIT)")
    return s


def _component_of(mask, connectivity, who):
    """-> (keep: float32 0 / 1 of mask's shape, info (4) int64), all on the device."""
    if not torch.is_tensor(mask):
        raise TypeError(f"{who}: a device tensor, got {type(mask).__name__}")
    if connectivity not in (1, 3):
        raise ValueError(f"{who}: connectivity = {connectivity!r}, 1 (6 neighbours) or 3 (26 neighbours)")
    if not (mask.dtype.is_floating_point or mask.dtype == torch.bool):
        raise TypeError(f"{who}: a float or bool volume, got {mask.dtype}")
    shape = _volume_shape(mask, who)
    if not mask.is_cuda:
        raise RuntimeError(f"{who}: gens_amd kernels need device tensors (no CPU path)")
    m = mask.detach()
    flat = _c(m if m.dtype == _f32 else (m > 0).to(_f32)).reshape(-1)        # (the decision `> 0` is taken in the volume's own dtype)
    n = flat.numel()
    words = torch.empty((n + 31) // 32, device=mask.device, dtype=torch.int32)
    L.call("gens_pack_mask_bits", L.ptr(flat), n, L.ptr(words, torch.int32), L.stream(), nbytes=4 * n + n // 8)
    kept, info = _largest_component_bits(words, shape, connectivity)
    keep = torch.empty(n, device=mask.device, dtype=_f32)
    L.call("gens_unpack_mask_bits", L.ptr(kept, torch.int32), n, L.ptr(keep), L.stream(), nbytes=4 * n + n // 8)
    return keep.reshape(mask.shape), info


def largest_component(mask, connectivity=3, return_info=False):
    """mask: a device tensor (X, Y, Z) or (1, 1, X, Y, Z), float or bool; a voxel is set where its value is > 0.  -> a tensor of the same
    shape and dtype: the voxels of the largest connected component unchanged, every other voxel 0.  connectivity 3: the 26 neighbours
    (skimage.measure.label's connectivity=3, what clean_volume uses), 1: the 6 face neighbours.  The largest component is the one with the
    most voxels; of several that large, the one whose first voxel comes first in C order.  return_info=True: also four 0-dim int64 device
    tensors -- the number of components, the winner's size, the linear index of its first voxel (-1: empty volume) and its label number
    (1 + the components whose first voxel comes before it; 0: empty volume).  Nothing is read back."""
    keep, info = _component_of(mask, connectivity, "largest_component")
    out = torch.where(keep > 0, mask.detach(), torch.zeros((), device=mask.device, dtype=mask.dtype))
    if return_info:
        return out, info[0], info[1], info[2], info[3]
    return out


def clean_volume(mask_volume):
    """utils/tools.py:34-50 with its own return contract, on the device.  mask_volume (w, h, d), or (1, 1, w, h, d): prints `Num region: N`
    (one read-back, for the line and the branch); N < 1: returns mask_volume itself; otherwise an int64 tensor of the same shape that is 0
    outside the largest 26-connected region and equals THAT REGION'S LABEL NUMBER inside -- the reference returns skimage's `label` array
    with the other regions zeroed, not a 0 / 1 mask, and this keeps that: test `> 0` to use it as a mask.  Labels are numbered from 1 in the
    C order of the components' first voxels (skimage's and scipy's numbering)."""
    keep, info = _component_of(mask_volume, 3, "clean_volume")
    num = int(info[0])
    print("Num region:", num)
    if num < 1:
        return mask_volume
    return keep.to(torch.int64) * info[3]


__all__ = [n_ for n_ in dir() if not n_.startswith("__")]
