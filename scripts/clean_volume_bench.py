#!/usr/bin/env python3
"""The largest SDF-band region on the device (K27, gens_largest_component): (i) the kernel alone on the band of a synthetic surface, against
the route the reference implies -- utils/tools.py:34-50 is a host function: a device-to-host copy, a CPU labelling pass, argmax, a
host-to-device copy; skimage is not installed, so scipy.ndimage.label(structure=ones((3, 3, 3))) stands in for skimage.measure.label;
(ii) GenS.filter_volume with and without keep_largest; (iii) through init_volumes with and without the option: live share of the masks, the
captured fine-tune step and a 307 200-ray validation image, against the filtered masks without the option in the same process
(scripts/filter_volume_bench.py's set-up).  Medians with p10 - p90.

    python scripts/clean_volume_bench.py [--iters 20] [--out profiles/r13_clean_volume.txt]
    python scripts/clean_volume_bench.py --kernel-only 256      # K27 alone, for a kernel trace (each launch's share)

The band of (i): |sdf| < 0.1 of a sphere of radius 0.5 plus two detached balls of radius 0.08 (three regions), at 256 .. 16 voxels per axis;
and a 256^3 random volume at 20 % fill (hundreds of thousands of regions)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from filter_volume_bench import quiet, stats, steps_with_and_without, timed  # noqa: E402


def band_volume(d0):
    ax = torch.linspace(-1, 1, d0, device="cuda")
    x, y, z = ax[:, None, None], ax[None, :, None], ax[None, None, :]
    u = torch.sqrt(x ** 2 + y ** 2 + z ** 2) - 0.5
    ball = lambda cx, cy, cz: torch.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) < 0.08  # noqa: E731
    return ((u.abs() < 0.1) | ball(0.0, 0.0, 0.0) | ball(0.8, 0.1, -0.2)).float().contiguous()


def host_route(mask):
    from scipy import ndimage
    m = mask.cpu().numpy() > 0
    lab, num = ndimage.label(m, structure=np.ones((3, 3, 3)))
    if num >= 1:
        big = int(np.argmax(np.bincount(lab.reshape(-1))[1:])) + 1
        lab[lab != big] = 0
    out = torch.from_numpy(lab).cuda()
    torch.cuda.synchronize()
    return out, num


def kernel_alone(mask, iters):
    """-> (ms of the entry point per run, info): bits packed once, events around gens_largest_component."""
    from gens_amd import lib as L
    from gens_amd.ops.filter import _largest_component_bits
    flat = mask.reshape(-1)
    words = torch.empty((flat.numel() + 31) // 32, device="cuda", dtype=torch.int32)
    L.call("gens_pack_mask_bits", L.ptr(flat), flat.numel(), L.ptr(words, torch.int32), L.stream())
    for _ in range(3):
        _, info = _largest_component_bits(words, tuple(mask.shape), 3)
    L.profile_begin(only={"gens_largest_component"})
    for _ in range(iters):
        _largest_component_bits(words, tuple(mask.shape), 3)
    return [ms for _, ms, _, _ in L.profile_end(raw=True)], info.tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-only", type=int, default=0, metavar="D0", help="run K27 alone on the D0^3 band and the 20 % fill, then stop")
    ap.add_argument("--skip-steps", action="store_true", help="leave out (iii)")
    args = ap.parse_args()
    from gens_amd import ops, synthetic
    from gens_amd.config import gens_model_conf
    from gens_amd.models.gens import GenS
    if args.kernel_only:
        d0 = args.kernel_only
        for name, vol in (("band", band_volume(d0)), ("fill 0.2", (torch.rand(d0, d0, d0, device="cuda") < 0.2).float())):
            ms, info = kernel_alone(vol, args.iters)
            print(f"{name} {d0}^3: {stats(ms)[0]:.3f} ms, (components, size, root, label) = {info}")
        return
    lines = [f"clean_volume_bench: {torch.cuda.get_device_name(0)}, {args.iters} runs per figure, median (p10 - p90); host route = D2H copy + "
             f"scipy.ndimage.label(structure=ones((3,3,3))) + argmax + H2D copy (scipy stands in for the absent skimage)"]
    g = torch.Generator(device="cuda").manual_seed(2)
    cases = [(f"band {d}^3", band_volume(d)) for d in (256, 128, 64, 32, 16)]
    cases.insert(1, ("fill 0.2 256^3", (torch.rand(256, 256, 256, device="cuda", generator=g) < 0.2).float()))
    for name, vol in cases:
        ms, info = kernel_alone(vol, args.iters)
        op = [timed(lambda: ops.largest_component(vol)) for _ in range(args.iters)]
        host = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ref, num = host_route(vol)
            host.append(1e3 * (time.perf_counter() - t0))
        got = ops.largest_component(vol)
        assert num == info[0] and torch.equal(got > 0, ref > 0), name
        k, o, h = stats(ms), stats(op), stats(host)
        lines.append(f"(i) {name}: set {float(vol.mean()):.4f}, {info[0]} regions, largest {info[1]} voxels; gens_largest_component (events around the call: "
                     f"two clears + six launches) {k[0]:.3f} ms ({k[1]:.3f} - {k[2]:.3f}); ops.largest_component (pack, kernel, unpack, select, "
                     f"allocations) {o[0]:.3f} ms ({o[1]:.3f} - {o[2]:.3f}); host route {h[0]:.1f} ms ({h[1]:.1f} - {h[2]:.1f}, 3 runs); results equal")
    del cases, vol, ref, got
    torch.cuda.empty_cache()
    for dims in ((256, 128, 64), (256, 128, 64, 32, 16)):
        gm = torch.Generator().manual_seed(1)
        masks = [(torch.rand(1, 1, d, d, d, generator=gm) < 0.945).float().cuda() for d in dims]
        torch.manual_seed(0)
        model = GenS(gens_model_conf(volume_dims=dims))
        model.has_vol = True
        model = model.cuda()
        vols = [v.cuda() for v in synthetic.make_volumes(dims, seed=3)]
        runs = {False: [], True: []}
        shares = {}

        def whole_runs():
            for it in range(3 + max(5, args.iters // 2)):
                for keep in (False, True):
                    model.filter_keep_largest = keep
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = model.filter_volume(vols, list(masks), 0.1)
                    torch.cuda.synchronize()
                    if it >= 3:
                        runs[keep].append(1e3 * (time.perf_counter() - t0))
                    shares[keep] = float(out[0].mean())
        quiet(whole_runs)
        u = model.implicit_surface.sdf_grid(vols, torch.tensor([-1.0] * 3).cuda(), torch.tensor([1.0] * 3).cuda(), dims[0])
        lat = [timed(lambda: model.implicit_surface.sdf_grid(vols, torch.tensor([-1.0] * 3).cuda(), torch.tensor([1.0] * 3).cuda(), dims[0]))
               for _ in range(max(5, args.iters // 2))]
        _, nb, nd, nr, nk = ops.filter_masks(u, masks, 0.1, keep_largest=True)
        a, b, l = stats(runs[False]), stats(runs[True]), stats(lat)
        lines.append(f"(ii) dims {dims}: GenS.filter_volume {a[0]:.2f} ms ({a[1]:.2f} - {a[2]:.2f}) without, {b[0]:.2f} ms ({b[1]:.2f} - {b[2]:.2f}) with keep_largest; "
                     f"the SDF lattice alone {l[0]:.2f} ms ({l[1]:.2f} - {l[2]:.2f}); band {int(nb)} voxels in {int(nr)} regions, kept {int(nk)}; level-0 live share "
                     f"{shares[False]:.4f} -> {shares[True]:.4f} (seeded geometric-initialisation surface, synthetic volumes)")
        del model, vols, masks, u
        torch.cuda.empty_cache()
        if not args.skip_steps:
            lines += steps_with_and_without(dims, args.iters, tag="(iii)", configs=(
                ("filter_thresh=0.1", {"filter_thresh": 0.1}), ("filter_thresh=0.1 + keep_largest", {"filter_thresh": 0.1, "filter_keep_largest": True})))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
