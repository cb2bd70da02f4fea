"""Times the stages of the DTU mesh finalising step (gens_amd.clean_meshes, K25 + K23) at DTU size with HIP events.

    python scripts/dtu_clean_bench.py [--lattice 512] [--warmup 20] [--reps 20] [--host] [--out profiles/r09_dtu_clean.txt]

The mesh is K12's extraction of a sphere on a --lattice^3 lattice scaled to a 99 mm sphere (512: ~1.3 M faces); cameras and masks are
tests/dtu_clean_reference.make_scene's (three views, 1200 x 1600).  Every device figure is the median (p10 / p90) of --reps timed runs after
--warmup runs, each between two HIP events on the current stream; an operator's host-side work (scans, read-backs, allocations) is inside
the events.  --host adds the same stages through the float64 restatement / scipy on this machine's CPU (one run each; the restated ray
cast is a brute force over all faces and is timed on a 1/64 sample of the rays and scaled)."""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_PEAK = 8.0e12       # bytes / s, the MI355X data sheet's figure


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = fn()
        e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e))
    q = statistics.quantiles(ms, n=10) if len(ms) > 1 else [ms[0]] * 9
    return statistics.median(ms), q[0], q[-1], out


def main():
    import dtu_clean_reference as R
    from gens_amd import clean_meshes as cm, io, ops
    from gens_amd.datasets.camera import load_K_Rt_from_P
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, H, W = args.lattice, 1200, 1600
    lin = torch.linspace(-1, 1, n, device=dev)
    x, y, z = torch.meshgrid(lin, lin, lin, indexing="ij")
    v, t = ops.marching_cubes(torch.sqrt(x * x + y * y + z * z) - 0.72, 0.0)
    del x, y, z
    v_np = ((v / (n - 1) * 2 - 1) * (49.6 / 0.72)).cpu().numpy().astype(np.float32)
    t_np = t.cpu().numpy()
    sc = R.make_scene(1, H=H, W=W, misses=True)
    P, masks = R.scene_P(sc), np.stack([R.disk_mask(d, H, W) for d in sc["disks"]])
    lines = [f"mesh: {len(v_np)} vertices, {len(t_np)} faces (K12, {n}^3 lattice, 99 mm sphere); 3 views of {H} x {W}; masked pixels per view "
             f"{[int((m > 128).sum()) for m in masks]}; median (p10 / p90) of {args.reps} runs after {args.warmup} warm-up runs, HIP events"]
    spans = ops.opencv_ellipse(11, 11)
    rgb = torch.from_numpy(np.repeat(masks[:1, :, :, None], 3, axis=3).copy()).to(dev)
    for label, img, ch in (("dilation, one view, 3 of 3 channels", rgb, 3), ("dilation, one view, channel 0 of 3", rgb, 1),
                           ("dilation, one view, grey", rgb[..., 0].contiguous(), 1)):
        med, lo, hi, _ = timed(lambda: ops.dilate_u8(img, spans, 11, channels=ch), args.warmup, args.reps)
        nbytes = H * W * 2 * ch
        lines.append(f"{label}: {med * 1e3:.1f} us ({lo * 1e3:.1f} / {hi * 1e3:.1f}); {nbytes / 1e6:.2f} MB algorithmic = "
                     f"{100 * nbytes / (med * 1e-3) / HBM_PEAK:.1f} % of the HBM peak")
    dil = cm.dilated_masks(masks, 11, dev)
    vd, td, Pd = torch.from_numpy(v_np.astype(np.float64)).to(dev), torch.from_numpy(t_np.astype(np.int64)).to(dev), torch.from_numpy(P).to(dev)
    med, lo, hi, _ = timed(lambda: ops.vertex_mask_votes(vd, Pd, dil), args.warmup, args.reps)
    lines.append(f"vertex votes, {len(v_np)} vertices x 3 views: {med:.3f} ms ({lo:.3f} / {hi:.3f})")
    med, lo, hi, grid = timed(lambda: ops.build_mesh_grid(vd, td), args.warmup, args.reps)
    lines.append(f"grid build: {med:.3f} ms ({lo:.3f} / {hi:.3f})")
    cams = [load_K_Rt_from_P(None, p[:3, :]) for p in P]
    intrs, c2ws = torch.from_numpy(np.stack([c[0] for c in cams])), torch.from_numpy(np.stack([c[1] for c in cams]))
    med, lo, hi, _ = timed(lambda: ops.view_rays_hit_counts(grid, dil, intrs, c2ws, 425), args.warmup, args.reps)
    lines.append(f"ray cast, 3 views in one launch: {med:.3f} ms ({lo:.3f} / {hi:.3f}) = {med / 3:.3f} ms per view")
    med, lo, hi, _ = timed(lambda: ops.face_components(td, len(v_np)), args.warmup, args.reps)
    lines.append(f"face adjacency + components: {med:.3f} ms ({lo:.3f} / {hi:.3f})")
    with tempfile.TemporaryDirectory() as tmp:
        root, out = os.path.join(tmp, "data"), os.path.join(tmp, "mesh")
        R.write_tree(root, out, {24: dict(sc, vertices=v_np, triangles=t_np)}, cm.VIEW_LISTS[0][:3])
        devnull = open(os.devnull, "w")

        def whole():
            old, sys.stdout = sys.stdout, devnull
            try:
                return cm.finalize_dtu_meshes(root, out, scans=(24,))
            finally:
                sys.stdout = old
        med, lo, hi, _ = timed(whole, 2, max(3, args.reps // 4))
        fv, ft = io.read_ply(os.path.join(out, "final", "scan24.ply"))
        lines.append(f"finalize_dtu_meshes, one scan, file I/O included: {med:.1f} ms ({lo:.1f} / {hi:.1f}); {len(ft)} faces kept")
    if args.host:
        from scipy import ndimage
        import mesh_clean_reference as M
        t0 = time.time()
        ndimage.grey_dilation(rgb.cpu().numpy()[0], footprint=R.ellipse_footprint(11, 11)[:, :, None], mode="constant", cval=0)
        lines.append(f"host: scipy.ndimage.grey_dilation, one view, 3 channels: {(time.time() - t0) * 1e3:.0f} ms")
        dil_np = dil.cpu().numpy()
        t0 = time.time()
        R.vertex_votes(v_np.astype(np.float64), P, dil_np)
        lines.append(f"host: restated vertex votes: {(time.time() - t0) * 1e3:.0f} ms")
        ro, rd, _ = R.view_rays(P[0], dil_np[0], H, W)
        t0 = time.time()
        M.first_hits(v_np.astype(np.float64), t_np, ro[::64], rd[::64])
        lines.append(f"host: restated brute-force ray cast, one view: {(time.time() - t0) * 64:.0f} s (1/64 of the rays timed, scaled)")
        t0 = time.time()
        io.drop_small_components(v_np, t_np)
        lines.append(f"host: io.drop_small_components (scipy): {(time.time() - t0) * 1e3:.0f} ms")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
