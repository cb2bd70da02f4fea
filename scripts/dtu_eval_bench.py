"""Times K24's three steps and the whole gens_amd.evaluation.dtu_chamfer at DTU-like size with HIP events.

    python scripts/dtu_eval_bench.py [--radius 90] [--stl 3000000] [--reps 5] [--out profiles/r08_dtu_eval.txt]

The surface is tests/dtu_eval_reference's jittered lat-long sphere, refined so that its triangles are a few lattice steps wide: radius 90
gives ~1.0e5 mm^2, i.e. ~2.5 M samples at density 0.2; the scan is --stl noisy points on the front of the sphere.  Every figure is the
median of --reps timed runs after one warm-up run, each run between two HIP events on the current stream (the host-side work of an
operator -- its scans, read-backs and allocations -- is inside the events: that is what a caller waits for)."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, reps):
    fn()                                            # warm-up: allocator, code objects
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = fn()
        e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e))
    return statistics.median(ms), min(ms), max(ms), out


def main():
    import dtu_eval_reference as R
    from gens_amd import evaluation, ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--radius", type=float, default=90.0)
    ap.add_argument("--stl", type=int, default=3000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n_lat = max(24, int(np.pi * args.radius / 0.7))
    centre = np.array([40.0, -150.0, 620.0])
    v, t = R.sphere_mesh(args.radius, centre, n_lat=n_lat, n_lon=2 * n_lat, jitter=0.02, rng=np.random.default_rng(1))
    rng = np.random.default_rng(2)
    d = rng.standard_normal((args.stl, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    d = d[d[:, 0] > -0.3]
    stl = centre + d * (args.radius + 0.1 * rng.standard_normal((len(d), 1)))
    half = args.radius + 2.0
    bb = np.stack([centre - half, centre + half])
    obs = np.ones((160, 160, 160), dtype=np.uint8)
    obs[:, :, :10] = 0
    res = 2 * half / 160
    plane = np.array([0.0, 0.0, 1.0, -(centre[2] - 0.4 * args.radius)])
    vd, td, sd = torch.as_tensor(R.f32(v), device=dev), torch.as_tensor(t, device=dev), torch.as_tensor(R.f32(stl), device=dev)

    lines = [f"K24 / dtu_chamfer on {torch.cuda.get_device_name(0)}: sphere of radius {args.radius:g} mm ({4 * np.pi * args.radius ** 2:.3g} mm^2), "
             f"{len(v)} vertices, {len(t)} triangles, density 0.2, {len(stl)} scan points; median (min .. max) of {args.reps} runs, HIP events"]
    ms, lo, hi, pcd = timed(lambda: ops.sample_mesh_points(vd, td, 0.2), args.reps)
    lines.append(f"sample_mesh_points   {ms:9.2f} ms ({lo:.2f} .. {hi:.2f})   {pcd.shape[0]} points")
    order = torch.from_numpy(np.random.default_rng(3).permutation(pcd.shape[0])).to(dev)
    shuffled = pcd[order]
    ms, lo, hi, mask = timed(lambda: ops.radius_downsample(shuffled, 0.2), args.reps)
    rounds = ops.points.last_downsample_rounds
    down = shuffled[mask]
    lines.append(f"radius_downsample    {ms:9.2f} ms ({lo:.2f} .. {hi:.2f})   {down.shape[0]} kept, {rounds} rounds")
    ms, lo, hi, (dist, _) = timed(lambda: ops.nearest_distance(down, sd, 20.0), args.reps)
    lines.append(f"nearest data -> scan {ms:9.2f} ms ({lo:.2f} .. {hi:.2f})   {down.shape[0]} queries, {sd.shape[0]} targets, "
                 f"{int(torch.isinf(dist).sum())} beyond the cap")
    ms, lo, hi, (dist, _) = timed(lambda: ops.nearest_distance(sd, down, 20.0), args.reps)
    lines.append(f"nearest scan -> data {ms:9.2f} ms ({lo:.2f} .. {hi:.2f})   {sd.shape[0]} queries, {down.shape[0]} targets, "
                 f"{int(torch.isinf(dist).sum())} beyond the cap")
    ms, lo, hi, r = timed(lambda: evaluation.dtu_chamfer(vd, td, sd, obs, bb, np.array([[res]]), plane, rng=np.random.default_rng(3)), args.reps)
    lines.append(f"dtu_chamfer (whole)  {ms:9.2f} ms ({lo:.2f} .. {hi:.2f})   {r}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
