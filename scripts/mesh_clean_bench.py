#!/usr/bin/env python3
"""Timings of K23, the ray-cast half of the validation-mesh cleaning (utils/clean_mesh.py:38-130), on a 512^3 marching-cubes mesh.

Mesh: ops.marching_cubes of an analytic SDF (eight wrinkled blobs and a thin floater) on a 512^3 lattice over [-1.1, 1.1]^3 (~2 M faces).
Views: 3 and 5 cameras of synthetic.make_cameras at 480 x 640; masks = the projected vertices, closed by a 5 x 5 max filter.
Prints, per view count (median of --reps runs, each synchronised): the grid build, the fused view-ray cast at upscale 2 (clean_mesh's
default: 960 x 1280 rays per view), the face components of the whole mesh (adjacency + union-find), the whole io.clean_mesh (its mask
half runs on the host), and the host io.drop_small_components on the same mesh.

    python scripts/mesh_clean_bench.py [--res 512] [--reps 3]
"""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gens_amd import io, ops, synthetic  # noqa: E402


def timed(fn, reps):
    out, ts = None, []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return out, statistics.median(ts)


def make_mesh(res, dev):
    lin = torch.linspace(-1.1, 1.1, res, device=dev)
    x, y, z = torch.meshgrid(lin, lin, lin, indexing="ij")
    d = None
    for c, r in (((-0.35, 0.0, 0.0), 0.45), ((0.35, 0.1, 0.05), 0.35), ((0.0, -0.45, 0.1), 0.3), ((0.1, 0.3, -0.35), 0.25),
                 ((0.45, -0.4, -0.3), 0.3), ((-0.5, 0.45, 0.3), 0.28), ((-0.1, -0.1, 0.55), 0.25), ((0.55, 0.45, 0.4), 0.2)):
        s = torch.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r
        d = s if d is None else torch.minimum(d, s)
    d = d + 0.015 * torch.sin(25 * x) * torch.sin(25 * y) * torch.sin(25 * z)      # wrinkles: more surface, faces of every orientation
    floater = torch.sqrt((x - 0.6) ** 2 + (y + 0.6) ** 2) - 0.01          # a thin rod, clipped to a short segment
    floater = torch.maximum(floater, (z - 0.05).abs() - 0.15)
    d = torch.minimum(d, floater)
    del x, y, z
    v, t = ops.marching_cubes(d.contiguous(), 0.0)
    return -1.1 + v * (2.2 / (res - 1)), t


def project_masks(vertices, intrs, c2ws, h, w):
    pts = torch.cat([vertices.float(), torch.ones_like(vertices[:, :1]).float()], 1)
    masks = []
    for i in range(intrs.shape[0]):
        cam = (torch.linalg.inv(c2ws[i].to(pts.device)) @ pts.T)[:3]
        uv = intrs[i, :3, :3].to(pts.device) @ cam
        x, y = (uv[0] / uv[2]).round().long(), (uv[1] / uv[2]).round().long()
        ok = (x >= 0) & (x < w) & (y >= 0) & (y < h) & (uv[2] > 0)
        m = torch.zeros(h * w, device=pts.device)
        m[y[ok] * w + x[ok]] = 1.0
        masks.append(F.max_pool2d(m.view(1, 1, h, w), 5, 1, 2)[0, 0])
    return torch.stack(masks).cpu()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.init()
    v, t = make_mesh(a.res, dev)
    print(f"mesh: {a.res}^3 lattice, {v.shape[0]} vertices, {t.shape[0]} faces", flush=True)
    v_np, t_np = v.cpu().numpy(), t.cpu().numpy()
    for nv in (3, 5):
        intrs, c2ws, _, _ = synthetic.make_cameras(nv, 480, 640)
        masks = project_masks(v, intrs, c2ws, 480, 640)
        grid, ms_grid = timed(lambda: ops.build_mesh_grid(v, t), a.reps)
        (flags, miss), ms_cast = timed(lambda: ops.visible_faces(grid, masks, intrs, c2ws, 2), a.reps)
        label, ms_cc = timed(lambda: ops.face_components(t, v.shape[0]), a.reps)
        (cv, ct), ms_clean = timed(lambda: io.clean_mesh(v_np, t_np, masks, intrs, c2ws), a.reps)
        n_rays = int((F.interpolate(masks[:, None], scale_factor=2, mode="nearest") > 0).sum())
        print(f"views {nv}: grid {grid.dims} cells, {grid.cell_faces.numel()} entries; {n_rays} masked rays of {nv * 960 * 1280}; "
              f"{int(flags.sum())} faces hit, any_miss {int(miss.item())}; {int(label.unique().numel())} components; "
              f"clean_mesh keeps {ct.shape[0]} faces, {cv.shape[0]} vertices", flush=True)
        print(f"views {nv}: grid build {ms_grid:.2f} ms | view-ray cast {ms_cast:.2f} ms | components {ms_cc:.2f} ms | "
              f"whole clean_mesh {ms_clean:.1f} ms", flush=True)
    _, ms_host = timed(lambda: io.drop_small_components(v_np, t_np, 500), 1)
    print(f"host drop_small_components (scipy) on the same mesh: {ms_host:.1f} ms", flush=True)


if __name__ == "__main__":
    main()
