"""The sphere-traced surface maps (K31, ImplicitSurface.render_surface) beside the volume rendering of the same rays (validate), on the scene
of scripts/sparse_lattice_bench.py: BASELINE config[1]'s synthetic volumes (256 / 128 / 64), the model bench.py builds
and its five 480 x 640 views; the network kernels in float32 MFMA ("transposed") and with three-term bfloat16 operands ("bf16x3", the default).

Two HIP event pairs per repeat, alternating in one process: one around render_surface (depth, normals and colours, read-back included), one
around validate of the same rays (geometry off, read-back included).  One warm-up of each, then the repeats; ms = median (min - max).  Also
recorded: the trace's stats (rounds, evaluations per ray, rays per status) and the event pairs per launch of one more render_surface call.
With --mesh-resolution R the R^3 mesh of the same surface is cast with the same rays (ops.ray_mesh_first_hit) and the agreement of the two
routes is recorded (what tests/test_hip_surface_trace.py prints for its small scene).

    python scripts/surface_render_bench.py --out profiles/r18_surface_render.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e), out


def summary(xs):
    return {"ms": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def mesh_agreement(surf, ops, vols, lo, hi, rays_o, rays_d, out, resolution):
    vertices, triangles = surf.extract_geometry(vols, lo, hi, resolution, 0.0, sparse=4)
    grid = ops.build_mesh_grid(torch.from_numpy(vertices).to(rays_o.device), torch.from_numpy(triangles).to(rays_o.device))
    face, t_mesh = ops.ray_mesh_first_hit(rays_o, rays_d, grid)
    face, t_mesh = face.cpu().numpy(), t_mesh.cpu().numpy()
    hit_t, hit_m = out["hit"].reshape(-1), face >= 0
    both = hit_t & hit_m
    h = 2.0 / (resolution - 1)
    cos = np.abs((rays_d.cpu().numpy().astype(np.float64) * out["normal"].reshape(-1, 3)).sum(axis=1))
    gap = np.abs(out["t"].reshape(-1).astype(np.float64) - t_mesh)[both] * cos[both] / h
    return {"resolution": resolution, "hit_trace": int(hit_t.sum()), "hit_mesh": int(hit_m.sum()), "hit_both": int(both.sum()),
            "flags_differ_share": round(float((hit_t != hit_m).mean()), 6), "gap_over_h_median": round(float(np.median(gap)), 5),
            "gap_over_h_p99": round(float(np.percentile(gap, 99)), 5), "gap_over_h_max": round(float(gap.max()), 5)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default="profiles/r18_surface_render.json")
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--views", type=int, default=5)
    p.add_argument("--dims", type=int, nargs="+", default=[256, 128, 64])
    p.add_argument("--resolution", type=int, default=512, help="min_step: the spacing of a lattice of this many points per axis")
    p.add_argument("--mesh-resolution", type=int, default=512, help="compare with the mesh of this resolution (0: skip)")
    p.add_argument("--kernels", nargs="+", default=["transposed", "bf16x3"], choices=["transposed", "bf16x3"])
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("surface_render_bench: needs the GPU (a CPU run measures nothing)")
    from gens_amd import lib as L, ops, synthetic
    from gens_amd.config import gens_model_conf
    from gens_amd.models.modules.implicit_surface import ImplicitSurface, Scene
    dev = torch.device("cuda", 0)
    raw = [v.to(dev) for v in synthetic.make_volumes(args.dims, seed=100)]
    sc = synthetic.make_scene(nv=args.views, h=480, w=640, n_levels=5, seed=0)
    imgs, intrs, c2ws = sc["imgs"].to(dev), sc["intrs"].to(dev), sc["c2ws"].to(dev)
    feats = [f.to(dev) for f in sc["features"]]
    near, far = sc["near"].to(dev), sc["far"].to(dev)
    masks = [torch.ones(1, 1, *v.shape[2:], device=dev) for v in raw]
    rays_o, rays_d = synthetic.make_rays(sc["intrs"], sc["c2ws"], 480, 640)
    rays_o, rays_d = rays_o.to(dev), rays_d.to(dev)
    torch.manual_seed(0)                                       # bench.py's build_model
    surf = ImplicitSurface(gens_model_conf(volume_dims=tuple(args.dims), n_feature_levels=5)["implicit_surface"]).to(dev).eval()
    lo, hi = torch.tensor([-1.0] * 3, device=dev), torch.tensor([1.0] * 3, device=dev)
    scene = Scene(raw, masks, imgs, feats, feats, intrs, c2ws)
    vols, views = scene.volumes_nograd(), scene.views
    result = {"workload": "BASELINE config[1] synthetic volumes %s, the model of bench.py, %d views of 480 x 640, 307 200 rays of view 0; "
                          "render_surface: depth + normals + colours at lipschitz %g, min_step = the spacing of a %d^3 lattice, max_steps 256, refine 2, "
                          "read-back included; validate: the same rays, geometry off, read-back included"
                          % (args.dims, args.views, surf.lattice_lipschitz, args.resolution),
              "timing": "HIP events around each call, alternating in one process; one warm-up of each, then %d repeats; ms = median (min - max)" % args.repeats,
              "device": torch.cuda.get_device_name(0), "runs": []}

    def surface():
        return surf.render_surface(rays_o, rays_d, near, far, vols, lo, hi, c2ws, views=views, resolution=args.resolution, hw=(480, 640))

    def volume_render():
        return surf.validate(rays_o, rays_d, near, far, raw, masks, imgs, feats, feats, intrs, c2ws, lo, hi, (480, 640), extract_geometry=False, scene=scene)

    for choice in args.kernels:
        ops.kernels.sdf_value = ops.kernels.sdf_grad = ops.kernels.blend = choice
        out = surface()                                        # warm-up of both
        volume_render()
        stats = dict(surf.last_surface_stats)
        entry = {"kernels": choice, "stats": stats, "evaluations_per_ray": round(stats["evaluated_points"] / stats["rays"], 3)}
        ms = {"render_surface": [], "validate": []}
        for _ in range(args.repeats):
            ms["render_surface"].append(timed(surface)[0])
            ms["validate"].append(timed(volume_render)[0])
        entry["render_surface"], entry["validate"] = summary(ms["render_surface"]), summary(ms["validate"])
        entry["render_surface_over_validate"] = round(entry["render_surface"]["ms"] / entry["validate"]["ms"], 4)
        L.profile_begin()
        surface()
        entry["render_surface_launches"] = {k: {"launches": v["launches"], "ms": round(v["ms"], 3)} for k, v in L.profile_end().items()}
        entry["render_surface_launch_ms"] = round(sum(v["ms"] for v in entry["render_surface_launches"].values()), 3)
        if args.mesh_resolution:
            entry["against_the_mesh"] = mesh_agreement(surf, ops, vols, lo, hi, rays_o, rays_d, out, args.mesh_resolution)
        result["runs"].append(entry)
        print(json.dumps(entry), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
