"""The fused point cloud (K32, ImplicitSurface.fuse_surface) on the scene of scripts/sparse_lattice_bench.py:
BASELINE config[1]'s synthetic volumes (256 / 128 / 64), the model bench.py builds and its five 480 x 640 views.

HIP event pairs per repeat around: the five traces (depth, normals and colours of every view, kept on the device), gens_fuse_depth_maps alone,
the compaction + gens_fused_points, and the whole fuse_surface (read-back included).  One warm-up of each, then the repeats; ms = median
(min - max).  Also recorded: the kept fraction and votes histogram per view, and the rate of the fusion kernel in (pixel, source) pairs per
second -- usable pixels times listed sources, the pairs that do the arithmetic.

    python scripts/surface_fusion_bench.py --out profiles/r20_surface_fusion.json
"""
import argparse
import json
import os
import statistics
import sys

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


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default="profiles/r20_surface_fusion.json")
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--views", type=int, default=5)
    p.add_argument("--dims", type=int, nargs="+", default=[256, 128, 64])
    p.add_argument("--resolution", type=int, default=512, help="min_step of the traces: the spacing of a lattice of this many points per axis")
    p.add_argument("--min-views", type=int, default=3)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("surface_fusion_bench: needs the GPU (a CPU run measures nothing)")
    from gens_amd import ops, synthetic
    from gens_amd.config import gens_model_conf
    from gens_amd.models.modules.implicit_surface import ImplicitSurface, Scene
    dev = torch.device("cuda", 0)
    h, w, nv = 480, 640, args.views
    raw = [v.to(dev) for v in synthetic.make_volumes(args.dims, seed=100)]
    sc = synthetic.make_scene(nv=nv, h=h, w=w, n_levels=5, seed=0)
    imgs, intrs, c2ws = sc["imgs"].to(dev), sc["intrs"].to(dev), sc["c2ws"].to(dev)
    feats = [f.to(dev) for f in sc["features"]]
    masks = [torch.ones(1, 1, *v.shape[2:], device=dev) for v in raw]
    torch.manual_seed(0)                                       # bench.py's build_model
    surf = ImplicitSurface(gens_model_conf(volume_dims=tuple(args.dims), n_feature_levels=5)["implicit_surface"]).to(dev).eval()
    lo, hi = torch.tensor([-1.0] * 3, device=dev), torch.tensor([1.0] * 3, device=dev)
    scene = Scene(raw, masks, imgs, feats, feats, intrs, c2ws)
    vols, views = scene.volumes_nograd(), scene.views
    cams = ops.fusion_cams(intrs, c2ws)
    near = torch.zeros(1, device=dev)
    far = torch.full((1,), float(torch.linalg.norm(c2ws[:, :3, 3], dim=1).max()) + 3.0 ** 0.5, device=dev)     # beyond every corner of the box

    def traces():
        depth = torch.empty(nv, h, w, device=dev)
        normal = torch.empty(nv, h, w, 3, device=dev)
        img = torch.empty(nv, h, w, 3, device=dev, dtype=torch.uint8)
        for v in range(nv):
            o, d = surf.view_rays(intrs, c2ws, v, (h, w))
            m = surf._trace_surface(o, d, near, far, vols, lo, hi, c2ws[[v]], views, ("depth", "normals", "colors"), args.resolution, 0.0, 1 << 21,
                                    None, None, 256, 2)
            depth[v], normal[v], img[v] = m["depth"].view(h, w), m["normal"].view(h, w, 3), m["img"].view(h, w, 3)
        return depth, normal, img

    def whole():
        return surf.fuse_surface(vols, intrs, c2ws, (h, w), lo, hi, views=views, resolution=args.resolution, min_views=args.min_views)

    depth, normal, img = traces()                              # warm-up of everything
    votes, keep, fused = ops.fuse_depth_maps(depth, cams, min_views=args.min_views)
    ops.fused_points(fused, cams, keep, normal, img)
    cloud = whole()
    stats = surf.last_fusion_stats
    ms = {"traces": [], "gens_fuse_depth_maps": [], "compact_and_gens_fused_points": [], "fuse_surface": []}
    for _ in range(args.repeats):
        ms["traces"].append(timed(traces)[0])
        ms["gens_fuse_depth_maps"].append(timed(lambda: ops.fuse_depth_maps(depth, cams, min_views=args.min_views))[0])
        ms["compact_and_gens_fused_points"].append(timed(lambda: ops.fused_points(fused, cams, keep, normal, img))[0])
        ms["fuse_surface"].append(timed(whole)[0])
    usable = sum(v["usable"] for v in stats["views"])
    pairs = usable * (nv - 1)
    result = {"workload": "BASELINE config[1] synthetic volumes %s, the model of bench.py, %d views of 480 x 640; traces: depth + normals + colours at "
                          "lipschitz %g, min_step = the spacing of a %d^3 lattice, max_steps 256, refine 2, maps kept on the device; fusion: every other view "
                          "votes, pix_tol 1, rel_tol 0.01, min_views %d; fuse_surface: all of it, read-back included"
                          % (args.dims, nv, surf.lattice_lipschitz, args.resolution, args.min_views),
              "timing": "HIP events around each part, alternating in one process; one warm-up of each, then %d repeats; ms = median (min - max)" % args.repeats,
              "device": torch.cuda.get_device_name(0)}
    result.update({k: summary(v) for k, v in ms.items()})
    fuse_ms = result["gens_fuse_depth_maps"]["ms"]
    result["fusion_over_traces"] = round((fuse_ms + result["compact_and_gens_fused_points"]["ms"]) / result["traces"]["ms"], 5)
    result["pixels"], result["usable_pixels"], result["pixel_source_pairs"] = nv * h * w, usable, pairs
    result["pixel_source_pairs_per_s"] = round(pairs / (fuse_ms * 1e-3))
    result["points"], result["kept_fraction_of_usable"] = int(len(cloud["points"])), round(len(cloud["points"]) / max(usable, 1), 5)
    result["views"] = [{"usable": v["usable"], "kept": v["kept"], "votes": v["votes"], "trace": v["trace"]} for v in stats["views"]]
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
