"""The per-vertex attribute pass (K30, ImplicitSurface.vertex_attributes) beside the extraction it follows, on the scene of
scripts/sparse_lattice_bench.py: BASELINE config[1]'s synthetic volumes (256 / 128 / 64), the model bench.py builds
and its five 480 x 640 views, at 512^3 and 1024^3 with bricks of 4 cells.

Two HIP event pairs per repeat: one around the extraction (sdf_grid(sparse=B) + ops.marching_cubes, the mesh left on the device), one around
the pass on that mesh (ops.vertex_points, then vertex_attributes: the network launches, ops.vertex_pack, and the read-back of the attributes).
One warm-up, then the repeats; ms = median (min - max).  The figure: the pass as a share of the extraction.  The profile table of one more
pass splits it into its launches.

    python scripts/vertex_attrs_bench.py --out profiles/r17_vertex_attrs.json
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


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default="profiles/r17_vertex_attrs.json")
    p.add_argument("--resolutions", type=int, nargs="+", default=[512, 1024])
    p.add_argument("--brick", type=int, default=4)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--views", type=int, default=5)
    p.add_argument("--dims", type=int, nargs="+", default=[256, 128, 64])
    p.add_argument("--sdf-precision", default="f32", choices=["f32", "f16x2"])
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vertex_attrs_bench: needs the GPU (a CPU run measures nothing)")
    from gens_amd import lib as L, ops, synthetic
    from gens_amd.config import gens_model_conf
    from gens_amd.models.modules.implicit_surface import ImplicitSurface
    dev = torch.device("cuda", 0)
    vols = ops.VolumeSet.packed([v.to(dev) for v in synthetic.make_volumes(args.dims, seed=100)])
    sc = synthetic.make_scene(nv=args.views, h=480, w=640, n_levels=5, seed=0)
    views = ops.SceneViews(sc["imgs"].to(dev), sc["intrs"].to(dev), sc["c2ws"].to(dev), [f.to(dev) for f in sc["features"]])
    torch.manual_seed(0)                                       # bench.py's build_model
    surf = ImplicitSurface(gens_model_conf(volume_dims=tuple(args.dims), n_feature_levels=5)["implicit_surface"]).to(dev).eval()
    surf.sdf_precision = args.sdf_precision
    lo, hi = torch.tensor([-1.0] * 3, device=dev), torch.tensor([1.0] * 3, device=dev)
    span, corner = [2.0] * 3, [-1.0] * 3
    names = ("normals", "colors")
    result = {"workload": "BASELINE config[1] synthetic volumes %s, the model of bench.py, %d views of 480 x 640, sdf_precision %s; mesh at threshold 0 "
                          "on [-1, 1]^3.  extraction: ImplicitSurface.sdf_grid(sparse=%d) + ops.marching_cubes; pass: ops.vertex_points + "
                          "ImplicitSurface.vertex_attributes(%r) on its vertices, read-back included" % (args.dims, args.views, args.sdf_precision, args.brick, names),
              "timing": "HIP events around each of the two; one warm-up, then %d repeats; ms = median (min - max)" % args.repeats,
              "device": torch.cuda.get_device_name(0), "meshes": []}
    for r in args.resolutions:
        def extraction():
            return ops.marching_cubes(surf.sdf_grid(vols, lo, hi, r, sparse=args.brick), 0.0)

        def attribute_pass(vertices):
            return surf.vertex_attributes(ops.vertex_points(vertices, r, span, corner), vols, views, names)

        mesh = extraction()                                    # warm-up of both
        attrs = attribute_pass(mesh[0])
        stats = dict(surf.last_lattice_stats)
        length = np.linalg.norm(attrs["normals"].astype(np.float64), axis=1)
        entry = {"resolution": r, "vertices": int(mesh[0].shape[0]), "triangles": int(mesh[1].shape[0]), "leaks": stats["leaks"],
                 "fell_back": stats["fell_back"], "zero_normals": int((length == 0).sum()), "seen_share": round(float(attrs["seen"].mean()), 4)}
        ms = {"extraction": [], "pass": []}
        for _ in range(args.repeats):
            t, mesh = timed(extraction)
            ms["extraction"].append(t)
            t, attrs = timed(lambda: attribute_pass(mesh[0]))
            ms["pass"].append(t)
        entry["extraction"], entry["pass"] = summary(ms["extraction"]), summary(ms["pass"])
        entry["pass_over_extraction"] = round(entry["pass"]["ms"] / entry["extraction"]["ms"], 4)
        L.profile_begin()
        attribute_pass(mesh[0])
        entry["pass_launches"] = {k: {"launches": v["launches"], "ms": round(v["ms"], 3)} for k, v in L.profile_end().items()}
        del mesh, attrs
        result["meshes"].append(entry)
        print(json.dumps(entry), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
