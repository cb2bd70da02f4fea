"""Dense against sparse SDF lattice (K28, ImplicitSurface.sdf_grid(sparse=B)) on the bench's scene: BASELINE config[1]'s synthetic volumes
(256 / 128 / 64) and the model bench.py builds, at 512^3 and -- memory allowing -- 1024^3, B in {4, 8, 16}.

Every variant is timed with HIP events around the whole sdf_grid call (which ends in its own host reads), after a warm-up of each shape;
the variants ALTERNATE inside every repeat, so a change of clocks or a neighbour on the host meets all of them; the figure is the median of
the repeats, with the smallest and the largest beside it.  Besides the time: the share of lattice points handed to the network, the leak
count, whether the call fell back, and whether marching cubes returns the dense lattice's vertices and triangles (torch.equal).

    python scripts/sparse_lattice_bench.py --out profiles/r07_sparse_lattice.json

--mesh: the mesh extraction instead of the lattice (K29).  Two routes alternate in one process: the parent route,
sdf_grid(sparse=B) + ops.marching_cubes, and the brick route, ops.brick_marching_cubes through extract_geometry's helper; both end with the
mesh on the device and their own host reads.  Beside the times: peak allocated memory of each route, V, T, the emitting-brick count, and
whether the two meshes are equal.  Resolutions in --brick-only (2048 by default) run the brick route alone: their dense lattice is beyond
the parent route.

    python scripts/sparse_lattice_bench.py --mesh --out profiles/r15_brick_mcubes.json
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


def peak_of(fn, dev):
    """fn() -> (its result, peak bytes allocated during it above what was allocated before)."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    out = fn()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated(dev) - base


def mesh_mode(args, surf, vols, lo, hi, dev):
    from gens_amd import ops
    b = args.mesh_brick
    result = {"workload": "BASELINE config[1] synthetic volumes %s, the model of bench.py, sdf_precision %s; mesh at threshold 0 on [-1, 1]^3, brick %d, "
                          "lattice_lipschitz %.1f.  parent: ImplicitSurface.sdf_grid(sparse=%d) + ops.marching_cubes; brick: ops.brick_marching_cubes "
                          "(ImplicitSurface._brick_mesh)" % (args.dims, args.sdf_precision, b, surf.lattice_lipschitz, b),
              "timing": "HIP events around each route, mesh left on the device; one warm-up per route, then %d repeats with the routes alternating; "
                        "ms = median (min - max).  peak_bytes: torch.cuda.max_memory_allocated over one call, above the scene's own" % args.repeats,
              "device": torch.cuda.get_device_name(0), "meshes": []}

    for r in list(args.resolutions) + list(args.brick_only):
        def parent():
            return ops.marching_cubes(surf.sdf_grid(vols, lo, hi, r, sparse=b), 0.0)

        def brick():
            return surf._brick_mesh(vols, lo, hi, r, 0.0, b)

        routes = {"brick": brick}
        if r in args.resolutions:
            routes["parent"] = parent
        entry = {"resolution": r}
        meshes = {}
        for name, fn in routes.items():                       # warm-up, and the figures that are no times
            meshes[name], peak = peak_of(fn, dev)
            if meshes[name] is None:
                raise SystemExit("sparse_lattice_bench: the brick route counted leaks at %d^3 (lattice_lipschitz %.1f): nothing to time" % (r, surf.lattice_lipschitz))
            stats = dict(surf.last_lattice_stats)
            v, t = meshes[name]
            entry[name] = {"vertices": int(v.shape[0]), "triangles": int(t.shape[0]), "peak_bytes": int(peak), "leaks": stats["leaks"],
                           "active_bricks": stats["active_bricks"], "bricks": stats["bricks"], "evaluated_share": stats["evaluated_points"] / r ** 3}
            if name == "brick":
                entry[name]["emitting_bricks"] = stats["emitting_bricks"]
        if "parent" in meshes:
            (v0, t0), (v1, t1) = meshes["parent"], meshes["brick"]
            entry["meshes_equal"] = bool(v0.shape == v1.shape and t0.shape == t1.shape and torch.equal(v0, v1) and torch.equal(t0, t1))
        del meshes
        ms = {name: [] for name in routes}
        for _ in range(args.repeats):
            for name, fn in routes.items():
                t, out = timed(fn)
                del out
                ms[name].append(t)
        for name in routes:
            entry[name].update(summary(ms[name]))
        if "parent" in routes:
            entry["parent_over_brick"] = round(entry["parent"]["ms"] / entry["brick"]["ms"], 3)
        result["meshes"].append(entry)
        print(json.dumps(entry), flush=True)
    return result


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default="profiles/r07_sparse_lattice.json")
    p.add_argument("--resolutions", type=int, nargs="+", default=[512, 1024])
    p.add_argument("--bricks", type=int, nargs="+", default=[4, 8, 16])
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--dims", type=int, nargs="+", default=[256, 128, 64])
    p.add_argument("--sdf-precision", default="f32", choices=["f32", "f16x2"])
    p.add_argument("--mesh", action="store_true", help="time the mesh extraction: sdf_grid(sparse) + marching_cubes against brick_marching_cubes")
    p.add_argument("--mesh-brick", type=int, default=4)
    p.add_argument("--brick-only", type=int, nargs="*", default=[2048], help="--mesh: resolutions for the brick route alone")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sparse_lattice_bench: needs the GPU (a CPU run measures nothing)")
    from gens_amd import ops, synthetic
    from gens_amd.config import gens_model_conf
    from gens_amd.models.modules.implicit_surface import ImplicitSurface
    dev = torch.device("cuda", 0)
    vols = ops.VolumeSet.packed([v.to(dev) for v in synthetic.make_volumes(args.dims, seed=100)])
    torch.manual_seed(0)                                       # bench.py's build_model
    surf = ImplicitSurface(gens_model_conf(volume_dims=tuple(args.dims), n_feature_levels=5)["implicit_surface"]).to(dev).eval()
    surf.sdf_precision = args.sdf_precision
    lo, hi = torch.tensor([-1.0] * 3, device=dev), torch.tensor([1.0] * 3, device=dev)
    if args.mesh:
        write(args.out, mesh_mode(args, surf, vols, lo, hi, dev))
        return
    result = {"workload": "BASELINE config[1] synthetic volumes %s, the model of bench.py, sdf_precision %s; ImplicitSurface.sdf_grid on [-1, 1]^3, "
                          "threshold 0, lattice_lipschitz %.1f" % (args.dims, args.sdf_precision, surf.lattice_lipschitz),
              "timing": "HIP events around each sdf_grid call; one warm-up per variant, then %d repeats with the variants alternating; ms = median "
                        "(min - max)" % args.repeats,
              "device": torch.cuda.get_device_name(0), "lattices": []}
    for r in args.resolutions:
        need = 4 * r ** 3 * 4                                  # two lattices and the iso-surface's per-cell bytes
        free = torch.cuda.mem_get_info(dev)[0]
        if need > free:
            result["lattices"].append({"resolution": r, "skipped": "needs about %.1f GB, %.1f GB free" % (need / 1e9, free / 1e9)})
            continue
        variants = [None] + list(args.bricks)
        runs = {v: (lambda v=v: surf.sdf_grid(vols, lo, hi, r, sparse=v)) for v in variants}
        dense = runs[None]()                                   # warm-up of the dense shape, and the lattice the meshes are compared with
        v0, t0 = ops.marching_cubes(dense, 0.0)
        entry = {"resolution": r, "dense": {"vertices": int(v0.shape[0]), "triangles": int(t0.shape[0])}, "sparse": {}}
        for b in args.bricks:
            u = runs[b]()                                      # warm-up
            stats = dict(surf.last_lattice_stats)
            v1, t1 = ops.marching_cubes(u, 0.0)
            entry["sparse"][str(b)] = {"evaluated_share": stats["evaluated_points"] / r ** 3, "active_bricks": stats["active_bricks"],
                                       "bricks": stats["bricks"], "leaks": stats["leaks"], "fell_back": stats["fell_back"],
                                       "vertices_equal": bool(v1.shape == v0.shape and torch.equal(v1, v0)),
                                       "triangles_equal": bool(t1.shape == t0.shape and torch.equal(t1, t0))}
            del u, v1, t1
        del dense, v0, t0
        ms = {v: [] for v in variants}
        for _ in range(args.repeats):
            for v in variants:
                t, u = timed(runs[v])
                del u
                ms[v].append(t)
        entry["dense"].update(summary(ms[None]))
        for b in args.bricks:
            entry["sparse"][str(b)].update(summary(ms[b]))
            entry["sparse"][str(b)]["dense_over_sparse"] = round(entry["dense"]["ms"] / entry["sparse"][str(b)]["ms"], 3)
        result["lattices"].append(entry)
        print(json.dumps(entry), flush=True)
    write(args.out, result)


def write(path, result):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
