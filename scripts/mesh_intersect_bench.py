"""Self-intersections (K41, ops.mesh_self_intersections) on the scene of scripts/sparse_lattice_bench.py: BASELINE
config[1]'s synthetic volumes (256 / 128 / 64) and the model bench.py builds, the mesh of 512^3 with sparse=4, its simplify=4 mesh, that mesh
repaired (ops.repair_mesh with max_hole_edges=64: the hole filler on) and the repaired mesh smoothed (ops.smooth_mesh's defaults): the meshes of sections 5m to 5q.

Per mesh, one warm-up and then the repeats; ms = median (min - max) of HIP events: ops.build_mesh_grid (K23), and inside
ops.mesh_self_intersections the three launches on their own (gens_mesh_isect_faces, _count, _emit) and the whole call; the counts, the
candidates per face, the share of candidates one strict plane separation decided alone, the longest cell list, and what the kernel's work
comes to: candidate pairs per second and the bytes of the gathers (per walked entry: a face id, a class byte and a 48-byte box).

    python scripts/mesh_intersect_bench.py --out profiles/r33_mesh_intersect.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K41 = ("gens_mesh_isect_faces", "gens_mesh_isect_count", "gens_mesh_isect_emit")


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
    p.add_argument("--out", default="profiles/r33_mesh_intersect.json")
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--dims", type=int, nargs="+", default=[256, 128, 64])
    p.add_argument("--resolution", type=int, default=512)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_intersect_bench: needs the GPU (a CPU run measures nothing)")
    from gens_amd import lib as L, ops, synthetic
    from gens_amd.config import gens_model_conf
    from gens_amd.models.modules.implicit_surface import ImplicitSurface
    dev = torch.device("cuda", 0)
    raw = [v.to(dev) for v in synthetic.make_volumes(args.dims, seed=100)]
    torch.manual_seed(0)                                       # bench.py's build_model
    surf = ImplicitSurface(gens_model_conf(volume_dims=tuple(args.dims), n_feature_levels=5)["implicit_surface"]).to(dev).eval()
    lo, hi = torch.tensor([-1.0] * 3, device=dev), torch.tensor([1.0] * 3, device=dev)
    vols = ops.VolumeSet.packed(raw)
    with torch.no_grad():
        dv, dt = ops.marching_cubes(surf.sdf_grid(vols, lo, hi, args.resolution, sparse=4), 0.0)
    meshes = {"extracted": (dv.to(torch.float64), dt)}
    sv, st = ops.simplify_mesh(dv, dt, 4.0, origin=(-0.5, -0.5, -0.5))[:2]
    meshes["simplify=4"] = (sv.to(torch.float64), st)
    rv, rt = ops.repair_mesh(*meshes["simplify=4"], max_hole_edges=64)[:2]      # (with the hole filler, which is off by default)
    meshes["repaired"] = (rv, rt)
    fv, ft = ops.smooth_mesh(rv, rt)[:2]
    meshes["smoothed"] = (fv, ft)
    result = {"workload": "BASELINE config[1] synthetic volumes %s, the model of bench.py, the mesh of %d^3 with sparse=4, its simplification at 4 "
                          "lattice spacings, that repaired, that smoothed; index coordinates" % (args.dims, args.resolution),
              "timing": "HIP events in one process; one warm-up of each, then %d repeats; ms = median (min - max)" % args.repeats,
              "device": torch.cuda.get_device_name(0), "meshes": {}}
    for name, (v, t) in meshes.items():
        row = {"vertices": v.shape[0], "faces": t.shape[0]}
        timed(lambda: ops.build_mesh_grid(v, t))
        runs = [timed(lambda: ops.build_mesh_grid(v, t)) for _ in range(args.repeats)]
        row["build_mesh_grid"], grid = summary([ms for ms, _ in runs]), runs[-1][1]
        lists = grid.cell_start[1:] - grid.cell_start[:-1]
        row["grid"] = {"dims": list(grid.dims), "entries": int(grid.cell_start[-1]), "longest_list": int(lists.max()),
                       "entries_walked": int((lists.long() * (lists.long() - 1) // 2).sum())}
        timed(lambda: ops.mesh_self_intersections(grid))
        whole, each = [], {k: [] for k in K41}
        for _ in range(args.repeats):
            ms, found = timed(lambda: ops.mesh_self_intersections(grid))
            whole.append(ms)
            L.profile_begin(only=set(K41))
            ops.mesh_self_intersections(grid)
            for k, one, *_ in L.profile_end(raw=True):
                each[k].append(one)
        row["mesh_self_intersections"] = summary(whole)
        for k in K41:
            row[k] = summary(each[k]) if each[k] else None
        c = found.counts
        row["counts"] = c
        row["candidates_per_face"] = round(c["candidates"] / max(1, c["faces"]), 3)
        row["plane_separated_share"] = round(c["plane_separated"] / max(1, c["candidates"]), 4)
        row["undecided_share"] = c["undecided"] / max(1, c["candidates"])
        count_s = row["gens_mesh_isect_count"]["ms"] * 1e-3
        row["count_kernel"] = {"pairs_walked_per_second": round(row["grid"]["entries_walked"] / count_s, 0),
                               "candidates_per_second": round(c["candidates"] / count_s, 0),
                               "gather_GBps": round((row["grid"]["entries_walked"] * 53 + c["candidates"] * (12 + 72)) / count_s / 1e9, 2)}
        if found.pairs is not None and found.pairs.shape[0]:
            row["first_pairs"] = {"pairs": found.pairs[:8].cpu().tolist(), "kinds": found.kinds[:8].cpu().tolist()}
        result["meshes"][name] = row
        print(name, json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
