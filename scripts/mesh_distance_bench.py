"""Point-to-mesh distance (K36, ops.mesh_distance) beside the extraction and simplification it judges, on the scene of
scripts/sparse_lattice_bench.py: BASELINE config[1]'s synthetic volumes (256 / 128 / 64) and the model bench.py
builds, at 512^3 with sparse=4.

HIP events, one warm-up of each, then the repeats; ms = median (min - max):
  - ops.mesh_distance(full mesh, simplify=2) and (full, simplify=4) at the default `samples`, split at its part boundaries
    (ops.mesh_distance's distance_section_hook): the two grid builds, the sampling, the two query launches, the reduction with its read-back;
  - the query launch alone (gens_mesh_closest_point against the full mesh's grid), scaled to a million queries: near queries (every k-th of
    a dense sample set of the simplify=2 mesh, a million spread over the whole mesh, in K24's triangle order), the same queries sorted by the grid cell they fall in, and queries uniform in the mesh's
    box (far from every face: each walks rings of empty cells; fewer of them are launched, the count is recorded);
  - extract_geometry(sparse=4, simplify=4) with and without simplify_error (read-back included);
  - the figures themselves, as Metro reports them: mean, RMS and Hausdorff in lattice spacings for cells 2 and 4.

    python scripts/mesh_distance_bench.py --out profiles/r24_mesh_distance.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PARTS = ("grids", "sampling", "query_a_to_b", "query_b_to_a", "reduce")


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e), out


def summary(xs, scale=1.0):
    return {"ms": round(statistics.median(xs) * scale, 3), "min": round(min(xs) * scale, 3), "max": round(max(xs) * scale, 3)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default="profiles/r24_mesh_distance.json")
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--dims", type=int, nargs="+", default=[256, 128, 64])
    p.add_argument("--resolution", type=int, default=512)
    p.add_argument("--cells", type=float, nargs="+", default=[2.0, 4.0])
    p.add_argument("--box-queries", type=int, default=16384)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_distance_bench: needs the GPU (a CPU run measures nothing)")
    from gens_amd import ops, synthetic
    from gens_amd.config import gens_model_conf
    from gens_amd.models.modules.implicit_surface import ImplicitSurface
    K36 = sys.modules["gens_amd.ops.mesh_distance"]            # (the attribute ops.mesh_distance is the function; the hook lives in the module)
    dev = torch.device("cuda", 0)
    raw = [v.to(dev) for v in synthetic.make_volumes(args.dims, seed=100)]
    torch.manual_seed(0)                                       # bench.py's build_model
    surf = ImplicitSurface(gens_model_conf(volume_dims=tuple(args.dims), n_feature_levels=5)["implicit_surface"]).to(dev).eval()
    lo, hi = torch.tensor([-1.0] * 3, device=dev), torch.tensor([1.0] * 3, device=dev)
    vols = ops.VolumeSet.packed(raw)
    r = args.resolution
    with torch.no_grad():
        dv, dt = ops.marching_cubes(surf.sdf_grid(vols, lo, hi, r, sparse=4), 0.0)
    simple = {f"{c:g}": ops.simplify_mesh(dv, dt, c, origin=(-0.5, -0.5, -0.5))[:2] for c in args.cells}

    def _event():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    marks = []
    parts = {k: {n: [] for n in PARTS + ("whole",)} for k in simple}
    figures = {}

    def run_parts(k, record):
        marks.clear()
        K36.distance_section_hook = lambda n: marks.append((n, _event()))
        try:
            out = ops.mesh_distance(dv, dt, *simple[k])
        finally:
            K36.distance_section_hook = None
        torch.cuda.synchronize()
        if record:
            for (n, e0), (_, e1) in zip(marks[:-1], marks[1:]):
                parts[k][n].append(e0.elapsed_time(e1))
            parts[k]["whole"].append(marks[0][1].elapsed_time(marks[-1][1]))
        return out

    # --- the query launch alone, against the full mesh's grid
    grid = ops.build_mesh_grid(dv, dt)
    first = sorted(simple)[0]
    dense = ops.sample_mesh_points(*simple[first], 0.05 * float(first))
    near = dense[::max(1, dense.shape[0] // 1_000_000)][:1_000_000].contiguous()     # every k-th sample: the whole mesh, still in triangle order
    del dense
    box = grid.box
    cell_of = [torch.clamp(((near[:, a] - box[a]) / box[3]).floor().long(), 0, grid.dims[a] - 1) for a in range(3)]
    near_sorted = near[torch.sort((cell_of[0] * grid.dims[1] + cell_of[1]) * grid.dims[2] + cell_of[2], stable=True)[1]].contiguous()
    g = torch.Generator(device=dev).manual_seed(1)
    vmin, vmax = dv.amin(0), dv.amax(0)
    uniform = (vmin + (vmax - vmin) * torch.rand(args.box_queries, 3, device=dev, dtype=torch.float64, generator=g)).contiguous()
    queries = {"near": near, "near_sorted_by_cell": near_sorted, "uniform_in_box": uniform}
    launch = {n: [] for n in queries}

    def extract(err):
        return surf.extract_geometry(vols, lo, hi, r, 0.0, sparse=4, simplify=4, simplify_error=err)

    whole = {"unset": [], "simplify_error": []}
    for k in simple:                                           # warm-up
        figures[k] = run_parts(k, False)
    for n, q in queries.items():
        ops.mesh_closest_dist2(q, grid)
    extract(None), extract(True)
    sorted_equal = bool(torch.equal(torch.sort(ops.mesh_closest_dist2(near, grid)[0])[0], torch.sort(ops.mesh_closest_dist2(near_sorted, grid)[0])[0]))
    for _ in range(args.repeats):
        for k in simple:
            run_parts(k, True)
        for n, q in queries.items():
            launch[n].append(timed(lambda: ops.mesh_closest_dist2(q, grid))[0])
        whole["unset"].append(timed(lambda: extract(None))[0])
        whole["simplify_error"].append(timed(lambda: extract(True))[0])
    result = {"workload": "BASELINE config[1] synthetic volumes %s, the model of bench.py, the mesh of 512^3 with sparse=4 (%d faces) against its "
                          "simplifications at %s lattice spacings (%s faces), index coordinates"
                          % (args.dims, dt.shape[0], ", ".join(simple), ", ".join(str(simple[k][1].shape[0]) for k in simple)),
              "timing": "HIP events, alternating in one process; one warm-up of each, then %d repeats; ms = median (min - max); a part of "
                        "mesh_distance runs from its mark to the next and includes the host reads that follow its launches" % args.repeats,
              "device": torch.cuda.get_device_name(0), "grid_of_the_full_mesh": list(grid.dims), "mesh_distance_parts": {}, "figures": figures,
              "query_launch_ms_per_million": {}, "query_launch": {}, "sorted_queries_give_the_same_distances": sorted_equal,
              "extract_geometry_sparse4_simplify4": {k: summary(v) for k, v in whole.items()}}
    for k in simple:
        result["mesh_distance_parts"][k] = {n: summary(v) for n, v in parts[k].items()}
    for n, q in queries.items():
        result["query_launch"][n] = {"queries": int(q.shape[0]), **summary(launch[n])}
        result["query_launch_ms_per_million"][n] = summary(launch[n], 1e6 / q.shape[0])
    base = result["extract_geometry_sparse4_simplify4"]["unset"]["ms"]
    result["extract_geometry_sparse4_simplify4"]["simplify_error"]["added_fraction"] = round(
        result["extract_geometry_sparse4_simplify4"]["simplify_error"]["ms"] / base - 1.0, 4)
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
