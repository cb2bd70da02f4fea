"""Mesh topology (K37, ops.mesh_topology) beside the extraction and simplification it judges, on the scene of
scripts/sparse_lattice_bench.py: BASELINE config[1]'s synthetic volumes (256 / 128 / 64) and the model bench.py
builds, at 512^3 with sparse=4.

HIP events, one warm-up of each, then the repeats; ms = median (min - max):
  - ops.mesh_topology with and without normals on the full mesh and on its simplify=2 mesh, split at its part boundaries
    (ops.mesh_topology's topology_section_hook) and summed into sorts (the two torch sorts with their run lengths and prefix sums) and
    kernels (K37's launches and K23's union-find); report() with its read-back on its own;
  - extract_geometry(sparse=4, simplify=4) with topology on and off (read-back included);
  - extract_geometry(sparse=4, simplify=4, simplify_error=...) with signed on and off;
  - the reports themselves.

    python scripts/mesh_topology_bench.py --out profiles/r28_mesh_topology.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PARTS = ("keys", "edge_sort", "edge_classify", "fans", "corner_sort", "vertex_classify", "components", "normals")
SORTS = ("edge_sort", "corner_sort")


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
    p.add_argument("--out", default="profiles/r28_mesh_topology.json")
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--dims", type=int, nargs="+", default=[256, 128, 64])
    p.add_argument("--resolution", type=int, default=512)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_topology_bench: needs the GPU (a CPU run measures nothing)")
    from gens_amd import ops, synthetic
    from gens_amd.config import gens_model_conf
    from gens_amd.models.modules.implicit_surface import ImplicitSurface
    K37 = sys.modules["gens_amd.ops.mesh_topology"]            # (the attribute ops.mesh_topology is the function; the hook lives in the module)
    dev = torch.device("cuda", 0)
    raw = [v.to(dev) for v in synthetic.make_volumes(args.dims, seed=100)]
    torch.manual_seed(0)                                       # bench.py's build_model
    surf = ImplicitSurface(gens_model_conf(volume_dims=tuple(args.dims), n_feature_levels=5)["implicit_surface"]).to(dev).eval()
    lo, hi = torch.tensor([-1.0] * 3, device=dev), torch.tensor([1.0] * 3, device=dev)
    vols = ops.VolumeSet.packed(raw)
    r = args.resolution
    with torch.no_grad():
        dv, dt = ops.marching_cubes(surf.sdf_grid(vols, lo, hi, r, sparse=4), 0.0)
    meshes = {"full": (dv, dt), "simplify_2": ops.simplify_mesh(dv, dt, 2.0, origin=(-0.5, -0.5, -0.5))[:2]}

    def _event():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    marks = []
    cases = [(m, n) for m in meshes for n in (False, True)]
    parts = {c: {k: [] for k in PARTS + ("whole", "sorts", "kernels", "report")} for c in cases}
    reports = {}

    def run_parts(case, record):
        marks.clear()
        K37.topology_section_hook = lambda n: marks.append((n, _event()))
        try:
            topo = ops.mesh_topology(*meshes[case[0]], normals=case[1])
        finally:
            K37.topology_section_hook = None
        torch.cuda.synchronize()
        t_report, rep = timed(topo.report)
        if record:
            sums = {"sorts": 0.0, "kernels": 0.0}
            for (n, e0), (_, e1) in zip(marks[:-1], marks[1:]):
                ms = e0.elapsed_time(e1)
                parts[case][n].append(ms)
                sums["sorts" if n in SORTS else "kernels"] += ms
            parts[case]["whole"].append(marks[0][1].elapsed_time(marks[-1][1]))
            parts[case]["sorts"].append(sums["sorts"])
            parts[case]["kernels"].append(sums["kernels"])
            parts[case]["report"].append(t_report)
        return rep

    def extract(**kw):
        return surf.extract_geometry(vols, lo, hi, r, 0.0, sparse=4, simplify=4, **kw)

    runs = {"unset": {}, "topology": {"topology": True}, "simplify_error": {"simplify_error": True},
            "simplify_error_signed": {"simplify_error": {"signed": True}}}
    whole = {k: [] for k in runs}
    for case in cases:                                         # warm-up
        reports[case[0]] = run_parts(case, False)
    for kw in runs.values():
        extract(**kw)
    extract(topology=True)
    stats = {"topology_before_simplify_4": surf.last_simplify_stats["topology_before"], "topology_after_simplify_4": surf.last_mesh_topology}
    extract(simplify_error={"signed": True})
    stats["simplify_4_error_signed"] = surf.last_simplify_stats["error"]
    for _ in range(args.repeats):
        for case in cases:
            run_parts(case, True)
        for k, kw in runs.items():
            whole[k].append(timed(lambda: extract(**kw))[0])
    result = {"workload": "BASELINE config[1] synthetic volumes %s, the model of bench.py, the mesh of 512^3 with sparse=4 (%d faces) and its "
                          "simplification at 2 lattice spacings (%d faces), index coordinates" % (args.dims, dt.shape[0], meshes["simplify_2"][1].shape[0]),
              "timing": "HIP events, alternating in one process; one warm-up of each, then %d repeats; ms = median (min - max); a part of "
                        "mesh_topology runs from its mark to the next and includes the host reads that follow its launches (the edge count after "
                        "the edge sort); sorts = edge_sort + corner_sort, kernels = the rest" % args.repeats,
              "device": torch.cuda.get_device_name(0), "mesh_topology_parts": {}, "reports": reports, **stats,
              "extract_geometry_sparse4_simplify4": {k: summary(v) for k, v in whole.items()}}
    for m, n in cases:
        result["mesh_topology_parts"][f"{m}, normals={n}"] = {k: summary(v) for k, v in parts[(m, n)].items() if v}
    ex = result["extract_geometry_sparse4_simplify4"]
    ex["topology"]["added_fraction"] = round(ex["topology"]["ms"] / ex["unset"]["ms"] - 1.0, 4)
    ex["simplify_error_signed"]["added_fraction_of_simplify_error"] = round(ex["simplify_error_signed"]["ms"] / ex["simplify_error"]["ms"] - 1.0, 4)
    ex["simplify_error_signed"]["added_fraction"] = round((ex["simplify_error_signed"]["ms"] - ex["simplify_error"]["ms"]) / ex["unset"]["ms"], 4)
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
