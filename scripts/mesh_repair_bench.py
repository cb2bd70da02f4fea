"""Mesh repair (K38, ops.repair_mesh) on the mesh that needs it, on the scene of scripts/mesh_topology_bench.py:
BASELINE config[1]'s synthetic volumes (256 / 128 / 64) and the model bench.py builds, at 512^3 with sparse=4 and simplify=4.

HIP events, one warm-up of each, then the repeats; ms = median (min - max):
  - ops.repair_mesh(min_component_faces=2, max_hole_edges=8) on the simplify=4 mesh, split at its stage boundaries (ops.repair_mesh's
    repair_section_hook); a stage includes K37's topology where it has to take it and the host reads that follow its launches;
  - extract_geometry(sparse=4, simplify=4) with repair unset, True and with those options (read-back included);
  - the topology reports before and after, and the repair's counts.

    python scripts/mesh_repair_bench.py --out profiles/r30_mesh_repair.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STAGES = ("dedupe", "split", "components", "orient", "fill")
OPTIONS = {"min_component_faces": 2, "max_hole_edges": 8}


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
    p.add_argument("--out", default="profiles/r30_mesh_repair.json")
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--dims", type=int, nargs="+", default=[256, 128, 64])
    p.add_argument("--resolution", type=int, default=512)
    p.add_argument("--simplify", type=float, default=4.0)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_repair_bench: needs the GPU (a CPU run measures nothing)")
    from gens_amd import ops, synthetic
    from gens_amd.config import gens_model_conf
    from gens_amd.models.modules.implicit_surface import ImplicitSurface
    K38 = sys.modules["gens_amd.ops.mesh_repair"]
    dev = torch.device("cuda", 0)
    raw = [v.to(dev) for v in synthetic.make_volumes(args.dims, seed=100)]
    torch.manual_seed(0)                                       # bench.py's build_model
    surf = ImplicitSurface(gens_model_conf(volume_dims=tuple(args.dims), n_feature_levels=5)["implicit_surface"]).to(dev).eval()
    lo, hi = torch.tensor([-1.0] * 3, device=dev), torch.tensor([1.0] * 3, device=dev)
    vols = ops.VolumeSet.packed(raw)
    r = args.resolution
    with torch.no_grad():
        dv, dt = ops.marching_cubes(surf.sdf_grid(vols, lo, hi, r, sparse=4), 0.0)
    sv, st = ops.simplify_mesh(dv, dt, args.simplify, origin=(-0.5, -0.5, -0.5))[:2]

    def _event():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    marks = []
    parts = {k: [] for k in STAGES + ("whole",)}

    def run_stages(record):
        marks.clear()
        K38.repair_section_hook = lambda n: marks.append((n, _event()))
        try:
            out = ops.repair_mesh(sv, st, **OPTIONS)
        finally:
            K38.repair_section_hook = None
        torch.cuda.synchronize()
        if record:
            for (n, e0), (_, e1) in zip(marks[:-1], marks[1:]):
                parts[n].append(e0.elapsed_time(e1))
            parts["whole"].append(marks[0][1].elapsed_time(marks[-1][1]))
        return out

    def extract(**kw):
        return surf.extract_geometry(vols, lo, hi, r, 0.0, sparse=4, simplify=args.simplify, **kw)

    runs = {"unset": {}, "repair_defaults": {"repair": True}, "repair_options": {"repair": OPTIONS}}
    whole = {k: [] for k in runs}
    out = run_stages(False)                                    # warm-up
    for kw in runs.values():
        extract(**kw)
    reports = {"before": ops.mesh_topology(sv, st).report(), "after_options": ops.mesh_topology(out[0], out[1]).report(), "stats_options": out[5]}
    plain = ops.repair_mesh(sv, st)
    reports["after_defaults"], reports["stats_defaults"] = ops.mesh_topology(plain[0], plain[1]).report(), plain[5]
    for _ in range(args.repeats):
        run_stages(True)
        for k, kw in runs.items():
            whole[k].append(timed(lambda: extract(**kw))[0])
    result = {"workload": "BASELINE config[1] synthetic volumes %s, the model of bench.py, the mesh of 512^3 with sparse=4 (%d faces) simplified at "
                          "%g lattice spacings (%d faces over %d vertices), index coordinates; repair options %s"
                          % (args.dims, dt.shape[0], args.simplify, st.shape[0], sv.shape[0], json.dumps(OPTIONS)),
              "timing": "HIP events, alternating in one process; one warm-up of each, then %d repeats; ms = median (min - max); a stage of "
                        "repair_mesh runs from its mark to the next and includes K37's topology where the stage takes it and the host reads "
                        "that follow its launches" % args.repeats,
              "device": torch.cuda.get_device_name(0), "repair_mesh_stages": {k: summary(v) for k, v in parts.items() if v}, **reports,
              "extract_geometry_sparse4_simplify": {k: summary(v) for k, v in whole.items()}}
    ex = result["extract_geometry_sparse4_simplify"]
    for k in ("repair_defaults", "repair_options"):
        ex[k]["added_fraction"] = round(ex[k]["ms"] / ex["unset"]["ms"] - 1.0, 4)
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
