"""Mesh fairing (K39, ops.smooth_mesh) on the mesh of scripts/mesh_repair_bench.py: BASELINE config[1]'s synthetic
volumes (256 / 128 / 64) and the model bench.py builds, at 512^3 with sparse=4, simplify=4, repaired (min_component_faces=2,
max_hole_edges=8) -- and, for the step's bandwidth at scale, on the unsimplified mesh of that lattice.

HIP events, one warm-up of each, then the repeats; ms = median (min - max):
  - ops.smooth_mesh at its defaults with uniform and with cotangent weights, split at its stage boundaries (ops.smooth_mesh's
    smooth_section_hook): topology (K37), neighbours (one sort), weights, steps (20 launches), stats (one read-back);
  - one gens_mesh_laplacian_step by itself (the profile table of gens_amd.lib), and its achieved bandwidth by algorithmic bytes,
    V (48 + 8) + 2 E (4 + 4 + 24 [+ 8]), against the 8 TB/s HBM peak (6.3 TB/s achievable) -- those bytes count a position once per
    neighbour that reads it, and most of those reads hit in cache, so the bytes that have to come from memory once,
    V (48 + 8) + 2 E (4 + 4) [+ 8 E], and their rate are given beside them;
  - extract_geometry(sparse=4, simplify=4, repair=...) with smooth unset and True (read-back included);
  - the stats with measure=True.

    python scripts/mesh_smooth_bench.py --out profiles/r31_mesh_smooth.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STAGES = ("topology", "neighbours", "weights", "steps", "stats")
REPAIR = {"min_component_faces": 2, "max_hole_edges": 8}
HBM_PEAK = 8.0e12


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e), out


def summary(xs):
    return {"ms": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default="profiles/r31_mesh_smooth.json")
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--dims", type=int, nargs="+", default=[256, 128, 64])
    p.add_argument("--resolution", type=int, default=512)
    p.add_argument("--simplify", type=float, default=4.0)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_smooth_bench: needs the GPU (a CPU run measures nothing)")
    from gens_amd import lib as L, ops, synthetic
    from gens_amd.config import gens_model_conf
    from gens_amd.models.modules.implicit_surface import ImplicitSurface
    K39 = sys.modules["gens_amd.ops.mesh_fairing"]
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
    rv, rt = ops.repair_mesh(sv, st, **REPAIR)[:2]
    meshes = {"repaired": (rv, rt), "full": (dv, dt)}

    def _event():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    marks = []

    def run_stages(mesh, kind, parts):
        marks.clear()
        K39.smooth_section_hook = lambda n: marks.append((n, _event()))
        try:
            out = ops.smooth_mesh(*mesh, weights=kind)
        finally:
            K39.smooth_section_hook = None
        torch.cuda.synchronize()
        if parts is not None:
            for (n, e0), (_, e1) in zip(marks[:-1], marks[1:]):
                parts[n].append(e0.elapsed_time(e1))
            parts["whole"].append(marks[0][1].elapsed_time(marks[-1][1]))
        return out

    def step_times(mesh, kind):
        """One gens_mesh_laplacian_step at a time: the per-launch times of the 20 steps of a default smoothing."""
        topo = ops.mesh_topology(*mesh)
        L.profile_begin(only={"gens_mesh_laplacian_step"})
        ops.smooth_mesh(*mesh, weights=kind, topology=topo)
        _, each = L.profile_end(per_launch=True)
        return each["gens_mesh_laplacian_step"], topo

    def extract(**kw):
        return surf.extract_geometry(vols, lo, hi, r, 0.0, sparse=4, simplify=args.simplify, repair=REPAIR, **kw)

    result = {"workload": "BASELINE config[1] synthetic volumes %s, the model of bench.py, the mesh of 512^3 with sparse=4 (%d faces over %d "
                          "vertices: 'full') simplified at %g lattice spacings and repaired with %s (%d faces over %d vertices: 'repaired'), "
                          "index coordinates; smoothing at its defaults (10 iterations, lam 0.5, mu -0.53, boundary fixed)"
                          % (args.dims, dt.shape[0], dv.shape[0], args.simplify, json.dumps(REPAIR), rt.shape[0], rv.shape[0]),
              "timing": "HIP events, alternating in one process; one warm-up of each, then %d repeats; ms = median (min - max); a stage of "
                        "smooth_mesh runs from its mark to the next; step_us: every gens_mesh_laplacian_step launch of those repeats by itself; "
                        "bandwidth = algorithmic bytes V (48 + 8) + 2 E (4 + 4 + 24 [+ 8 with weights]) over the median step; unique = the bytes that "
                        "must come from memory once, V (48 + 8) + 2 E (4 + 4) [+ 8 E]" % args.repeats,
              "device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK}
    for name, mesh in meshes.items():
        for kind in K39.SMOOTH_WEIGHTS:
            parts = {k: [] for k in STAGES + ("whole",)}
            run_stages(mesh, kind, None)                       # warm-up
            step_times(mesh, kind)
            steps = []
            for _ in range(args.repeats):
                run_stages(mesh, kind, parts)
                each, topo = step_times(mesh, kind)
                steps += each
            nbytes = K39.step_bytes(topo.n_vertices, topo.n_edges, kind == "cotangent")
            unique = topo.n_vertices * (48 + 8) + 2 * topo.n_edges * (4 + 4) + (8 * topo.n_edges if kind == "cotangent" else 0)
            us = statistics.median(steps) * 1e3
            floor_us = nbytes / HBM_PEAK * 1e6
            result[f"{name}_{kind}"] = {"vertices": topo.n_vertices, "edges": topo.n_edges, "stages": {k: summary(v) for k, v in parts.items() if v},
                                        "step_us": {"median": round(us, 2), "min": round(min(steps) * 1e3, 2), "max": round(max(steps) * 1e3, 2),
                                                    "launches": len(steps)},
                                        "step_bytes": nbytes, "step_bytes_per_s": round(nbytes / (us * 1e-6), 0),
                                        "fraction_of_hbm_peak": round(nbytes / (us * 1e-6) / HBM_PEAK, 4), "floor_us_at_peak": round(floor_us, 2),
                                        "times_the_floor": round(us / floor_us, 1),
                                        "step_unique_bytes": unique, "step_unique_bytes_per_s": round(unique / (us * 1e-6), 0),
                                        "unique_fraction_of_hbm_peak": round(unique / (us * 1e-6) / HBM_PEAK, 4),
                                        "times_the_unique_floor": round(us / (unique / HBM_PEAK * 1e6), 1),
                                        "stats_measured": ops.smooth_mesh(*mesh, weights=kind, measure=True)[2]}
    runs = {"unset": {}, "smooth_defaults": {"smooth": True}, "smooth_cotangent_measured": {"smooth": {"weights": "cotangent", "measure": True}}}
    whole = {k: [] for k in runs}
    for kw in runs.values():
        extract(**kw)
    for _ in range(args.repeats):
        for k, kw in runs.items():
            whole[k].append(timed(lambda: extract(**kw))[0])
    ex = result["extract_geometry_sparse4_simplify_repair"] = {k: summary(v) for k, v in whole.items()}
    for k in ("smooth_defaults", "smooth_cotangent_measured"):
        ex[k]["added_fraction"] = round(ex[k]["ms"] / ex["unset"]["ms"] - 1.0, 4)
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
