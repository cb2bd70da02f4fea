"""Generalised winding numbers (K40, ops.build_winding_plan / winding_number / mesh_inside) on the scene of scripts/sparse_lattice_bench.py
(DESIGN.md section 5e): BASELINE config[1]'s synthetic volumes (256 / 128 / 64) and the model bench.py builds, the mesh of 512^3 with
sparse=4 and its simplify=4 mesh (the pair of section 5n).

HIP events, one warm-up of each, then the repeats; ms = median (min - max):
  - build_winding_plan of the full mesh (the Morton sort in torch and the moments launch);
  - exact mode for a subset of 10 000 of the simplified mesh's ~10^6 mesh_distance samples against the full mesh, one launch (chunk = the
    subset);
  - the far field at beta = 2, 3, 4 (and 6, 8) for all the samples, as sampled and Morton-sorted (the sort timed on its own), chunk = 2^18: the time,
    the share of undecided samples (ops.mesh_inside's -1), the largest bound, the largest |fast - exact| on the subset;
  - ops.mesh_distance(signed=True) of the pair with both signs, and what K40 says where K37 has no sign.

    python scripts/winding_bench.py --out profiles/r32_winding.json
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BETAS = (2.0, 3.0, 4.0, 6.0, 8.0)      # the three candidates for mesh_distance's default, and two more rungs should none of them do
CHUNK = 1 << 18


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e), out


def summary(xs):
    return {"ms": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def repeat(fn, repeats, long_ms=4000.0):
    warm = timed(fn)[0]                                        # warm-up
    if warm > long_ms:                                         # (a pass of seconds: one repeat, and the figure says so)
        repeats = 1
    runs = [timed(fn) for _ in range(repeats)]
    return {**summary([ms for ms, _ in runs]), "repeats": repeats}, runs[-1][1]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default="profiles/r32_winding.json")
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--dims", type=int, nargs="+", default=[256, 128, 64])
    p.add_argument("--resolution", type=int, default=512)
    p.add_argument("--samples", type=int, default=1_000_000)
    p.add_argument("--subset", type=int, default=10_000)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("winding_bench: needs the GPU (a CPU run measures nothing)")
    from gens_amd import ops, synthetic
    from gens_amd.config import gens_model_conf
    from gens_amd.models.modules.implicit_surface import ImplicitSurface
    from gens_amd.ops.winding import _spread3
    dev = torch.device("cuda", 0)
    raw = [v.to(dev) for v in synthetic.make_volumes(args.dims, seed=100)]
    torch.manual_seed(0)                                       # bench.py's build_model
    surf = ImplicitSurface(gens_model_conf(volume_dims=tuple(args.dims), n_feature_levels=5)["implicit_surface"]).to(dev).eval()
    lo, hi = torch.tensor([-1.0] * 3, device=dev), torch.tensor([1.0] * 3, device=dev)
    vols = ops.VolumeSet.packed(raw)
    with torch.no_grad():
        dv, dt = ops.marching_cubes(surf.sdf_grid(vols, lo, hi, args.resolution, sparse=4), 0.0)
    dv = dv.to(torch.float64)
    sv, st = ops.simplify_mesh(dv, dt, 4.0, origin=(-0.5, -0.5, -0.5))[:2]
    sv = sv.to(torch.float64)
    result = {"workload": "BASELINE config[1] synthetic volumes %s, the model of bench.py, the mesh of %d^3 with sparse=4 (%d faces) and its "
                          "simplification at 4 lattice spacings (%d faces), index coordinates" % (args.dims, args.resolution, dt.shape[0], st.shape[0]),
              "timing": "HIP events in one process; one warm-up of each, then %d repeats; ms = median (min - max)" % args.repeats,
              "device": torch.cuda.get_device_name(0), "chunk": CHUNK}
    print(result["workload"], flush=True)

    result["build_winding_plan"], plan = repeat(lambda: ops.build_winding_plan(dv, dt), args.repeats)
    result["plan"] = {"faces": plan.n_faces, "leaves": plan.n_leaves, "nodes": plan.n_nodes,
                      "leaf_radius_median": float(plan.leaf_radius2.sqrt().median()), "node_radius_median": float(plan.node_radius2.sqrt().median())}
    print(json.dumps({k: result[k] for k in ("build_winding_plan", "plan")}), flush=True)

    area = float(0.5 * torch.linalg.cross(sv[st[:, 1].long()] - sv[st[:, 0].long()], sv[st[:, 2].long()] - sv[st[:, 0].long()]).norm(dim=1).sum())
    samples = ops.sample_mesh_points(sv, st, math.sqrt(area / args.samples))
    n = samples.shape[0]

    def morton_sorted():
        lo_, hi_ = samples.amin(dim=0), samples.amax(dim=0)
        cell = ((samples - lo_) / (hi_ - lo_) * 1024.0).floor().clamp(0.0, 1023.0).long()
        key = (_spread3(cell[:, 0]) << 2) | (_spread3(cell[:, 1]) << 1) | _spread3(cell[:, 2])
        return samples[torch.sort(key, stable=True)[1]].contiguous()

    result["morton_sort_of_the_samples"], ordered = repeat(morton_sorted, args.repeats)
    subset = samples[:: max(1, n // args.subset)][:args.subset].contiguous()
    result["samples"], result["subset"] = n, subset.shape[0]
    result["exact"], exact = repeat(lambda: ops.winding_number(subset, plan, chunk=subset.shape[0]), args.repeats)
    result["exact"]["solid_angles_per_second"] = round(subset.shape[0] * plan.n_faces / (result["exact"]["ms"] * 1e-3), 0)
    result["exact"]["w_min_max"] = [float(exact.min()), float(exact.max())]
    print(json.dumps({"samples": n, "exact": result["exact"]}), flush=True)

    result["fast"] = {}
    for beta in BETAS:
        row = {}
        for name, pts in (("unsorted", samples), ("sorted", ordered)):
            row[name], (w, bound) = repeat(lambda: ops.winding_number(pts, plan, beta=beta, bound=True, chunk=CHUNK), args.repeats)
            verdict = torch.full_like(w, -1.0)
            verdict[w - bound >= 0.5] = 1.0
            verdict[w + bound < 0.5] = 0.0
            row[name].update(undecided=int((verdict < 0).sum()), undecided_share=float((verdict < 0).double().mean()), inside=int((verdict == 1).sum()),
                             bound_max=float(bound.max()), bound_median=float(bound.median()))
        fast = ops.winding_number(subset, plan, beta=beta)
        row["max_abs_fast_minus_exact_on_subset"] = float((fast - exact).abs().max())
        row["sorted_over_unsorted"] = round(row["sorted"]["ms"] / row["unsorted"]["ms"], 4)
        result["fast"][str(beta)] = row
        print(json.dumps({"beta": beta, **row}), flush=True)
    qualifying = [b for b in BETAS if result["fast"][str(b)]["unsorted"]["undecided_share"] < 1e-4]
    result["smallest_beta_with_fewer_than_1e-4_undecided"] = qualifying[0] if qualifying else None
    result["mesh_distance_default_beta"] = ops.MESH_DISTANCE_BETA
    chosen = qualifying[0] if qualifying else BETAS[-1]
    result["mesh_distance_signed_beta"] = chosen

    # the pair of section 5n under both signs
    signs = {}
    for sign in ("pseudonormal", "winding"):
        signs[sign], out = repeat(lambda: ops.mesh_distance(dv, dt, sv, st, signed=True, sign=sign, return_samples=True,
                                                                **({"beta": chosen} if sign == "winding" else {})), min(args.repeats, 3))
        signs[sign]["a_to_b"], signs[sign]["b_to_a"] = out["a_to_b"], out["b_to_a"]
        if sign == "pseudonormal":
            lost = {s: out["samples_" + s][out["signed_" + s].isnan() & torch.isfinite(out["dist_" + s])] for s in "ab"}
    other = {"a": ops.build_winding_plan(sv, st), "b": plan}   # a's samples are signed by b = the simplified mesh, and the reverse
    signs["where_k37_has_no_sign"] = {}
    for s in "ab":
        if lost[s].shape[0]:
            w, bound = ops.winding_number(lost[s].contiguous(), other[s], beta=chosen, bound=True)
            exact_w = ops.winding_number(lost[s].contiguous(), other[s])
            signs["where_k37_has_no_sign"][s] = {"samples": lost[s].cpu().tolist()[:8], "w": w.cpu().tolist()[:8], "bound": bound.cpu().tolist()[:8],
                                                 "w_exact": exact_w.cpu().tolist()[:8],
                                                 "mesh_inside": ops.mesh_inside(lost[s].contiguous(), other[s], beta=chosen).cpu().tolist()[:8]}
    result["mesh_distance_signed"] = signs
    print(json.dumps(signs), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
