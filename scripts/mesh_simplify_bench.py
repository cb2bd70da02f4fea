"""Mesh simplification (K33, ops.simplify_mesh) beside the extraction it follows, on the scene of scripts/sparse_lattice_bench.py (DESIGN.md
section 5e): BASELINE config[1]'s synthetic volumes (256 / 128 / 64) and the model bench.py builds, at 512^3.

HIP event pairs per repeat around the whole of ImplicitSurface.extract_geometry (read-back included) with `simplify` unset, 2 and 4, on the
dense route and on `sparse=4`, alternating in one process; and, on the device-resident 512^3 mesh, events at the part boundaries of
ops.simplify_mesh (ops.simplify.section_hook): the host checks, the keys kernel, the sorts, the triangles kernel, the duplicate removal and
output numbering, the solve kernel.  A part's time runs from its mark to the next, so it includes the host reads of sizes that follow its
launches.  One warm-up of each, then the repeats; ms = median (min - max).  Also recorded: vertex, face and PLY byte counts (write_ply, bare
mesh) per setting, and simplify_mesh's stats.

    python scripts/mesh_simplify_bench.py --out profiles/r21_mesh_simplify.json
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PARTS = ("checks", "keys", "sorts", "triangles", "duplicates", "solve")


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
    p.add_argument("--out", default="profiles/r21_mesh_simplify.json")
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--dims", type=int, nargs="+", default=[256, 128, 64])
    p.add_argument("--resolution", type=int, default=512)
    p.add_argument("--cells", type=float, nargs="+", default=[2.0, 4.0])
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_simplify_bench: needs the GPU (a CPU run measures nothing)")
    from gens_amd import io as gio, ops
    from gens_amd import synthetic
    from gens_amd.config import gens_model_conf
    from gens_amd.models.modules.implicit_surface import ImplicitSurface
    from gens_amd.ops import simplify as K33
    dev = torch.device("cuda", 0)
    raw = [v.to(dev) for v in synthetic.make_volumes(args.dims, seed=100)]
    torch.manual_seed(0)                                       # bench.py's build_model
    surf = ImplicitSurface(gens_model_conf(volume_dims=tuple(args.dims), n_feature_levels=5)["implicit_surface"]).to(dev).eval()
    lo, hi = torch.tensor([-1.0] * 3, device=dev), torch.tensor([1.0] * 3, device=dev)
    vols = ops.VolumeSet.packed(raw)
    r = args.resolution
    settings = [None] + list(args.cells)
    routes = {"dense": {}, "sparse4": {"sparse": 4}}
    name = lambda s: "unset" if s is None else f"simplify_{s:g}"  # noqa: E731

    def extract(route, s):
        return surf.extract_geometry(vols, lo, hi, r, 0.0, simplify=s, **routes[route])

    # --- the device-resident mesh and the parts of simplify_mesh on it
    with torch.no_grad():
        dv, dt = ops.marching_cubes(surf.sdf_grid(vols, lo, hi, r, sparse=4), 0.0)
    marks = []
    parts = {f"{c:g}": {k: [] for k in PARTS + ("whole",)} for c in args.cells}
    stats = {}

    def run_parts(c, record):
        marks.clear()
        K33.section_hook = lambda n: marks.append((n, _event()))
        try:
            out = ops.simplify_mesh(dv, dt, c, origin=(-0.5, -0.5, -0.5))
        finally:
            K33.section_hook = None
        torch.cuda.synchronize()
        if record:
            acc = {k: 0.0 for k in PARTS}
            for (n, e0), (_, e1) in zip(marks[:-1], marks[1:]):
                acc[n] += e0.elapsed_time(e1)
            for k in PARTS:
                parts[f"{c:g}"][k].append(acc[k])
            parts[f"{c:g}"]["whole"].append(marks[0][1].elapsed_time(marks[-1][1]))
        return out

    def _event():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    for c in args.cells:                                       # warm-up
        stats[f"{c:g}"] = run_parts(c, False)[3]
    meshes = {route: {name(s): extract(route, s) for s in settings} for route in routes}
    whole = {route: {name(s): [] for s in settings} for route in routes}
    for _ in range(args.repeats):
        for c in args.cells:
            run_parts(c, True)
        for route in routes:
            for s in settings:
                whole[route][name(s)].append(timed(lambda: extract(route, s))[0])
    # --- counts and PLY bytes
    sizes = {}
    with tempfile.TemporaryDirectory() as tmp:
        for s in settings:
            v, t = meshes["sparse4"][name(s)]
            path = os.path.join(tmp, "m.ply")
            gio.write_ply(path, v, t)
            sizes[name(s)] = {"vertices": int(len(v)), "faces": int(len(t)), "ply_bytes": os.path.getsize(path)}
    same = all(len(meshes["dense"][name(s)][0]) == len(meshes["sparse4"][name(s)][0]) and (meshes["dense"][name(s)][0] == meshes["sparse4"][name(s)][0]).all()
               and (meshes["dense"][name(s)][1] == meshes["sparse4"][name(s)][1]).all() for s in settings)
    result = {"workload": "BASELINE config[1] synthetic volumes %s, the model of bench.py, extract_geometry at %d^3 (threshold 0, read-back included) with "
                          "simplify unset and at %s lattice spacings, on the dense route and on sparse=4; the parts of ops.simplify_mesh on the "
                          "device-resident mesh of that lattice (origin -0.5)" % (args.dims, r, ", ".join(f"{c:g}" for c in args.cells)),
              "timing": "HIP events around each call and at the part boundaries, alternating in one process; one warm-up of each, then %d repeats; "
                        "ms = median (min - max); a part runs from its mark to the next and includes the host reads of sizes that follow its launches"
                        % args.repeats,
              "device": torch.cuda.get_device_name(0), "routes_return_equal_meshes": bool(same), "meshes": sizes,
              "simplify_mesh_stats": stats, "extract_geometry": {}, "simplify_mesh_parts": {}}
    for route in routes:
        result["extract_geometry"][route] = {k: summary(v) for k, v in whole[route].items()}
        base = result["extract_geometry"][route]["unset"]["ms"]
        for s in args.cells:
            result["extract_geometry"][route][name(s)]["added_fraction"] = round(result["extract_geometry"][route][name(s)]["ms"] / base - 1.0, 4)
    for c in args.cells:
        result["simplify_mesh_parts"][f"{c:g}"] = {k: summary(v) for k, v in parts[f"{c:g}"].items()}
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
