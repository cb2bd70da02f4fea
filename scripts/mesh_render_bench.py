"""The mesh render (K35, ops.render_mesh) beside the two other ways the package shows a view, on the scene of scripts/sparse_lattice_bench.py
(DESIGN.md section 5e): BASELINE config[1]'s synthetic volumes (256 / 128 / 64), the model bench.py builds and five 480 x 640 views, meshes
extracted at 512^3 with sparse=4.

HIP event pairs around the three steps of ops.render_mesh -- ops.build_mesh_grid, ops.ray_mesh_first_hit, ops.shade_mesh_hits -- for view
0's 307 200 rays, on the full mesh with its vertex colours and on the simplify=4 mesh with its texels = 16 atlas; one warm-up, then the
repeats; ms = median (min - max).  Beside them, timed the same way in the same process: ImplicitSurface.render_surface (K31) and validate's
volume render (extract_geometry=False) of the same view.  Then the three fidelity figures of DESIGN.md section 5k through ops.compare_maps:
the simplify=4 mesh with interpolated vertex colours, with the texels = 16 atlas, and with the atlas of snap=2, each against
render_surface's maps of view 0.

    python scripts/mesh_render_bench.py --out profiles/r23_mesh_render.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SECTION_5K = {"vertex_colours_interpolated": 33.07, "texture_16": 8.52, "texture_16_snap_2": 8.54}


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
    p.add_argument("--out", default="profiles/r23_mesh_render.json")
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--views", type=int, default=5)
    p.add_argument("--dims", type=int, nargs="+", default=[256, 128, 64])
    p.add_argument("--resolution", type=int, default=512)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_render_bench: needs the GPU (a CPU run measures nothing)")
    from gens_amd import ops, synthetic
    from gens_amd.config import gens_model_conf
    from gens_amd.models.modules.implicit_surface import ImplicitSurface, Scene
    dev = torch.device("cuda", 0)
    raw = [v.to(dev) for v in synthetic.make_volumes(args.dims, seed=100)]
    sc = synthetic.make_scene(nv=args.views, h=480, w=640, n_levels=5, seed=0)
    imgs, intrs, c2ws = sc["imgs"].to(dev), sc["intrs"].to(dev), sc["c2ws"].to(dev)
    feats = [f.to(dev) for f in sc["features"]]
    near, far = sc["near"].to(dev), sc["far"].to(dev)
    masks = [torch.ones(1, 1, *v.shape[2:], device=dev) for v in raw]
    rays_o, rays_d = synthetic.make_rays(sc["intrs"], sc["c2ws"], 480, 640)
    rays_o, rays_d = rays_o.to(dev), rays_d.to(dev)
    torch.manual_seed(0)                                       # bench.py's build_model
    surf = ImplicitSurface(gens_model_conf(volume_dims=tuple(args.dims), n_feature_levels=5)["implicit_surface"]).to(dev).eval()
    lo, hi = torch.tensor([-1.0] * 3, device=dev), torch.tensor([1.0] * 3, device=dev)
    scene = Scene(raw, masks, imgs, feats, feats, intrs, c2ws)
    vols, views = scene.volumes_nograd(), scene.views
    r = args.resolution
    rot = views.cams.rot_inv
    up = lambda a, dtype: torch.as_tensor(a).to(device=dev, dtype=dtype).contiguous()  # noqa: E731

    # --- the two meshes, on the device as render_mesh takes them
    v, t, attrs = surf.extract_geometry(vols, lo, hi, r, 0.0, sparse=4, views=views, attributes=("colors",))
    full = {"vertices": up(v, torch.float64), "triangles": up(t, torch.int32),
            "kw": {"colors": up(attrs["colors"], torch.uint8), "seen": up(attrs["seen"], torch.uint8)}}
    v4, t4, attrs4, tex = surf.extract_geometry(vols, lo, hi, r, 0.0, sparse=4, views=views, simplify=4, texture=16, attributes=("colors",))
    atlas = {"vertices": up(v4, torch.float64), "triangles": up(t4, torch.int32),
             "kw": {"texture": up(tex["texture"], torch.uint8), "texture_seen": up(tex["texture_seen"], torch.uint8), "texels": 16}}
    steps = {}
    for name, mesh in (("full_mesh_vertex_colours", full), ("simplify_4_texture_16", atlas)):
        times = {"build_mesh_grid": [], "ray_mesh_first_hit": [], "shade_mesh_hits": []}
        for k in range(args.repeats + 1):
            t_grid, grid = timed(lambda: ops.build_mesh_grid(mesh["vertices"], mesh["triangles"]))
            t_hit, (face, tt) = timed(lambda: ops.ray_mesh_first_hit(rays_o, rays_d, grid))
            t_shade, out = timed(lambda: ops.shade_mesh_hits(grid, rays_o, rays_d, face, tt, rot, **mesh["kw"]))
            if k:                                              # (the first round is the warm-up)
                for key, ms in (("build_mesh_grid", t_grid), ("ray_mesh_first_hit", t_hit), ("shade_mesh_hits", t_shade)):
                    times[key].append(ms)
        steps[name] = {"faces": int(mesh["triangles"].shape[0]), "vertices": int(mesh["vertices"].shape[0]), "rays": int(rays_o.shape[0]),
                       "hits": int(out["hit"].sum()), "grid_cells": grid.dims[0] * grid.dims[1] * grid.dims[2],
                       **{key: summary(x) for key, x in times.items()},
                       "total": summary([a + b + c for a, b, c in zip(*times.values())])}

    # --- beside: the traced surface and validate's volume render of the same view
    def trace():
        return surf.render_surface(rays_o, rays_d, near, far, vols, lo, hi, c2ws, views=views, resolution=r, hw=(480, 640))

    def volume_render():
        return surf.validate(rays_o, rays_d, near, far, raw, masks, imgs, feats, feats, intrs, c2ws, lo, hi, (480, 640), extract_geometry=False,
                             scene=scene)

    beside = {}
    for name, fn in (("render_surface", trace), ("validate_volume_render", volume_render)):
        fn()
        beside[name] = summary([timed(fn)[0] for _ in range(args.repeats)])

    # --- section 5k's fidelity figures through compare_maps
    ref = trace()
    fidelity = {}
    shaped = lambda out: {k: x.cpu().numpy() for k, x in out.items()}  # noqa: E731
    kw4 = {"colors": up(attrs4["colors"], torch.uint8), "seen": up(attrs4["seen"], torch.uint8)}
    fidelity["vertex_colours_interpolated"] = ops.compare_maps(shaped(ops.render_mesh(atlas["vertices"], atlas["triangles"], rays_o, rays_d, rot, **kw4)), ref)
    fidelity["texture_16"] = ops.compare_maps(shaped(ops.render_mesh(atlas["vertices"], atlas["triangles"], rays_o, rays_d, rot, **atlas["kw"])), ref)
    v5, t5, _, tex5 = surf.extract_geometry(vols, lo, hi, r, 0.0, sparse=4, views=views, simplify=4, texture={"texels": 16, "snap": 2})
    kw5 = {"texture": up(tex5["texture"], torch.uint8), "texture_seen": up(tex5["texture_seen"], torch.uint8), "texels": 16}
    fidelity["texture_16_snap_2"] = ops.compare_maps(shaped(ops.render_mesh(up(v5, torch.float64), up(t5, torch.int32), rays_o, rays_d, rot, **kw5)), ref)
    for key, fig in fidelity.items():
        print(f"{key}: colour mean {fig['color_mean']:.4f} (section 5k, host look-up: {SECTION_5K[key]}), max {fig['color_max']}, "
              f"both {fig['both']}, depth median {fig['depth_median']:.3g}", flush=True)
    result = {"workload": "BASELINE config[1] synthetic volumes %s, the model of bench.py, %d views of 480 x 640; meshes of extract_geometry at %d^3 "
                          "with sparse=4 (threshold 0): the full mesh with vertex colours, and simplify=4 with texture=16; view 0's %d rays"
                          % (args.dims, args.views, r, rays_o.shape[0]),
              "timing": "HIP events around each step, in one process; one warm-up, then %d repeats; ms = median (min - max); render_surface and "
                        "validate(extract_geometry=False) of the same view timed the same way" % args.repeats,
              "device": torch.cuda.get_device_name(0), "render_mesh": steps, "beside": beside,
              "fidelity": {"what": "ops.compare_maps(mesh maps, render_surface's maps) of view 0 for the simplify=4 mesh; section_5k: the host "
                                   "look-up's mean colour differences (unrounded colours) that DESIGN.md section 5k records",
                           "section_5k": SECTION_5K, **fidelity}}
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f_:
        json.dump(result, f_, indent=1)
        f_.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
