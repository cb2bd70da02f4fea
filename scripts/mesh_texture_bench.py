"""Texture atlases (K34, ImplicitSurface.texture_mesh) beside the extraction they follow, on the scene of scripts/sparse_lattice_bench.py
(DESIGN.md section 5e): BASELINE config[1]'s synthetic volumes (256 / 128 / 64), the model bench.py builds and five 480 x 640 views, at
512^3 with sparse=4.

HIP event pairs per repeat around the whole of ImplicitSurface.extract_geometry (read-back included) with the texture unset, texture=8 on
the full mesh, simplify=4 + texture=16, and the same with snap=2, alternating in one process; one warm-up of each, then the repeats;
ms = median (min - max).  One more call per setting under lib.profile_begin gives the per-launch times of the K34 kernels beside the
network launches they feed.  Also recorded: atlas sizes, PNG / OBJ bytes against the vertex-coloured PLY, texture_mesh's stats, and the
image fidelity of the simplified mesh: view 0's rays are cast at the mesh (ops.ray_mesh_first_hit), the colour at the hit is looked up
three ways on the host -- vertex colours interpolated, the atlas sampled bilinearly, the atlas of snap=2 -- and compared with
render_surface's colour map of the same view (mean absolute difference in 8-bit units over the pixels both hit).

    python scripts/mesh_texture_bench.py --out profiles/r22_mesh_texture.json
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K34 = ("gens_texture_points", "gens_texture_snap", "gens_texture_keep_better", "gens_texture_pack", "gens_texture_uv")


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e), out


def summary(xs):
    return {"ms": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def bilinear(image, uv):
    """image (H, W, 3) uint8 sampled at uv (n, 2) float64 (origin bottom-left, texel centres at integer + 0.5), taps clamped -> (n, 3) float64."""
    h, w = image.shape[:2]
    xc, yc = uv[:, 0] * w - 0.5, (1.0 - uv[:, 1]) * h - 0.5
    x0, y0 = np.floor(xc).astype(np.int64), np.floor(yc).astype(np.int64)
    fx, fy = (xc - x0)[:, None], (yc - y0)[:, None]
    cx, cy = (lambda v: np.clip(v, 0, w - 1)), (lambda v: np.clip(v, 0, h - 1))
    img = image.astype(np.float64)
    top = img[cy(y0), cx(x0)] * (1 - fx) + img[cy(y0), cx(x0 + 1)] * fx
    bot = img[cy(y0 + 1), cx(x0)] * (1 - fx) + img[cy(y0 + 1), cx(x0 + 1)] * fx
    return top * (1 - fy) + bot * fy


def barycentric(p, a, b, c):
    """Weights (n, 3) of the points p in the triangles (a, b, c), all (n, 3) float64 (p on the triangle's plane up to rounding)."""
    v0, v1, v2 = b - a, c - a, p - a
    d00, d01, d11 = (v0 * v0).sum(1), (v0 * v1).sum(1), (v1 * v1).sum(1)
    d20, d21 = (v2 * v0).sum(1), (v2 * v1).sum(1)
    den = d00 * d11 - d01 * d01
    v = (d11 * d20 - d01 * d21) / den
    w = (d00 * d21 - d01 * d20) / den
    return np.stack([1.0 - v - w, v, w], axis=1)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default="profiles/r22_mesh_texture.json")
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--views", type=int, default=5)
    p.add_argument("--dims", type=int, nargs="+", default=[256, 128, 64])
    p.add_argument("--resolution", type=int, default=512)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_texture_bench: needs the GPU (a CPU run measures nothing)")
    from gens_amd import io as gio, lib as L, ops, synthetic
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
    settings = {"unset": {}, "texture_8": {"texture": 8}, "simplify_4_texture_16": {"simplify": 4, "texture": 16},
                "simplify_4_texture_16_snap_2": {"simplify": 4, "texture": {"texels": 16, "snap": 2}}}

    def extract(name, **more):
        return surf.extract_geometry(vols, lo, hi, r, 0.0, sparse=4, views=views, **settings[name], **more)

    meshes, stats = {}, {}
    for name in settings:                                      # warm-up
        meshes[name] = extract(name)
        stats[name] = surf.last_texture_stats if name != "unset" else None
    whole = {name: [] for name in settings}
    for _ in range(args.repeats):
        for name in settings:
            whole[name].append(timed(lambda: extract(name))[0])
    # --- the launches of one call per setting: K34 beside the network launches it feeds
    launches = {}
    for name in settings:
        if name == "unset":
            continue
        L.profile_begin()
        extract(name)
        table = L.profile_end()
        k34 = sum(v["ms"] for k, v in table.items() if k in K34)
        blend = sum(v["ms"] for k, v in table.items() if k.startswith("gens_blend_views"))
        launches[name] = {"kernels": {k: {"launches": v["launches"], "ms": round(v["ms"], 4), "ms_per_launch": round(v["ms"] / v["launches"], 4)}
                                      for k, v in table.items() if k in K34 or k.startswith("gens_blend_views") or k.startswith("gens_sdf")},
                          "k34_ms": round(k34, 4), "blend_ms": round(blend, 4), "k34_over_blend": round(k34 / blend, 5) if blend else None}
    # --- sizes: the atlas, its PNG and OBJ, the vertex-coloured PLY
    sizes = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in settings:
            if name == "unset":
                continue
            simplify = settings[name].get("simplify")
            v, t, attrs = surf.extract_geometry(vols, lo, hi, r, 0.0, sparse=4, views=views, simplify=simplify, attributes=("colors",))
            ply = os.path.join(tmp, "m.ply")
            gio.write_ply(ply, v, t, colors=attrs["colors"])
            tex = meshes[name][3]
            entry = {"vertices": int(len(v)), "faces": int(len(t)), "atlas": list(tex["texture"].shape[:2]), "ply_vertex_colours_bytes": os.path.getsize(ply)}
            if simplify is not None:                               # (the full mesh's OBJ is 4.6 M lines of text: its PNG alone is measured)
                paths = gio.write_obj(os.path.join(tmp, "m"), v, t, tex["texture_uv"], tex["texture"], seen=tex["texture_seen"])
                entry["obj_bytes"], entry["png_bytes"] = os.path.getsize(paths[0]), os.path.getsize(paths[2])
            else:
                from PIL import Image
                png = os.path.join(tmp, "a.png")
                Image.fromarray(tex["texture"]).save(png)
                entry["png_bytes"] = os.path.getsize(png)
            sizes[name] = entry
    # --- image fidelity of the simplified mesh against the traced colour map of view 0
    ref = surf.render_surface(rays_o, rays_d, near, far, vols, lo, hi, c2ws, views=views, resolution=r, hw=(480, 640))
    v, t, attrs = surf.extract_geometry(vols, lo, hi, r, 0.0, sparse=4, views=views, simplify=4, attributes=("colors",))
    grid = ops.build_mesh_grid(torch.from_numpy(v).to(dev), torch.from_numpy(t).to(dev))
    face, t_mesh = ops.ray_mesh_first_hit(rays_o, rays_d, grid)
    face, t_mesh = face.cpu().numpy(), t_mesh.cpu().numpy().astype(np.float64)
    both = ref["hit"].reshape(-1) & (face >= 0)
    o, d = rays_o.cpu().numpy().astype(np.float64)[both], rays_d.cpu().numpy().astype(np.float64)[both]
    f = face[both]
    hit = o + t_mesh[both][:, None] * d
    bary = barycentric(hit, v[t[f, 0]], v[t[f, 1]], v[t[f, 2]])
    want = ref["img"].reshape(-1, 3)[both].astype(np.float64)
    fidelity = {"pixels": int(both.sum()), "hit_trace": int(ref["hit"].sum()), "hit_mesh": int((face >= 0).sum()), "faces": int(len(t))}
    by_vertex = (bary[:, :, None] * attrs["colors"][t[f]].astype(np.float64)).sum(axis=1)
    fidelity["vertex_colours_interpolated"] = round(float(np.abs(by_vertex - want).mean()), 4)
    for key, name in (("texture_16", "simplify_4_texture_16"), ("texture_16_snap_2", "simplify_4_texture_16_snap_2")):
        tex = meshes[name][3]
        assert np.array_equal(meshes[name][1], t)
        uv = (bary[:, :, None] * tex["texture_uv"][f].astype(np.float64)).sum(axis=1)
        fidelity[key] = round(float(np.abs(bilinear(tex["texture"], uv) - want).mean()), 4)
    result = {"workload": "BASELINE config[1] synthetic volumes %s, the model of bench.py, %d views of 480 x 640; extract_geometry at %d^3 with sparse=4 "
                          "(threshold 0, read-back included) with the texture unset, texture=8 on the full mesh, simplify=4 + texture=16, and the same "
                          "with snap=2" % (args.dims, args.views, r),
              "timing": "HIP events around each call, alternating in one process; one warm-up of each, then %d repeats; ms = median (min - max); the "
                        "launches of one further call per setting under lib.profile_begin (an event pair per launch)" % args.repeats,
              "device": torch.cuda.get_device_name(0), "extract_geometry": {k: summary(x) for k, x in whole.items()}, "launches": launches,
              "texture_stats": stats, "sizes": sizes,
              "fidelity": {"what": "mean absolute colour difference, 8-bit units, against render_surface's img of view 0 over the pixels whose ray hits both "
                                   "the traced surface and the simplify=4 mesh; the mesh colour is looked up on the host at the ray's first hit", **fidelity}}
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f_:
        json.dump(result, f_, indent=1)
        f_.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
