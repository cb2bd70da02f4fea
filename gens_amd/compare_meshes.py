"""python -m gens_amd.compare_meshes A.{ply,obj} B.{ply,obj} [--density D | --samples N] [--max-dist M] [--signed [--sign {pseudonormal,winding}] [--beta B]] [--json OUT] [--device D]

The two-sided distance between two triangle meshes on the device (K36; io.compare_meshes, ops.mesh_distance): each mesh is sampled -- its
vertices, then lattice points at spacing D on its triangles (default: about N = 1 000 000 per mesh) -- and every sample is given its exact
distance to the other mesh.  Prints one line per direction (mean, RMS, maximum and quantiles, in the meshes' units) and the two summaries:
the Hausdorff distance (the larger maximum) and the Chamfer distance (the mean of the two means).  Unsigned unless --signed, which adds per
direction the mean signed distance (positive on the side the other mesh's face normals point to), the samples inside and those without a sign
(K37) -- or, with --sign winding, the sign from the other mesh's generalised winding number (K40; DESIGN.md,
section 5q: for open, pinched or folded meshes and soups, whose edges give K37 no sign; --beta B > 1 sets the far field's opening, default
ops.MESH_DISTANCE_BETA; an inside-out mesh has nothing inside it: python -m gens_amd.repair_mesh re-orients); samples with nothing within M are counted as unmatched and left out of the figures."""
import argparse
import json
import sys

from . import io as gio


def read_mesh(path):
    """A .obj through io.read_obj, anything else through io.read_ply -> (vertices, triangles)."""
    if path.lower().endswith(".obj"):
        mesh = gio.read_obj(path)
        return mesh["vertices"], mesh["triangles"]
    return gio.read_ply(path)


def compare_files(a, b, device=None, **kw):
    """read_mesh twice -> io.compare_meshes; -> its dict, with the meshes' sizes."""
    va, ta = read_mesh(a)
    vb, tb = read_mesh(b)
    out = gio.compare_meshes(va, ta, vb, tb, device=device, **kw)
    return {**out, "vertices_a": len(va), "triangles_a": len(ta), "vertices_b": len(vb), "triangles_b": len(tb)}


def format_direction(name, d):
    line = (f"{name}: n {d['n']}  mean {d['mean']:.6g}  rms {d['rms']:.6g}  max {d['max']:.6g}  q50 {d['q50']:.6g}  q90 {d['q90']:.6g}  "
            f"q99 {d['q99']:.6g}  unmatched {d['unmatched']}")
    if "signed_mean" in d:
        line += f"  signed_mean {d['signed_mean']:.6g}  inside {d['inside']}  no_sign {d['no_sign']}"
    return line


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m gens_amd.compare_meshes", description=__doc__.split("\n\n")[1])
    ap.add_argument("a", metavar="A.{ply,obj}")
    ap.add_argument("b", metavar="B.{ply,obj}")
    how = ap.add_mutually_exclusive_group()
    how.add_argument("--density", type=float, default=None, help="sample spacing on both meshes, in the meshes' units")
    how.add_argument("--samples", type=int, default=None, help="lattice samples per mesh, about (default 1000000): spacing sqrt(area / N)")
    ap.add_argument("--max-dist", type=float, default=None, help="samples with nothing within this distance are counted, not averaged")
    ap.add_argument("--signed", action="store_true", help="also the signed mean, the samples inside and those without a sign, per direction")
    ap.add_argument("--sign", choices=("pseudonormal", "winding"), default=None,
                    help="with --signed: the sign from K37's pseudonormals (default) or from K40's generalised winding number")
    ap.add_argument("--beta", type=float, default=None, help="with --sign winding: clusters farther than B radii count as dipoles (B > 1)")
    ap.add_argument("--json", default=None, metavar="OUT", help="also write the figures to this file")
    ap.add_argument("--device", default=None)
    args = ap.parse_args(argv)
    if args.sign is not None and not args.signed:
        ap.error("--sign needs --signed")
    if args.beta is not None and args.sign != "winding":
        ap.error("--beta needs --sign winding")
    kw = {k: v for k, v in (("density", args.density), ("samples", args.samples), ("max_dist", args.max_dist)) if v is not None}
    if args.signed:
        kw["signed"] = True
    if args.sign is not None:
        kw["sign"] = args.sign
    if args.beta is not None:
        kw["beta"] = args.beta
    try:
        out = compare_files(args.a, args.b, device=args.device, **kw)
    except (ValueError, OSError, RuntimeError) as e:      # bad keywords or meshes; a file that cannot be read; a density too fine for the sampler
        print(f"gens_amd.compare_meshes: {e}", file=sys.stderr)
        return 2
    print(format_direction("a_to_b", out["a_to_b"]))
    print(format_direction("b_to_a", out["b_to_a"]))
    print(f"hausdorff {out['hausdorff']:.6g}  chamfer {out['chamfer']:.6g}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f)
    return 0


if __name__ == "__main__":
    sys.exit(main())
