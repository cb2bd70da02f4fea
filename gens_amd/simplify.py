"""python -m gens_amd.simplify IN.ply OUT.ply --cell C [--reg R] [--origin X Y Z] [--device D]

Simplify a triangle mesh on the device by vertex clustering with quadric-optimal representatives (K33; io.simplify_mesh,
ops.simplify_mesh): one vertex per cell of edge C that the surface passes through, placed where the planes of the cell's triangles meet.
Per-vertex normals and colours of the input (nx ny nz, red green blue) are carried over from the input vertex nearest to each new vertex,
never averaged.  Topology is not preserved and no distance to the input surface is promised."""
import argparse
import json
import os
import sys

from . import io as gio


def simplify_file(src, dst, cell, reg=1e-3, origin=None, device=None):
    """read_ply(attributes=True) -> io.simplify_mesh -> write_ply; -> the stats dict, with the two files' sizes in bytes."""
    vertices, triangles, attrs = gio.read_ply(src, attributes=True)
    out_v, out_t, out = gio.simplify_mesh(vertices, triangles, cell, origin=origin, normals=attrs.get("normals"), colors=attrs.get("colors"),
                                         device=device, reg=reg)
    gio.write_ply(dst, out_v, out_t, normals=out.get("normals"), colors=out.get("colors"))
    return {**out["stats"], "input_bytes": os.path.getsize(src), "output_bytes": os.path.getsize(dst)}


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m gens_amd.simplify", description=__doc__.split("\n\n")[1])
    ap.add_argument("src", metavar="IN.ply")
    ap.add_argument("dst", metavar="OUT.ply")
    ap.add_argument("--cell", type=float, required=True, help="edge of the clustering cells, in the mesh's units")
    ap.add_argument("--reg", type=float, default=1e-3, help="pull towards the cluster mean along unconstrained directions (default 1e-3)")
    ap.add_argument("--origin", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"),
                    help="a corner of the cell grid at or below the mesh (default: aligned to multiples of the cell)")
    ap.add_argument("--device", default=None)
    args = ap.parse_args(argv)
    try:
        stats = simplify_file(args.src, args.dst, args.cell, reg=args.reg, origin=args.origin, device=args.device)
    except ValueError as e:
        print(f"gens_amd.simplify: {e}", file=sys.stderr)
        return 2
    print(json.dumps(stats))
    return 0


if __name__ == "__main__":
    sys.exit(main())
