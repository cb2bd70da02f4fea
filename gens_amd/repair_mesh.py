"""python -m gens_amd.repair_mesh IN.{ply,obj} OUT.ply [--fill N] [--min-component M] [--no-orient] [--no-split] [--device D]

Repairs a triangle mesh on the device (K38; io.repair_mesh, ops.repair_mesh): invalid and duplicate faces are dropped, every pinched vertex
and non-manifold edge is split, components of fewer than M faces are dropped, every orientable component is re-oriented by majority and
boundary loops of up to N edges are closed.  A PLY's normals and colours are carried.  Prints three JSON lines: the topology report (K37)
before, the report after, and the repair's counts."""
import argparse
import json
import sys

from . import io as gio, ops


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m gens_amd.repair_mesh", description=__doc__.split("\n\n")[1])
    ap.add_argument("mesh", metavar="IN.{ply,obj}")
    ap.add_argument("out", metavar="OUT.ply")
    ap.add_argument("--fill", type=int, default=0, metavar="N", help="close boundary loops of up to N edges (0: none)")
    ap.add_argument("--min-component", type=int, default=0, metavar="M", help="drop components of fewer than M faces (0: none)")
    ap.add_argument("--no-orient", action="store_true")
    ap.add_argument("--no-split", action="store_true")
    ap.add_argument("--device", default=None)
    args = ap.parse_args(argv)
    kw = {"split": not args.no_split, "orient": not args.no_orient, "min_component_faces": args.min_component, "max_hole_edges": args.fill}
    try:
        ops.repair_request("repair_mesh", **kw)          # (a bad option: before the files and the device are looked at)
        attrs = {}
        if args.mesh.lower().endswith(".obj"):
            mesh = gio.read_obj(args.mesh)
            vertices, triangles = mesh["vertices"], mesh["triangles"]
        else:
            vertices, triangles, attrs = gio.read_ply(args.mesh, attributes=True)
        before = gio.mesh_report(vertices, triangles, device=args.device)
        out_v, out_t, out = gio.repair_mesh(vertices, triangles, normals=attrs.get("normals"), colors=attrs.get("colors"), device=args.device,
                                            **kw)
        after = gio.mesh_report(out_v, out_t, device=args.device)
        gio.write_ply(args.out, out_v, out_t, normals=out.get("normals"), colors=out.get("colors"))
    except (ValueError, OSError, RuntimeError) as e:     # a file that cannot be read or written; a mesh that is no (n, 3) arrays; a bad option
        print(f"gens_amd.repair_mesh: {e}", file=sys.stderr)
        return 2
    print(json.dumps(before))
    print(json.dumps(after))
    print(json.dumps(out["stats"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
