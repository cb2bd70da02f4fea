"""python -m gens_amd.mesh_report MESH.{ply,obj} [--roughness] [--self-intersections [--max-pairs N]] [--device D]

The topology report of a triangle mesh on the device (K37; io.mesh_report, ops.mesh_topology), printed as one JSON line: vertices, faces and
edges by class (boundary, manifold, flipped, non-manifold), pinched vertices, components, boundary loops, the Euler characteristic, whether
the mesh is closed, oriented, manifold and watertight, its genus if it is, its area and its signed volume.

--roughness adds the key "roughness": the number, mean, RMS and maximum of the dihedral angles between the normals of the faces either
side of every manifold edge (K39; ops.mesh_roughness).

--self-intersections adds the key "self_intersections": the candidate pairs of faces and how many of them intersect or are undecided, the
degenerate and uncertain faces, the duplicate pairs (K41; ops.mesh_self_intersections); with --max-pairs N the
first N pairs and their kinds (1 intersecting, 2 undecided) go under "pairs"."""
import argparse
import json
import sys

from . import io as gio
from .compare_meshes import read_mesh


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m gens_amd.mesh_report", description=__doc__.split("\n\n")[1])
    ap.add_argument("mesh", metavar="MESH.{ply,obj}")
    ap.add_argument("--roughness", action="store_true", help="add the dihedral roughness report (K39)")
    ap.add_argument("--self-intersections", action="store_true", help="add the self-intersection counts (K41)")
    ap.add_argument("--max-pairs", type=int, default=None, metavar="N", help="with --self-intersections: list the first N pairs")
    ap.add_argument("--device", default=None)
    args = ap.parse_args(argv)
    more = {"roughness": True} if args.roughness else {}
    if args.self_intersections or args.max_pairs is not None:
        more.update(self_intersections=args.self_intersections, max_pairs=args.max_pairs)
    try:
        vertices, triangles = read_mesh(args.mesh)
        out = gio.mesh_report(vertices, triangles, device=args.device, **more)
    except (ValueError, OSError, RuntimeError) as e:     # a file that cannot be read; a mesh that is no (n, 3) arrays
        print(f"gens_amd.mesh_report: {e}", file=sys.stderr)
        return 2
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
