"""K38: mesh repair on the device (repair_mesh): drop invalid and duplicate faces, split every vertex into its fans (which removes every
pinch and every non-manifold edge), drop small components, re-orient every orientable component by majority and close small boundary loops.
The rules are the comment of K38 in include/gens_hip.h; tests/mesh_repair_reference.py restates them in numpy with
dicts and loops.

Part of gens_amd.ops (see ops/__init__.py)."""
from .base import *  # noqa: F401,F403
from .lookup import compact_valid
from .mesh_topology import EDGE_BOUNDARY, VERTEX_BOUNDARY, _check_mesh, _union_labels, mesh_topology

_f64, _i32, _i64, _u8 = torch.float64, torch.int32, torch.int64, torch.uint8
_KEY_SENTINEL = 2 ** 63 - 1            # both keys of a face that is not valid
REPAIR_KEYS = ("split", "orient", "min_component_faces", "max_hole_edges", "dedupe")
REPAIR_STAT_KEYS = ("faces_invalid", "faces_duplicate", "faces_small_component", "vertices_split", "components_flipped",
                    "components_nonorientable", "loops_filled", "loops_open", "fill_faces", "fill_vertices", "split_rounds")

repair_section_hook = None             # a callable(name), called where a stage of repair_mesh begins (scripts/mesh_repair_bench.py records HIP events there)


def _repair_section(name):
    if repair_section_hook is not None:
        repair_section_hook(name)


def repair_request(who, split=True, orient=True, min_component_faces=0, max_hole_edges=0, dedupe=True, **unknown):
    """The options of repair_mesh, checked -> dict.  ValueError for an unknown keyword, a switch that is no bool, a count that is no whole
    number in [0, 2^31), or a fill without the split and the orientation (its loops are those of the oriented manifold mesh)."""
    if unknown:
        raise ValueError(f"{who}: unknown keyword {sorted(unknown)[0]!r} (repair takes {', '.join(REPAIR_KEYS)})")
    for name, x in (("split", split), ("orient", orient), ("dedupe", dedupe)):
        if not isinstance(x, bool):
            raise ValueError(f"{who}: {name} = {x!r}: True or False")
    for name, x in (("min_component_faces", min_component_faces), ("max_hole_edges", max_hole_edges)):
        if isinstance(x, bool) or not isinstance(x, int) or not 0 <= x < 2 ** 31:
            raise ValueError(f"{who}: {name} = {x!r}: a whole number from 0 (off) to below 2^31")
    if max_hole_edges and not (split and orient):
        raise ValueError(f"{who}: max_hole_edges = {max_hole_edges} needs split and orient: the loops are those of the oriented manifold mesh")
    return {"split": split, "orient": orient, "min_component_faces": min_component_faces, "max_hole_edges": max_hole_edges, "dedupe": dedupe}


def _where(flags, count):
    """The indices of the `count` set entries of flags (n) bool in ascending order -> (count) int64 (ops.compact_valid; `count` is known
    to the caller, which leaves the rescue of an all-clear input out)."""
    if count == 0:
        return torch.zeros(0, device=flags.device, dtype=_i64)
    return compact_valid(flags)[0][:count]


def _counts_of(sorted_keys, keys):
    """How often each of `keys` occurs in `sorted_keys`: by search, not by a histogram (see MeshTopology.report)."""
    return torch.searchsorted(sorted_keys, keys, right=True) - torch.searchsorted(sorted_keys, keys)


def repair_mesh(vertices, triangles, split=True, orient=True, min_component_faces=0, max_hole_edges=0, dedupe=True):
    """K38.  vertices (V, 3) float64, triangles (T, 3) int32 on the device, any indices -> (vertices' (V', 3) float64, triangles' (T', 3)
    int32, vertex_source (V') int32, face_source (T') int32, face_flipped (T') bool, stats).  The stages, in this order:
      dedupe: faces that are not valid are dropped (always); with dedupe=True so are faces with the vertex set of an earlier face;
      split: every vertex becomes one vertex per fan at the same position, which removes every pinch and every non-manifold edge in one
        round; unreferenced vertices are dropped (False: vertices and indices stay as they are);
      min_component_faces = m > 0: components (K37's face_component) of fewer than m faces are dropped with their vertices;
      orient: in every orientable component the side with fewer faces is re-wound to (a, c, b) (a tie: the side without the component's
        smallest face); non-orientable components are left alone and counted;
      max_hole_edges = n > 0 (needs split and orient): every boundary loop of 3 to n edges outside non-orientable components is closed (but for
        the rim of a lone triangle, whose closing face would be its duplicate), a loop of 3 by one face, a longer one by a fan about a new vertex at the loop's centroid.  Longer loops stay open.  A centroid fan
        over a strongly non-planar loop can intersect itself or the mesh: that is not detected.
    Kept vertices are bit-identical to vertices[vertex_source]; a centroid has source -1, a fill face source -1.  stats: faces_invalid,
    faces_duplicate, faces_small_component, vertices_split (added by the split), components_flipped (with a re-wound face),
    components_nonorientable, loops_filled, loops_open (counted where the fill runs), fill_faces, fill_vertices, split_rounds.
    Deterministic.  K37's topology up to three times, K38's kernels, K23's union-find; sorts and prefix sums in torch.  ValueError before
    any launch for what ops.mesh_topology refuses or what repair_request refuses."""
    who = "repair_mesh"
    _check_mesh(who, vertices, triangles)
    opt = repair_request(who, split, orient, min_component_faces, max_hole_edges, dedupe)
    v, t = _c(vertices.detach()), _c(triangles.detach())
    dev, nv, nt = v.device, v.shape[0], t.shape[0]
    stats = dict.fromkeys(REPAIR_STAT_KEYS, 0)
    # ------------------------------------------------------------------------------------------------ a. dedupe
    _repair_section("dedupe")
    major, minor = torch.empty(nt, device=dev, dtype=_i64), torch.empty(nt, device=dev, dtype=_i64)
    if nt:
        L.call("gens_mesh_face_keys", L.ptr(t, _i32), nt, nv, L.ptr(major, _i64), L.ptr(minor, _i64), L.stream(), nbytes=nt * 28)
    valid = major != _KEY_SENTINEL
    keep = valid
    if opt["dedupe"] and nt:
        minor_s, first_order = torch.sort(minor, stable=True)
        major_s, second_order = torch.sort(major[first_order], stable=True)
        order, minor_s = first_order[second_order], minor_s[second_order]      # equal triples adjacent, in ascending face id
        first = torch.ones(nt, device=dev, dtype=torch.bool)
        first[1:] = (major_s[1:] != major_s[:-1]) | (minor_s[1:] != minor_s[:-1])
        keep = torch.zeros(nt, device=dev, dtype=torch.bool)
        keep[order] = first & (major_s != _KEY_SENTINEL)
    n_valid, n_keep = (int(x) for x in torch.stack([valid.sum(), keep.sum()]).tolist()) if nt else (0, 0)
    stats["faces_invalid"], stats["faces_duplicate"] = nt - n_valid, n_valid - n_keep
    face_source = _where(keep, n_keep).to(_i32)
    tri = _c(t[face_source.long()])
    n_faces = n_keep
    vertex_source = torch.arange(nv, device=dev, dtype=_i32)
    topo = None                                     # K37's topology of (v[vertex_source], tri) while that mesh stands
    # ------------------------------------------------------------------------------------------------ b. split
    if opt["split"]:
        _repair_section("split")
        stats["split_rounds"] = 1
        first_topo = mesh_topology(v, tri)
        fans = first_topo.fans
        base = _c((torch.cumsum(fans, 0) - fans).to(_i32))
        n_new, n_referenced = (int(x) for x in torch.stack([fans.sum(), (fans > 0).sum()]).tolist()) if nv else (0, 0)
        stats["vertices_split"] = n_new - n_referenced
        new_corner = torch.empty(3 * n_faces, device=dev, dtype=_i32)
        vertex_source = torch.empty(n_new, device=dev, dtype=_i32)
        if n_faces:
            L.call("gens_mesh_split_corners", L.ptr(first_topo.corner_order, _i32), L.ptr(first_topo.corner_start, _i32),
                   L.ptr(first_topo.corner_label, _i32), L.ptr(base, _i32), nv, 3 * n_faces, n_new, L.ptr(new_corner, _i32),
                   L.ptr(vertex_source, _i32), L.stream(), nbytes=nv * 8 + n_faces * 36 + n_new * 4)
        tri = new_corner.view(n_faces, 3)
        del first_topo
    position = lambda: _c(v[vertex_source.long()])  # noqa: E731
    # ------------------------------------------------------------------------------------------------ c. small components
    if opt["min_component_faces"] > 0 and n_faces:
        _repair_section("components")
        topo = mesh_topology(position(), tri)
        label = torch.sort(topo.face_component)[0]
        big = _counts_of(label, topo.face_component) >= opt["min_component_faces"]
        n_big = int(big.sum())
        stats["faces_small_component"] = n_faces - n_big
        if n_big < n_faces:
            idx = _where(big, n_big)
            tri, face_source, n_faces = tri[idx], _c(face_source[idx]), n_big
            used = torch.zeros(vertex_source.shape[0], device=dev, dtype=torch.bool)
            used[tri.reshape(-1).long()] = True
            rank = (torch.cumsum(used, 0) - 1).to(_i32)
            tri = _c(rank[tri.long()])
            vertex_source = _c(vertex_source[_where(used, int(used.sum()))])
            topo = None
    n_vertices = vertex_source.shape[0]
    flipped = torch.zeros(n_faces, device=dev, dtype=torch.bool)
    twisted = torch.zeros(n_faces, device=dev, dtype=torch.bool)          # faces of non-orientable components
    # ------------------------------------------------------------------------------------------------ d. orient
    if opt["orient"] and n_faces:
        _repair_section("orient")
        topo = mesh_topology(position(), tri) if topo is None else topo
        ne = topo.n_edges
        pairs = torch.empty(2 * ne, 2, device=dev, dtype=_i32)
        if ne:
            L.call("gens_mesh_orient_pairs", L.ptr(topo.edge_halfedges, _i32), L.ptr(topo.edge_class, _u8), ne, n_faces, L.ptr(pairs, _i32),
                   L.stream(), nbytes=ne * 25)
        label = _union_labels(pairs, 2 * n_faces).view(n_faces, 2).long()
        l0, l1 = label[:, 0], label[:, 1]
        twisted = l0 == l1
        side = torch.div(torch.minimum(l0, l1), 2, rounding_mode="floor") * 2            # 2 x the component's smallest face: its side's key
        far = l0 > l1                                                                  # on the other side than that face
        keys = torch.sort(torch.where(twisted, torch.full_like(side, 2 * n_faces), side + far.long()))[0]
        near_faces, far_faces = _counts_of(keys, side), _counts_of(keys, side + 1)
        flipped = ~twisted & torch.where(far, near_faces >= far_faces, far_faces > near_faces)
        me = torch.arange(n_faces, device=dev, dtype=_i64)
        flipped_side = torch.sort(torch.where(flipped, side, torch.full_like(side, 2 * n_faces)))[0]
        has_flip = _counts_of(flipped_side, side) > 0
        figures = torch.stack([flipped.sum(), (has_flip & (side == 2 * me) & ~twisted).sum(), (twisted & (l0 == 2 * me)).sum()]).tolist()
        n_flipped, stats["components_flipped"], stats["components_nonorientable"] = (int(x) for x in figures)
        if n_flipped:
            out = torch.empty(n_faces, 3, device=dev, dtype=_i32)
            L.call("gens_mesh_apply_flips", L.ptr(_c(tri), _i32), L.ptr(flipped.view(_u8), _u8), n_faces, L.ptr(out, _i32), L.stream(),
                   nbytes=n_faces * 25)
            tri, topo = out, None
    tri = _c(tri)
    out_vertices = position()
    # ------------------------------------------------------------------------------------------------ e. fill
    if opt["max_hole_edges"] > 0 and n_faces:
        _repair_section("fill")
        topo = mesh_topology(out_vertices, tri) if topo is None else topo
        rim_edge = topo.edge_class == EDGE_BOUNDARY
        on_rim = (topo.vertex_flags & VERTEX_BOUNDARY) != 0
        n_rim, n_rim_edges = (int(x) for x in torch.stack([on_rim.sum(), rim_edge.sum()]).tolist())
        if n_rim != n_rim_edges:
            raise RuntimeError(f"{who}: {n_rim_edges} boundary edges over {n_rim} boundary vertices: the split mesh is not manifold")
        if n_rim:
            rim = _c(torch.where(rim_edge[:, None], topo.edges, torch.full_like(topo.edges, -1)))
            name = torch.where(on_rim, _union_labels(rim, n_vertices), torch.full((n_vertices,), n_vertices, device=dev, dtype=_i32))
            name_s, by_loop = torch.sort(name, stable=True)                             # the boundary vertices by loop name, then id
            loop_vertices = _c(by_loop[:n_rim].to(_i32))
            _, length = torch.unique_consecutive(name_s[:n_rim], return_counts=True)
            n_loops = length.shape[0]
            loop_start = torch.zeros(n_loops + 1, device=dev, dtype=_i32)
            loop_start[1:] = torch.cumsum(length, 0).to(_i32)
            loop_of_vertex = torch.full((n_vertices,), -1, device=dev, dtype=_i32)
            loop_of_vertex[loop_vertices.long()] = torch.repeat_interleave(torch.arange(n_loops, device=dev, dtype=_i32), length)
            rim_half = _c(torch.sort(topo.edge_halfedges[rim_edge, 0])[0])
            half_loop = loop_of_vertex[tri.reshape(-1)[rim_half.long()].long()].long()
            barred = torch.zeros(n_loops, device=dev, dtype=torch.bool)
            half_face = torch.div(rim_half, 3, rounding_mode="floor").long()
            barred[half_loop[twisted[half_face]]] = True
            first_face, last_face = torch.full((n_loops,), n_faces, device=dev, dtype=_i64), torch.full((n_loops,), -1, device=dev, dtype=_i64)
            first_face.scatter_reduce_(0, half_loop, half_face, "amin")
            last_face.scatter_reduce_(0, half_loop, half_face, "amax")
            barred |= first_face == last_face                                          # a lone triangle: its closing face would be its duplicate
            chosen = (length >= 3) & (length <= opt["max_hole_edges"]) & ~barred
            fan, three = chosen & (length > 3), chosen & (length == 3)
            loop_slot = _c(torch.where(fan, torch.cumsum(fan, 0) - 1, torch.full_like(length, -1)).to(_i32))
            loop_apex = _c(torch.where(fan, loop_slot + n_vertices, torch.full_like(loop_slot, -1)))
            first_half = torch.full((n_loops,), 3 * n_faces, device=dev, dtype=_i64)
            first_half.scatter_reduce_(0, half_loop, rim_half.long(), "amin")
            emit = fan[half_loop] | (three[half_loop] & (rim_half.long() == first_half[half_loop]))
            rim_slot = _c(torch.where(emit, torch.cumsum(emit, 0) - 1, torch.full_like(half_loop, -1)).to(_i32))
            n_chosen, n_centroids, n_fill = (int(x) for x in torch.stack([chosen.sum(), fan.sum(), emit.sum()]).tolist())
            if n_vertices + n_centroids >= 2 ** 31 or 3 * (n_faces + n_fill) >= 2 ** 31:
                raise RuntimeError(f"{who}: the fill would make {n_vertices + n_centroids} vertices and {n_faces + n_fill} faces (V and 3 T below 2^31)")
            stats.update(loops_filled=n_chosen, loops_open=n_loops - n_chosen, fill_faces=n_fill, fill_vertices=n_centroids)
            if n_centroids:
                centroids = torch.empty(n_centroids, 3, device=dev, dtype=_f64)
                L.call("gens_mesh_loop_centroids", L.ptr(out_vertices, _f64), n_vertices, L.ptr(loop_start, _i32), L.ptr(loop_vertices, _i32),
                       n_loops, n_rim, L.ptr(loop_slot, _i32), n_centroids, L.ptr(centroids, _f64), L.stream(), nbytes=n_rim * 28 + n_centroids * 24)
                out_vertices = torch.cat([out_vertices, centroids])
                vertex_source = torch.cat([vertex_source, torch.full((n_centroids,), -1, device=dev, dtype=_i32)])
            if n_fill:
                faces = torch.empty(n_fill, 3, device=dev, dtype=_i32)
                L.call("gens_mesh_fill_emit", L.ptr(tri, _i32), n_faces, n_vertices, L.ptr(rim_half, _i32), L.ptr(rim_slot, _i32), n_rim,
                       L.ptr(loop_of_vertex, _i32), L.ptr(loop_start, _i32), L.ptr(loop_vertices, _i32), L.ptr(loop_apex, _i32), n_loops, n_fill,
                       L.ptr(faces, _i32), L.stream(), nbytes=n_rim * 24 + n_fill * 12)
                tri = torch.cat([tri, faces])
                face_source = torch.cat([face_source, torch.full((n_fill,), -1, device=dev, dtype=_i32)])
                flipped = torch.cat([flipped, torch.zeros(n_fill, device=dev, dtype=torch.bool)])
    _repair_section("end")
    return out_vertices, tri, _c(vertex_source), _c(face_source), flipped, stats


__all__ = [n_ for n_ in dir() if not n_.startswith("__")]
