"""K23 on the MI355X: first hits against a float64 brute force, watertightness, the fused view-ray flags, face components, and the whole
of utils/clean_mesh.py's clean_mesh against the float64 restatement in tests/mesh_clean_reference.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_clean_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _g14():
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "g14_clean_mesh.npz"))
    return g["vertices"], g["faces"], torch.from_numpy(g["masks"]), torch.from_numpy(g["intrs"]), torch.from_numpy(g["c2ws"])


def _mc(sdf, n, lo=-1.0, hi=1.0):
    """marching_cubes of an analytic SDF on an n^3 lattice over [lo, hi]^3 -> world vertices (V,3) float64, triangles (F,3) int64 (numpy)."""
    from gens_amd import ops
    lin = torch.linspace(lo, hi, n, dtype=torch.float64)
    x, y, z = torch.meshgrid(lin, lin, lin, indexing="ij")
    v, t = ops.marching_cubes(sdf(x, y, z).float().to(DEV), 0.0)
    return (lo + v.cpu().numpy() * (hi - lo) / (n - 1)), t.cpu().numpy().astype(np.int64)


def _sphere(c, r):
    return lambda x, y, z: torch.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r


def _blobs():
    """Two overlapping blobs and a thin floater (< 500 faces) in front of the cameras of synthetic.make_cameras."""
    a, b, c = _sphere((-0.3, 0.0, 0.0), 0.45), _sphere((0.35, 0.1, 0.05), 0.35), _sphere((0.05, 0.62, -0.2), 0.07)
    return _mc(lambda x, y, z: torch.minimum(torch.minimum(a(x, y, z), b(x, y, z)), c(x, y, z)), 48)


def _first_hit_check(v, t, ro, rd, max_ambiguous=0.01):
    from gens_amd import ops
    grid = ops.build_mesh_grid(torch.from_numpy(v).to(DEV), torch.from_numpy(t).to(DEV))
    f1, t1 = ops.ray_mesh_first_hit(ro.to(DEV), rd.to(DEV), grid)
    f2, t2 = ops.ray_mesh_first_hit(ro.to(DEV), rd.to(DEV), grid)
    assert torch.equal(f1, f2) and torch.equal(t1.view(torch.int32), t2.view(torch.int32))           # bit-identical
    face, tt, amb = R.first_hits(v, t, ro, rd, device=DEV)
    f1, t1 = f1.cpu().long(), t1.cpu().double()
    ok = ~amb
    assert amb.float().mean() < max_ambiguous
    assert torch.equal(f1[ok], face[ok]), int((f1[ok] != face[ok]).sum())
    hit = ok & (face >= 0)
    assert hit.sum() > 0.2 * len(face)
    assert ((t1[hit] - tt[hit]).abs() <= 1e-5 * tt[hit]).all()
    assert torch.isinf(t1[ok & (face < 0)]).all()
    return f1, face, amb


def test_first_hit_matches_float64_brute_force_on_the_g14_scene():
    v, t, masks, intrs, c2ws = _g14()
    rays = [R.view_rays(intrs[i], c2ws[i], masks[i], 2) for i in range(5)]
    _first_hit_check(v, t, torch.cat([r[0] for r in rays]), torch.cat([r[1] for r in rays]))


def test_first_hit_matches_float64_brute_force_on_a_triangle_soup():
    rng = np.random.default_rng(23)
    n = 600
    centres = rng.uniform(-1, 1, (n, 1, 3))
    v = (centres + rng.normal(0, 0.08, (n, 3, 3)))
    v[:20] = centres[:20] + rng.normal(0, 0.9, (20, 3, 3))               # triangles across many cells
    v[20:40, 1] = v[20:40, 0]                                           # zero-area faces
    v[40:60] = v[60:80]                                                 # coincident duplicates: the smaller index wins
    v = v.reshape(-1, 3)
    t = np.arange(3 * n).reshape(n, 3)
    perm = rng.permutation(n)
    t = t[perm]
    o = rng.normal(0, 1, (20000, 3))
    o = 3.0 * o / np.linalg.norm(o, axis=1, keepdims=True)
    d = rng.uniform(-0.8, 0.8, (20000, 3)) - o
    aim = t[np.concatenate([rng.integers(0, n, 4000), np.nonzero((perm >= 40) & (perm < 80))[0].repeat(50)])]
    d[:6000] = (v[aim[:, 0]] + v[aim[:, 1]] + v[aim[:, 2]]) / 3.0 - o[:6000]          # aimed at face centroids, the duplicates' too
    ro, rd = torch.from_numpy(o).float(), torch.from_numpy(d).float()
    f1, _, _ = _first_hit_check(v, t, ro, rd, max_ambiguous=0.2)          # (a ray that hits an exact duplicate first is a tie: ambiguous)
    # the tie rule: with the larger-index copy of every duplicate removed, a ray the float64 brute force calls unambiguous and that hits
    # the smaller copy first must get that smaller index on the full mesh (both copies give bit-equal t)
    inv = np.argsort(perm)
    pairs = np.stack([inv[np.arange(40, 60)], inv[np.arange(60, 80)]], 1)
    low, high = pairs.min(1), pairs.max(1)
    keep = np.setdiff1d(np.arange(n), high)
    face, _, amb = R.first_hits(v, t[keep], ro, rd, device=DEV)
    full = torch.where(face >= 0, torch.from_numpy(keep)[face.clamp(min=0)], face)
    tie = ~amb & torch.from_numpy(np.isin(full.numpy(), low))
    assert tie.sum() > 200
    assert torch.equal(f1[tie], full[tie])


def test_first_hit_matches_float64_brute_force_on_a_marching_cubes_sphere():
    v, t = _mc(_sphere((0.05, -0.02, 0.03), 0.6), 40)
    rng = np.random.default_rng(5)
    o = rng.normal(0, 1, (20000, 3))
    o = 2.5 * o / np.linalg.norm(o, axis=1, keepdims=True)
    d = rng.uniform(-0.7, 0.7, (20000, 3)) - o
    o[:3000] = rng.uniform(-0.2, 0.2, (3000, 3))                        # from inside: the back faces count too
    _first_hit_check(v, t, torch.from_numpy(o).float(), torch.from_numpy(d).float())


def test_rays_through_every_vertex_and_edge_midpoint_never_leak():
    """Rays from outside a closed marching-cubes sphere that pass EXACTLY through every vertex and every edge midpoint (o + 1 * d = target
    in exact arithmetic, checked) all stop there: the watertight test counts a zero edge function as inside and the two faces of an edge
    compute it as exact negatives.  A test with strict inequalities lets the rays whose sheared target lands exactly on an edge or
    vertex through, to the far side of the sphere."""
    from gens_amd import ops
    c = np.array([19.5, 19.25, 19.75])
    v, t = _mc(lambda x, y, z: torch.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - 12.0, 40, lo=0.0, hi=39.0)   # lattice units
    v = np.round(v * 256.0) / 256.0             # multiples of 2^-8 below 64: vertices and edge midpoints are exact in float32
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    targets = np.concatenate([v, 0.5 * (v[e[:, 0]] + v[e[:, 1]])])
    assert (targets.astype(np.float32).astype(np.float64) == targets).all() and targets.min() > 7.0
    rng = np.random.default_rng(8)
    out = (targets - c) / np.linalg.norm(targets - c, axis=1, keepdims=True) + rng.uniform(-0.4, 0.4, targets.shape)
    o = (targets + 3.0 * out / np.linalg.norm(out, axis=1, keepdims=True)).astype(np.float32)
    # every origin component lies within a factor of two of the target's (targets > 7, offsets <= 3): target - o is exact (Sterbenz)
    d = (targets.astype(np.float32) - o).astype(np.float32)
    assert (o.astype(np.float64) + d.astype(np.float64) == targets).all()
    grid = ops.build_mesh_grid(torch.from_numpy(v).to(DEV), torch.from_numpy(t).to(DEV))
    face, tt = ops.ray_mesh_first_hit(torch.from_numpy(o).to(DEV), torch.from_numpy(d).to(DEV), grid)
    assert len(face) > 5000
    assert int((face < 0).sum()) == 0, f"{int((face[:len(v)] < 0).sum())} vertex rays and {int((face[len(v):] < 0).sum())} midpoint rays leaked"
    # none passes through its target (a leak on a closed surface shows up as a hit on the far side): the first hit is the target
    # itself or a face in front of it
    through = (tt > 1.0 + 1e-6).cpu()
    assert int(through.sum()) == 0, f"{int(through[:len(v)].sum())} vertex rays and {int(through[len(v):].sum())} midpoint rays passed through"


def _view_flags_check(v, t, masks, intrs, c2ws, upscale):
    from gens_amd import ops
    grid = ops.build_mesh_grid(torch.from_numpy(v).to(DEV), torch.from_numpy(t).to(DEV))
    flags, any_miss = ops.visible_faces(grid, masks, intrs, c2ws, upscale)
    want = np.zeros(len(t), dtype=np.uint8)
    miss = False
    n_amb = 0
    for i in range(masks.shape[0]):
        ro, rd, act = R.view_rays(intrs[i], c2ws[i], masks[i], upscale)
        face, _, amb = R.first_hits(v, t, ro[act], rd[act], device=DEV)
        if amb.any():                           # a ray whose answer depends on the last bit: the general kernel's answer for the same ray
            face = face.clone()
            face[amb] = ops.ray_mesh_first_hit(ro[act][amb].to(DEV), rd[act][amb].to(DEV), grid)[0].cpu().long()
            n_amb += int(amb.sum())
        want[face[face >= 0].numpy()] = 1
        miss = miss or bool((face < 0).any())
    assert n_amb < 50
    assert np.array_equal(flags.cpu().numpy(), want) and bool(any_miss.item()) == miss
    assert want.sum() > 20
    return want, miss


def test_view_ray_flags_are_the_union_of_first_hits_on_g14():
    v, t, masks, intrs, c2ws = _g14()
    for up in (2, 4):
        _view_flags_check(v, t, masks, intrs, c2ws, up)
    # colour masks, averaged: a pixel casts for any value > 0 of the raw average (0.2 here), not for > 0.5
    m4 = torch.stack([masks, 0.6 * masks, torch.zeros_like(masks)], -1)
    m4[:, 20:28, 8:16, 1] = 0.6
    _view_flags_check(v, t, m4.mean(-1), intrs, c2ws, 2)


def _strip(n, rng):
    """A strip of n triangles (manifold; open): vertex ids 0 .. n + 1."""
    k = np.arange(n)
    return np.where((k % 2 == 0)[:, None], np.stack([k, k + 1, k + 2], 1), np.stack([k + 1, k, k + 2], 1))


def _manifold_case(sizes, rng, touch=False):
    tris, base = [], 0
    for s in sizes:
        tris.append(_strip(s, rng) + base)
        base += s + 2 - (1 if touch else 0)                 # touch: the next strip starts on this one's last vertex (a vertex, no edge)
    t = np.concatenate(tris) if tris else np.zeros((0, 3), np.int64)
    nv = base + (1 if touch else 0)
    perm = rng.permutation(nv)
    t = perm[t][rng.permutation(len(t))]
    return rng.normal(size=(nv, 3)), t


def test_components_equal_the_host_pass_on_manifold_meshes():
    from gens_amd import io
    rng = np.random.default_rng(4)
    cases = [_manifold_case([1, 499, 500, 501, 10000], rng), _manifold_case([300, 300, 700], rng, touch=True),
             _manifold_case([499, 501, 2], rng, touch=True), (np.zeros((4, 3)), np.zeros((0, 3), np.int64))]
    for v, t in cases:
        gv, gt = io._drop_small_components_device(v, t, 500)
        hv, ht = io.drop_small_components(v, t, 500)
        assert np.array_equal(gv, hv) and np.array_equal(gt, ht) and gt.dtype == ht.dtype
    assert len(io._drop_small_components_device(*cases[0], 500)[1]) == 11001
    assert len(io._drop_small_components_device(*cases[1], 500)[1]) == 700          # vertex contact joins nothing


def test_components_follow_the_exactly_two_rule_on_a_non_manifold_edge():
    from gens_amd import ops
    rng = np.random.default_rng(6)
    # three strips whose first faces share one edge (0, 1): that edge joins none of them
    strips = []
    base = 2
    for s in (40, 50, 60):
        k = np.arange(s)
        ids = np.concatenate([[0, 1], base + np.arange(s)])
        strips.append(ids[np.stack([k, k + 1, k + 2], 1)])
        base += s
    t = np.concatenate(strips)[rng.permutation(150)]
    tt = torch.from_numpy(t).to(DEV)
    label = ops.face_components(tt, base).cpu().numpy()
    pairs = R.face_adjacency(t)
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    _, want = connected_components(coo_matrix((np.ones(len(pairs)), (pairs[:, 0], pairs[:, 1])), shape=(150, 150)), directed=False)
    first = np.full(want.max() + 1, 150)
    np.minimum.at(first, want, np.arange(150))
    assert np.array_equal(label, first[want]) and len(np.unique(label)) == 3
    got_pairs = np.sort(ops.face_adjacency(tt, base).cpu().numpy(), 1)
    assert sorted(map(tuple, got_pairs.tolist())) == sorted(map(tuple, np.sort(pairs, 1).tolist()))
    # a face with a repeated vertex uses its edge twice: no pair of the face with itself, as trimesh
    deg = torch.tensor([[0, 0, 1], [2, 3, 4], [3, 2, 5]], device=DEV)
    assert np.sort(ops.face_adjacency(deg, 6).cpu().numpy(), 1).tolist() == [[1, 2]]       # (a pair's order is the sort's)


def _assert_same_mesh(got, want):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (got[0].shape, want[0].shape, got[1].shape, want[1].shape)


def test_clean_mesh_matches_the_restatement_on_g14_and_a_blob_scene():
    from gens_amd import io, synthetic
    v, t, masks, intrs, c2ws = _g14()
    want = R.clean_mesh(v, t, masks, intrs, c2ws, upscale=2, min_faces=10, device=DEV)
    got = io.clean_mesh(v, t, masks, intrs, c2ws, upscale=2, min_faces=10)
    _assert_same_mesh(got, want)
    assert 0 < len(got[1]) <= len(io.clean_mesh_by_mask(v, t, io.dilate_masks(masks), intrs, c2ws)) < len(t)
    empty = io.clean_mesh(v, t, masks, intrs, c2ws)                 # 338 faces < 500: the reference raises, this returns an empty mesh
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3)

    v, t = _blobs()
    intrs, c2ws, _, _ = synthetic.make_cameras(5, 48, 64)
    yy, xx = torch.meshgrid(torch.arange(48.0), torch.arange(64.0), indexing="ij")
    m = torch.stack([(((xx - 32 - 3 * i) / 20) ** 2 + ((yy - 22) / 16) ** 2 < 1).float() for i in range(5)])
    m4 = torch.stack([m, m, 0.5 * m], -1)                               # colour masks: averaged first
    want = R.clean_mesh(v, t, m4, intrs, c2ws, device=DEV)
    got = io.clean_mesh(v, t, m4, intrs, c2ws)
    _assert_same_mesh(got, want)
    assert len(got[1]) >= 500                                        # (the visible front of the blobs; the floater is gone)


def test_values_quirk_drops_the_smallest_face_when_every_masked_ray_hits():
    from gens_amd import io, synthetic
    v, t = _blobs()
    intrs, c2ws, _, _ = synthetic.make_cameras(3, 48, 64)
    masks = []
    for i in range(3):                          # a pixel is masked iff all four of its upsampled rays hit (unambiguously)
        ro, rd, _ = R.view_rays(intrs[i], c2ws[i], torch.ones(48, 64), 2)
        face, _, amb = R.first_hits(v, t, ro, rd, device=DEV)
        ok = ((face >= 0) & ~amb).reshape(48, 2, 64, 2).all(3).all(1)
        masks.append(ok.float())
    masks = torch.stack(masks)
    lists, _ = R.frustum_hit_lists(v, t, masks, intrs, c2ws, 2, device=DEV)
    assert all((lst >= 0).all() for lst in lists) and sum(len(lst) for lst in lists) > 100
    want = R.clean_mesh_outside_frustum(v, t, masks, intrs, c2ws, upscale=2, min_faces=500, device=DEV)
    got = io.clean_mesh_outside_frustum(v, t, masks, intrs, c2ws, upscale=2, min_faces=500)
    _assert_same_mesh(got, want)
    from gens_amd import ops
    grid = ops.build_mesh_grid(torch.from_numpy(v).to(DEV), torch.from_numpy(t).to(DEV))
    flags, any_miss = ops.visible_faces(grid, masks, intrs, c2ws, 2)
    assert int(any_miss.item()) == 0 and flags.sum() > 100


def _axis_views():
    """Three 48 x 64 views of the origin from 3 units away.  Focal length 64 and principal point (31.5, 23.5): every entry of K^-1 is a
    dyadic rational, so inverting the 4x4 and inverting its 3x3 block give the same bits (asserted where it is used)."""
    intr = torch.tensor([[64.0, 0, 31.5, 0], [0, 64.0, 23.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    c2ws = []
    for rot in (torch.eye(3), torch.tensor([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]]),
                torch.tensor([[np.cos(0.5), 0, np.sin(0.5)], [0, 1, 0], [-np.sin(0.5), 0, np.cos(0.5)]], dtype=torch.float32)):
        c2w = torch.eye(4)
        c2w[:3, :3] = rot
        c2w[:3, 3] = -3.0 * rot[:, 2]
        c2ws.append(c2w)
    return intr.repeat(3, 1, 1), torch.stack(c2ws)


@pytest.mark.parametrize("radii,misses", [((18, 18, 8), [1, 1, 0]), ((8, 8, 8), [0, 0, 0])])
def test_one_view_ray_kernel_serves_both_cleaners_bit_for_bit(radii, misses):
    """The two instantiations of the view-ray kernel on one scene: K23's (float masks > 0, upscale 1, no advance, one row of flags) marks
    the union of what K25's (uint8 masks > 128, dep_min = 0, one row per view) marks per view, the miss flags agree, and `values[1:]` with
    num_com_vis = 1 on K25's outputs keeps the faces io.clean_mesh_outside_frustum keeps.  A 0.6 sphere (silhouette radius 13 pixels) and
    a detached floater on a 32^3 lattice; centred disk masks of `radii` pixels: 18 reaches past the silhouette (rays miss), 8 does not
    (no ray misses: the smallest hit face is the one dropped, on both paths)."""
    from gens_amd import io, ops
    a, b = _sphere((0.02, -0.01, 0.03), 0.6), _sphere((0.0, 0.85, 0.0), 0.08)
    v, t = _mc(lambda x, y, z: torch.minimum(a(x, y, z), b(x, y, z)), 32)
    intrs, c2ws = _axis_views()
    assert torch.equal(ops.view_ray_cams(intrs, c2ws, "4x4"), ops.view_ray_cams(intrs, c2ws, "3x3"))
    yy, xx = torch.meshgrid(torch.arange(48.0), torch.arange(64.0), indexing="ij")
    mask_float = torch.stack([0.25 * ((xx - 31.5) ** 2 + (yy - 23.5) ** 2 < r * r).float() for r in radii])
    mask_u8 = (255 * (mask_float > 0)).to(torch.uint8)
    grid = ops.build_mesh_grid(torch.from_numpy(v).to(DEV), torch.from_numpy(t).to(DEV))
    flags23, miss23 = ops.visible_faces(grid, mask_float, intrs, c2ws, upscale=1)
    counts, flags25, miss25 = ops.view_rays_hit_counts(grid, mask_u8, intrs, c2ws, dep_min=0)
    assert flags25.shape == (3, len(t)) and flags25.dtype == flags23.dtype == torch.uint8
    assert torch.equal(flags23, flags25.amax(0)) and torch.equal(counts, flags25.sum(0, dtype=torch.int32))
    assert miss25.cpu().tolist() == misses and int(miss23.item()) == int(any(misses))
    assert all(int(f.sum()) > 50 for f in flags25)
    keep, n_values = ops.kept_after_quirk(counts, miss25, 1)
    assert torch.equal(keep, ops.kept_after_quirk(flags23, miss23, 1)[0])          # what clean_mesh_outside_frustum hands its component step
    hit = torch.nonzero(flags23).reshape(-1)
    dropped = torch.nonzero(flags23.bool() & ~keep).reshape(-1).cpu().tolist()
    assert dropped == ([] if any(misses) else [int(hit[0])]) and n_values == len(hit) + int(any(misses))
    want = ops.large_components(v, t.dtype, torch.from_numpy(t).to(DEV)[keep], 1)
    _assert_same_mesh(io.clean_mesh_outside_frustum(v, t, mask_float, intrs, c2ws, upscale=1, min_faces=1), want)
    assert len(want[1]) > 100


def test_save_validation_outputs_with_and_without_the_frustum_step(tmp_path):
    from gens_amd import io, synthetic
    v, t = _blobs()
    intrs, c2ws, _, _ = synthetic.make_cameras(5, 48, 64)
    yy, xx = torch.meshgrid(torch.arange(48.0), torch.arange(64.0), indexing="ij")
    masks = torch.stack([(((xx - 32) / 20) ** 2 + ((yy - 22) / 16) ** 2 < 1).float() for _ in range(5)])
    depth = np.linspace(0, 2, 12 * 16, dtype=np.float32).reshape(12, 16)
    outputs = {"vertices": v, "triangles": t.astype(np.int32), "img_fine": np.full((12, 16, 3), 100.0), "normal_img": np.full((12, 16, 3), 128.0),
               "sdf_depth": depth, "render_depth": depth}
    scale = torch.eye(4)
    scale[:3, 3] = torch.tensor([0.5, -1.0, 2.0])
    inputs = {"scene": "scan1", "file_name": "scan1_view0", "scale_mat": scale, "masks": masks, "intrs": intrs, "c2ws": c2ws}
    paths = io.save_validation_outputs(str(tmp_path / "a"), outputs, inputs, "epoch1", clean=True, clean_frustum=True)
    cv, ct = io.clean_mesh(v, t.astype(np.int32), masks, intrs, c2ws)
    io.write_ply(str(tmp_path / "want.ply"), io.transform_vertices(cv, scale.numpy()), ct)
    assert open(paths["mesh"], "rb").read() == open(tmp_path / "want.ply", "rb").read() and 0 < len(ct) < len(t)
    # clean=True alone: the mask half only, every vertex kept -- what the writer did before the frustum step existed
    paths = io.save_validation_outputs(str(tmp_path / "b"), outputs, inputs, "epoch1", clean=True)
    kept = io.clean_mesh_by_mask(v, t.astype(np.int32), io.dilate_masks(masks), intrs, c2ws)
    io.write_ply(str(tmp_path / "mask.ply"), io.transform_vertices(v, scale.numpy()), kept)
    assert open(paths["mesh"], "rb").read() == open(tmp_path / "mask.ply", "rb").read()
