"""Generator of tests/golden/g21_dtu_clean.npz: the reference's OWN evaluation/clean_meshes.py, its two functions called as written on a
seeded synthetic DTU tree of two scans at the script's 1200 x 1600.

    python tests/golden/make_golden_dtu_clean.py /path/to/reference

The script is loaded with runpy.run_path (its `__main__` block does not run: the two functions it holds are called with the arguments the
block gives them); nothing in it is edited and no line of it is repeated here.  None of the packages it imports is installed, so stub
modules are put in sys.modules for the run:

  * cv2: imread reads the PNG with PIL and returns BGR; getStructuringElement(MORPH_ELLIPSE, (kw, kh)) is OpenCV's construction
    (r = kh // 2, c = kw // 2, dx = round_half_even(c * sqrt((r^2 - dy^2) / r^2)), columns max(c - dx, 0) .. min(c + dx + 1, kw) - 1);
    dilate is scipy.ndimage.grey_dilation per channel with that footprint and a constant border of 0 (OpenCV's default border for
    dilation takes no part); decomposeProjectionMatrix is scipy.linalg.rq + the null vector of P by SVD, a different route from the
    product's (numpy QR + a linear solve), as for g12.
  * trimesh: load / Trimesh.export go through gens_amd.io.read_ply / write_ply (float32 vertices in the file, float64 in memory, as
    trimesh; no merging of coincident vertices -- the product's stated deviation); ray.ray_pyembree.RayMeshIntersector.intersects_first is
    the float64 brute force tests/mesh_clean_reference.first_hits (-1 for a miss), which also marks the rays a last-bit difference could
    change; face_adjacency is mesh_clean_reference.face_adjacency (pinned by g14); graph.connected_components goes through
    scipy.sparse.csgraph (nodes = the faces in the adjacency, components of at least min_len nodes); update_faces and
    remove_unreferenced_vertices are the direct definitions.
  * open3d: an empty module.  tqdm: tqdm(iterable) returns the iterable, and tells the recorder that a new view begins (the script wraps
    each view's chunk loop in one).
  * numpy has removed np.long and (in some versions) np.bool, which the script uses: they are supplied as attributes of the numpy module
    while the script's functions run, and removed again.

What is recorded comes from the stubs' inputs and outputs: the vertex mask clean_points_by_mask returns (the module attribute is wrapped
for the run), the faces intersects_first returns per view, the masks update_faces receives, every exported mesh, and the printed lines.

The scans are tests/dtu_clean_reference.golden_scenes(): scan 24 has masks past the silhouette, scan 37 masks inside it.  For each scan
the script's chain runs (mask step with minimal_vis = 1, then the ray step on the file the mask step wrote: "chain").  In the chain both
scans have misses in at least two views (the mask step removes what only one view's mask covers, and that view's rays then miss), so the
ray step is also run on scan 37's unfiltered mesh ("raw"), where fewer than two views have a miss and `values[1:]` drops the smallest hit
face.  The generator asserts that both branches occur.

Conditions (asserted here, on the reference's own run): vertices whose projection lies within 1e-9 of a half-integer and, per view,
faces whose hit status rests only on ambiguous rays are each at most 0.5 % of their population; no view's miss flag rests only on
ambiguous rays."""
import contextlib
import io as _io
import os
import runpy
import sys
import tempfile
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import dtu_clean_reference as R  # noqa: E402
import mesh_clean_reference as M  # noqa: E402

CAP = 0.005


class Recorder:
    def __init__(self):
        self.reset()

    def reset(self):
        self.views, self.updates, self.exports, self.vertex_masks = [], [], [], []

    def new_view(self):
        self.views.append(dict(faces=[], amb=[], ro=[], rd=[]))


REC = Recorder()


def _stub_cv2():
    import scipy.linalg
    from PIL import Image
    from scipy import ndimage
    cv2 = types.ModuleType("cv2")
    cv2.MORPH_ELLIPSE = 2

    def imread(path):
        with Image.open(path) as im:
            return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])

    def getStructuringElement(shape, ksize):
        assert shape == cv2.MORPH_ELLIPSE
        kw, kh = ksize
        r, c = kh // 2, kw // 2
        elem = np.zeros((kh, kw), dtype=np.uint8)
        for i in range(kh):
            dy = i - r
            dx = int(np.rint(c * np.sqrt((r * r - dy * dy) * (1.0 / (r * r) if r else 0.0))))      # (np.rint: half to even, as cvRound)
            elem[i, max(c - dx, 0):min(c + dx + 1, kw)] = 1
        return elem

    def dilate(img, kernel, iterations=1):
        assert iterations == 1 and img.dtype == np.uint8
        fp = kernel.astype(bool)
        if img.ndim == 2:
            return ndimage.grey_dilation(img, footprint=fp, mode="constant", cval=0)
        return np.stack([ndimage.grey_dilation(img[:, :, k], footprint=fp, mode="constant", cval=0) for k in range(img.shape[2])], -1)

    def decomposeProjectionMatrix(P):
        Pd = np.asarray(P, dtype=np.float64)
        K, Rm = scipy.linalg.rq(Pd[:, :3])
        D = np.diag(np.sign(np.diag(K)))
        K, Rm = K @ D, D @ Rm
        c = np.linalg.svd(Pd)[2][-1]
        return K.astype(P.dtype), Rm.astype(P.dtype), c.reshape(4, 1).astype(P.dtype), None, None, None, None

    cv2.imread, cv2.getStructuringElement, cv2.dilate, cv2.decomposeProjectionMatrix = imread, getStructuringElement, dilate, decomposeProjectionMatrix
    return cv2


def _stub_trimesh():
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components as cc
    from gens_amd import io
    trimesh = types.ModuleType("trimesh")

    class Trimesh:
        def __init__(self, vertices, faces):
            self.vertices = np.asarray(vertices, dtype=np.float64)
            self.faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)

        @property
        def face_adjacency(self):
            return M.face_adjacency(self.faces)

        def update_faces(self, mask):
            mask = np.asarray(mask, dtype=bool)
            REC.updates.append(mask.copy())
            self.faces = self.faces[mask]

        def remove_unreferenced_vertices(self):
            used = np.zeros(len(self.vertices), dtype=bool)
            used[self.faces.reshape(-1)] = True
            self.vertices, self.faces = self.vertices[used], (np.cumsum(used) - 1)[self.faces]

        def export(self, path):
            REC.exports.append((path, self.vertices.astype(np.float32), self.faces.copy()))
            io.write_ply(path, self.vertices.astype(np.float32), self.faces)

    def load(path):
        v, t = io.read_ply(path)
        return Trimesh(v, t)

    def connected_components(edges, min_len=1):
        edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
        if len(edges) == 0:
            return []
        n = int(edges.max()) + 1
        _, label = cc(coo_matrix((np.ones(len(edges), np.int8), (edges[:, 0], edges[:, 1])), shape=(n, n)), directed=False)
        nodes = np.unique(edges)
        groups = {}
        for node in nodes:
            groups.setdefault(label[node], []).append(node)
        return [np.array(g) for g in groups.values() if len(g) >= min_len]

    class RayMeshIntersector:
        def __init__(self, mesh):
            self.v, self.t = mesh.vertices.copy(), mesh.faces.copy()

        def intersects_first(self, ray_origins, ray_directions):
            o, d = np.asarray(ray_origins), np.asarray(ray_directions)
            if len(o) == 0:
                return np.zeros(0, dtype=np.int64)
            face, _, amb = M.first_hits(self.v, self.t, o, d)
            view = REC.views[-1]
            view["faces"].append(face.numpy())
            view["amb"].append(amb.numpy())
            view["ro"].append(o[amb.numpy()])
            view["rd"].append(d[amb.numpy()])
            return face.numpy()

    trimesh.Trimesh, trimesh.load = Trimesh, load
    trimesh.graph = types.SimpleNamespace(connected_components=connected_components)
    trimesh.ray = types.SimpleNamespace(ray_pyembree=types.SimpleNamespace(RayMeshIntersector=RayMeshIntersector))
    return trimesh


def _stub_tqdm():
    mod = types.ModuleType("tqdm")

    def tqdm(iterable, *a, **k):
        REC.new_view()
        return iterable

    mod.tqdm = tqdm
    return mod


@contextlib.contextmanager
def reference_module(reference_root):
    """The script's globals, with the stubs in place and np.long / np.bool supplied for as long as the block runs."""
    stubs = {"cv2": _stub_cv2(), "trimesh": _stub_trimesh(), "open3d": types.ModuleType("open3d"), "tqdm": _stub_tqdm()}
    saved = {k: sys.modules.get(k) for k in stubs}
    added = [n for n in ("long", "bool") if n not in np.__dict__]
    sys.modules.update(stubs)
    if "long" in added:
        np.long = np.int64
    if "bool" in added:
        np.bool = np.bool_
    try:
        g = runpy.run_path(os.path.join(reference_root, "evaluation", "clean_meshes.py"), run_name="reference_clean_meshes")
        inner = g["clean_points_by_mask"]

        def recording(*a, **k):
            mask = inner(*a, **k)
            REC.vertex_masks.append(np.asarray(mask).copy())
            return mask

        g["clean_mesh_faces_by_mask"].__globals__["clean_points_by_mask"] = recording
        yield g
    finally:
        for n in added:
            delattr(np, n)
        for k, v in saved.items():
            if v is None:
                del sys.modules[k]
            else:
                sys.modules[k] = v


def ray_step(g, args, scan, old_file, new_file, imgs_idx, out, prefix):
    """The script's second function on old_file; what the stubs saw goes into `out` under `prefix`."""
    from gens_amd import io
    REC.reset()
    buf = _io.StringIO()
    with contextlib.redirect_stdout(buf):
        g["clean_mesh_faces_outside_frustum"](args, scan, old_file, new_file, imgs_idx, mask_dilated_size=11)
    lines = buf.getvalue().splitlines()
    v_in, t_in = io.read_ply(old_file)
    F = len(t_in)
    assert lines[0].startswith("Surfaces/Kept: ") and len(REC.views) == len(imgs_idx) and len(REC.updates) == 2 and len(REC.exports) == 2
    n_faces, n_values = (int(x) for x in lines[0].split(": ")[1].split("/"))
    assert n_faces == F
    shaky, miss = np.zeros((len(imgs_idx), F), dtype=bool), []
    for i, view in enumerate(REC.views):
        face, amb = np.concatenate(view["faces"]), np.concatenate(view["amb"])
        hits = np.unique(face)
        sure = np.zeros(F, dtype=bool)
        sure[face[(face >= 0) & ~amb]] = True
        if amb.any():
            import torch
            shaky[i] = ~sure & R._near_ambiguous(v_in.astype(np.float64), t_in, torch.from_numpy(np.concatenate(view["ro"])),
                                                 torch.from_numpy(np.concatenate(view["rd"])), None)
        sure_miss, any_miss = bool(((face < 0) & ~amb).any()), bool((face < 0).any())
        assert sure_miss == any_miss, "a view's miss flag rests only on ambiguous rays: change the scene"
        miss.append(any_miss)
        assert shaky[i].mean() <= CAP, (prefix, i, shaky[i].mean())
        sub = slice(0, None, R.G21_SUBSAMPLE)
        out[f"{prefix}_hits_{i}"] = hits.astype(np.int32)
        out[f"{prefix}_sub_face_{i}"], out[f"{prefix}_sub_amb_{i}"] = face[sub].astype(np.int32), amb[sub]
        out[f"{prefix}_n_cast_{i}"] = np.int64(len(face))
        print(f"  {prefix} view {i}: {len(face)} rays cast, {int(amb.sum())} ambiguous, {len(hits)} entries, miss {any_miss}, shaky faces {int(shaky[i].sum())}")
    fv, ft = REC.exports[1][1], REC.exports[1][2]
    # a face is undecided if the views that surely hit it are fewer than two while those and the shaky ones together are at least two (or
    # the other way round for a hit that only ambiguous rays give): its place in `values` could change with a last bit.  None may be.
    listed = np.zeros((len(imgs_idx), F), dtype=bool)
    for i in range(len(imgs_idx)):
        h = out[f"{prefix}_hits_{i}"]
        listed[i, h[h >= 0]] = True
    low, high = (listed & ~shaky).sum(0), (listed | shaky).sum(0)
    assert not ((low < 2) & (high >= 2)).any(), "a face's place in `values` rests on ambiguous rays: change the scene"
    out[f"{prefix}_shaky"], out[f"{prefix}_miss"] = np.packbits(shaky, axis=1), np.array(miss)
    out[f"{prefix}_printed"] = np.array([n_faces, n_values], dtype=np.int64)
    out[f"{prefix}_keep_values"], out[f"{prefix}_keep_components"] = np.packbits(REC.updates[0]), np.packbits(REC.updates[1])
    out[f"{prefix}_final_vertices"], out[f"{prefix}_final_faces"] = fv, ft.astype(np.int32)
    rv, rt = io.read_ply(new_file)
    assert np.array_equal(rv, fv) and np.array_equal(rt, ft)
    return miss, int(REC.updates[0].sum()), n_values, len(ft)


def main():
    from gens_amd import io
    reference_root = sys.argv[1]
    scenes = R.golden_scenes()
    imgs_idx = R.VIEW_LISTS[0][:3]
    out = dict(scan_ids=np.array(list(scenes)), seeds=np.array([R.G21_SCANS[s]["seed"] for s in scenes]), focal_scale=R.G21_FOCAL_SCALE,
               subsample=R.G21_SUBSAMPLE, view_ids=np.array(imgs_idx))
    t0 = time.time()
    branches = set()
    with tempfile.TemporaryDirectory() as tmp, reference_module(reference_root) as g:
        root, mesh_dir = os.path.join(tmp, "DTU_TEST"), os.path.join(tmp, "outputs", "mesh")
        R.write_tree(root, mesh_dir, scenes, imgs_idx, colour=True)
        os.makedirs(os.path.join(mesh_dir, "final"))
        args = types.SimpleNamespace(root_dir=root, out_dir=mesh_dir)
        for scan, sc in scenes.items():
            p = f"s{scan}"
            old = os.path.join(mesh_dir, f"dtu_scan{scan}_epoch0.ply")
            clean = os.path.join(mesh_dir, "final", "clean_%03d.ply" % scan)
            final = os.path.join(mesh_dir, "final", "scan%d.ply" % scan)
            out[f"{p}_vertices"], out[f"{p}_triangles"] = sc["vertices"], sc["triangles"].astype(np.int32)
            out[f"{p}_P"], out[f"{p}_disks"] = R.scene_P(sc), np.array(sc["disks"] if len({len(d) for d in sc["disks"]}) == 1 else
                                                                     [d + [(0.0, 0.0, -1.0)] * (2 - len(d)) for d in sc["disks"]])
            _, near = R.vertex_votes(sc["vertices"].astype(np.float64), R.scene_P(sc), np.zeros((3, sc["H"], sc["W"]), dtype=np.uint8))
            assert near.mean() <= CAP
            out[f"{p}_near_half"] = near
            REC.reset()
            g["clean_mesh_faces_by_mask"](args, old, clean, scan, imgs_idx, minimal_vis=1, mask_dilated_size=11)
            keep = REC.vertex_masks[0]
            cv, ct = io.read_ply(clean)
            assert 0 < keep.sum() < len(keep) and len(cv) == keep.sum() and 0 < len(ct) < len(sc["triangles"])
            out[f"{p}_keep_vertices"], out[f"{p}_clean_faces"] = keep, ct.astype(np.int32)
            print(f"scan {scan}: mask step keeps {int(keep.sum())}/{len(keep)} vertices, {len(ct)}/{len(sc['triangles'])} faces; near-half {int(near.sum())}")
            runs = [("chain", clean, final)] + ([("raw", old, os.path.join(tmp, "raw_%d.ply" % scan))] if not R.G21_SCANS[scan]["misses"] else [])
            for name, src, dst in runs:
                miss, n_kept, n_values, n_final = ray_step(g, args, scan, src, dst, imgs_idx, out, f"{p}_{name}")
                branches.add(sum(miss) >= 2)
                assert (n_values - n_kept == 1) and n_final >= 500, (n_values, n_kept, n_final)
                print(f"scan {scan} {name}: misses {miss}, values {n_values}, kept {n_kept}, final faces {n_final}  ({time.time() - t0:.0f} s)")
    assert branches == {True, False}, "both branches of values[1:] must occur"
    np.savez_compressed(os.path.join(HERE, "g21_dtu_clean.npz"), **out)
    print(f"wrote g21_dtu_clean.npz ({os.path.getsize(os.path.join(HERE, 'g21_dtu_clean.npz'))} bytes) in {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
