"""The DTU mesh finalising step (the reference's evaluation/clean_meshes.py) on the GPU, without OpenCV / trimesh / pyembree / open3d:

    python -m gens_amd.clean_meshes --root_dir DTU_TEST --out_dir outputs/mesh [--n_view 3] [--set 0]

turns every {out_dir}/*scan{n}_epoch0.ply into {out_dir}/final/clean_{n:03}.ply (the mask step) and {out_dir}/final/scan{n}.ply (the
ray-cast step), the files `python -m gens_amd.evaluation` scores.  The kernels are K25 (ops.dilate_u8, ops.vertex_mask_votes,
ops.view_rays_hit_counts) and K23 (grid, first hit, face components).  Citations are to evaluation/clean_meshes.py.

The script's quirks are the specification, and are kept:
  * world millimetres at the masks' full resolution (1200 x 1600, hard-coded at :130-134 and the defaults of :189); cameras from
    cameras/{vid:0>8}_cam.txt as float32 K4 @ E (:13-29 -- not datasets/camera.py's read_cam_file, which returns the two factors);
  * masks dilated with OpenCV's 11 x 11 ellipse (ops.opencv_ellipse: row widths 1, 7, 9, 11 x 5, 9, 7, 1), then channel 0 of cv.imread's
    BGR image (blue for a colour PNG) compared with > 128;
  * the vertex test (:118-139) has no test for points behind the camera; the shifted coordinates are tested against 0 <= u <= W,
    0 <= v <= H and looked up in the mask framed by one pixel of ones, so a point that rounds onto the frame counts as inside; a vertex
    stays if MORE than minimal_vis views hold it (1 in the main loop: at least two views);
  * rays start dep_min = 425 mm down the ray (:239), so geometry nearer to a camera is skipped by that view;
  * a face counts once per view that hits it first (np.unique per view, :245) and stays if at least num_com_vis = 2 views do (:251-255);
    the -1 of the misses goes through the same Counter, so it is in `values` only if at least two views had a masked ray that missed;
    `values[1:]` (:260) then drops the -1, and otherwise the smallest hit face index;  "Surfaces/Kept" prints len(values), not the kept count;
  * components of at least 500 faces by trimesh's rule (face_adjacency: edges of exactly two faces; a face without such a neighbour is in
    no component), then the unreferenced vertices go (:275-281);
  * the first step's result goes through a float32 PLY (:162, :207), so the second sees float32-rounded vertices.
Where numpy's behaviour is undefined the choice is stated: a vertex with q[2] == 0 (:121-122 casts inf / nan to int32) is "not inside".

Two deliberate deviations, the same as io.clean_mesh_outside_frustum's: where no component survives the reference raises inside
np.concatenate([]) (:278) -- this returns (and writes) an empty mesh; trimesh merges coincident vertices when it loads a mesh (:145, :207,
:268, :275) -- no merge is done here (K12 emits one vertex per lattice edge)."""
import argparse
import os
from glob import glob

import numpy as np
import torch

from .evaluation import DTU_TEST_SCANS
from .io import device_of
from .ops import kept_after_quirk  # noqa: F401  (:248-260, the `values[1:]` rule both cleaners share)

VIEW_LISTS = ([23, 24, 33, 22, 15, 34, 14, 32, 16, 35, 25], [43, 33, 44, 42, 34, 32, 45, 23, 41, 24, 31])       # :322-325


def read_cam_file(filename):
    """:13-29: the 4x4 float32 product K4 @ E of an MVSNet-style cam.txt (extrinsics on lines 1-4, intrinsics on lines 7-9)."""
    with open(filename) as f:
        lines = [line.rstrip() for line in f.readlines()]
    extrinsics = np.array(" ".join(lines[1:5]).split(), dtype=np.float32).reshape(4, 4)
    intrinsics = np.float32(np.diag([1, 1, 1, 1]))
    intrinsics[:3, :3] = np.array(" ".join(lines[7:10]).split(), dtype=np.float32).reshape(3, 3)
    return intrinsics @ extrinsics


def read_mask(filename):
    """Channel 0 of cv.imread(filename): an (H,W) uint8 array, the blue channel of a colour image, the grey value of a grey one."""
    from PIL import Image
    with Image.open(filename) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, 2])


def _channel0(masks, dev):
    m = torch.as_tensor(np.asarray(masks) if not isinstance(masks, torch.Tensor) else masks).to(dev)
    if m.dtype != torch.uint8 or m.dim() not in (3, 4):
        raise ValueError("masks: (nv,H,W[,c]) uint8")
    return m if m.dim() == 3 else m[..., 0].contiguous()


def dilated_masks(masks, mask_dilated_size=11, device=None):
    """:124-128 / :213-216 for all views at once: channel 0 of masks (nv,H,W[,c]) uint8 dilated by OpenCV's ellipse -> (nv,H,W) uint8 on
    the device (the script dilates all three channels and reads channel 0)."""
    from . import ops
    k = int(mask_dilated_size)
    return ops.dilate_u8(_channel0(masks, device_of(device=device)), ops.opencv_ellipse(k, k), k)


@torch.no_grad()
def clean_mesh_faces_by_mask(vertices, triangles, P, masks, minimal_vis=0, mask_dilated_size=11, device=None):
    """:144-162 on arrays: vertices (V,3), triangles (F,3), P (nv,4,4) float32 (read_cam_file), masks (nv,H,W[,c]) uint8 as read from
    the files -> (vertices, triangles) numpy: the vertices inside the dilated masks of more than `minimal_vis` views, the faces whose three
    vertices stay, re-indexed."""
    from . import ops
    dev = device_of(device=device)
    v_np, t_np = np.asarray(vertices), np.asarray(triangles).reshape(-1, 3)
    votes = ops.vertex_mask_votes(torch.as_tensor(v_np.astype(np.float64)).to(dev), torch.as_tensor(np.asarray(P, dtype=np.float32)).to(dev),
                                  dilated_masks(masks, mask_dilated_size, dev))
    keep = votes > minimal_vis
    t = torch.as_tensor(t_np.astype(np.int64)).to(dev)
    index = torch.cumsum(keep, 0) - 1
    t = t[keep[t].all(dim=1)] if len(t) else t
    return v_np[keep.cpu().numpy()], index[t].cpu().numpy().astype(t_np.dtype)


@torch.no_grad()
def clean_mesh_faces_outside_frustum(vertices, triangles, P, masks, H=1200, W=1600, mask_dilated_size=11, dep_min=425, num_com_vis=2,
                                     min_faces=500, device=None, stats=None):
    """:189-295 on arrays: keep the faces that the masked, full-resolution rays of at least `num_com_vis` views hit first (from dep_min down
    each ray), minus the first of the sorted list (see the module docstring), then the components of at least `min_faces` faces by trimesh's
    rule, then the referenced vertices.  masks (nv,H,W[,c]) uint8 as read from the files -> (vertices, triangles) numpy.  stats: a dict
    that receives n_faces and n_values, the two numbers of the script's "Surfaces/Kept" line.
    Deviations (both as io.clean_mesh_outside_frustum): an empty result where the reference raises because no component survives, and no
    merging of coincident vertices."""
    from . import ops
    from .datasets.camera import load_K_Rt_from_P
    dev = device_of(device=device)
    v_np, t_np = np.asarray(vertices), np.asarray(triangles).reshape(-1, 3)
    m = dilated_masks(masks, mask_dilated_size, dev)
    if tuple(m.shape[1:]) != (int(H), int(W)):
        raise ValueError(f"clean_mesh_faces_outside_frustum: masks of {tuple(m.shape[1:])}, rays of {(H, W)}")
    P = np.asarray(P, dtype=np.float32)
    cams = [load_K_Rt_from_P(None, P[i][:3, :]) for i in range(len(P))]                  # (:220: float32 in, float32 factors out)
    intrs = torch.from_numpy(np.stack([c[0] for c in cams]))
    c2ws = torch.from_numpy(np.stack([c[1] for c in cams]))
    t = torch.as_tensor(t_np.astype(np.int64)).to(dev)
    n_values = 0
    if len(t):
        grid = ops.build_mesh_grid(torch.as_tensor(v_np.astype(np.float64)).to(dev), t)
        counts, _, any_miss = ops.view_rays_hit_counts(grid, m, intrs, c2ws, dep_min)
        keep, n_values = ops.kept_after_quirk(counts, any_miss, num_com_vis)
        t = t[keep]
    if stats is not None:
        stats.update(n_faces=len(t_np), n_values=n_values)
    return ops.large_components(v_np, t_np.dtype, t, min_faces)


def finalize_dtu_meshes(root_dir, out_dir, n_view=3, set=0, scans=DTU_TEST_SCANS, device=None):  # noqa: A002 (the script's argument name)
    """The script's main loop (:318-344): for every scan, {out_dir}/*scan{n}_epoch0.ply -> {out_dir}/final/clean_{n:03}.ply (mask step,
    minimal_vis = 1) -> {out_dir}/final/scan{n}.ply (ray-cast step), with the cameras {root_dir}/cameras/{vid:0>8}_cam.txt and the masks
    {root_dir}/scan{n}/mask/{vid:0>3}.png of the first n_view views of the chosen list.  H and W, which the script hard-codes as 1200 x 1600, are the size of the mask files here,
    in both steps (the vertex step takes them from the masks it is given, the ray step is handed the same).  Prints the script's lines ->
    the written paths."""
    from . import io
    imgs_idx = VIEW_LISTS[0 if set == 0 else 1][:n_view]
    os.makedirs(os.path.join(out_dir, "final"), exist_ok=True)
    written = []
    for scan in scans:
        print("processing scan%d" % scan)
        old_mesh_file = glob(os.path.join(out_dir, "*scan%d_epoch0.ply" % scan))[0]
        clean_mesh_file = os.path.join(out_dir, "final", "clean_%03d.ply" % scan)
        final_mesh_file = os.path.join(out_dir, "final", "scan%d.ply" % scan)
        P = np.stack([read_cam_file(os.path.join(root_dir, "cameras/{:0>8}_cam.txt".format(vid))) for vid in imgs_idx])
        masks = np.stack([read_mask(os.path.join(root_dir, "scan{}/mask/{:0>3}.png".format(scan, vid))) for vid in imgs_idx])
        v, t = io.read_ply(old_mesh_file)
        v, t = clean_mesh_faces_by_mask(v, t, P, masks, minimal_vis=1, mask_dilated_size=11, device=device)
        io.write_ply(clean_mesh_file, v, t)
        v, t = io.read_ply(clean_mesh_file)
        stats = {}
        v, t = clean_mesh_faces_outside_frustum(v, t, P, masks, H=masks.shape[1], W=masks.shape[2], mask_dilated_size=11, device=device,
                                                stats=stats)
        print(f"Surfaces/Kept: {stats['n_faces']}/{stats['n_values']}")
        print("save to {:s}".format(final_mesh_file))
        io.write_ply(final_mesh_file, v, t)
        print("finishing removing triangles")
        print("finish processing scan%d" % scan)
        written.append(final_mesh_file)
    return written


def main(argv=None):
    parser = argparse.ArgumentParser(description="finalise the DTU validation meshes (the reference's evaluation/clean_meshes.py) on the GPU")
    parser.add_argument("--root_dir", dest="root_dir", type=str, default="./DTU_TEST", help="dataset")
    parser.add_argument("--out_dir", dest="out_dir", type=str, default="./outputs/mesh", help="directory of to save test result")
    parser.add_argument("--n_view", dest="n_view", type=int, default=3)
    parser.add_argument("--set", dest="set", type=int, default=0)
    args = parser.parse_args(argv)
    finalize_dtu_meshes(args.root_dir, args.out_dir, n_view=args.n_view, set=args.set)


if __name__ == "__main__":
    main()
