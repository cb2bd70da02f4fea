"""The reference's DTU scoring (evaluation/dtu_eval.py) on the device: the Chamfer distance every GenS table quotes.

    dtu_chamfer     the loop body of dtu_eval.py:49-165 for one scan, on arrays: sample the mesh (K24), shuffle, radius down-sampling
                    (K24), the bounding-box and observation-mask tests (element-wise torch on the device), data -> scan and scan -> data
                    nearest neighbours with the cap (K24), the three means
    evaluate_dtu    the script's loop over the 15 test scans with the script's file layout and the script's printed lines
    python -m gens_amd.evaluation --out_dir ... --dataset_dir ...     the script's command line

Neither open3d nor sklearn is needed; scipy reads the .mat files.  Citations are relative to the reference tree (prstrive/GenS)."""
import argparse
import os

import numpy as np
import torch

DTU_TEST_SCANS = (24, 37, 40, 55, 63, 65, 69, 83, 97, 105, 106, 110, 114, 118, 122)


def _f64_dev(x, dev):
    if isinstance(x, torch.Tensor):
        return x.detach().to(device=dev, dtype=torch.float64)
    return torch.as_tensor(np.ascontiguousarray(np.asarray(x), dtype=np.float64), device=dev)


@torch.no_grad()
def dtu_chamfer(vertices, triangles, stl_points, obs_mask, bb, res, plane, *, points=None, density=0.2, patch=60, max_dist=20, rng=None):
    """One scan of evaluation/dtu_eval.py (:49-165) -> {"d2s", "s2d", "overall"} (floats: mean data -> scan distance, mean scan -> data
    distance, their mean) and the sizes of the steps, {"n_sampled", "n_down", "n_in", "n_in_obs", "n_stl_above"}.

    vertices (V,3), triangles (F,3): the mesh (arrays or tensors; `--mode mesh`).  points=(N,3) given instead (vertices = triangles = None)
    is the script's `--mode pcd`: the cloud is scored as it is.  stl_points (S,3): the scan.  obs_mask (X,Y,Z), bb (2,3), res: `ObsMask`,
    `BB`, `Res` of ObsMask{scan}_10.mat; plane (4,): `P` of Plane{scan}.mat.  density, patch, max_dist: the script's
    --downsample_density, --patch_size, --max_dist.  rng: a numpy.random.Generator for the shuffle; None draws a fresh one, as the script
    does.  The visiting order is rng.permutation(n), drawn on the host -- the permutation Generator.shuffle(rows, axis=0) applies with the
    same seed -- and only the indices go to the device.

    The script's quirks are kept:
      * BB is cast to float32, and the two bounds BB[0] - patch and BB[1] + 2 * patch are float32 sums (:108, 111);
      * `inbound` is asymmetric: >= BB[0] - patch and < BB[1] + 2 * patch (:111);
      * the grid index is np.around, which rounds halves to even (:114);
      * data -> scan measures `data_in_obs` against the WHOLE scan (:127-130);
      * scan -> data measures the scan points above the plane against `data_in`, not `data_in_obs` (:140-142);
      * distances at or beyond max_dist are dropped from the means, and the mean of an empty selection is NaN (:130, 142).
    All geometry is float64, as in the script."""
    from . import ops
    from .io import as_numpy, device_of
    dev = device_of(vertices, triangles, stl_points, points)
    if points is None:
        v = _f64_dev(vertices, dev).reshape(-1, 3)
        t = torch.as_tensor(as_numpy(triangles).astype(np.int64), device=dev).reshape(-1, 3)
        data_pcd = ops.sample_mesh_points(v, t, density)
    else:
        data_pcd = _f64_dev(points, dev).reshape(-1, 3)
    n = data_pcd.shape[0]
    rng = np.random.default_rng() if rng is None else rng
    order = torch.from_numpy(rng.permutation(n)).to(dev)
    data_pcd = data_pcd[order]                                                   # :89-90
    data_down = data_pcd[ops.radius_downsample(data_pcd, density)]               # :94-102

    bb32 = np.asarray(bb).astype(np.float32)                                     # :108
    lo = torch.as_tensor((bb32[:1] - patch).astype(np.float64), device=dev)      # float32 arithmetic, compared in float64
    hi = torch.as_tensor((bb32[1:] + patch * 2).astype(np.float64), device=dev)
    inbound = ((data_down >= lo) & (data_down < hi)).sum(dim=-1) == 3            # :111
    data_in = data_down[inbound]
    res = torch.as_tensor(np.asarray(res, dtype=np.float64).reshape(-1)[:1], device=dev)
    mask = torch.as_tensor(as_numpy(obs_mask) != 0, device=dev)
    data_grid = torch.round((data_in - torch.as_tensor(bb32[:1].astype(np.float64), device=dev)) / res).to(torch.int64)      # :114
    shape = torch.tensor(list(mask.shape), device=dev)
    grid_inbound = ((data_grid >= 0) & (data_grid < shape)).sum(dim=-1) == 3     # :115
    g = data_grid[grid_inbound]
    in_obs = mask[g[:, 0], g[:, 1], g[:, 2]]                                     # :117
    data_in_obs = data_in[grid_inbound][in_obs]

    stl = _f64_dev(stl_points, dev).reshape(-1, 3)
    dist_d2s, _ = ops.nearest_distance(data_in_obs, stl, max_dist)               # :127-128
    mean_d2s = dist_d2s[dist_d2s < max_dist].mean()                              # :130

    p = torch.as_tensor(as_numpy(plane).astype(np.float64).reshape(4), device=dev)
    above = (((p[0] * stl[:, 0] + p[1] * stl[:, 1]) + p[2] * stl[:, 2]) + p[3]) > 0      # :136-137 (numpy sums the four products left to right)
    stl_above = stl[above]
    dist_s2d, _ = ops.nearest_distance(stl_above, data_in, max_dist)             # :140-141
    mean_s2d = dist_s2d[dist_s2d < max_dist].mean()                              # :142

    d2s, s2d = float(mean_d2s), float(mean_s2d)
    return {"d2s": d2s, "s2d": s2d, "overall": (d2s + s2d) / 2, "n_sampled": int(n), "n_down": int(data_down.shape[0]),
            "n_in": int(data_in.shape[0]), "n_in_obs": int(data_in_obs.shape[0]), "n_stl_above": int(stl_above.shape[0])}


def _loadmat(path):
    try:
        from scipy.io import loadmat
    except ImportError as e:
        raise ImportError("gens_amd.evaluation reads the DTU ObsMask / Plane .mat files with scipy.io.loadmat: scipy is not importable") from e
    return loadmat(path)


def evaluate_dtu(out_dir, dataset_dir, scans=DTU_TEST_SCANS, mode="mesh", density=0.2, patch=60, max_dist=20, rng=None, device=None,
                 quiet=False):
    """The script's loop (dtu_eval.py:47-171) over its file layout: {out_dir}/meshes/final/scan{n}.ply (mode "mesh") or
    {out_dir}/pcd/scan{n}.ply (mode "pcd"); {dataset_dir}/ObsMask/ObsMask{n}_10.mat, {dataset_dir}/ObsMask/Plane{n}.mat,
    {dataset_dir}/Points/stl/stl{n:03}_total.ply.  Prints the script's lines unless quiet -> {"scans": {n: dtu_chamfer's result},
    "d2s", "s2d", "overall": the means over the scans}."""
    from . import io
    if mode not in ("mesh", "pcd"):
        raise ValueError(f"evaluate_dtu: mode {mode!r} (mesh or pcd)")
    dev = io.device_of(device=device)
    results = {}
    for scan in scans:
        if mode == "mesh":
            v, t = io.read_ply(os.path.join(out_dir, "meshes", "final", f"scan{scan}.ply"))
            mesh = dict(vertices=torch.as_tensor(v.astype(np.float64), device=dev), triangles=torch.as_tensor(t.astype(np.int64), device=dev))
        else:
            pts, _ = io.read_ply(os.path.join(out_dir, "pcd", f"scan{scan}.ply"))
            mesh = dict(vertices=None, triangles=None, points=torch.as_tensor(pts.astype(np.float64), device=dev))
        obs = _loadmat(f"{dataset_dir}/ObsMask/ObsMask{scan}_10.mat")
        plane = _loadmat(f"{dataset_dir}/ObsMask/Plane{scan}.mat")["P"]
        stl, _ = io.read_ply(f"{dataset_dir}/Points/stl/stl{scan:03}_total.ply")
        r = dtu_chamfer(stl_points=torch.as_tensor(stl.astype(np.float64), device=dev), obs_mask=obs["ObsMask"], bb=obs["BB"], res=obs["Res"],
                        plane=plane, density=density, patch=patch, max_dist=max_dist, rng=rng, **mesh)
        results[scan] = r
        if not quiet:
            print(scan, r["d2s"], r["s2d"], r["overall"])
    summary = {k: float(np.mean([r[k] for r in results.values()])) for k in ("d2s", "s2d", "overall")}
    if not quiet:
        print("final result")
        print(summary["d2s"], summary["s2d"], summary["overall"])
    return {"scans": results, **summary}


def main(argv=None):
    parser = argparse.ArgumentParser(description="DTU Chamfer distance of the 15 test scans (the reference's evaluation/dtu_eval.py) on the GPU")
    parser.add_argument("--out_dir", type=str, default="./outputs")
    parser.add_argument("--scan", type=int, default=1)                     # (the script takes it and never reads it)
    parser.add_argument("--mode", type=str, default="mesh", choices=["mesh", "pcd"])
    parser.add_argument("--dataset_dir", type=str, default="./dtu_points")
    parser.add_argument("--vis_out_dir", type=str, default=".")            # (the script's visualisation is commented out)
    parser.add_argument("--downsample_density", type=float, default=0.2)
    parser.add_argument("--patch_size", type=float, default=60)
    parser.add_argument("--max_dist", type=float, default=20)
    parser.add_argument("--visualize_threshold", type=float, default=10)
    args = parser.parse_args(argv)
    evaluate_dtu(args.out_dir, args.dataset_dir, mode=args.mode, density=args.downsample_density, patch=args.patch_size, max_dist=args.max_dist)


if __name__ == "__main__":
    main()
