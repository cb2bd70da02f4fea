"""Generator of tests/golden/g20_dtu_eval.npz: the reference's OWN evaluation/dtu_eval.py, run as written on 15 synthetic scans.

    python tests/golden/make_golden_dtu_eval.py /path/to/reference [--time RADIUS N_STL]

The script is executed with runpy.run_path(..., run_name="__main__"); nothing in it is edited.  Three things around it are arranged:

  * `open3d` is not installed, and the script needs only two readers from it.  A stub module named open3d is put in sys.modules whose
    io.read_triangle_mesh(path) and io.read_point_cloud(path) return objects with the arrays (.vertices / .triangles, .points) of the
    synthetic scan the path names.  The .mat files are REAL files written with scipy.io.savemat into a temporary dataset directory.
  * numpy.random.default_rng is replaced, for the run, by a function that returns numpy's own generator seeded SHUFFLE_SEED + k for the
    k-th call: the script calls it once per scan, for the shuffle.  Generator.shuffle(rows, axis=0) applies the permutation that
    Generator.permutation(n) returns for the same seed, which is how the product and the tests reproduce it.
  * the script's `from numpy import *` shadows the builtin `max`, and sample_single_tri's `max(n1, 1e-7)` then calls numpy.max(n1, axis=1e-7)
    and raises TypeError under current numpy.  The intended meaning is the builtin (the upstream DTU evaluator has no star import).  The one
    name "max" is hidden from numpy.__all__ for the duration of the run; `mean`, which the script's last line takes from the star import,
    is untouched.

The inputs are regenerated from seeds by tests/dtu_eval_reference.make_scan (the tests import the same helper), so the file stores only
results: the 15 printed triples, the per-scan counts, and the last scan's intermediates (data_down, the masks that select data_in /
data_in_obs / stl_above, both distance arrays).  Arrays and numbers only.

--time RADIUS N_STL replaces the last scan by ONE larger synthetic scan and prints the wall time of the script's whole run: the CPU
figure profiles/r08_dtu_eval.txt sets the device times against."""
import contextlib
import io
import os
import runpy
import sys
import tempfile
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import dtu_eval_reference as R  # noqa: E402


def run_script(reference_root, scans):
    """scans: {scan id: make_scan dict} for the 15 ids -> (printed lines, the script's globals after the run, seconds)."""
    import scipy.io
    script = os.path.join(reference_root, "evaluation", "dtu_eval.py")
    ids = list(R.SCAN_IDS)

    def scan_of(path):
        digits = "".join(ch for ch in os.path.basename(path).split("_")[0] if ch.isdigit())
        return scans[int(digits)]

    o3d = types.ModuleType("open3d")
    o3d.io = types.SimpleNamespace(
        read_triangle_mesh=lambda path: types.SimpleNamespace(vertices=scan_of(path)["vertices"].copy(), triangles=scan_of(path)["triangles"].copy()),
        read_point_cloud=lambda path: types.SimpleNamespace(points=scan_of(path)["stl"].copy()))
    real_rng, real_all, real_argv, calls = np.random.default_rng, np.__all__, sys.argv, [0]

    def seeded_rng(*seed):
        if seed:                                    # (a library's own seeded generator, not the script's bare call)
            return real_rng(*seed)
        calls[0] += 1
        return real_rng(R.SHUFFLE_SEED + calls[0] - 1)

    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "ObsMask"))
        for n in ids:
            s = scans[n]
            scipy.io.savemat(os.path.join(tmp, "ObsMask", f"ObsMask{n}_10.mat"), {"ObsMask": s["ObsMask"], "BB": s["BB"], "Res": s["Res"]})
            scipy.io.savemat(os.path.join(tmp, "ObsMask", f"Plane{n}.mat"), {"P": s["P"]})
        out = io.StringIO()
        sys.modules["open3d"] = o3d
        np.random.default_rng = seeded_rng
        np.__all__ = [name for name in real_all if name != "max"]
        sys.argv = [script, "--out_dir", tmp, "--dataset_dir", tmp, "--downsample_density", str(R.DENSITY), "--patch_size", str(R.PATCH),
                    "--max_dist", str(R.MAX_DIST)]
        t0 = time.time()
        try:
            with contextlib.redirect_stdout(out):
                g = runpy.run_path(script, run_name="__main__")
        finally:
            seconds = time.time() - t0
            sys.argv, np.__all__, np.random.default_rng = real_argv, real_all, real_rng
            del sys.modules["open3d"]
    return out.getvalue().splitlines(), g, seconds


def main():
    reference_root = sys.argv[1]
    if "--time" in sys.argv:
        a = sys.argv.index("--time")
        scans = {n: R.make_scan(k) for k, n in enumerate(R.SCAN_IDS)}
        scans[R.SCAN_IDS[-1]] = R.make_scan(0, radius=float(sys.argv[a + 1]), n_stl=int(sys.argv[a + 2]))
        lines, g, seconds = run_script(reference_root, scans)
        print(f"dtu_eval.py: {seconds:.1f} s on {os.cpu_count()} cores for the 14 small scans of g20 (about 5 s together) and one of "
              f"{len(g['data_pcd'])} sampled points, {len(g['data_down'])} after down-sampling, {len(g['stl'])} scan points")
        return
    scans = {n: R.make_scan(k) for k, n in enumerate(R.SCAN_IDS)}
    lines, g, seconds = run_script(reference_root, scans)
    assert lines[-2] == "final result", lines[-3:]
    triples = np.array([[float(w) for w in line.split()[1:]] for line in lines[:15]])
    assert [int(line.split()[0]) for line in lines[:15]] == list(R.SCAN_IDS)
    final = np.array([float(w) for w in lines[-1].split()])
    # the per-scan counts are not printed: the float64 restatement supplies them, after it has reproduced the script's triple of that scan
    counts = []
    for k, n in enumerate(R.SCAN_IDS):
        r = R.dtu_chamfer(scans[n], rng=np.random.default_rng(R.SHUFFLE_SEED + k))
        assert np.allclose([r["d2s"], r["s2d"], r["overall"]], triples[k], rtol=1e-10, atol=0, equal_nan=True), (n, r["d2s"], triples[k])
        counts.append([r[c] for c in ("n_sampled", "n_down", "n_in", "n_in_obs", "n_stl_above")])
    last = [len(g[name]) for name in ("data_pcd", "data_down", "data_in", "data_in_obs", "stl_above")]
    assert last == counts[-1], (last, counts[-1])
    in_obs = np.zeros(len(g["data_down"]), dtype=bool)
    in_obs[np.where(g["inbound"])[0][g["grid_inbound"]][g["in_obs"]]] = True
    np.savez_compressed(os.path.join(HERE, "g20_dtu_eval.npz"), scan_ids=np.array(R.SCAN_IDS), triples=triples, final=final,
                        counts=np.array(counts, dtype=np.int64), density=R.DENSITY, patch=R.PATCH, max_dist=R.MAX_DIST,
                        shuffle_seed=R.SHUFFLE_SEED, last_data_down=g["data_down"], last_inbound=g["inbound"], last_in_obs=in_obs,
                        last_above=g["above"], last_dist_d2s=g["dist_d2s"][:, 0], last_dist_s2d=g["dist_s2d"][:, 0])
    print(f"wrote g20_dtu_eval.npz: 15 scans in {seconds:.1f} s; last scan {last}")
    for line in lines:
        print(line)


if __name__ == "__main__":
    main()
