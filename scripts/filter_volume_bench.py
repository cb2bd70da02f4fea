#!/usr/bin/env python3
"""GenS.filter_volume on the device: (i) gens_filter_masks (K26) against the torch-operator chain a user would write without it
(tests/filter_volume_reference.filter_chain), same GPU, same process, runs alternating; (ii) the whole filter_volume (SDF lattice + kernel);
(iii) the survival ratios; (iv) a fine-tune step and a validation image with `init_volumes(ipts)` against `init_volumes(ipts,
filter_thresh=0.1)`.  Medians with p10 - p90; the kernel's share of the HBM peak by algorithmic bytes.

    python scripts/filter_volume_bench.py [--iters 30] [--out profiles/r12_filter_volume.txt]

The lattice of (i) is the signed distance to a sphere of radius 0.5 (u = 0.5 - |p|): a shell-shaped band, as a pretrained surface gives.
(ii) and (iii) run a seeded GenS (geometric initialisation, synthetic volumes) as bench.py builds its surface.
(iv) is bench.py's synthetic scene (5 views of 480 x 640) through the model's own init_volumes (feature CNN, volume build, U-Net, seeded
weights), twice from the same seed, once with the threshold; then scripts/train_step_bench.py's fine-tune step (512 rays + 2048 pseudo
points, the shipped fine-tune loss, backward, Adam, the loss read back; captured behind forward after two eager calls) and bench.py's
validation image (all 307 200 rays, geometry off), the two models taking turns.  Both models of a pyramid (feature CNN, U-Net, frozen volumes
and feature pyramid, a captured step each) and the 307 200-ray buffers are alive at once, after (i) - (iii) of that pyramid have freed theirs:
a few GB at 256^3, far inside the 288 GB of an MI355X, too much for a small card.

The torch chain of (i) is the restatement the tests use, tests/filter_volume_reference.py: run this script from a source checkout."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12       # bytes / s, MI355X


def stats(ms):
    s = sorted(ms)
    q = lambda f: s[min(len(s) - 1, int(f * len(s)))]  # noqa: E731
    return q(0.5), q(0.1), q(0.9)


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def quiet(fn):
    real = sys.stdout
    try:
        sys.stdout = open(os.devnull, "w")
        return fn()
    finally:
        sys.stdout.close()
        sys.stdout = real


def steps_with_and_without(dims, iters, thresh=0.1, configs=None, tag="(iv)"):
    """(iv): -> report lines.  configs: (name, init_volumes keywords) pairs, the first one the base of the ratios (default: the visibility
    masks against the filtered ones)."""
    from gens_amd import synthetic
    from gens_amd.config import gens_loss_conf, gens_model_conf
    from gens_amd.losses import Loss
    from gens_amd.models.gens import GenS
    dev = torch.device("cuda:0")
    nv, h, w = 5, 480, 640
    sc = synthetic.make_scene(nv=nv, h=h, w=w, n_levels=5, seed=0)
    imgs, intrs, c2ws = sc["imgs"].to(dev), sc["intrs"].to(dev), sc["c2ws"].to(dev)
    near, far = sc["near"].to(dev), sc["far"].to(dev)
    g = torch.Generator().manual_seed(3)
    pix = torch.stack([torch.randint(0, w, (512,), generator=g), torch.randint(0, h, (512,), generator=g)], -1)
    ro, rd = synthetic.make_rays(sc["intrs"], sc["c2ws"], h, w, pixels=pix)
    ipts = {"imgs": imgs, "intrs": intrs, "c2ws": c2ws, "rays_o": ro.to(dev), "rays_d": rd.to(dev), "near": near, "far": far,
            "pseudo_pts": (torch.rand(2048, 3, generator=g) - 0.5).to(dev), "view_ids": list(range(nv))}
    targets = {"color": torch.rand(512, 3, generator=g).to(dev)}
    loss_fn = Loss(gens_loss_conf(finetune=True)).to(dev)
    all_o, all_d = synthetic.make_rays(sc["intrs"], sc["c2ws"], h, w)
    all_o, all_d = all_o.to(dev), all_d.to(dev)
    runs = {}
    for name, kw in configs or (("visibility masks", {}), (f"filter_thresh={thresh}", {"filter_thresh": thresh})):
        torch.manual_seed(0)
        model = GenS(gens_model_conf(volume_dims=tuple(dims))).to(dev).train()
        quiet(lambda: model.init_volumes({"imgs": imgs, "intrs": intrs, "c2ws": c2ws}, **kw))
        torch.cuda.empty_cache()
        opt = torch.optim.Adam(model.get_optim_params({"mlp_lr": 5e-4, "vol_lr": [5e-4] * len(dims)}))

        def step(model=model, opt=opt):
            opt.zero_grad(set_to_none=True)
            loss = loss_fn(model("train", ipts, cos_anneal_ratio=0.5), targets)["loss"]
            loss.backward()
            opt.step()
            return float(loss)

        def image(model=model):
            surf = model.implicit_surface
            with torch.no_grad():
                surf.validate(all_o, all_d, near, far, list(model.volumes), list(model.mask_volmes), imgs, list(model.features), list(model.features),
                              intrs, c2ws, None, None, (1, all_o.shape[0]), extract_geometry=False)
        runs[name] = {"model": model, "step": step, "image": image, "live": [float(m.mean()) for m in model.mask_volmes], "step_ms": [], "image_ms": []}
    for r in runs.values():
        for _ in range(5):
            r["step"]()
    for _ in range(iters):
        for r in runs.values():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r["step"]()
            torch.cuda.synchronize()
            r["step_ms"].append(1e3 * (time.perf_counter() - t0))
    for r in runs.values():
        r["model"].eval()
        r["image"]()
    for _ in range(max(5, iters // 4)):
        for r in runs.values():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r["image"]()
            torch.cuda.synchronize()
            r["image_ms"].append(1e3 * (time.perf_counter() - t0))
    out = []
    for name, r in runs.items():
        s, i = stats(r["step_ms"]), stats(r["image_ms"])
        out.append(f"{tag} dims {tuple(dims)}, {name}: live share per level {[round(v, 4) for v in r['live']]}; fine-tune step {s[0]:.2f} ms ({s[1]:.2f} - {s[2]:.2f}); "
                   f"validation image 480 x 640 {i[0]:.1f} ms ({i[1]:.1f} - {i[2]:.1f})")
    (base, a), (last, b) = list(runs.items())[0], list(runs.items())[-1]
    what = "filtered / unfiltered" if configs is None else f"{last} / {base}"
    out.append(f"{tag} dims {tuple(dims)}: {what} = {stats(b['step_ms'])[0] / stats(a['step_ms'])[0]:.3f} (fine-tune step), "
               f"{stats(b['image_ms'])[0] / stats(a['image_ms'])[0]:.3f} (validation image)")
    for r in runs.values():
        r["model"].implicit_surface.join_speculation()
    runs.clear()
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-steps", action="store_true", help="leave out (iv)")
    args = ap.parse_args()
    try:
        import filter_volume_reference as FR
    except ImportError as e:
        raise SystemExit(f"filter_volume_bench: the torch chain it measures against is tests/filter_volume_reference.py of a source checkout ({e})")
    from gens_amd import ops, synthetic
    from gens_amd.config import gens_model_conf
    from gens_amd.models.gens import GenS
    lines = [f"filter_volume_bench: {torch.cuda.get_device_name(0)}, {args.iters} alternating runs per figure, median (p10 - p90)"]
    for dims in ((256, 128, 64), (256, 128, 64, 32, 16)):
        d0 = dims[0]
        ax = torch.linspace(-1, 1, d0, device="cuda")
        u = (0.5 - torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)).contiguous()
        g = torch.Generator().manual_seed(1)
        masks = [(torch.rand(1, 1, d, d, d, generator=g) < 0.945).float().cuda() for d in dims]
        for _ in range(3):
            ops.filter_masks(u, masks, 0.1)
            FR.filter_chain(u, masks, 0.1)
        kern, chain = [], []
        for _ in range(args.iters):
            kern.append(timed(lambda: ops.filter_masks(u, masks, 0.1)))
            chain.append(timed(lambda: FR.filter_chain(u, masks, 0.1)))
        from gens_amd import lib as L
        L.profile_begin(only={"gens_filter_masks"})
        for _ in range(args.iters):
            ops.filter_masks(u, masks, 0.1)
        e = stats([ms for _, ms, _, _ in L.profile_end(raw=True)])
        outs, nb, nd = ops.filter_masks(u, masks, 0.1)
        ref = FR.filter_chain(u, masks, 0.1)
        assert all(torch.equal(a, b) for a, b in zip(outs, ref["masks"]))
        n_all = sum(d ** 3 for d in dims)
        nbytes = 4 * d0 ** 3 + 8 * n_all + n_all // 8 + d0 ** 3 // 4
        k, c = stats(kern), stats(chain)
        lines.append(f"(i) dims {dims}: ops.filter_masks (allocations included) {k[0]:.3f} ms ({k[1]:.3f} - {k[2]:.3f}), torch chain {c[0]:.3f} ms ({c[1]:.3f} - {c[2]:.3f}), "
                     f"chain / operator = {c[0] / k[0]:.1f} x; the entry point alone (events around the call: clearing the counts + two launches) {e[0]:.3f} ms "
                     f"({e[1]:.3f} - {e[2]:.3f}); {nbytes / 1e6:.1f} MB algorithmic -> {100 * nbytes / (e[0] * 1e-3) / HBM_PEAK:.1f} % of the HBM peak; "
                     f"results equal; band {int(nb) / d0 ** 3:.4f}, dilated {int(nd) / d0 ** 3:.4f} of the lattice")
        torch.manual_seed(0)
        model = GenS(gens_model_conf(volume_dims=dims))
        model.has_vol = True
        model = model.cuda()
        vols = [v.cuda() for v in synthetic.make_volumes(dims, seed=3)]
        whole = []

        def whole_runs():
            for it in range(3 + max(5, args.iters // 3)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = model.filter_volume(vols, list(masks), 0.1)
                torch.cuda.synchronize()
                if it >= 3:
                    whole.append(1e3 * (time.perf_counter() - t0))
            return out
        out = quiet(whole_runs)
        w = stats(whole)
        live0, live1 = float(masks[0].mean()), float(out[0].mean())
        lines.append(f"(ii) dims {dims}: GenS.filter_volume (SDF lattice {d0}^3 + kernel + the read-back of the counts) {w[0]:.2f} ms ({w[1]:.2f} - {w[2]:.2f}), "
                     f"precision route '{model.implicit_surface.sdf_precision}'")
        lines.append(f"(iii) dims {dims}: level-0 mask live share {live0:.4f} -> {live1:.4f} after filtering (seeded geometric-initialisation surface, synthetic volumes)")
        del model, vols, out, masks, u
        torch.cuda.empty_cache()
        if not args.skip_steps:
            lines += steps_with_and_without(dims, args.iters)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
