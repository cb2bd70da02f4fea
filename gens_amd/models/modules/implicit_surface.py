"""Mirror of the reference's models/modules/implicit_surface.py (NeuS-style renderer), re-organised around the
per-ray HIP kernels of libgens_hip.so:

    reference method (file:line)              here
    ----------------------------------------  -----------------------------------------------------------------
    sample_pdf            :14-44              fused into ops.upsample (K6)
    up_sample             :60-109             ImplicitSurface.up_sample      -> ops.upsample (K5+K6, one wave per ray)
    cat_z_vals            :111-133            ImplicitSurface.cat_z_vals     -> ops.merge_samples (K7)
    tv_regularization     :135-150            ops.tv_regularization (K10)
    render_core           :152-349            ImplicitSurface.render_core    -> K3, K2(+K2''), K4, K8, K9
    render                :351-405            ImplicitSurface.render
    extract_geometry      :407-427            ImplicitSurface.extract_geometry (device lattice, one D2H copy)
    validate              :429-470            ImplicitSurface.validate
    forward               :472-499            ImplicitSurface.forward

Same constructor, method names, argument order and output keys as the reference, so models/gens.py drives it
unchanged.  Host RNG draws (`torch.rand([B,1])`, `torch.rand([1024,3])` from the CPU generator, :256,:362) are
kept in the reference's order so a seeded run renders the same jitter.
"""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops
from .blending_network import BlendingNetwork
from .projector import lookup_feature, surface_patch_warp
from .sdf_network import SDFNetwork
from .variance_network import SingleVarianceNetwork

REFERENCE_CHUNK = 256      # rays per render() call in the reference's validate (:437-438)
N_RANDOM_PTS = 1024        # sparse-SDF probe points per render_core call (:256)


class Scene:
    """Per-scene device state shared by every ray chunk: mask pyramid, packed volumes, texel views, warp features."""

    def __init__(self, volumes, mask_volumes, imgs, features, match_features, intrs, c2ws):
        self.volumes = list(volumes)
        self.mask_volumes = list(mask_volumes)
        self.masks = ops.VolumeSet.masks(self.mask_volumes)
        self.imgs, self.features, self.match_features = imgs, features, match_features
        self.intrs, self.c2ws = intrs, c2ws
        self.views = ops.SceneViews(imgs, intrs, c2ws, features)
        self._packed = None
        self._warp = {}

    def ref_rotation(self):
        """Row-major inverse of the reference camera's rotation (implicit_surface.py:242,245): nine floats ON THE DEVICE from the scene's
        set-up launch (the compositing kernel reads them there; round 2 read them back to the host once per scene, a synchronisation per
        training step)."""
        return self.views.cams.rot_inv

    def volumes_nograd(self):
        """Packed (X,Y,Z,4) texel copy for passes that never need d/dvolume (sampling rounds, inference)."""
        if self._packed is None:
            self._packed = ops.VolumeSet.packed(self.volumes)
        return self._packed

    def warp_features(self, use_match):
        """cat([f0, up(f1), up(f2)]) texels, built once per scene (the reference rebuilds them per chunk, :313-326)."""
        if use_match not in self._warp:
            src = self.match_features if use_match else self.features
            self._warp[use_match] = ops.build_warp_features(src[:3])
        return self._warp[use_match]


def _jitter_block(n_rays, chunk=REFERENCE_CHUNK, generator=None):
    """Jitter of `n_rays` rays (a whole number of reference chunks, except possibly the last) in the reference's draw order:
    per chunk `torch.rand([chunk, 1])` followed by the `torch.rand([1024, 3])` of render_core (implicit_surface.py:256,362).
    The CPU generator produces one float per 32-bit draw, so ONE large call yields the same stream as the 2*k small ones.
    generator: None = the default CPU generator (the reference's), else a private one standing at the state the draws start from."""
    full, rem = divmod(n_rays, chunk)
    out = []
    if full:
        per = chunk + 3 * N_RANDOM_PTS
        out.append(torch.rand(full * per, generator=generator).reshape(full, per)[:, :chunk].reshape(-1, 1))
    if rem:
        out.append(torch.rand([rem, 1], generator=generator))
        torch.rand([N_RANDOM_PTS, 3], generator=generator)
    return torch.cat(out, 0) if out else torch.zeros(0, 1)


def reference_jitter(n_rays, chunk=REFERENCE_CHUNK):
    """The (n_rays,1) stratified-jitter draws `validate` would make chunk by chunk, so any chunking here renders the same image."""
    return _jitter_block(n_rays, chunk)


class JitterStream:
    """reference_jitter() produced group by group on a helper thread, so the ~4 M host RNG draws of a 480x640 image overlap
    with GPU work instead of preceding it.

    generator=None draws from the default CPU generator -- then nothing else may draw from it while the thread runs (validate() joins the
    thread before it returns).  With a PRIVATE generator (validate()'s head start on the next image, ImplicitSurface._speculate_jitter) the
    thread touches nothing shared: the draws become the default generator's past only if they are used (its state is moved to
    `end_state()` then)."""

    def __init__(self, n_rays, group, buf=None, generator=None):
        """buf: optional (n_rays, 1) host buffer to fill -- a page-locked one makes the per-chunk upload asynchronous."""
        import threading
        group = max(REFERENCE_CHUNK, group // REFERENCE_CHUNK * REFERENCE_CHUNK)
        self.bounds = [(s, min(s + group, n_rays)) for s in range(0, n_rays, group)]
        self.buf = buf if buf is not None else torch.empty(n_rays, 1)
        self.generator = generator
        self.ready = [threading.Event() for _ in self.bounds]
        self.thread = threading.Thread(target=self._run, daemon=False)    # (joined at interpreter exit: a daemon thread killed inside torch's generator aborts the process)
        self.thread.start()

    def _run(self):
        for k, (s, e) in enumerate(self.bounds):
            self.buf[s:e] = _jitter_block(e - s, generator=self.generator)
            self.ready[k].set()

    def slice(self, s, e):
        for k, (bs, be) in enumerate(self.bounds):
            if be <= s or bs >= e:
                continue
            self.ready[k].wait()
        return self.buf[s:e]

    def join(self):
        self.thread.join()

    def end_state(self):
        """(after join) the generator state behind the image's last draw"""
        return self.generator.get_state()


class ImplicitSurface(nn.Module):
    def __init__(self, confs):
        super().__init__()
        self.n_samples = confs.get_int("render.n_samples")
        self.n_importance = confs.get_int("render.n_importance")
        self.up_sample_steps = confs.get_int("render.up_sample_steps")
        self.perturb = confs.get_float("render.perturb")
        self.sdf_network = SDFNetwork(**confs["sdf_network"])
        self.color_network = BlendingNetwork(**confs["color_network"])
        self.deviation_network = SingleVarianceNetwork(**confs["variance_network"])
        self.val_chunk = None          # rays per chunk in validate(); rays are independent, so this is a free knob.  None: equal chunks of at most
                                       # 32 768 rays over the ray range (chunking.balanced_chunk) -- the setting every committed measurement uses
        self.speculate_jitter = True   # validate() draws the NEXT image's jitter ahead of time on a private generator (see _speculate_jitter)
        self.fused_sdf = True          # inference: evaluate the SDF network with the fused MFMA kernel (gens_sdf_mlp)
        self.sdf_precision = "f32"     # "f32": exact float32 MFMA; "f16x2": split-half operands (~1e-6 rel.), float32 fallback on overflow
        self._sdf_plan = None
        self.fused_blend = True        # inference: source-view look-up + colour network in one kernel (gens_blend_views)
        self._blend_plan = None
        self.fused_train = True        # training: SDF value / gradient / smooth and their backward in the K17 kernels (gens_sdf_train_*)
        self.fused_sampling = True     # one launch per sampling round (gens_merge_upsample) instead of merge + up-sample (+ mid-points) launches

    # ----------------------------------------------------------------------------------------------------------
    # masked SDF evaluation (Q7, Q8)
    # ----------------------------------------------------------------------------------------------------------
    @staticmethod
    def _select(valid):
        """Indices of valid points; if none is valid the first 10 are used (:123-124,176-177,372-373)."""
        idx = torch.nonzero(valid, as_tuple=False)[:, 0]
        if idx.numel() < 1:
            idx = torch.arange(min(10, valid.numel()), device=valid.device)
        return idx

    def _fused_plan(self, volumes):
        """The packed-weight plan for gens_sdf_mlp, or None when the fused kernel does not apply (autograd needed,
        planar volumes, or a non-shipped architecture) -- then the PyTorch layers run on top of the K2 kernels."""
        if not self.fused_sdf or torch.is_grad_enabled():
            return None
        if not (isinstance(volumes, ops.VolumeSet) and volumes.layout == 1 and 1 <= volumes.n <= 5):
            return None
        net = self.sdf_network
        if not ops.SdfMlpPlan.supported(net) or net.init_feat_channels != 4 * volumes.n:
            return None
        if self._sdf_plan is None or self._sdf_plan.key != ops.SdfMlpPlan.version(net):
            self._sdf_plan = ops.SdfMlpPlan(net)
        return self._sdf_plan

    def _fused_blend_plan(self, views, features=None, imgs=None):
        """The packed-weight plan of gens_blend_views, or None when the fused kernel does not apply.  It has no backward: under autograd it
        runs only if NOTHING on the colour path asks for a gradient (a frozen colour network over frozen feature maps / images)."""
        if not self.fused_blend:
            return None
        if torch.is_grad_enabled():
            wants = any(p.requires_grad for p in self.color_network.parameters())
            wants = wants or any(t.requires_grad for t in (features or [])) or (imgs is not None and imgs.requires_grad)
            if wants or features is None:
                return None
        net = self.color_network
        if not ops.BlendPlan.supported(net) or len(views.feat_tex) > 5 or net.rgb_fc[0].weight.shape[1] != 37:
            return None
        if self._blend_plan is None or self._blend_plan.key != ops.BlendPlan.version(net):
            self._blend_plan = ops.BlendPlan(net)
        return self._blend_plan if self._blend_plan.n_feat == 3 + 4 * len(views.feat_tex) else None

    def _precision(self, plan, want_grad=False):
        """The arithmetic of one SDF launch.  The split-half kernels pre-scale their weight streams by 100 / ln 2, so they have their own
        range condition (plan.value_ok / plan.grad_pieces: |w|, |b| below ~416); a network that fails it is evaluated in float32, it does
        not raise."""
        if self.sdf_precision != "f16x2":
            return "f32"
        if want_grad:
            return "f16x2" if getattr(plan, "grad_pieces", None) is not None else "f32"
        return "f16x2" if getattr(plan, "value_ok", False) else "f32"

    def _train_net(self, scene, lean=False):
        """This step's fused SDF evaluator (ops.SdfTrainStep: the effective weights packed once for the sampling passes, render_core
        and the backward), or None outside training / for architectures the K17 kernels do not cover."""
        if lean or not self.fused_train or not torch.is_grad_enabled():
            return None
        if not any(p.requires_grad for p in self.sdf_network.parameters()) and not any(v.requires_grad for v in scene.volumes):
            return None
        cached = getattr(scene, "_train_net_cache", None)        # one evaluator (weight norm + stream packing) per scene object = per step
        if cached is None:
            cached = scene._train_net_cache = (self.sdf_network.train_step(scene.volumes, scene.volumes_nograd(), tv_masks=scene.mask_volumes),)
        return cached[0]

    def _split_half_overflowed(self):
        """True if a split-half launch met a value outside the half range since the last check (one device sync)."""
        return self.sdf_precision == "f16x2" and self._sdf_plan is not None and self._sdf_plan.overflowed()

    def _masked_sdf(self, pts, valid, volumes, net=None):
        plan = net if net is not None else self._fused_plan(volumes)
        if plan is not None:              # compaction + count stay on the device: no host synchronisation; the unselected rows' 100 rides on it
            sdf = torch.empty(pts.shape[0], 1, device=pts.device, dtype=torch.float32)
            idx, count = ops.compact_fill(valid, sdf=sdf)
            ops.sdf_mlp(plan, volumes, pts, index=idx, sdf_out=sdf, precision=self._precision(plan), count=count)
        else:
            sdf = torch.full((pts.shape[0], 1), 100.0, device=pts.device, dtype=pts.dtype)
            idx = self._select(valid)
            sdf[idx] = self.sdf_network.sdf(pts[idx], volumes)
        return sdf

    # ----------------------------------------------------------------------------------------------------------
    # hierarchical sampling
    # ----------------------------------------------------------------------------------------------------------
    def up_sample(self, rays_o, rays_d, z_vals, sdf, n_importance, mask_volumes, inv_s):
        """Importance samples for a fixed inv_s (:60-109) -> (B, n_importance)."""
        return ops.upsample(rays_o, rays_d, z_vals, sdf.reshape(z_vals.shape), n_importance, mask_volumes, inv_s)[0]

    def cat_z_vals(self, rays_o, rays_d, z_vals, new_z_vals, sdf, volumes, mask_volumes, last=False):
        """Merge new depths (and, unless `last`, their SDF values) into the sorted sample list (:111-133)."""
        if last:
            return ops.merge_samples(z_vals, new_z_vals)[0], sdf
        pts, valid = ops.ray_points(rays_o, rays_d, new_z_vals, mask_volumes)
        new_sdf = self._masked_sdf(pts, valid, volumes).reshape(new_z_vals.shape)
        return ops.merge_samples(z_vals, new_z_vals, sdf.reshape(z_vals.shape), new_sdf)

    def tv_regularization(self, volume_feat_cas, volume_mask_cas=None):
        if volume_mask_cas is None:
            volume_mask_cas = [torch.ones_like(v[:, :1]) for v in volume_feat_cas]
        return ops.tv_regularization(list(volume_feat_cas), list(volume_mask_cas))

    @torch.no_grad()
    def _sample_rays(self, rays_o, rays_d, z_vals, scene, net=None, mid_points=None):
        """The hierarchical sampling of render() (:364-393).  One launch per round between two evaluations of the network: the merge of round i
        (cat_z_vals, :111-133) and the up-sampling of round i + 1 (:60-109) are one kernel (gens_merge_upsample); with `mid_points` =
        sample_dist the last merge also produces render_core's section mid-points and their mask decisions (:163-173), left in
        self._mid_points for the render_core call that follows with the returned z_vals.  `fused_sampling = False` runs the operators one by
        one (gens_upsample / gens_merge_samples: the same bits)."""
        masks, vols = scene.masks, scene.volumes_nograd()
        b = rays_o.shape[0]
        self._mid_points = None
        pts, valid = ops.ray_points(rays_o, rays_d, z_vals, masks)
        sdf = self._masked_sdf(pts, valid, vols, net).reshape(b, -1)
        n_new = self.n_importance // self.up_sample_steps
        valid = valid.reshape(b, -1)                       # mask decisions travel with the samples through the merges
        if not getattr(self, "fused_sampling", True) or self.up_sample_steps < 1:
            for i in range(self.up_sample_steps):
                z_new, pts_new, valid_new = ops.upsample(rays_o, rays_d, z_vals, sdf, n_new, masks, 64 * 2 ** i, valid_in=valid)
                if i + 1 == self.up_sample_steps:
                    z_vals, _ = ops.merge_samples(z_vals, z_new)
                else:
                    sdf_new = self._masked_sdf(pts_new, valid_new, vols, net).reshape(b, n_new)
                    z_vals, sdf, valid = ops.merge_samples(z_vals, z_new, sdf, sdf_new, valid, valid_new)
            return z_vals
        z_new, pts_new, valid_new = ops.upsample(rays_o, rays_d, z_vals, sdf, n_new, masks, 64, valid_in=valid)
        for i in range(1, self.up_sample_steps):
            sdf_new = self._masked_sdf(pts_new, valid_new, vols, net).reshape(b, n_new)
            z_vals, sdf, valid, z_new, pts_new, valid_new = ops.merge_upsample(rays_o, rays_d, z_vals, sdf, valid, z_new, sdf_new, valid_new, n_new, masks,
                                                                               64 * 2 ** i)
        if mid_points is None:
            z_vals, _ = ops.merge_samples(z_vals, z_new)
        else:
            z_vals, pts_mid, valid_mid = ops.merge_mid_points(rays_o, rays_d, z_vals, z_new, masks, mid_points)
            self._mid_points = (z_vals, float(mid_points), pts_mid, valid_mid)
        return z_vals

    # ----------------------------------------------------------------------------------------------------------
    # render_core
    # ----------------------------------------------------------------------------------------------------------
    def _host_draws(self, dev, b=None):
        """The host-generator draws of a render in the reference's order -- torch.rand([B, 1]) (:362, when b is given), then
        torch.rand([1024, 3]) (:256) -- staged through ONE page-locked buffer: a pageable host-to-device copy waits for the stream to drain
        on ROCm (the launch queue ran empty once per step), a pinned one is just another asynchronous launch.  -> (t_rand (B,1) or None,
        pts_random (1024,3) in [-1, 1)) on the device.  The ` * 2 - 1` of :256 happens on the host: the same two float32 operations."""
        n_t = 0 if b is None else b
        capturing = torch.cuda.is_current_stream_capturing()
        buf = getattr(self, "_pinned_draws", None)
        if buf is None or buf.numel() != n_t + 3 * N_RANDOM_PTS:
            buf = torch.empty(n_t + 3 * N_RANDOM_PTS, dtype=torch.float32, pin_memory=True)
            self._pinned_draws = buf
            self._pinned_draws_event = None
        elif self._pinned_draws_event is not None and not capturing:
            self._pinned_draws_event.synchronize()           # the previous step's copy out of this buffer has long finished
        self._pinned_draws_layout = (n_t, b)
        self.refresh_host_draws()
        on_dev = buf.to(dev, non_blocking=True)              # (captured into a graph this is a copy node that reads the buffer at every replay)
        if not capturing:
            self._pinned_draws_event = torch.cuda.Event()
            self._pinned_draws_event.record()
        return (on_dev[:n_t].view(b, 1) if n_t else None), on_dev[n_t:].view(N_RANDOM_PTS, 3)

    def refresh_host_draws(self, buf=None, layout=None):
        """Draw the step's host random numbers into the page-locked staging buffer (the reference's generator, its order and shapes).  A step
        replayed from a captured graph (gens_amd.graph.GraphedStep / AutoGraph) calls this before every replay: the graph's copy node then
        carries the new draws to the device.  The previous replay must have finished reading the buffer.  buf / layout: the buffer a captured
        step owns (AutoGraph keeps one per captured signature); default: this module's own."""
        n_t, b = self._pinned_draws_layout if layout is None else layout
        buf = self._pinned_draws if buf is None else buf
        if n_t:
            buf[:n_t] = torch.rand([b, 1]).reshape(-1)
        buf[n_t:] = (torch.rand([N_RANDOM_PTS, 3]) * 2 - 1).reshape(-1)

    def begin_capture(self):
        """Before a step is captured into a HIP graph: fresh page-locked buffers for the host draws and the deferred checks, allocated NOW (a
        page-locked allocation is not a capturable operation) in the sizes the eager calls before this one used; the captured copy nodes will
        read / write these, and end_capture() hands them to the graph's owner."""
        old = getattr(self, "_pinned_draws", None)
        self._pinned_draws = None if old is None else torch.empty(old.numel(), dtype=torch.float32, pin_memory=True)
        self._pinned_draws_event = None
        self._deferred_host = torch.zeros(4, dtype=torch.int32, pin_memory=True)
        self._deferred = None

    def end_capture(self):
        """-> (draw buffer, its layout, deferred-check words) of the capture that has just ended; this module forgets them, so that an eager call
        allocates its own and never refills or reallocates what a graph's copy nodes point at."""
        got = (getattr(self, "_pinned_draws", None), getattr(self, "_pinned_draws_layout", None), getattr(self, "_deferred_host", None))
        self._pinned_draws = None
        self._pinned_draws_event = None
        self._deferred_host = None
        self._deferred = None
        return got

    def _train_fused_ok(self, scene, net, lean):
        """The fused TRAINING path of render_core: K17 (net) + K18 on a device-side selection (ops.StepPoints), no host synchronisation."""
        if lean or net is None or not self.fused_train or not torch.is_grad_enabled():
            return False
        nf = len(scene.views.feat_tex)
        return (ops.BlendPlan.supported(self.color_network) and nf <= 5 and self.color_network.ray_dir_fc[2].weight.shape[0] == 3 + 4 * nf
                and scene.views.nv >= 2)

    def _render_core_train(self, rays_o, rays_d, z_vals, sample_dist, scene, intrs, c2ws, cos_anneal_ratio, step, net, pts_random, extra_pts,
                           extra_valid):
        """render_core (:152-349) in training mode on the fused kernels, with the masked evaluation's selection left on the device:
        [ray samples | random points | extra (pseudo) points] share ONE K17 forward / backward pair; dense outputs carry the reference's
        defaults for unselected rows (Q8).  extra_valid: uint8 flags of extra_pts, or None (all of them are evaluated)."""
        b, n = z_vals.shape
        dev = z_vals.device
        n_ray, n_r = b * n, pts_random.shape[0]
        n_x = 0 if extra_pts is None else extra_pts.shape[0]
        total = n_ray + n_r + n_x
        pts_all = torch.empty(total, 3, device=dev, dtype=torch.float32)
        valid_all = torch.empty(total, device=dev, dtype=torch.uint8)
        ops.ray_points(rays_o, rays_d, z_vals, scene.masks, mid=True, sample_dist=sample_dist, out=(pts_all[:n_ray], valid_all[:n_ray]))
        pts_all[n_ray:n_ray + n_r].copy_(pts_random)
        if n_x:
            pts_all[n_ray + n_r:].copy_(extra_pts)
            if extra_valid is None:
                valid_all[n_ray + n_r:].fill_(1)
            else:
                valid_all[n_ray + n_r:].copy_(extra_valid)
        s_views = scene.views.nv - 1
        sel = ops.StepPoints(pts_all, valid_all, n_ray, n_r, s_views, z=z_vals, variance=self.deviation_network.variance)
        with_tv = ops.tv_levels_ok(scene.volumes, scene.mask_volumes)       # the regulariser rides on the network's Function: one gradient buffer
        y_all, g_all, s_all, *tv_reg = net(pts_all, sel, tv=with_tv)
        sampled_color, src_vis = ops.blend_train(self.color_network, scene.views, pts_all, sel)
        comp = ops.composite_train(sel, rays_o, rays_d, z_vals, sample_dist, y_all, g_all, s_all, sampled_color, self.deviation_network.variance,
                                   valid_all[:n_ray], sel.vis, cos_anneal_ratio, scene.ref_rotation())
        out = {
            "color_fine": comp["color"],
            "render_depth": comp["depth"],
            "normal": comp["normal"],
            "weights": comp["weights"],
            "weight_sum": comp["wsum"][:, None],
            "weight_max": comp["wmax"][:, None],
            "inside_sphere": comp["inside"],
            "valid_mask": comp["valid"].bool()[:, None],
            "mid_inside_sphere": comp["mid_in"][:, None],
            "sdf_depth": comp["sdf_depth"][:, None],
            "gradients": g_all[:n_ray].reshape(b, n, 3),
            "s_val": sel.scalars[2:3].detach().reshape(1, 1).expand(b * n, 1),
            "gradient_error": comp["gradient_error"],
            "smooth_error": comp["smooth_error"],
            "sparse_sdf": torch.cat([y_all[n_ray:n_ray + n_r], y_all[:n_ray]]),
            "tv_reg": tv_reg[0] if with_tv else self.tv_regularization(scene.volumes, scene.mask_volumes),
        }
        if n_x:
            out["_extra_sdf_dense"] = y_all[n_ray + n_r:]
        self._last_step_counts = sel.counts            # (device; forward() hands it to the deferred checks)
        # surface point of the first sign change (written by the compositing launch), its SDF gradient (the reference builds the second-order
        # graph here too and throws it away: the normal is used detached, :306-310), and the plane-induced patch warp in ONE launch
        g0 = net.first_order(comp["pts_cross"])
        warp = scene.warp_features(use_match=not (step is None or step < 5))
        out["ref_gray_val"], out["sampled_gray_val"] = ops.patch_warp(comp["z_cross"], rays_o, rays_d, g0, scene.views.cams, warp)
        return out

    def render_core(self, rays_o, rays_d, z_vals, sample_dist, volumes, mask_volumes, features, match_features, imgs, intrs, c2ws,
                    cos_anneal_ratio, step, scene=None, lean=False, pts_random=None, extra_pts=None, net=None, extra_valid=None):
        """Everything after sampling (:152-349).  `lean` (validate only) skips the quantities validate discards:
        second derivatives, random-point SDF, TV, the surface-point gradient and the patch warp.
        extra_pts: more points whose SDF the caller wants from the same network pass (forward()'s pseudo points, :484-497):
        returned under the private key "_extra_sdf" -- or, with extra_valid (their uint8 mask flags, left on the device), as the dense
        "_extra_sdf_dense" (zeros where the flag is clear, the reference's pseudo_sdf) of the fused training path."""
        if scene is None:
            scene = Scene(volumes, mask_volumes, imgs, features, match_features, intrs, c2ws)
        b, n = z_vals.shape
        dev = z_vals.device
        if net is None:                                # training: one fused evaluator for every SDF query of this step
            net = self._train_net(scene, lean)
        if self._train_fused_ok(scene, net, lean) and (features is not None):
            if pts_random is None:
                pts_random = self._host_draws(dev)[1]                                      # CPU generator, :256
            return self._render_core_train(rays_o, rays_d, z_vals, sample_dist, scene, intrs, c2ws, cos_anneal_ratio, step, net, pts_random,
                                           extra_pts, extra_valid)
        if extra_valid is not None:                    # the generic path evaluates the selected extra points only
            extra_pts = extra_pts[torch.nonzero(extra_valid)[:, 0]]
        need_vol_grad = torch.is_grad_enabled() and any(v.requires_grad for v in scene.volumes)
        vols = scene.volumes if need_vol_grad else scene.volumes_nograd()

        cached = getattr(self, "_mid_points", None)
        self._mid_points = None
        if cached is not None and cached[0] is z_vals and cached[1] == float(sample_dist):      # _sample_rays' last launch already made them
            pts, valid = cached[2], cached[3]
        else:
            pts, valid = ops.ray_points(rays_o, rays_d, z_vals, scene.masks, mid=True, sample_dist=sample_dist)
        plan = self._fused_plan(vols) if lean else None
        bplan = self._fused_blend_plan(scene.views) if lean else self._fused_blend_plan(scene.views, features, imgs)
        sdf_random = extra_sdf = None
        if plan is not None and bplan is not None:     # fully fused inference: nothing in this branch synchronises with the host
            sdf, gradients = torch.empty(b * n, 1, device=dev), torch.empty(b * n, 3, device=dev)
            sampled_color = torch.empty(b * n, 3, device=dev)
            src_vis = torch.empty(b * n, scene.views.nv - 1, device=dev, dtype=torch.uint8)
            idx, count = ops.compact_fill(valid, sdf=sdf, grad=gradients, rgb=sampled_color, vis=src_vis)      # (defaults of the unselected rows, Q8)
            ops.sdf_mlp(plan, vols, pts, index=idx, want_grad=True, sdf_out=sdf, grad_out=gradients, precision=self._precision(plan, True), count=count)
            smooth = None
            ops.blend_views(bplan, scene.views, pts, index=idx, rgb_out=sampled_color, vis_out=src_vis, count=count)
        else:
            idx = self._select(valid)
            pts_v = pts[idx]
            if plan is not None:                       # fused look-up + MLP + d/dx, scattered straight into the dense arrays
                sdf = torch.full((b * n, 1), 100.0, device=dev)
                gradients = torch.zeros(b * n, 3, device=dev)
                ops.sdf_mlp(plan, vols, pts, index=idx, want_grad=True, sdf_out=sdf, grad_out=gradients, precision=self._precision(plan, True))
                smooth = None
            else:
                if lean:
                    with torch.enable_grad():
                        x = pts_v.clone().requires_grad_(True)
                        sdf_v = self.sdf_network.sdf(x, vols)
                        grad_v = torch.autograd.grad(sdf_v, x, torch.ones_like(sdf_v))[0]
                    sdf_v, smooth_v = sdf_v.detach(), None
                elif net is not None:                      # K17: the ray samples, the 1024 random points (:256-257) and the caller's extra
                    if pts_random is None:                 # points share ONE forward / backward pair of launches
                        pts_random = torch.rand([N_RANDOM_PTS, 3]).to(dev) * 2 - 1             # CPU generator, :256
                    batch = [pts_v, pts_random] + ([extra_pts] if extra_pts is not None else [])
                    y_all, g_all, s_all = net(torch.cat(batch))
                    n_v, n_r = pts_v.shape[0], pts_random.shape[0]
                    sdf_v, grad_v, smooth_v = y_all[:n_v], g_all[:n_v], s_all[:n_v]
                    sdf_random = y_all[n_v:n_v + n_r]
                    extra_sdf = y_all[n_v + n_r:] if extra_pts is not None else None
                else:                                      # one forward pass for :179 (sdf) and :188 (gradient, smooth)
                    sdf_v, grad_v, smooth_v = self.sdf_network.sdf_gradient_smooth(pts_v.clone(), vols)
                sdf = torch.full((b * n, 1), 100.0, device=dev).index_put((idx,), sdf_v)
                gradients = torch.zeros(b * n, 3, device=dev).index_put((idx,), grad_v)
                smooth = None if smooth_v is None else torch.zeros(b * n, 3, device=dev).index_put((idx,), smooth_v)
            if bplan is not None:                      # K4 + colour network fused, scattered into the dense arrays
                sampled_color, src_vis = ops.blend_views(bplan, scene.views, pts, index=idx)
            elif (self.fused_train and torch.is_grad_enabled() and ops.BlendPlan.supported(self.color_network) and len(scene.views.feat_tex) <= 5
                  and self.color_network.ray_dir_fc[2].weight.shape[0] == 3 + 4 * len(scene.views.feat_tex)):
                color_v, vis_v = ops.blend_train(self.color_network, scene.views, pts_v)      # K18: forward / backward in one launch each
                sampled_color = torch.zeros(b * n, 3, device=dev).index_put((idx,), color_v)
                src_vis = torch.zeros(b * n, vis_v.shape[1], dtype=torch.bool, device=dev).index_put((idx,), vis_v)
            else:
                feat_views, ray_diff, vis_v = lookup_feature(pts_v, imgs, intrs, c2ws, features, views=scene.views)
                color_v = self.color_network(feat_views, ray_diff, vis_v)
                sampled_color = torch.zeros(b * n, 3, device=dev).index_put((idx,), color_v)
                src_vis = torch.zeros(b * n, vis_v.shape[1], dtype=torch.bool, device=dev).index_put((idx,), vis_v)

        inv_s = self.deviation_network(torch.zeros([1, 3], device=dev))[:, :1].clip(1e-6, 1e6)
        comp = ops.composite(rays_o, rays_d, z_vals, sample_dist, sdf, gradients, smooth, sampled_color, valid, src_vis, inv_s,
                             cos_anneal_ratio, scene.ref_rotation())
        gradients = gradients.reshape(b, n, 3)
        out = {
            "color_fine": comp["color"],
            "render_depth": comp["depth"],
            "normal": comp["normal"],
            "weights": comp["weights"],
            "weight_sum": comp["wsum"][:, None],
            "weight_max": comp["wmax"][:, None],
            "inside_sphere": comp["inside"],
            "valid_mask": comp["valid"].bool()[:, None],
            "mid_inside_sphere": comp["mid_in"][:, None],
            "sdf_depth": comp["sdf_depth"][:, None],
            "gradients": gradients,
            "s_val": (1.0 / inv_s).expand(b * n, 1),
            "gradient_error": comp["eik_num"].sum() / (comp["eik_den"].sum() + 1e-5),
        }
        if lean:
            return out
        out["smooth_error"] = torch.linalg.norm(comp["smooth_vec"], ord=2, dim=-1).abs().mean()

        if pts_random is None:
            pts_random = torch.rand([N_RANDOM_PTS, 3]).to(dev) * 2 - 1                     # CPU generator, :256
        if sdf_random is None:
            sdf_random = self.sdf_network.sdf(pts_random, vols)
        out["sparse_sdf"] = torch.cat([sdf_random, sdf])
        if extra_pts is not None:
            out["_extra_sdf"] = extra_sdf if extra_sdf is not None else self.sdf_network.sdf(extra_pts, vols)
        out["tv_reg"] = self.tv_regularization(scene.volumes, scene.mask_volumes)

        # surface point of the first sign change and the plane-induced patch warp (:288-328)
        pts_sdf0 = rays_o[:, None, :] + rays_d[:, None, :] * comp["z_cross"][:, None, None]
        # the reference builds the second-order graph here too and throws it away: the normal is used detached (:306-310)
        if net is not None:
            g0 = net.first_order(pts_sdf0)
        else:
            g0, _ = self.sdf_network.gradient(pts_sdf0.detach().reshape(-1, 3).clone(), vols, second_order=False)
        g0 = g0.reshape(b, 1, 3)
        g0_norm = torch.linalg.norm(g0, ord=2, dim=-1, keepdim=True)
        g0 = g0 / torch.where(g0_norm <= 0, torch.full_like(g0_norm, 1e-8), g0_norm)
        normals_ref = (g0 @ c2ws[0, :3, :3]).detach()                                       # R^T n as row vectors
        warp = scene.warp_features(use_match=not (step is None or step < 5))
        out["ref_gray_val"], out["sampled_gray_val"] = surface_patch_warp(pts_sdf0, normals_ref, warp, intrs, c2ws)
        return out

    # ----------------------------------------------------------------------------------------------------------
    # render
    # ----------------------------------------------------------------------------------------------------------
    def _coarse_steps(self, dev):
        """torch.linspace(0, 1, n_samples) as the reference computes it (on the host, implicit_surface.py:357), uploaded ONCE per
        device: a pageable host-to-device copy waits for the stream to drain on ROCm, which put the host in lock-step with the GPU
        once per ray chunk (10 ms of idle GPU per 480x640 image)."""
        cached = getattr(self, "_steps_cache", None)
        if cached is None or cached[0] != self.n_samples or cached[1].device != dev:
            cached = (self.n_samples, torch.linspace(0.0, 1.0, self.n_samples).to(dev))
            self._steps_cache = cached
        return cached[1]

    def render(self, rays_o, rays_d, near, far, volumes, mask_volumes, imgs, features, match_features, intrs, c2ws, cos_anneal_ratio, step,
               scene=None, lean=False, t_rand=None, pts_random=None, extra_pts=None, extra_valid=None):
        if scene is None:
            scene = Scene(volumes, mask_volumes, imgs, features, match_features, intrs, c2ws)
        b = len(rays_o)
        dev = rays_o.device
        net = self._train_net(scene, lean)
        if self.perturb > 0 and t_rand is None and pts_random is None and self._train_fused_ok(scene, net, lean):
            t_rand, pts_random = self._host_draws(dev, b)          # both host draws of the step (:362, then :256) through one pinned copy
        rays_o, rays_d = rays_o.float().contiguous(), rays_d.float().contiguous()
        sample_dist = 2.0 / self.n_samples                                                  # unit-sphere assumption (:355)
        steps = self._coarse_steps(dev)
        if self.perturb > 0 and t_rand is None:
            t_rand = torch.rand([b, 1])                                                     # CPU generator, :362
        z_vals = ops.coarse_z(near, far, steps, t_rand.to(dev, non_blocking=True) if self.perturb > 0 else None, b)      # (:356-363, one launch)
        if self.n_importance > 0:
            # (the fused TRAINING path writes its mid-points into slices of the step's point array itself)
            z_vals = self._sample_rays(rays_o, rays_d, z_vals, scene, net, mid_points=None if self._train_fused_ok(scene, net, lean) else sample_dist)
        return self.render_core(rays_o, rays_d, z_vals, sample_dist, volumes, mask_volumes, features, match_features, imgs, intrs, c2ws,
                                cos_anneal_ratio, step, scene=scene, lean=lean, pts_random=pts_random, extra_pts=extra_pts, net=net,
                                extra_valid=extra_valid)

    # ----------------------------------------------------------------------------------------------------------
    # geometry + validation
    # ----------------------------------------------------------------------------------------------------------
    sparse_lattice = None          # brick edge of the two-level lattice (ops.sparse_lattice, K28); None: the dense lattice, True: SPARSE_BRICK
    lattice_lipschitz = 2.0        # assumed bound on |d sdf| per unit length between lattice points: twice the eikonal target.  A heuristic;
                                   # the leak count of every sparse call checks it and falls back to the dense lattice when it fails
    last_lattice_stats = None      # ops.sparse_lattice's stats of the last sdf_grid call (None: that call was dense)
    SPARSE_BRICK = 4               # what `sparse=True` means: the brick edge that measured best at 512^3 and 1024^3
    sparse_mesh = None             # True: extract_geometry runs marching cubes on the sparse lattice's bricks (ops.brick_marching_cubes, K29) and
                                   # builds no dense lattice; needs a sparse brick of 2 to 8 cells.  None / False: off
    mesh_attributes = None         # ("normals", "colors") or one of them: extract_geometry / validate also return per-vertex attributes
                                   # (vertex_attributes, K30).  None / (): off
    VERTEX_ATTRIBUTES = ("normals", "colors")
    mesh_simplify = None           # a cell edge in lattice spacings: extract_geometry / validate simplify the mesh on the device by quadric vertex
                                   # clustering (ops.simplify_mesh, K33) before attributes and read-back.  None / False / 0: off
    last_simplify_stats = None     # ops.simplify_mesh's stats of the last extract_geometry call (None: that call did not simplify)

    def _simplify_request(self, simplify):
        """The simplification a mesh call asks for (None: the attribute `mesh_simplify`) -> the cell edge in lattice spacings as a float, or
        None for off (None, False, 0).  ValueError, before anything is launched, for anything else that is not a positive finite number."""
        simplify = self.mesh_simplify if simplify is None else simplify
        if simplify is None or simplify is False or (not isinstance(simplify, bool) and isinstance(simplify, (int, float)) and simplify == 0):
            return None
        if isinstance(simplify, bool):
            raise ValueError("simplify = True: pass the cell edge in lattice spacings (a positive number; None, False or 0: off)")
        return ops.simplify_request("simplify", simplify)[0]

    mesh_simplify_error = None     # True or a dict of ops.mesh_distance's keywords (density, samples, max_dist, signed, sign, beta): extract_geometry / validate measure the
                                   # simplified mesh against the mesh it came from (K36) -> last_simplify_stats["error"].  None / False: off

    def _simplify_error_request(self, simplify_error, simplify):
        """The error measurement a mesh call asks for (None: the attribute `mesh_simplify_error`) beside its checked `simplify` -> a dict of
        ops.mesh_distance's keywords, or None for none.  ValueError for anything but None, a bool or such a dict, and when it is asked for
        with the simplification off."""
        simplify_error = self.mesh_simplify_error if simplify_error is None else simplify_error
        if simplify_error is None or simplify_error is False:
            return None
        if simplify_error is True:
            simplify_error = {}
        if not isinstance(simplify_error, dict):
            raise ValueError(f"simplify_error = {simplify_error!r}: True, or a dict of ops.mesh_distance's keywords (None or False: off)")
        unknown = sorted(set(simplify_error) - set(ops.MESH_DISTANCE_KEYS), key=str)
        if unknown:
            raise ValueError(f"simplify_error: unknown keyword {unknown[0]!r} (ops.mesh_distance's {', '.join(ops.MESH_DISTANCE_KEYS)})")
        ops.mesh_distance_keywords("simplify_error", simplify_error)
        if simplify is None:
            raise ValueError("simplify_error measures the simplified mesh against the extracted one: it needs simplify (a cell edge in lattice spacings)")
        return dict(simplify_error)

    mesh_topology = None           # True: extract_geometry / validate take the topology report of the mesh they return (ops.mesh_topology, K37) ->
                                   # last_mesh_topology.  None / False: off
    last_mesh_topology = None      # ops.MeshTopology.report() of the mesh the last extract_geometry call returned (None: that call did not ask)

    mesh_self_intersections = None       # True: extract_geometry / validate count the self-intersections of the mesh they return (ops.mesh_self_
                                         # intersections, K41) -> last_mesh_self_intersections.  None / False: off
    last_mesh_self_intersections = None  # the counts dict for the mesh the last extract_geometry call returned (None: that call did not ask)

    def _self_intersections_request(self, self_intersections):
        """The self-intersection report a mesh call asks for (None: the attribute `mesh_self_intersections`) -> bool.  ValueError for anything
        but None or a bool."""
        asked = self.mesh_self_intersections if self_intersections is None else self_intersections
        if asked is None:
            return False
        if not isinstance(asked, bool):
            raise ValueError(f"self_intersections = {asked!r}: True (None or False: off)")
        return asked

    def _topology_request(self, topology):
        """The topology report a mesh call asks for (None: the attribute `mesh_topology`) -> bool.  ValueError for anything but None or a bool."""
        topology = self.mesh_topology if topology is None else topology
        if topology is None:
            return False
        if not isinstance(topology, bool):
            raise ValueError(f"topology = {topology!r}: True (None or False: off)")
        return topology

    mesh_repair = None             # True or a dict of ops.repair_mesh's keywords (split, orient, min_component_faces, max_hole_edges, dedupe): extract_geometry /
                                   # validate repair the mesh on the device (K38) after the simplification -> last_repair_stats.  None / False: off
    last_repair_stats = None       # ops.repair_mesh's stats of the last extract_geometry call (None: that call did not repair)

    def _repair_request(self, repair):
        """The repair a mesh call asks for (None: the attribute `mesh_repair`) -> a dict of ops.repair_mesh's checked keywords, or None for
        off (None, False).  ValueError for anything but None, a bool or a dict that ops.repair_request accepts."""
        repair = self.mesh_repair if repair is None else repair
        if repair is None or repair is False:
            return None
        if repair is True:
            repair = {}
        if not isinstance(repair, dict) or not all(isinstance(k, str) for k in repair):
            raise ValueError(f"repair = {repair!r}: True, or a dict of ops.repair_mesh's keywords (None or False: off)")
        return ops.repair_request("repair", **repair)

    mesh_smooth = None             # True or a dict of ops.smooth_mesh's keywords (iterations, lam, mu, weights, fix_boundary, measure): extract_geometry /
                                   # validate smooth the mesh on the device (K39) after the repair -> last_smooth_stats.  None / False: off
    last_smooth_stats = None       # ops.smooth_mesh's stats of the last extract_geometry call, displacements in lattice spacings (None: that call did not smooth)

    def _smooth_request(self, smooth):
        """The smoothing a mesh call asks for (None: the attribute `mesh_smooth`) -> a dict of ops.smooth_mesh's checked keywords, or None
        for off (None, False).  ValueError for anything but None, a bool or a dict that ops.smooth_request accepts."""
        smooth = self.mesh_smooth if smooth is None else smooth
        if smooth is None or smooth is False:
            return None
        return ops.smooth_request(smooth, "smooth")

    mesh_texture = None            # the tile edge in texels (3 to 64), or a dict of texture_mesh's keywords (texels, snap, max_move, chunk):
                                   # extract_geometry / validate also return a texture atlas of the mesh (texture_mesh, K34).  None / False / 0:
                                   # off
    last_texture_stats = None      # H, W, samples, the unseen share and the snap counts of the last texture_mesh call
    _TEXTURE_KEYS = ("texels", "snap", "max_move", "threshold", "chunk")

    def _texture_option(self, texture):
        """The texture a mesh call asks for (None: the attribute `mesh_texture`) -> a dict of texture_mesh's keywords, or None for off (None,
        False, 0).  An integer is the tile edge `texels`.  ValueError for anything else."""
        texture = self.mesh_texture if texture is None else texture
        if texture is None or texture is False or (not isinstance(texture, bool) and isinstance(texture, (int, float)) and texture == 0):
            return None
        if isinstance(texture, dict):
            unknown = [k for k in texture if k not in self._TEXTURE_KEYS]
            if unknown:
                raise ValueError(f"texture: unknown keywords {unknown!r} (texture_mesh takes {self._TEXTURE_KEYS!r})")
            return dict(texture)
        if isinstance(texture, bool) or not isinstance(texture, (int, np.integer)):
            raise ValueError(f"texture = {texture!r}: the tile edge in texels (an integer from {ops.TEXTURE_MIN_TEXELS} to {ops.TEXTURE_MAX_TEXELS}), "
                             "a dict of texture_mesh's keywords, or None / False / 0 for off")
        return {"texels": int(texture)}

    def _texture_request(self, n_faces, volumes, views, texels=8, snap=0, max_move=None):
        """texture_mesh's arguments, checked before anything is launched -> (texels, snap, max_move).  n_faces: the face count, or None where
        the mesh does not exist yet (extract_geometry checks the rest first and the atlas once the mesh is known).  The limits on networks
        and views are _attribute_request's for "colors" (and for "normals" with a snap, which needs the gradient)."""
        ops.texture_layout(0, texels)                  # (ValueError for texels that is not an integer from 3 to 64)
        s = int(texels)
        if isinstance(snap, bool) or not isinstance(snap, (int, np.integer)) or snap < 0:
            raise ValueError(f"texture_mesh: snap = {snap!r}: the number of Newton rounds, an integer >= 0")
        if max_move is not None:
            if isinstance(max_move, bool) or not isinstance(max_move, (int, float, np.integer, np.floating)) or not float(max_move) > 0.0:
                raise ValueError(f"texture_mesh: max_move = {max_move!r}: a positive length (None: the longest edge of the texel's triangle)")
            max_move = float(max_move)
        if views is None:
            raise ValueError("texture_mesh needs the scene's views (views=scene.views): the colour is a function of the point and the views")
        self._attribute_request(("normals", "colors") if snap else ("colors",), volumes, views)
        if n_faces is not None:
            h, w = ops.texture_layout(n_faces, s)[:2]
            if h > ops.TEXTURE_MAX_EDGE or w > ops.TEXTURE_MAX_EDGE:
                fit = ops.texture_fit(n_faces)
                raise ValueError(f"texture_mesh: {n_faces} faces at texels = {s} need an atlas of {h} x {w} pixels, above {ops.TEXTURE_MAX_EDGE} a side; "
                                 + (f"the largest texels that fits is {fit}" if fit is not None else "no tile edge fits")
                                 + "; reduce the mesh first (extract_geometry(simplify=), ops.simplify_mesh)")
        return s, int(snap), max_move

    @torch.no_grad()
    def _texture_samples(self, pts, tri, vols, texels, snap, max_move, threshold, chunk):
        """The points of every atlas sample of the device mesh (pts (V, 3) float32, tri (T, 3) int32), after `snap` guarded Newton rounds ->
        (points (T P, 3) float32 on the device, steps skipped, steps turned back).  Per chunk snap + 1 value + gradient evaluations: each
        round's evaluation is also the guard of the round before (ops.texture_keep_better), and one more guards the last.  They run through
        _lattice_passes(want_grad=True): a split-half overflow repeats all of it from the unsnapped points in float32."""
        if not snap or not tri.shape[0]:
            return ops.texture_points(pts, tri, texels), 0, 0
        chunk = max(1, int(chunk))
        if self._fused_plan(vols) is None:
            raise ValueError("texture_mesh: snap needs the fused SDF kernels; these volumes do not take them")

        def run(evaluate):
            if max_move is None:
                samples, limit = ops.texture_points(pts, tri, texels, with_edge=True)
            else:
                samples, limit = ops.texture_points(pts, tri, texels), None
            skipped = torch.zeros((), device=samples.device, dtype=torch.int64)
            reverted = torch.zeros((), device=samples.device, dtype=torch.int64)
            for s in range(0, samples.shape[0], chunk):
                e = min(s + chunk, samples.shape[0])
                p, origin = samples[s:e], None
                for k in range(snap + 1):
                    sdf, grad = evaluate(p)[:2]
                    sdf = sdf.reshape(-1)
                    if origin is not None:                 # the step that led here did not lower |g|: back to its origin, with that state
                        reverted += ops.texture_keep_better(p, sdf, grad, *origin, threshold).sum()
                    if k == snap:
                        break
                    origin = (p.clone(), sdf, grad)
                    taken = ops.texture_snap(p, sdf, grad, threshold, limit=None if limit is None else limit[s:e], max_move=max_move)
                    skipped += (e - s) - taken.sum()
            return samples, skipped, reverted

        samples, skipped, reverted = self._lattice_passes(vols, None, run, want_grad=True)
        return samples, int(skipped), int(reverted)

    @torch.no_grad()
    def texture_mesh(self, points, triangles, volumes, views, texels=8, snap=0, max_move=None, threshold=0.0, chunk=1 << 21):
        """A texture atlas for a triangle mesh in the model's frame (K34): points (V,3) and triangles (T,3), numpy or
        tensors, from anywhere -- an extracted mesh, a simplified or cleaned one, a file (the points are evaluated as float32).  Every
        triangle gets texels (texels + 1) / 2 texels of an image whose resolution does not depend on the face count; each texel is coloured
        by the blending network at its point on the triangle, so the detail of the source images survives a coarse mesh.
        -> dict of numpy arrays: "texture" (H,W,3) uint8 (row 0 at the top; validate's img_fine convention, K30's rule), "texture_seen" (H,W)
        bool (some source view has the texel's point in its frustum; elsewhere, and where no triangle owns the texel, the colour is
        arbitrary / 0 and writers use mid-grey) and "texture_uv" (T,3,2) float32, one coordinate pair per corner, origin bottom-left
        (io.write_obj writes all three).  The layout is ops.texture_layout's: H = rows texels by W = cols (texels + 1).
        snap (default 0): Newton rounds that move each texel's point towards the surface sdf + threshold = 0 before it is coloured, for
        simplified meshes, whose faces are chords of the surface (a point off the surface projects into the source views with parallax).
        A step longer than max_move (default: the longest edge of the texel's triangle), or with a value or gradient that is not finite,
        is skipped, and a step after which |g| is not lower (as the evaluator sees it: each round's evaluation checks the round before,
        one more checks the last) is turned back, so no point ends with a larger |g| than it began with.  One or two rounds of Newton's
        method: NOTHING else is promised about convergence; self.last_texture_stats counts the skipped and the turned-back steps.  chunk: points per network launch; the result does not depend on it.
        Bilinear filtering inside a triangle reads that triangle's texels only.  Not promised: anything under mip-mapping, and seam-free
        colour across triangle edges (two triangles sample a shared edge at the same points only up to their different extrapolations).
        ValueError before any launch (_texture_request): texels outside 3 .. 64, snap < 0, max_move <= 0, an atlas edge above 16 384 pixels,
        missing views, or networks outside the fused kernels.  self.last_texture_stats: "H", "W", "samples", "unseen" (the share of owned
        texels no view sees), "snap", "snap_skipped", "snap_reverted"."""
        tri_host = triangles.detach() if torch.is_tensor(triangles) else np.asarray(triangles)
        if tri_host.ndim != 2 or tri_host.shape[1] != 3:
            raise ValueError(f"texture_mesh: triangles are {tuple(tri_host.shape)}, expected (T, 3)")
        n_faces = int(tri_host.shape[0])
        texels, snap, max_move = self._texture_request(n_faces, volumes, views, texels, snap, max_move)
        if not math.isfinite(float(threshold)):
            raise ValueError(f"texture_mesh: threshold = {threshold!r} (finite)")
        vols = volumes if isinstance(volumes, ops.VolumeSet) else ops.VolumeSet.packed(volumes)
        dev = vols.tensors[0].device
        pts = torch.as_tensor(points).detach().reshape(-1, 3).to(device=dev, dtype=torch.float32).contiguous()
        tri = torch.as_tensor(tri_host).to(device=dev, dtype=torch.int32).contiguous()
        if n_faces and (int(tri.min()) < 0 or int(tri.max()) >= pts.shape[0]):
            raise ValueError(f"texture_mesh: triangle indices {int(tri.min())} .. {int(tri.max())} outside the {pts.shape[0]} vertices")
        h, w, _, _, per_face = ops.texture_layout(n_faces, texels)
        atlas = torch.zeros(h, w, 3, device=dev, dtype=torch.uint8)
        seen = torch.zeros(h, w, device=dev, dtype=torch.uint8)
        samples, skipped, reverted = self._texture_samples(pts, tri, vols, texels, snap, max_move, float(threshold), chunk)
        self._point_chain(samples, vols, views, False, True, chunk, lambda s, e, grad, rgb, vis: ops.texture_pack(
            rgb, vis, n_faces, texels, s, e, atlas=atlas, seen=seen))
        uv = ops.texture_uv(n_faces, texels, dev)
        out = {"texture": atlas.cpu().numpy(), "texture_seen": seen.cpu().numpy().astype(bool), "texture_uv": uv.cpu().numpy()}
        n = n_faces * per_face
        self.last_texture_stats = {"H": h, "W": w, "samples": n, "unseen": 1.0 - float(out["texture_seen"].sum()) / n if n else 0.0,
                                   "snap": snap, "snap_skipped": skipped, "snap_reverted": reverted}
        return out

    def _lattice_route(self, sparse, sparse_mesh, shard):
        """The options of sdf_grid (sparse_mesh=False) and extract_geometry -> (route, brick edge): "dense" (the dense lattice, brick None),
        "lattice" (ops.sparse_lattice, K28) or "mesh" (ops.brick_marching_cubes, K29).  None = the attribute of that name; sparse False =
        dense, True = SPARSE_BRICK.  With a shard neither option is in effect: one warning each, and the brick limit of K29 is not looked at."""
        def unsharded(once, what):                     # -> the route with a shard
            if not getattr(self, once, False):
                import warnings
                warnings.warn(f"gens_amd: {what}", RuntimeWarning, stacklevel=4)
                setattr(self, once, True)
            return "dense", None

        sparse = self.sparse_lattice if sparse is None else sparse
        sparse_mesh = self.sparse_mesh if sparse_mesh is None else sparse_mesh
        off = sparse is None or sparse is False
        if sparse_mesh and off:
            raise ValueError("sparse_mesh needs the sparse lattice: pass sparse (a brick edge of 2 to 8 cells, or True) or set `sparse_lattice`")
        if off:
            return "dense", None
        if sparse_mesh and shard is not None:          # (before the brick is looked at: with a shard the option is not in effect)
            return unsharded("_warned_sparse_mesh_shard", "sparse_mesh is not sharded: with a shard the lattice is gathered and marching cubes runs on it")
        brick = self.SPARSE_BRICK if sparse is True else int(sparse)
        if sparse_mesh:
            if not 2 <= brick <= ops.BRICK_MC_MAX:
                raise ValueError(f"sparse_mesh: sparse = {sparse!r}, the brick-sparse marching cubes takes bricks of 2 to {ops.BRICK_MC_MAX} cells")
            return "mesh", brick
        if brick < 1:
            raise ValueError(f"sparse = {sparse!r}: the brick edge in cells, at least 1 (or True / None)")
        if shard is not None:
            return unsharded("_warned_sparse_shard", "the sparse lattice is not sharded: with a shard the dense lattice is evaluated")
        return "lattice", brick

    def _lattice_passes(self, vols, shard, run, want_grad=False):
        """run(evaluate) with the SDF evaluator of the mesh passes (the fused plan and this scene's precision, else the PyTorch layers) -> its
        result.  evaluate(pts) -> sdf, or (sdf, gradient) with want_grad (the fused plan only: vertex_attributes checks for it).  A
        split-half launch that met a value outside the half range repeats the WHOLE run in float32, like the image."""
        split_half = None
        for _ in range(2):
            def evaluate(pts):
                plan = self._fused_plan(vols)
                prec = "f32" if split_half is False else self._precision(plan, want_grad) if plan is not None else "f32"
                if want_grad:
                    return ops.sdf_mlp(plan, vols, pts, want_grad=True, precision=prec)
                return ops.sdf_mlp(plan, vols, pts, precision=prec) if plan is not None else self.sdf_network.sdf(pts, vols)

            out = run(evaluate)
            overflowed = split_half is not False and self._split_half_overflowed()
            if shard is not None and split_half is not False and self.sdf_precision == "f16x2":
                overflowed = shard.any(overflowed)
            if not overflowed:
                break
            split_half = False
        return out

    @torch.no_grad()
    def sdf_grid(self, volumes, bound_min, bound_max, resolution, chunk=1 << 21, shard=None, sparse=None, threshold=0.0):
        """u = -sdf on the resolution^3 lattice (:407-421), kept on the device.  shard (gens_amd.distributed.Shard): this rank evaluates
        the chunks `index mod world` and the slabs are gathered on every rank (None under Shard.single until the last shard arrives).
        sparse (a brick edge in cells, True for SPARSE_BRICK; default: the attribute `sparse_lattice`, None = off): the network is evaluated
        on every sparse-th point and inside the bricks that can hold the surface u = threshold, under the bound `lattice_lipschitz`
        (ops.sparse_lattice); marching cubes at `threshold` then returns the dense lattice's mesh.  Ignored with a shard."""
        vols = volumes if isinstance(volumes, ops.VolumeSet) else ops.VolumeSet.packed(volumes)
        dev = vols.tensors[0].device
        total = resolution ** 3
        n_chunks = -(-total // chunk)
        own = range(n_chunks) if shard is None else shard.chunks(n_chunks)
        brick = self._lattice_route(sparse, False, shard)[1]
        self.last_lattice_stats = None
        if brick is None:
            u = torch.zeros(len(own), chunk, device=dev) if shard is not None else torch.empty(total, device=dev)

        def run(evaluate):
            if brick is not None:                      # coarse and fine passes together; an overflow repeats both
                us, self.last_lattice_stats = ops.sparse_lattice(evaluate, bound_min.tolist(), bound_max.tolist(), resolution, threshold, brick,
                                                                 self.lattice_lipschitz, chunk=chunk, device=dev)
                return us.reshape(-1)
            for k, c in enumerate(own):
                first = c * chunk
                count = min(chunk, total - first)
                pts = ops.lattice_points(bound_min.tolist(), bound_max.tolist(), resolution, first, count, dev)
                sdf = evaluate(pts)
                if shard is not None:
                    u[k, :count] = -sdf[:, 0]
                else:
                    u[first:first + count] = -sdf[:, 0]
            return u

        u = self._lattice_passes(vols, shard, run)
        if shard is not None:
            u = shard.gather_chunks(u, n_chunks)
            if u is None:
                return None
            u = u.reshape(-1)[:total]
        return u.reshape(resolution, resolution, resolution)

    @torch.no_grad()
    def _brick_mesh(self, volumes, bound_min, bound_max, resolution, threshold, brick):
        """Vertices (index coordinates) and triangles on the device through ops.brick_marching_cubes; None if the leak count refutes the bound
        `lattice_lipschitz` and the dense lattice can still be built (the caller takes that route); RuntimeError if it cannot."""
        import warnings
        vols = volumes if isinstance(volumes, ops.VolumeSet) else ops.VolumeSet.packed(volumes)
        dev = vols.tensors[0].device
        lo, hi = bound_min.tolist(), bound_max.tolist()
        vertices, triangles, stats = self._lattice_passes(vols, None, lambda evaluate: ops.brick_marching_cubes(
            evaluate, lo, hi, resolution, threshold, brick, self.lattice_lipschitz, device=dev))
        self.last_lattice_stats = stats
        if not stats["leaks"]:
            return vertices, triangles
        dense_fits = resolution ** 3 < 1 << 31
        then = "extracting from the dense lattice instead" if dense_fits else "there is no dense lattice at this resolution"
        warnings.warn(ops.lattice_leak_message("sparse_mesh", stats["leaks"], threshold, self.lattice_lipschitz, resolution, brick, then),
                      RuntimeWarning, stacklevel=4)
        if not dense_fits:
            raise RuntimeError(f"sparse_mesh: {stats['leaks']} leaks at resolution {resolution}: the mesh would have holes, and {resolution}^3 points "
                               "are beyond the dense lattice (2^31): raise lattice_lipschitz")
        return None

    def _attribute_request(self, attributes, volumes, views):
        """The attributes a mesh call asks for (None: the attribute `mesh_attributes`; a name or a sequence of names) -> a tuple in the order
        of VERTEX_ATTRIBUTES, () for none.  Raises ValueError, before anything is launched, for what vertex_attributes cannot serve: an
        unknown name, colours without views, volumes or networks outside the fused kernels."""
        attributes = self.mesh_attributes if attributes is None else attributes
        if attributes is None:
            return ()
        names = (attributes,) if isinstance(attributes, str) else tuple(attributes)
        unknown = [a for a in names if a not in self.VERTEX_ATTRIBUTES]
        if unknown:
            raise ValueError(f"mesh attributes {unknown!r}: the known ones are {self.VERTEX_ATTRIBUTES!r}")
        names = tuple(a for a in self.VERTEX_ATTRIBUTES if a in names)
        if not names:
            return ()
        if "colors" in names and views is None:
            raise ValueError('mesh attributes: "colors" needs the scene\'s views (views=scene.views): the colour is a function of the point and the views')
        if "normals" in names:
            packed = isinstance(volumes, ops.VolumeSet)
            n_levels = volumes.n if packed else len(volumes)
            net = self.sdf_network
            if not 1 <= n_levels <= 5 or (packed and volumes.layout != 1):
                raise ValueError(f"mesh attributes: the fused SDF kernels take 1 to 5 packed volume levels, not {n_levels}"
                                 f"{'' if not packed or volumes.layout == 1 else ' planar ones'}; there is no other route for the normals")
            if not self.fused_sdf or not ops.SdfMlpPlan.supported(net) or net.init_feat_channels != 4 * n_levels:
                raise ValueError("mesh attributes: the normals need the fused SDF kernels (fused_sdf, the shipped SDF architecture, "
                                 f"init_feat_channels = 4 x {n_levels} levels)")
        if "colors" in names:
            if not isinstance(views, ops.SceneViews):
                raise ValueError("mesh attributes: views is the scene's ops.SceneViews (Scene.views)")
            with torch.no_grad():
                if self._fused_blend_plan(views) is None:
                    raise ValueError("mesh attributes: the colours need the fused blending kernel (fused_blend, the shipped colour network, at most "
                                     "5 feature levels that match its width)")
        return names

    @torch.no_grad()
    def vertex_attributes(self, points, volumes, views=None, attributes=("normals", "colors"), chunk=1 << 21):
        """Per-vertex attributes of a mesh in the model's frame.  points (V,3), numpy or tensor, float32 or float64 (evaluated as float32),
        from anywhere: an extracted mesh, a cleaned one, a file.  -> dict of numpy arrays, limited to what `attributes` names:
            "normals" (V,3) float32: grad sdf / |grad sdf| (zero rows where the gradient is zero or not finite) -- the shading normal;
            "colors"  (V,3) uint8:   the blending network's output at the point in validate's img_fine convention, trunc(clip(256 c, 0, 255));
            "seen"    (V,) bool (with "colors"): some source view has the point in its frustum; elsewhere the colour is arbitrary.
        Per chunk: ops.sdf_mlp(want_grad=True), ops.blend_views, ops.vertex_pack (K30).  The evaluator is the lattice's (_lattice_passes): this
        scene's precision, and a split-half overflow repeats the whole pass in float32.  No mask volume is consulted (the lattice is not
        masked either).  ValueError before any launch where the fused kernels do not apply (_attribute_request): there is no slow route."""
        names = self._attribute_request(attributes, volumes, views)
        vols = volumes if isinstance(volumes, ops.VolumeSet) else ops.VolumeSet.packed(volumes)
        dev = vols.tensors[0].device
        pts = torch.as_tensor(points).detach().reshape(-1, 3).to(device=dev, dtype=torch.float32).contiguous()
        n = pts.shape[0]
        want_n, want_c = "normals" in names, "colors" in names
        normals = torch.empty(n, 3, device=dev, dtype=torch.float32) if want_n else None
        colors = torch.empty(n, 3, device=dev, dtype=torch.uint8) if want_c else None
        seen = torch.empty(n, device=dev, dtype=torch.uint8) if want_c else None
        if names:
            self._point_chain(pts, vols, views, want_n, want_c, chunk, lambda s, e, grad, rgb, vis: ops.vertex_pack(
                grad, rgb, vis, normals=normals[s:e] if want_n else None, colors=colors[s:e] if want_c else None, seen=seen[s:e] if want_c else None))
        out = {}
        if want_n:
            out["normals"] = normals.cpu().numpy()
        if want_c:
            out["colors"] = colors.cpu().numpy()
            out["seen"] = seen.cpu().numpy().astype(bool)
        return out

    def _point_chain(self, pts, vols, views, want_n, want_c, chunk, sink):
        """The network chain of vertex_attributes and render_surface on device points (n, 3) float32, `chunk` at a time:
        ops.sdf_mlp(want_grad=True) (want_n) and ops.blend_views (want_c), then sink(s, e, grad, rgb, vis) for the rows s .. e - 1 (None for
        what was not asked for).  The evaluator is _lattice_passes': a split-half overflow repeats the whole pass, sinks included, in float32."""
        n, chunk = pts.shape[0], max(1, int(chunk))
        if want_n and self._fused_plan(vols) is None:      # (what _attribute_request could not see before the volumes were packed)
            raise ValueError("mesh attributes: the normals need the fused SDF kernels; these volumes do not take them")
        bplan = self._fused_blend_plan(views) if want_c else None

        def run(evaluate):
            for s in range(0, n, chunk):
                e = min(s + chunk, n)
                grad = evaluate(pts[s:e])[1] if want_n else None
                rgb, vis = ops.blend_views(bplan, views, pts[s:e]) if want_c else (None, None)
                sink(s, e, grad, rgb, vis)

        if n and (want_n or want_c):
            if want_n:
                self._lattice_passes(vols, None, run, want_grad=True)
            else:
                run(None)

    surface_render = None          # validate also traces its rays to the surface (render_surface, K31) and returns surface_depth, surface_normal_img,
                                   # surface_img and surface_hit.  None / False: off; True: every output; or a dict of render_surface's keywords
                                   # (outputs, resolution, lipschitz, min_step, max_steps, refine)
    last_surface_stats = None      # ops.sphere_trace's stats of the last render_surface call
    SURFACE_OUTPUTS = ("depth", "normals", "colors")

    def _surface_request(self, outputs, volumes, views, resolution, lipschitz, min_step, max_steps, refine, bound_min, bound_max):
        """render_surface's arguments, checked before anything is launched -> (outputs in the order of SURFACE_OUTPUTS, lipschitz, min_step,
        max_steps, refine).  The limits of the normals and colours are _attribute_request's."""
        names = (outputs,) if isinstance(outputs, str) else tuple(outputs)
        unknown = [a for a in names if a not in self.SURFACE_OUTPUTS]
        if unknown:
            raise ValueError(f"surface outputs {unknown!r}: the known ones are {self.SURFACE_OUTPUTS!r}")
        names = tuple(a for a in self.SURFACE_OUTPUTS if a in names)
        if not names:
            raise ValueError(f"surface outputs: at least one of {self.SURFACE_OUTPUTS!r}")
        self._attribute_request(("normals",) + tuple(a for a in names if a == "colors"), volumes, views)     # (the trace itself needs the fused SDF plan)
        lipschitz = float(self.lattice_lipschitz if lipschitz is None else lipschitz)
        if not lipschitz > 0.0 or lipschitz == float("inf"):
            raise ValueError(f"render_surface: lipschitz = {lipschitz!r}, a positive finite bound")
        if min_step is None:
            if int(resolution) < 2:
                raise ValueError(f"render_surface: resolution = {resolution}, at least 2 points per axis")
            lo, hi = bound_min.tolist(), bound_max.tolist()
            min_step = min((float(b) - float(a)) / (int(resolution) - 1) for a, b in zip(lo, hi))
        min_step = float(min_step)
        if not min_step > 0.0 or min_step == float("inf"):
            raise ValueError(f"render_surface: min_step = {min_step!r}, a positive finite length")
        if int(max_steps) < 1:
            raise ValueError(f"render_surface: max_steps = {max_steps}, at least 1")
        if int(refine) < 0:
            raise ValueError(f"render_surface: refine = {refine}, at least 0")
        return names, lipschitz, min_step, int(max_steps), int(refine)

    @torch.no_grad()
    def render_surface(self, rays_o, rays_d, near, far, volumes, bound_min, bound_max, c2ws, views=None, outputs=("depth", "normals", "colors"),
                       resolution=512, threshold=0.0, chunk=1 << 21, lipschitz=None, min_step=None, max_steps=256, refine=2, hw=None):
        """The surface sdf + threshold = 0 as the rays see it, by sphere tracing (ops.sphere_trace, K31): per ray one
        value evaluation per march round while it is LIVE, `refine` more on its bracket, and at a hit one value + gradient and one blend
        evaluation -- validate's volume rendering takes 128 of each.  rays_o / rays_d (n, 3) or (H, W, 3), near / far (one value or one per
        ray), bound_min / bound_max: device tensors; c2ws: the scene's poses (rot = inverse(c2ws[0][:3,:3]), the rotation validate's normal
        image uses); views: the scene's ops.SceneViews, needed for "colors".
        lipschitz (default: the attribute `lattice_lipschitz`): the assumed bound on |d sdf| per unit length, the heuristic of the sparse
        lattice -- a steeper field can be stepped through.  min_step (default: the smallest spacing of a `resolution`-point lattice over the
        box, so the map is bracketed as finely as that mesh's cells): a sheet thinner than it can be stepped over.
        -> dict of host arrays shaped (H, W, ...) by hw or the rays' own leading shape, else flat:
            "t", "status" (uint8, ops.TRACE_*), "steps", "hit" (bool)   always;
            "depth" float32: t (rot d)_z at a hit, else 0;
            "normal" (.., 3) float32 unit grad sdf and "normal_img" (.., 3) float32 in validate's normal_img convention ("normals");
            "img" (.., 3) uint8 in validate's img_fine convention and "seen" bool ("colors").  Everything is 0 where the ray is not a hit.
        INSIDE and EXHAUSTED rays are counted in self.last_surface_stats (ops.sphere_trace's stats), not hidden.  The evaluator is the
        lattice's (_lattice_passes): this scene's sdf_precision, and a split-half overflow repeats the whole trace in float32; no mask
        volume is consulted.  ValueError before any launch for what _attribute_request refuses and for a bad lipschitz / min_step / max_steps."""
        shape = tuple(int(v) for v in hw) if hw is not None else tuple(rays_o.shape[:-1])
        out = self._trace_surface(rays_o, rays_d, near, far, volumes, bound_min, bound_max, c2ws, views, outputs, resolution, threshold, chunk,
                                  lipschitz, min_step, max_steps, refine)
        return {k: v.cpu().numpy().reshape(shape + tuple(v.shape[1:])) for k, v in out.items()}

    @torch.no_grad()
    def _trace_surface(self, rays_o, rays_d, near, far, volumes, bound_min, bound_max, c2ws, views, outputs, resolution, threshold, chunk, lipschitz,
                       min_step, max_steps, refine):
        """render_surface on the device: its arguments -> its dict as flat per-ray device tensors (nothing is copied to the host but the
        counts the trace reads anyway); self.last_surface_stats as render_surface leaves it."""
        names, lipschitz, min_step, max_steps, refine = self._surface_request(outputs, volumes, views, resolution, lipschitz, min_step, max_steps,
                                                                              refine, bound_min, bound_max)
        vols = volumes if isinstance(volumes, ops.VolumeSet) else ops.VolumeSet.packed(volumes)
        o, d = rays_o.reshape(-1, 3), rays_d.reshape(-1, 3)
        lo, hi = bound_min.tolist(), bound_max.tolist()
        traced, stats = self._lattice_passes(vols, None, lambda evaluate: ops.trace_rays(
            evaluate, o, d, near, far, lo, hi, lipschitz, min_step, max_steps, refine, threshold, chunk))
        self.last_surface_stats = stats
        want_n, want_c = "normals" in names, "colors" in names
        # the nine floats validate's normal image uses, from the same set-up launch (the rotation does not depend on the intrinsics: unit ones)
        rot = ops.SceneCams(torch.eye(4, device=c2ws.device).expand(c2ws.shape[0], 4, 4).contiguous(), c2ws).rot_inv
        packed = ops.surface_pack(traced["status"], traced["t"], d, rot)
        if (want_n or want_c) and stats["hit"]:
            hits = ops.compact_valid(traced["status"] == ops.TRACE_HIT)[0][:stats["hit"]]
            pts = ops.trace_gather(traced["points"], hits, stats["hit"])
            self._point_chain(pts, vols, views, want_n, want_c, chunk, lambda s, e, grad, rgb, vis: ops.surface_pack(
                traced["status"], traced["t"], d, rot, grad, rgb, vis, index=hits[s:e], out=packed))
        n = o.shape[0]
        out = {"t": traced["t"], "status": traced["status"], "steps": traced["steps"], "hit": packed["hit"].bool(), "depth": packed["depth"]}
        if want_n:
            out["normal"] = packed.get("normal", torch.zeros(n, 3, device=o.device))
            out["normal_img"] = packed.get("normal_img", torch.zeros(n, 3, device=o.device))
        if want_c:
            out["img"] = packed.get("img", torch.zeros(n, 3, device=o.device, dtype=torch.uint8))
            out["seen"] = packed.get("seen", torch.zeros(n, device=o.device, dtype=torch.uint8)).bool()
        if "depth" not in names:
            del out["depth"]
        return out

    mesh_render = None             # validate also casts its rays at the mesh it extracted (render_mesh, K35) and returns mesh_depth, mesh_normal_img,
                                   # mesh_img and mesh_hit (and mesh_fidelity beside surface_render).  None / False: off; True: on; or a dict of
                                   # render_mesh's keywords (shading, chunk)
    last_mesh_render_stats = None  # rays, hits, grid cells and faces of the last render_mesh call
    _MESH_RENDER_KEYS = ("shading", "chunk")

    def _mesh_render_option(self, mesh_render):
        """The mesh render validate asks for (None: the attribute `mesh_render`) -> a dict of render_mesh's keywords, or None for off."""
        mesh_render = self.mesh_render if mesh_render is None else mesh_render
        if mesh_render is None or mesh_render is False:
            return None
        if mesh_render is True:
            return {}
        if not isinstance(mesh_render, dict):
            raise ValueError(f"mesh_render = {mesh_render!r}: None / False, True, or a dict of {self._MESH_RENDER_KEYS!r}")
        unknown = [k for k in mesh_render if k not in self._MESH_RENDER_KEYS]
        if unknown:
            raise ValueError(f"mesh_render: unknown keywords {unknown!r}: the known ones are {self._MESH_RENDER_KEYS!r}")
        if mesh_render.get("shading", "flat") not in ops.MESH_SHADINGS:
            raise ValueError(f"mesh_render: shading = {mesh_render['shading']!r}: one of {ops.MESH_SHADINGS!r}")
        return dict(mesh_render)

    @torch.no_grad()
    def render_mesh(self, points, triangles, rays_o, rays_d, c2ws, normals=None, colors=None, seen=None, texture=None, texture_seen=None,
                    texels=None, shading="flat", hw=None, chunk=None):
        """A triangle mesh in the model's frame as the rays see it (K35): the counterpart of render_surface for the
        asset that is written to disk.  points (V, 3) and triangles (T, 3), rays_o / rays_d (n, 3) or (H, W, 3), c2ws: numpy arrays or
        tensors, from anywhere -- an extracted, simplified, cleaned or read mesh; everything is moved to the device of this module's
        parameters (rays and poses that are device tensors already decide it).  It needs no volumes and no network.
        normals (V, 3), colors (V, 3) uint8, seen (V): vertex_attributes' dict; texture (H, W, 3) uint8, texture_seen, texels:
        texture_mesh's atlas of this very mesh and the tile edge it was made with (default: read off the atlas' shape) -- the atlas is used
        where given, else the vertex colours, else only depth and normals are produced.  shading "flat" (the face's normal) or "smooth"
        (the vertex normals interpolated; needs `normals`).  rot = inverse(c2ws[0][:3,:3]), as validate and render_surface form it.
        -> dict of host arrays shaped (H, W, ...) by hw or the rays' own leading shape, else flat: "face" int32 (-1: miss), "t" float32
        (+inf: miss), "hit" bool, "bary" (.., 3), "depth" = t (rot d)_z, "normal" (.., 3), "normal_img" (.., 3) float32 in validate's
        convention, and with colours "img" (.., 3) uint8, with their flags "seen" bool.  Everything is 0 where the ray misses the mesh.
        One sample per ray: no anti-aliasing, mip-maps or lighting.  self.last_mesh_render_stats: "rays", "hits", "cells", "faces"."""
        shape = tuple(int(v) for v in hw) if hw is not None else tuple(rays_o.shape[:-1])
        out = self._render_mesh(points, triangles, rays_o, rays_d, c2ws, normals, colors, seen, texture, texture_seen, texels, shading, chunk)
        out["hit"] = out["hit"].bool()
        if "seen" in out:
            out["seen"] = out["seen"].bool()
        return {k: v.cpu().numpy().reshape(shape + tuple(v.shape[1:])) for k, v in out.items()}

    @torch.no_grad()
    def _render_mesh(self, points, triangles, rays_o, rays_d, c2ws, normals, colors, seen, texture, texture_seen, texels, shading, chunk):
        """render_mesh on the device: its arguments -> ops.render_mesh's dict of flat per-ray device tensors."""
        dev = next((t.device for t in (rays_o, rays_d, c2ws, points) if torch.is_tensor(t) and t.is_cuda), None)
        if dev is None:
            dev = next(self.parameters()).device
        tri = torch.as_tensor(triangles)
        if tri.dim() != 2 or tri.shape[1] != 3:
            raise ValueError(f"render_mesh: triangles are {tuple(tri.shape)}, expected (T, 3)")
        if shading not in ops.MESH_SHADINGS:
            raise ValueError(f"render_mesh: shading = {shading!r}: one of {ops.MESH_SHADINGS!r}")
        if shading == "smooth" and normals is None:
            raise ValueError("render_mesh: smooth shading needs the vertex normals")
        if seen is not None and colors is None:
            raise ValueError("render_mesh: seen flags come with the vertex colours")
        if texture_seen is not None and texture is None:
            raise ValueError("render_mesh: texture_seen without a texture")
        n_faces = int(tri.shape[0])
        if texture is not None:
            tex_shape = tuple(texture.shape)
            if texels is None:
                texels = ops.atlas_texels(n_faces, tex_shape)
            if ops.texture_layout(n_faces, texels)[:2] + (3,) != tex_shape:
                raise ValueError(f"render_mesh: a texture of {tex_shape} for {n_faces} triangles with texels = {texels}: expected "
                                 f"{ops.texture_layout(n_faces, texels)[:2] + (3,)}")
        if not torch.is_tensor(c2ws) and np.asarray(c2ws).shape[-2:] != (4, 4):
            raise ValueError(f"render_mesh: c2ws are {np.asarray(c2ws).shape}, expected (nv, 4, 4)")
        up = lambda v, dtype, cols: None if v is None else torch.as_tensor(v).detach().to(device=dev).reshape((-1,) + cols).to(dtype).contiguous()  # noqa: E731
        f32, u8 = torch.float32, torch.uint8
        c2ws = up(c2ws, f32, (4, 4))
        o, d = up(rays_o, f32, (3,)), up(rays_d, f32, (3,))
        grid = ops.build_mesh_grid(up(points, torch.float64, (3,)), up(tri, torch.int32, (3,)))
        rot = ops.SceneCams(torch.eye(4, device=dev).expand(c2ws.shape[0], 4, 4).contiguous(), c2ws).rot_inv
        if texture is not None:
            texture = torch.as_tensor(texture).detach().to(device=dev, dtype=u8).contiguous()
            texture_seen = None if texture_seen is None else torch.as_tensor(texture_seen).detach().to(device=dev).to(u8).contiguous()
        out = ops.render_mesh(None, None, o, d, rot, grid=grid, chunk=chunk, normals=up(normals, f32, (3,)), colors=up(colors, u8, (3,)),
                              seen=up(seen, u8, ()), texture=texture, texture_seen=texture_seen, texels=texels, shading=shading)
        self.last_mesh_render_stats = {"rays": int(o.shape[0]), "hits": int(out["hit"].sum()), "faces": n_faces,
                                       "cells": grid.dims[0] * grid.dims[1] * grid.dims[2]}
        return out

    surface_fusion = None          # validate also fuses the sphere-traced depth maps of the item's views into a point cloud (fuse_surface, K32) and
                                   # returns fused_points, fused_normals, fused_colors and fused_seen.  None / False: off; True: on; or a dict of
                                   # fuse_surface's keywords (pairs, pix_tol, rel_tol, min_views, normal_cos, dedupe_radius, and render_surface's)
                                   # 
    last_fusion_stats = None       # per view: usable and kept pixels, the votes histogram and the trace stats of the last fuse_surface call
    _FUSION_KEYS = ("pix_tol", "rel_tol", "min_views", "normal_cos")
    _FUSION_TRACE_KEYS = ("resolution", "threshold", "chunk", "lipschitz", "min_step", "max_steps", "refine")

    @staticmethod
    def view_rays(intrs, c2ws, v, hw):
        """The rays of every pixel of view v, formed on the device of intrs / c2ws with synthetic.make_rays' arithmetic (dtu.py:390-403):
        pixel (x, y), integers, is the ray through K^-1 [x, y, 1], normalised and rotated by the pose -> (rays_o, rays_d) (H W, 3) float32."""
        h, w = int(hw[0]), int(hw[1])
        dev = c2ws.device
        py, px = torch.meshgrid(torch.linspace(0, h - 1, h, device=dev), torch.linspace(0, w - 1, w, device=dev), indexing="ij")
        px, py = px.reshape(-1), py.reshape(-1)
        p = torch.stack([px, py, torch.ones_like(py)], dim=-1)
        p = (torch.inverse(intrs[v, :3, :3].float())[None] @ p[:, :, None])[:, :, 0]
        d = p / torch.linalg.norm(p, dim=-1, keepdim=True)
        rays_d = (c2ws[v, :3, :3].float()[None] @ d[:, :, None])[:, :, 0]
        rays_o = c2ws[v, :3, 3].float()[None].expand_as(rays_d).contiguous()
        return rays_o, rays_d.contiguous()

    @torch.no_grad()
    def fuse_surface(self, volumes, intrs, c2ws, hw, bound_min, bound_max, views=None, pairs=None, near=None, far=None,
                     attributes=("normals", "colors"), dedupe_radius=None, **keywords):
        """The surface as a fused point cloud (K32): every view of the scene is traced to the surface (render_surface's
        machinery with that view's pose, so the depth is the view's own z-depth), the maps stay on the device, and a pixel is kept when at
        least min_views of the views `pairs` lists for it confirm its surface point (ops.fuse_depth_maps); the kept pixels are averaged with
        their voters and lifted (ops.fused_points).  intrs, c2ws (nv, 4, 4) device tensors, hw = (H, W); views: the scene's ops.SceneViews,
        needed for "colors"; near (default 0) / far (default: the largest distance from a camera centre to a corner of the box, so that the
        slab test alone bounds a ray): one value each.  keywords: ops.fuse_depth_maps' pix_tol, rel_tol, min_views, normal_cos (needs
        "normals") and render_surface's resolution, threshold, chunk, lipschitz, min_step, max_steps, refine.
        -> dict of host arrays: "points" (N, 3) float64, "view" (N,) int32 and "pixel" (N,) int64 (the flat index (view H + y) W + x), and
        "normals" (N, 3) float32 / "colors" (N, 3) uint8 with "seen" (N,) bool as `attributes` names them.  A surface point is emitted by
        every view that keeps it unless dedupe_radius thins the cloud (ops.fused_points).  Where "seen" is False no source view has the
        point in its frustum and the colour is arbitrary: the point stays, writers colour it mid-grey.  self.last_fusion_stats: per view
        "usable", "kept", "votes" (histogram, index = votes) and "trace" (ops.sphere_trace's stats), and "points".
        ValueError before any launch for what _attribute_request, _surface_request and ops.fuse_depth_maps refuse."""
        unknown = [k for k in keywords if k not in self._FUSION_KEYS + self._FUSION_TRACE_KEYS]
        if unknown:
            raise TypeError(f"fuse_surface: unknown keywords {unknown!r}")
        fusion_kw = {k: keywords[k] for k in self._FUSION_KEYS if k in keywords}
        trace_kw = {"resolution": 512, "threshold": 0.0, "chunk": 1 << 21, "lipschitz": None, "min_step": None, "max_steps": 256, "refine": 2,
                    **{k: keywords[k] for k in self._FUSION_TRACE_KEYS if k in keywords}}
        names = self._attribute_request(attributes, volumes, views) if attributes is not None else ()
        outputs = ("depth",) + names
        self._surface_request(outputs, volumes, views, trace_kw["resolution"], trace_kw["lipschitz"], trace_kw["min_step"], trace_kw["max_steps"],
                              trace_kw["refine"], bound_min, bound_max)
        h, w = int(hw[0]), int(hw[1])
        if h < 1 or w < 1:
            raise ValueError(f"fuse_surface: hw = {tuple(hw)!r}")
        cams = ops.fusion_cams(intrs, c2ws)
        nv = cams.shape[0]
        want_n, want_c = "normals" in names, "colors" in names
        pairs, pix_tol, rel_tol, min_views, normal_cos = ops.fusion_request(
            "fuse_surface", nv, pairs, fusion_kw.get("pix_tol", 1.0), fusion_kw.get("rel_tol", 0.01), fusion_kw.get("min_views", 3), want_n,
            fusion_kw.get("normal_cos"))
        dedupe_radius = ops._radius("fuse_surface", dedupe_radius)
        if nv * h * w >= 2 ** 31:
            raise ValueError(f"fuse_surface: {nv} maps of {h} x {w} pixels (nv H W below 2^31)")
        dev = c2ws.device
        lo, hi = bound_min.detach().double().cpu(), bound_max.detach().double().cpu()
        near = torch.full((1,), 0.0 if near is None else float(near), device=dev)
        if far is None:
            corners = torch.stack([torch.stack([(lo, hi)[(i >> a) & 1][a] for a in range(3)]) for i in range(8)])
            far = float((corners[None] - torch.as_tensor(cams[:, 21:])[:, None]).norm(dim=-1).max())
        far = torch.full((1,), float(far), device=dev)
        depth = torch.empty(nv, h, w, device=dev)
        normal = torch.empty(nv, h, w, 3, device=dev) if want_n else None
        img = torch.empty(nv, h, w, 3, device=dev, dtype=torch.uint8) if want_c else None
        seen = torch.empty(nv, h, w, device=dev, dtype=torch.bool) if want_c else None
        trace_stats = []
        for v in range(nv):
            o, d = self.view_rays(intrs, c2ws, v, (h, w))
            maps = self._trace_surface(o, d, near, far, volumes, bound_min, bound_max, c2ws[[v]], views, outputs, trace_kw["resolution"],
                                       trace_kw["threshold"], trace_kw["chunk"], trace_kw["lipschitz"], trace_kw["min_step"],
                                       trace_kw["max_steps"], trace_kw["refine"])
            trace_stats.append(self.last_surface_stats)
            depth[v] = maps["depth"].view(h, w)
            if want_n:
                normal[v] = maps["normal"].view(h, w, 3)
            if want_c:
                img[v], seen[v] = maps["img"].view(h, w, 3), maps["seen"].view(h, w)
        votes, keep, fused = ops.fuse_depth_maps(depth, cams, pairs, pix_tol, rel_tol, min_views, normal if normal_cos is not None else None,
                                                 normal_cos)
        points, normals, colors, pixel = ops.fused_points(fused, cams, keep, normal, img, dedupe_radius)
        usable = (torch.isfinite(depth) & (depth > 0)).view(nv, -1).sum(dim=1).tolist()
        kept = keep.view(nv, -1).sum(dim=1).tolist()
        hist = [torch.bincount(votes[v].reshape(-1).long(), minlength=pairs.shape[1] + 1).tolist() for v in range(nv)]
        self.last_fusion_stats = {"points": int(points.shape[0]), "views": [
            {"usable": int(usable[v]), "kept": int(kept[v]), "votes": hist[v], "trace": trace_stats[v]} for v in range(nv)]}
        out = {"points": points.cpu().numpy(), "view": (pixel // (h * w)).to(torch.int32).cpu().numpy(), "pixel": pixel.cpu().numpy()}
        if want_n:
            out["normals"] = normals.cpu().numpy()
        if want_c:
            out["colors"] = colors.cpu().numpy()
            out["seen"] = seen.view(-1)[pixel].cpu().numpy()
        return out

    def extract_geometry(self, volumes, bound_min, bound_max, resolution, threshold, shard=None, sparse=None, sparse_mesh=None, attributes=None,
                         views=None, simplify=None, texture=None, simplify_error=None, topology=None, repair=None, smooth=None,
                         self_intersections=None):
        """-> vertices (V,3) float64, triangles (T,3) int32 as numpy arrays (implicit_surface.py:407-427).  The SDF lattice and
        the marching cubes both run on the device (the reference: 512 D2H copies + PyMCubes on the host); only the mesh is copied.
        sparse: sdf_grid's option of that name, with this call's threshold.  sparse_mesh (default: the attribute of that name, None = off):
        together with a sparse brick of 2 to 8 cells, marching cubes runs on the bricks (ops.brick_marching_cubes) and no dense lattice is
        built -- the same mesh, resolutions beyond 1290 included.  A leak count above zero warns and takes the dense lattice (RuntimeError
        where resolution^3 >= 2^31 leaves none); with a shard the option is ignored with one warning.
        attributes (default: the attribute `mesh_attributes`, None / () = off): "normals", "colors" or both -> a third result, the dict of
        vertex_attributes at the float32 rounding of the returned vertices (formed on the device, gens_vertex_points, before the mesh is
        copied); views: the scene's ops.SceneViews, needed for the colours.  The same pass on every route, the leak fallback included; with a
        shard, on every rank that holds the gathered mesh.
        simplify (default: the attribute `mesh_simplify`; None, False or 0 = off): a cell edge in lattice spacings.  The device-resident mesh
        is simplified by quadric vertex clustering (ops.simplify_mesh, K33) in index coordinates with origin (-0.5, -0.5, -0.5), so that for
        whole-number edges lattice points are interior to cells -- after marching cubes on every route, the leak fallback included, before
        the attribute pass (normals and colours are evaluated at the new vertices, not carried) and before the copy to the host; with a shard,
        on every rank that holds the gathered mesh.  self.last_simplify_stats: its counts (None when off).  Topology is not preserved and no
        distance to the surface is promised.  ValueError before any launch for a cell edge that is not a positive
        finite number.
        simplify_error (default: the attribute `mesh_simplify_error`; None or False = off): True, or a dict of ops.mesh_distance's keywords
        (density, samples, max_dist).  The device-resident mesh from before the simplification is kept until after it and the two are
        compared in index coordinates (ops.mesh_distance with A = the extracted mesh, B = the simplified one; K36): the dict goes into
        self.last_simplify_stats["error"], in lattice spacings -- b_to_a.max bounds how far a simplified vertex is from the extracted surface,
        a_to_b what of that surface the simplified mesh lost.  Off: nothing is kept or launched and the stats have no such key.  ValueError
        before any launch for another value, unknown or bad keywords, or when simplify is off.  With "signed": True in the dict each
        direction also holds signed_mean, inside and no_sign (K37): whether the simplification shrinks or inflates the surface.
        topology (default: the attribute `mesh_topology`; None or False = off): True -> self.last_mesh_topology holds
        ops.mesh_topology(...).report() of the mesh this call returns (K37: edges by class, closed / oriented / manifold / watertight, Euler
        characteristic, genus, components, boundary loops, pinched vertices; area and volume in lattice spacings), taken on the
        device-resident mesh after the simplification and before the read-back, on every route; with simplify also on,
        self.last_simplify_stats["topology_before"] holds the report of the mesh before it.  Off: nothing is launched and
        last_mesh_topology is None.  ValueError before any launch for another value.
        self_intersections (default: the attribute `mesh_self_intersections`; None or False = off): True -> self.last_mesh_self_intersections
        holds the counts of ops.mesh_self_intersections for the mesh this call returns (K41: candidate pairs of faces, how many intersect,
        how many are undecided, degenerate and uncertain faces), taken where the topology report is taken, after
        simplify / repair / smooth; with simplify, repair or smooth on, that stage's stats also hold "self_intersections_before", the
        counts of the mesh before it, so a stage that introduces intersections shows it.  Off: nothing is launched and
        last_mesh_self_intersections is None.  ValueError before any launch for another value.
        repair (default: the attribute `mesh_repair`; None or False = off): True, or a dict of ops.repair_mesh's keywords (split, orient,
        min_component_faces, max_hole_edges, dedupe).  The device-resident mesh is repaired (K38: duplicate faces dropped, pinches and
        non-manifold edges split, small components dropped, components re-oriented, small holes closed) after the simplification and its
        simplify_error comparison and before the topology report, the attribute pass, the texture pass and the read-back, so that
        last_mesh_topology, the attributes and the atlas are those of the mesh this call returns.  self.last_repair_stats: its counts and,
        with topology on, "topology_before", the report of the mesh before the repair.  Off: nothing is launched, last_repair_stats is None
        and the mesh is what it was.  ValueError before any launch for another value or what ops.repair_request refuses.
        smooth (default: the attribute `mesh_smooth`; None or False = off): True, or a dict of ops.smooth_mesh's keywords (iterations, lam,
        mu, weights, fix_boundary, measure).  The device-resident mesh is smoothed in index coordinates (K39: Taubin's lambda | mu steps,
        or plain Laplacian ones with mu = 0; the triangles are untouched) after the simplification, its simplify_error comparison and the
        repair, and before the topology report, the attribute pass, the texture pass and the read-back, so that normals, colours, atlas and
        report are those of the mesh this call returns.  self.last_smooth_stats: ops.smooth_mesh's stats, displacements in lattice
        spacings.  Off: nothing is launched, last_smooth_stats is None and the mesh is what it was.  ValueError before any launch for
        what ops.smooth_request refuses.
        texture (default: the attribute `mesh_texture`; None, False or 0 = off): the tile edge in texels (3 to 64) or a dict of texture_mesh's
        keywords (texels, snap, max_move, chunk) -> a further result after the attribute dict (whose place holds None when only the
        texture is asked for): texture_mesh's dict for the returned mesh (K34), computed after marching cubes and
        the simplification on the device-resident mesh, where the attribute pass runs (with a shard, on every rank that holds the gathered
        mesh); this call's threshold unless the dict names one.  views is needed.  ValueError before any launch for what _texture_request
        refuses; the atlas edge (at most 16 384 pixels) can only be checked once the mesh exists, before any texture launch."""
        attributes = self._attribute_request(attributes, volumes, views)
        simplify = self._simplify_request(simplify)
        simplify_error = self._simplify_error_request(simplify_error, simplify)
        topology = self._topology_request(topology)
        self_intersections = self._self_intersections_request(self_intersections)
        repair = self._repair_request(repair)
        smooth = self._smooth_request(smooth)
        texture = self._texture_option(texture)
        if texture is not None:
            texture = {"threshold": threshold, **texture}
            self._texture_request(None, volumes, views, *(texture.get(k, d) for k, d in (("texels", 8), ("snap", 0), ("max_move", None))))
        self.last_simplify_stats = None
        self.last_mesh_topology = None
        self.last_mesh_self_intersections = None
        self.last_repair_stats = None
        self.last_smooth_stats = None
        route, brick = self._lattice_route(sparse, sparse_mesh, shard)
        mesh = None
        if route == "mesh":
            mesh = self._brick_mesh(volumes, bound_min, bound_max, resolution, threshold, brick)
            if mesh is None:                           # the bound failed: the dense lattice, evaluated once
                stats = self.last_lattice_stats
                u = self.sdf_grid(volumes, bound_min, bound_max, resolution, shard=None, sparse=False, threshold=threshold)
                self.last_lattice_stats = {**stats, "evaluated_points": stats["evaluated_points"] + resolution ** 3, "fell_back": True}
                mesh = ops.marching_cubes(u, threshold)
        else:
            u = self.sdf_grid(volumes, bound_min, bound_max, resolution, shard=shard, sparse=sparse, threshold=threshold)
            if u is None:
                return (None,) * (4 if texture is not None else 3 if attributes else 2)
            mesh = ops.marching_cubes(u, threshold)
        vertices, triangles = mesh
        if simplify is not None:
            full = (vertices, triangles) if simplify_error is not None else None
            before = ops.mesh_topology(vertices, triangles).report() if topology else None
            crossing = ops.self_intersection_counts(vertices, triangles) if self_intersections else None
            vertices, triangles, _, self.last_simplify_stats = ops.simplify_mesh(vertices, triangles, simplify, origin=(-0.5, -0.5, -0.5))
            if before is not None:
                self.last_simplify_stats["topology_before"] = before
            if crossing is not None:
                self.last_simplify_stats["self_intersections_before"] = crossing
            if full is not None:
                self.last_simplify_stats["error"] = ops.mesh_distance(*full, vertices, triangles, **simplify_error)
                del full
        if repair is not None:
            before = ops.mesh_topology(vertices, triangles).report() if topology else None
            crossing = ops.self_intersection_counts(vertices, triangles) if self_intersections else None
            vertices, triangles, _, _, _, self.last_repair_stats = ops.repair_mesh(vertices, triangles, **repair)
            if before is not None:
                self.last_repair_stats["topology_before"] = before
            if crossing is not None:
                self.last_repair_stats["self_intersections_before"] = crossing
        if smooth is not None:
            crossing = ops.self_intersection_counts(vertices, triangles) if self_intersections else None
            vertices, triangles, self.last_smooth_stats = ops.smooth_mesh(vertices, triangles, **smooth)
            if crossing is not None:
                self.last_smooth_stats["self_intersections_before"] = crossing
        if topology:
            self.last_mesh_topology = ops.mesh_topology(vertices, triangles).report()
        if self_intersections:
            self.last_mesh_self_intersections = ops.self_intersection_counts(vertices, triangles)
        b_max, b_min = bound_max.detach().cpu().numpy(), bound_min.detach().cpu().numpy()
        attrs = tex = None
        if attributes or texture is not None:          # on the device-resident vertices; span: the host expression's (float32) difference, widened
            points = ops.vertex_points(vertices, resolution, (b_max - b_min).astype(np.float64).tolist(), b_min.astype(np.float64).tolist())
        if attributes:
            attrs = self.vertex_attributes(points, volumes, views, attributes)
        if texture is not None:
            tex = self.texture_mesh(points, triangles, volumes, views, **texture)
        vertices, triangles = vertices.cpu().numpy(), triangles.cpu().numpy()
        vertices = vertices / (resolution - 1.0) * (b_max - b_min)[None, :] + b_min[None, :]
        if texture is not None:
            return vertices, triangles, attrs, tex
        return (vertices, triangles, attrs) if attributes else (vertices, triangles)

    @torch.no_grad()
    def validate(self, rays_o, rays_d, near, far, volumes, mask_volumes, imgs, features, match_features, intrs, c2ws, bound_min, bound_max,
                 hw, cos_anneal_ratio=1.0, step=None, extract_geometry=True, mesh_resolution=512, threshold=0.0, scene=None, shard=None, sparse=None,
                 sparse_mesh=None, mesh_attributes=None, surface_render=None, surface_fusion=None, mesh_simplify=None, mesh_texture=None,
                 mesh_render=None, mesh_simplify_error=None, mesh_topology=None, mesh_repair=None, mesh_smooth=None,
                 mesh_self_intersections=None):
        """shard (gens_amd.distributed.Shard, optional): render only this rank's contiguous ray range and evaluate only its lattice
        chunks; the (P, 8) image buffer / the lattice slabs are gathered over RCCL, so every rank returns the whole image.  The jitter
        of EVERY ray is drawn on every rank from the identically seeded CPU generator (the reference's draw order) and sliced with
        the rays: the image does not depend on the partition.  sparse, sparse_mesh: extract_geometry's options (the two-level lattice, marching cubes
        on its bricks).  mesh_attributes: extract_geometry's `attributes` with this scene's views -> outputs["vertex_normals"],
        ["vertex_colors"], ["vertex_seen"] beside the mesh.  surface_render (default: the attribute of that name, None / False = off; True, or
        a dict of render_surface's keywords): the rays of this image are also traced to the surface (render_surface, K31) ->
        outputs["surface_depth"], ["surface_normal_img"], ["surface_img"], ["surface_hit"]; not with a shard.  surface_fusion (default: the
        attribute of that name, None / False = off; True, or a dict of fuse_surface's keywords): every view of this item (its intrs, c2ws, hw
        and views) is traced to the surface and the depth maps are fused into a point cloud (fuse_surface, K32) -> outputs["fused_points"],
        ["fused_normals"], ["fused_colors"], ["fused_seen"]; not with a shard.  mesh_simplify: extract_geometry's `simplify` (a cell edge in
        lattice spacings; default: the attribute of that name, None / False / 0 = off): outputs["vertices"], ["triangles"] and the vertex
        attributes are those of the simplified mesh (K33); self.last_simplify_stats holds its counts.  mesh_simplify_error: extract_geometry's
        `simplify_error` (True or a dict of ops.mesh_distance's keywords; default: the attribute of that name, None / False = off): the
        simplified mesh is measured against the extracted one (K36) into self.last_simplify_stats["error"]; ValueError before any launch
        when the simplification is off.  mesh_topology: extract_geometry's `topology` (True; default: the attribute of that name, None /
        False = off): self.last_mesh_topology holds the topology report of the returned mesh (K37).  mesh_self_intersections: extract_geometry's
        `self_intersections` (True; default: the attribute of that name, None / False = off): self.last_mesh_self_intersections holds the
        self-intersection counts of the returned mesh (K41).  mesh_repair: extract_geometry's `repair`
        (True or a dict of ops.repair_mesh's keywords; default: the attribute of that name, None / False = off): the mesh is repaired on the
        device (K38) before the report, the attributes and the texture; self.last_repair_stats holds its counts.  mesh_smooth: extract_geometry's
        `smooth` (True or a dict of ops.smooth_mesh's keywords; default: the attribute of that name, None / False = off): the mesh is smoothed
        on the device (K39) after the repair; self.last_smooth_stats holds its stats.  mesh_texture: extract_geometry's
        `texture` with this scene's views (the tile edge in texels or a dict of texture_mesh's keywords; default: the attribute of that name,
        None / False / 0 = off) -> outputs["texture"], ["texture_seen"], ["texture_uv"] (K34), which save_validation_outputs writes as an
        OBJ beside the PLY.  mesh_render (default: the attribute of that name, None / False = off; True, or a dict of render_mesh's keywords
        shading and chunk): after extract_geometry the rays of this image are cast at the mesh it returned (render_mesh, K35), with the
        atlas where that call made one, else the vertex colours where it made them, else neither -> outputs["mesh_depth"],
        ["mesh_normal_img"], ["mesh_hit"] and, with colours, ["mesh_img"]; beside surface_render also outputs["mesh_fidelity"] =
        ops.compare_maps(mesh maps, surface maps).  ValueError before any launch with a shard, with extract_geometry=False, or for
        smooth shading when mesh_attributes does not ask for "normals"."""
        outputs = {}
        mesh_render = self._mesh_render_option(mesh_render)
        if mesh_render is not None and (shard is not None or not extract_geometry):
            raise ValueError("mesh_render casts the rays at the mesh of this call on one rank: not with a shard, not with extract_geometry=False "
                             "(render_mesh takes any mesh)")
        if mesh_render is not None and mesh_render.get("shading") == "smooth":
            asked = self.mesh_attributes if mesh_attributes is None else mesh_attributes
            if "normals" not in ((asked,) if isinstance(asked, str) else tuple(asked or ())):
                raise ValueError("mesh_render: smooth shading needs mesh_attributes with \"normals\"")
        mesh_simplify = self._simplify_request(mesh_simplify) if extract_geometry else None      # (refused before anything is launched)
        mesh_simplify_error = self._simplify_error_request(mesh_simplify_error, mesh_simplify) if extract_geometry else None
        mesh_topology = self._topology_request(mesh_topology) if extract_geometry else False
        mesh_self_intersections = self._self_intersections_request(mesh_self_intersections) if extract_geometry else False
        mesh_repair = self._repair_request(mesh_repair) if extract_geometry else None
        mesh_smooth = self._smooth_request(mesh_smooth) if extract_geometry else None
        mesh_texture = self._texture_option(mesh_texture) if extract_geometry else None
        surface_fusion = self.surface_fusion if surface_fusion is None else surface_fusion
        if surface_fusion:
            if shard is not None:
                raise ValueError("surface_fusion is not sharded: fuse the views on one rank (fuse_surface)")
            fusion_kw = {"resolution": mesh_resolution, **(surface_fusion if isinstance(surface_fusion, dict) else {})}
            fusion_kw["attributes"] = ("normals", "colors")
        surface_render = self.surface_render if surface_render is None else surface_render
        if surface_render:
            if shard is not None:
                raise ValueError("surface_render is not sharded: trace the rays on one rank (render_surface)")
            surface_kw = {"resolution": mesh_resolution, **(surface_render if isinstance(surface_render, dict) else {})}
            surface_kw["outputs"] = self.SURFACE_OUTPUTS
        if scene is None:
            scene = Scene(volumes, mask_volumes, imgs, features, match_features, intrs, c2ws)
        height, width = int(hw[0]), int(hw[1])
        n_rays = rays_o.shape[0]
        r0, r1 = (0, n_rays) if shard is None else shard.rays(n_rays)
        # the jitter thread starts first: its ~1.5 ms per 32 768 rays (the reference's draw order costs 13 draws per ray) then hide behind
        # the mesh extraction, which draws nothing from the generator
        chunk = self.val_chunk_for(r1 - r0)
        self.last_val_chunk = chunk
        jitter = None
        if self.perturb > 0:
            jitter = self._take_speculated_jitter(n_rays)
            if jitter is None:
                jitter = JitterStream(n_rays, chunk, self._pinned(n_rays, 1, "_pinned_jitter"))
        if extract_geometry:
            import time
            t_geo = time.perf_counter()
            mesh = self.extract_geometry(scene.volumes_nograd(), bound_min, bound_max, mesh_resolution, threshold, shard=shard, sparse=sparse,
                                         sparse_mesh=sparse_mesh, attributes=mesh_attributes, views=scene.views,
                                         simplify=0 if mesh_simplify is None else mesh_simplify, texture=0 if mesh_texture is None else mesh_texture,
                                         simplify_error=False if mesh_simplify_error is None else mesh_simplify_error, topology=mesh_topology,
                                         repair=False if mesh_repair is None else mesh_repair, smooth=False if mesh_smooth is None else mesh_smooth,
                                         self_intersections=mesh_self_intersections)
            outputs["vertices"], outputs["triangles"] = mesh[0], mesh[1]
            for name, values in ((mesh[2] or {}) if len(mesh) >= 3 else {}).items():
                outputs["vertex_" + name] = values
            outputs.update(mesh[3] or {} if len(mesh) == 4 else {})
            self.last_geometry_s = time.perf_counter() - t_geo     # (ends with the mesh's read-back: wall time is the item's share; bench.py's default_path)
        # one (P, 8) device buffer [rgb | normal | sdf_depth | render_depth] filled chunk by chunk: ONE D2H copy per image
        # into a pinned host buffer (the reference copies 4 tensors per 256-ray chunk, implicit_surface.py:446-453)
        import time as _time
        t_render = _time.perf_counter()                 # (the image's share of the call, as last_geometry_s is the mesh's: bench.py's default_path)
        image = torch.empty(r1 - r0, 8, device=rays_o.device, dtype=torch.float32)

        def render_image():
            for s in range(r0, r1, chunk):
                e = min(s + chunk, r1)
                r = self.render(rays_o[s:e], rays_d[s:e], near, far, volumes, mask_volumes, imgs, features, match_features, intrs, c2ws,
                                cos_anneal_ratio, step, scene=scene, lean=True, t_rand=None if jitter is None else jitter.slice(s, e))
                image[s - r0:e - r0, 0:3] = r["color_fine"]
                image[s - r0:e - r0, 3:6] = (r["gradients"] * r["weights"][..., None] * r["inside_sphere"][..., None]).sum(dim=1)
                image[s - r0:e - r0, 6] = r["sdf_depth"].reshape(-1)
                image[s - r0:e - r0, 7] = r["render_depth"].reshape(-1)

        render_image()
        if jitter is not None:
            jitter.join()
            if jitter.generator is not None:           # the head start was used: its draws are the default generator's past now
                torch.set_rng_state(jitter.end_state())
        overflowed = self._split_half_overflowed()
        if shard is not None and self.sdf_precision == "f16x2":
            overflowed = shard.any(overflowed)         # every rank re-renders or none does: the gathered image never mixes precisions
        if overflowed:                                 # a value left the half range: the same image, same jitter, in float32
            saved, self.sdf_precision = self.sdf_precision, "f32"
            try:
                render_image()
            finally:
                self.sdf_precision = saved
        if shard is not None:               # RCCL all_gather of the rendered buffers (config 4), device to device
            image = shard.gather_rows(image, n_rays, key="image")
            if image is None:               # Shard.single: the other shards have not been rendered yet
                return None
        self.last_device_image = image      # (P, 8) [rgb | normal | sdf_depth | render_depth] on the device: what a multi-GPU driver gathers
        # the 8-bit-range images (implicit_surface.py:455-463: colour * 256, rot @ normal * 128 + 128, clipped) are formed on the DEVICE and
        # travel in the same single copy: the host only reshapes (on 307 200 pixels the numpy versions cost milliseconds with the GPU idle)
        # and laid out as five CONTIGUOUS blocks [rgb (P,3) | img_fine (P,3) | normal_img (P,3) | sdf_depth (P) | render_depth (P)], so the host
        # makes one plain copy out of the reused page-locked buffer and hands out views of it (strided column copies cost 4.6 ms of idle GPU per image)
        p_ = image.shape[0]
        rot = scene.views.cams.rot_inv.view(3, 3)
        post = torch.empty(11 * p_, device=image.device, dtype=image.dtype)
        post[0:3 * p_].view(p_, 3).copy_(image[:, 0:3])
        torch.clamp(image[:, 0:3] * 256, 0, 255, out=post[3 * p_:6 * p_].view(p_, 3))
        n0, n1, n2 = image[:, 3:4], image[:, 4:5], image[:, 5:6]
        torch.clamp(((n0 * rot[:, 0] + n1 * rot[:, 1]) + n2 * rot[:, 2]) * 128 + 128, 0, 255, out=post[6 * p_:9 * p_].view(p_, 3))   # rot @ n per pixel
        post[9 * p_:10 * p_].copy_(image[:, 6])
        post[10 * p_:11 * p_].copy_(image[:, 7])
        host = self._pinned(11 * n_rays, 1, "_pinned_post")
        host.copy_(post.view(-1, 1), non_blocking=True)
        if self.perturb > 0 and self.speculate_jitter:
            self._speculate_jitter(n_rays, chunk)      # image after image (runner.py:215's loop): the next image's draws start while this one drains
        status = scene.views.cams.status.cpu()         # (rides behind the image copy: a singular camera matrix raises, as torch.inverse does)
        torch.cuda.current_stream().synchronize()
        if int(status) != 0:
            raise RuntimeError("linalg.inv: a camera pose or intrinsics matrix of the scene is singular")
        flat = host.numpy().reshape(-1).copy()
        outputs["color_fine"] = torch.from_numpy(flat[0:3 * p_].reshape(p_, 3))
        outputs["img_fine"] = flat[3 * p_:6 * p_].reshape([height, width, 3])
        outputs["normal_img"] = flat[6 * p_:9 * p_].reshape([height, width, 3])
        outputs["sdf_depth"] = flat[9 * p_:10 * p_].reshape([height, width])
        outputs["render_depth"] = flat[10 * p_:11 * p_].reshape([height, width])
        self.last_render_s = _time.perf_counter() - t_render
        if surface_render:
            surf = self.render_surface(rays_o, rays_d, near.to(rays_o.device), far.to(rays_o.device), scene.volumes_nograd(), bound_min, bound_max, c2ws, views=scene.views,
                                       threshold=threshold, hw=(height, width), **surface_kw)
            outputs["surface_depth"], outputs["surface_normal_img"] = surf["depth"], surf["normal_img"]
            outputs["surface_img"], outputs["surface_hit"] = surf["img"], surf["hit"]
        if mesh_render is not None:
            maps = self.render_mesh(outputs["vertices"], outputs["triangles"], rays_o, rays_d, c2ws, normals=outputs.get("vertex_normals"),
                                    colors=outputs.get("vertex_colors"), seen=outputs.get("vertex_seen") if "vertex_colors" in outputs else None,
                                    texture=outputs.get("texture"), texture_seen=outputs.get("texture_seen"),
                                    texels=None if mesh_texture is None else mesh_texture.get("texels", 8), hw=(height, width), **mesh_render)
            outputs["mesh_depth"], outputs["mesh_normal_img"], outputs["mesh_hit"] = maps["depth"], maps["normal_img"], maps["hit"]
            if "img" in maps:
                outputs["mesh_img"] = maps["img"]
            if surface_render:
                outputs["mesh_fidelity"] = ops.compare_maps(maps, surf)
        if surface_fusion:
            cloud = self.fuse_surface(scene.volumes_nograd(), intrs, c2ws, (height, width), bound_min, bound_max, views=scene.views,
                                      **{"threshold": threshold, **fusion_kw})
            outputs["fused_points"], outputs["fused_normals"] = cloud["points"], cloud["normals"]
            outputs["fused_colors"], outputs["fused_seen"] = cloud["colors"], cloud["seen"]
        return outputs

    def val_chunk_for(self, n_rays):
        """Rays per render() chunk for a range of n_rays rays: `val_chunk` when the caller set one, else equal chunks of at most 32 768."""
        from ...chunking import balanced_chunk
        return int(self.val_chunk) if self.val_chunk else balanced_chunk(n_rays)

    def _speculate_jitter(self, n_rays, chunk=None):
        """Draw the NEXT validate() call's jitter now, on a helper thread with a PRIVATE generator that starts at the default CPU generator's
        current state.  The reference's draw order costs 13 generator draws per ray -- 14 ms of host time for a 480 x 640 image -- and a rank
        that renders the LAST rays of a ray-sharded image needs the state behind all the others': without the head start the first chunk waits
        1.5 ms per image for its draws, the last rank of eight ~12 ms of a 35 ms step.  The next validate() uses the draws only if it asks for
        the same number of rays AND the default generator still stands where the draws started (nobody drew in between: image after image, as
        runner.py:215's loop renders them); it then moves the default generator behind them.  Otherwise they are dropped -- a training step
        between two validations sees exactly the reference's stream, whatever was drawn ahead."""
        pending = getattr(self, "_jitter_ahead", None)
        state = torch.get_rng_state()
        if pending is not None:
            if pending[0] == n_rays and torch.equal(pending[1], state):
                return                                 # already drawing exactly this
            pending[2].join()                          # (its page-locked buffer is about to be reused)
        g = torch.Generator()
        g.set_state(state)
        # two page-locked buffers take turns: the image being rendered reads one while the next image's draws fill the other
        self._jitter_parity = 1 - getattr(self, "_jitter_parity", 0)
        buf = self._pinned(n_rays, 1, "_pinned_jitter_ahead%d" % self._jitter_parity)
        self._jitter_ahead = (n_rays, state, JitterStream(n_rays, chunk or self.val_chunk_for(n_rays), buf, generator=g))

    def prefetch_jitter(self, n_rays):
        """Rounds 2 - 5's explicit head start for drivers that render image after image; validate() now does it itself (_speculate_jitter).
        Kept for callers that want the draws started before the FIRST image."""
        if self.perturb > 0:
            self._speculate_jitter(n_rays)

    def _take_speculated_jitter(self, n_rays):
        pending = getattr(self, "_jitter_ahead", None)
        self._jitter_ahead = None
        if pending is None:
            return None
        if pending[0] != n_rays or not torch.equal(pending[1], torch.get_rng_state()):
            pending[2].join()                          # drawn for nothing -- on its own generator: the default one never moved
            return None
        return pending[2]

    def join_speculation(self):
        """Wait for a head start that will not be used (before interpreter shutdown in scripts that time themselves)."""
        pending = getattr(self, "_jitter_ahead", None)
        if pending is not None:
            pending[2].join()

    def _pinned(self, n_rays, cols=8, slot="_pinned_image"):
        """Page-locked (P, cols) staging buffer (rendered image / ray jitter), kept between validate() calls, which end with a
        stream synchronisation, so reuse is safe."""
        buf = getattr(self, slot, None)
        if buf is None or buf.shape[0] != n_rays:
            buf = torch.empty(n_rays, cols, dtype=torch.float32, pin_memory=True)
            setattr(self, slot, buf)
        return buf

    def _defer_checks(self, counts, cam_status):
        """Host-side checks of a fused training step, taken off its critical path: the counts of gens_compact_points and the scene set-up's
        status word travel to page-locked memory behind the step's launches."""
        host = getattr(self, "_deferred_host", None)
        if host is None:
            host = self._deferred_host = torch.zeros(4, dtype=torch.int32, pin_memory=True)
        host[:3].copy_(counts, non_blocking=True)
        host[3:4].copy_(cam_status, non_blocking=True)
        if torch.cuda.is_current_stream_capturing():         # (a captured step: the copies are graph nodes; the replaying loop checks after its own synchronisation)
            self._deferred = None
            return
        ev = torch.cuda.Event()
        ev.record()
        self._deferred = ev

    def check_deferred(self):
        """Raise what the last fused training step would have raised in the reference (no valid pseudo point, implicit_surface.py:494-495; a
        singular camera matrix, torch.inverse).  Called at the start of every forward().  The reference raises INSIDE the bad step's forward
        (before its backward and optimiser step); here the bad step's pseudo-point term is zero (value and gradient) and the error arrives one
        call later, so a loop that must not apply the bad step's update -- or that ends -- calls this itself once the step's forward has run:
        after the loss read-back (free: the read-back synchronised) and before optimizer.step(), as distributed.FinetuneStepper does."""
        ev = getattr(self, "_deferred", None)
        if ev is None or torch.cuda.is_current_stream_capturing():
            return
        self._deferred = None
        ev.synchronize()
        self.check_deferred_host()

    def check_deferred_host(self):
        """The same checks on what the last step left in page-locked memory; the caller has synchronised with that step (a graph replay
        followed by the loss read-back)."""
        host = getattr(self, "_deferred_host", None)
        if host is None:
            return
        if int(host[3]) != 0:
            raise RuntimeError("linalg.inv: a camera pose or intrinsics matrix of the previous step's scene is singular")
        if int(host[2]) < 1:
            raise RuntimeError("No valid pseudo pts!")

    # inputs of a training step that change from call to call (copied into a captured step's static tensors); everything else in `ipts` is
    # either consumed by the caller's loss (colour, depths, masks) or describes the item (scene, file names)
    STEP_INPUTS = ("imgs", "intrs", "c2ws", "rays_o", "rays_d", "near", "far", "pseudo_pts")

    def _auto_graph_ok(self, mode, ipts, volumes, features):
        """May this call run as a captured step (gens_amd.graph.AutoGraph)?  Training / fine-tune steps on the device that take the fused path
        (K17 + K18 on a device-side selection: nothing in them is read back by the host)."""
        from ... import graph
        if mode == "val" or not getattr(self, "auto_graph", True) or not graph.auto_graph_enabled() or not torch.is_grad_enabled():
            return False
        if getattr(self, "_auto_suppressed", False):          # an enclosing GenS.forward manages this step
            return False
        rays = ipts["rays_o"]
        if not (torch.is_tensor(rays) and rays.is_cuda) or torch.cuda.is_current_stream_capturing():
            return False
        if not self.fused_train or self.n_importance <= 0 or features is None or ipts["imgs"].shape[0] < 2:
            return False
        if not any(p.requires_grad for p in self.sdf_network.parameters()) and not any(v.requires_grad for v in volumes):
            return False
        nf = len(features)
        if not (ops.BlendPlan.supported(self.color_network) and nf <= 5 and self.color_network.ray_dir_fc[2].weight.shape[0] == 3 + 4 * nf):
            return False
        return ops.SdfTrainStep.supported(self.sdf_network, len(volumes)) and all(v.dim() == 5 and v.shape[1] == 4 for v in volumes)

    def forward(self, mode, ipts, volumes, mask_volumes, features, match_features, cos_anneal_ratio=1.0, step=None):
        """implicit_surface.py:472-499.  A training / fine-tune call that qualifies (_auto_graph_ok) runs as a CAPTURED step after two eager
        ones: forward and backward are one HIP graph replay each (gens_amd.graph.AutoGraph), behind this unchanged signature -- the loop of
        runner.py:157-166 stays as it is.  `self.auto_graph = False` or GENS_AUTO_GRAPH=0: every call eager."""
        if not self._auto_graph_ok(mode, ipts, volumes, features):
            return self._forward_impl(mode, ipts, volumes, mask_volumes, features, match_features, cos_anneal_ratio, step)
        from ... import graph
        auto = getattr(self, "_auto", None)
        if auto is None:
            auto = self._auto = graph.AutoGraph()
        copied, refs, layout = {}, [], []

        def take(name, t):
            """persistent tensors (parameters, leaves the caller optimises) are used where they are; the rest is copied per call"""
            if isinstance(t, nn.Parameter) or (t.is_leaf and t.requires_grad):
                refs.append(t)
                layout.append((name, len(refs) - 1))
            else:
                copied[name] = t
                layout.append((name, None))
        for k in self.STEP_INPUTS:
            if k in ipts:
                take(k, ipts[k])
        same_match = all(a is b for a, b in zip(features, match_features)) and len(features) == len(match_features)
        groups = [("volumes", volumes), ("mask_volumes", mask_volumes), ("features", features)] + ([] if same_match else [("match_features", match_features)])
        for gname, group in groups:
            for i, t in enumerate(group):
                take(f"{gname}.{i}", t)
        params = [p for p in self.parameters()]
        n_in = len(refs)
        refs = refs + params
        use_match = not (step is None or step < 5)
        counts = tuple(len(g) for _, g in groups)

        where = dict(layout)

        def body(cp, sc, alias):
            def get(name):
                return cp[name] if name in cp else alias(refs[where[name]])
            ip = dict(ipts)
            for k in self.STEP_INPUTS:
                if k in ipts:
                    ip[k] = get(k)
            lists = {gname: [get(f"{gname}.{i}") for i in range(len(group))] for gname, group in groups}
            feats = lists["features"]
            return self._forward_impl(mode, ip, lists["volumes"], lists["mask_volumes"], feats, feats if same_match else lists["match_features"],
                                      sc["cos_anneal_ratio"], 5.0 if use_match else 0.0)
        key = ("ImplicitSurface", mode, use_match, same_match, counts, tuple(n for n, _ in layout), n_in, self.training)
        return auto.run(key, copied, refs, {"cos_anneal_ratio": float(cos_anneal_ratio)}, body, [self], module=self)

    def _forward_impl(self, mode, ipts, volumes, mask_volumes, features, match_features, cos_anneal_ratio=1.0, step=None):
        imgs, intrs, c2ws = ipts["imgs"], ipts["intrs"], ipts["c2ws"]
        rays_o, rays_d, near, far = ipts["rays_o"], ipts["rays_d"], ipts["near"], ipts["far"]
        scene = Scene(volumes, mask_volumes, imgs, features, match_features, intrs, c2ws)
        self.check_deferred()                          # what the previous fused training step left to verify (see below)
        pseudo_pts = idx = None
        fused = mode != "val" and "pseudo_pts" in ipts and self._train_fused_ok(scene, self._train_net(scene, False), False)
        if fused:
            # (:484-497) on the fused training path the pseudo points ride on the render's network pass with their mask flags LEFT ON THE
            # DEVICE: nothing is read back in the middle of the step.  The reference's `raise "No valid pseudo pts!"` (:494-495) needs the
            # count on the host; it travels behind the step through a page-locked copy and is raised by check_deferred() -- at the next
            # forward() at the latest (such a step's pseudo_sdf is all zeros, so its loss term and gradient are zero).
            pseudo_pts = ipts["pseudo_pts"].float().contiguous()
            flags = torch.empty(pseudo_pts.shape[0], device=pseudo_pts.device, dtype=torch.uint8)
            ops.lookup_mask(pseudo_pts, scene.masks, out=flags)
            outputs = self.render(rays_o, rays_d, near, far, volumes, mask_volumes, imgs, features, match_features, intrs, c2ws,
                                  cos_anneal_ratio, step, scene=scene, extra_pts=pseudo_pts, extra_valid=flags)
            outputs["pseudo_sdf"] = outputs.pop("_extra_sdf_dense")
            self._defer_checks(self._last_step_counts, scene.views.cams.status)
            return outputs
        host = getattr(self, "_deferred_host", None)
        if host is not None and not torch.cuda.is_current_stream_capturing():
            # this step leaves nothing to verify later (it raises on the spot, or carries no pseudo points): what an EARLIER fused step parked in
            # page-locked memory was checked two lines up and must not be read again by check_deferred_host() / GraphedStep.check()
            host[2], host[3] = 1, 0
        if "pseudo_pts" in ipts:                       # (:484-497) the mask look-up draws nothing from the generator, so it can come first
            pseudo_pts = ipts["pseudo_pts"].float()
            valid = ops.lookup_mask(pseudo_pts, scene.masks)
            if int(valid.sum()) < 1:
                raise RuntimeError("No valid pseudo pts!")                                  # the reference raises a str (:494-495)
            idx = torch.nonzero(valid)[:, 0]
        if mode == "val":
            outputs = self.validate(rays_o, rays_d, near, far, volumes, mask_volumes, imgs, features, match_features, intrs, c2ws,
                                    ipts["bound_min"], ipts["bound_max"], ipts["hw"], cos_anneal_ratio, step, scene=scene)
            extra = None
        else:                                          # the pseudo points ride on the render's network pass
            outputs = self.render(rays_o, rays_d, near, far, volumes, mask_volumes, imgs, features, match_features, intrs, c2ws,
                                  cos_anneal_ratio, step, scene=scene, extra_pts=None if idx is None else pseudo_pts[idx])
            extra = outputs.pop("_extra_sdf", None)
        if pseudo_pts is not None:
            if extra is None:
                vols = scene.volumes if any(v.requires_grad for v in scene.volumes) else scene.volumes_nograd()
                extra = self.sdf_network.sdf(pseudo_pts[idx], vols)
            outputs["pseudo_sdf"] = torch.zeros_like(pseudo_pts[:, :1]).index_put((idx,), extra)
        return outputs
