"""K6 (the fused SDF network in inference) and K17 (the SDF network of a training step).  K6's weight streams: ops/sdf_pack.py.

Part of gens_amd.ops (see ops/__init__.py); citations are relative to /root/reference."""
from .base import *  # noqa: F401,F403
from .sdf_pack import *  # noqa: F401,F403

# ------------------------------------------------------------------------------------------------------------------
# K6  fused SDF network (inference): look-up + encodings + 7 layers on fp32 MFMA (+ d sdf/dx)   (sdf_network.py:98-146)
# ------------------------------------------------------------------------------------------------------------------
class SdfMlpPlan:
    """Weights of an SDFNetwork re-packed for gens_sdf_mlp.  Only the shipped architecture is supported
    (`supported(net)`); anything else keeps using the PyTorch layers on top of the K2 look-up kernels."""

    @staticmethod
    def supported(net):
        return (net.num_layers == 8 and tuple(net.skip_in) == (3,) and net.embed_fn_fine is not None and net.embed_fn_feat is not None
                and net.lin0.weight_v.shape == (128, 27) and net.init_feat_channels in (4, 8, 12, 16, 20)
                and net.lin6.weight_v.shape[1] == 128 + 5 * net.init_feat_channels and net.lin2.weight_v.shape[0] == 101)

    @staticmethod
    def version(net):
        return tuple(p._version for p in net.parameters()) + tuple(p.data_ptr() for p in net.parameters())

    def __init__(self, net):
        assert SdfMlpPlan.supported(net), "gens_sdf_mlp is built for the architecture of confs/gens.conf:69-86"
        with torch.no_grad():
            ws, bs = [], []
            for l in range(7):
                lin = getattr(net, f"lin{l}")
                v, g = lin.weight_v.detach().to(_f32), lin.weight_g.detach().to(_f32)
                ws.append(v * (g / torch.linalg.norm(v, dim=1, keepdim=True)))
                bs.append(lin.bias.detach().to(_f32))
            dev = ws[0].device
            self.n_levels = net.init_feat_channels // 4
            self.wf, self.wb, self.bias = [], [], []
            c = 100.0 / math.log(2.0)      # pre-scaled forward streams (k6_sdfmlp.hip::softplus_t): hidden units travel as c * softplus
            for l in range(6):
                w = torch.zeros(128, ws[l].shape[1], device=dev, dtype=_f32)
                w[:ws[l].shape[0]] = ws[l]
                b = torch.zeros(128, device=dev, dtype=_f32)
                b[:bs[l].shape[0]] = bs[l]
                wbias = torch.cat([w, b[:, None]], 1)                              # bias = extra reduction row K_l (constant-1 input column)
                hidden = 0 if l == 0 else (101 if l == 3 else 128)                  # leading columns fed by (scaled) hidden units
                wbias[:, hidden:] *= c                                              # point encoding / skip columns / volume features / bias
                self.wf.append(_pack_b_groups(wbias))
                self.wb.append(_pack_b_groups(w.t().contiguous()))
                self.bias.append(b)
            # (the kernels' max / median activations drop NaNs: non-finite WEIGHTS are answered with NaN outputs, as the reference's layers would)
            self.finite = bool(torch.stack([torch.isfinite(w).all() for w in ws] + [torch.isfinite(b).all() for b in bs]).all())
            self.w_last = _c(ws[6][0].clone())
            self.w_last_scaled = self.w_last.clone()
            self.w_last_scaled[:128] /= c
            self.b_last = float(bs[6][0])
            self.scale = float(net.scale)
            self.value_stream, self.value_row = _pack_value_stream(ws, bs, self.n_levels)
            self.grad_stream, self.grad_row = _pack_grad_stream(ws, bs, self.n_levels)
            assert self.grad_stream.shape[0] == L.load().gens_sdf_grad_groups(self.n_levels) + 2
            # the split-half kernels (k6v / k6gh, the opt-in sdf_precision="f16x2") are built for 3 and 5 levels: other counts stay in float32
            self.value_units = self.value_w_out = None
            self.value_ok = False
            if self.n_levels in (3, 5):
                self.value_units, self.value_w_out, vmax = _pack_value_units(ws, bs, self.n_levels)
                self.value_ok = vmax < 6.0e4
            self.grad_pieces = None                        # the split-half value + gradient kernel: None if a weight leaves the half range
            n_pieces = L.load().gens_sdf_grad_f16_pieces(self.n_levels) if self.n_levels in (3, 5) else 0
            if n_pieces:
                self.grad_pieces, gvmax = _pack_grad_pieces(ws, bs, self.n_levels, n_pieces)
                assert self.grad_pieces.shape[0] == n_pieces
                top = float(ws[6][0, :128].abs().max())
                # gradients travel times a power of two that puts |w_last| near 256: lo parts of normal halfs, 128 x of head room
                self.grad_scale = 2.0 ** min(14, max(-10, round(math.log2(256.0 / top)))) if top > 0 and math.isfinite(top) else 1.0
                if not gvmax < 6.0e4:
                    self.grad_pieces = None
            # the three-term bfloat16 kernels (k6b, generation "bf16x3" of the "f32" arithmetic): 3 and 5 levels, no range limit
            # The library says how its kernels walk the stream: how many hidden blocks layer 3 reads, and whether the value kernel reads the
            # forward prefix of the gradient kernel's stream (the shipped build) or a tile-major stream of its own (make k6b_tile_major).
            self.bf16x3_pieces = self.bf16x3_value_pieces = None
            n_pieces = L.load().gens_sdf_bf16x3_pieces(self.n_levels) if self.n_levels in (3, 5) else 0
            if n_pieces:
                layout = (C.c_int * 3)()
                if L.load().gens_sdf_bf16x3_layout(self.n_levels, layout) != 0:
                    raise RuntimeError(L.load().gens_last_error().decode())
                n_value, tile_major, hid3 = layout
                self.bf16x3_pieces, _ = _pack_grad_pieces(ws, bs, self.n_levels, n_pieces, terms=3, hid3=hid3)
                assert self.bf16x3_pieces.shape[0] == n_pieces
                self.bf16x3_value_pieces = self.bf16x3_pieces
                if tile_major:
                    self.bf16x3_value_pieces, _ = _pack_grad_pieces(ws, bs, self.n_levels, n_value, terms=3, hid3=hid3, order="tile")
                    assert self.bf16x3_value_pieces.shape[0] == n_value
            self.overflow = torch.zeros(1, device=dev, dtype=torch.int32)
        self.wf_table, self.wb_table, self.bias_table = L.ptr_table(self.wf), L.ptr_table(self.wb), L.ptr_table(self.bias)
        self.key = SdfMlpPlan.version(net)

    def overflowed(self):
        """True if any split-half launch since the last call met a value outside the half range (synchronises)."""
        hit = bool(self.overflow.item())
        if hit:
            self.overflow.zero_()
        return hit


# What differs between the launches of the stream kernels: entry point -> (the plan's weight stream, its dtype, the plan's output row, whether
# plan.grad_scale is passed, the stash of a gradient pass, whether the overflow word is passed).
_SDF_STREAMS = {
    "gens_sdf_grad_f16": ("grad_pieces", torch.float16, "grad_row", True, sdf_grad_f16_stash, True),
    "gens_sdf_grad_bf16x3": ("bf16x3_pieces", torch.bfloat16, "grad_row", False, sdf_grad_f16_stash, False),
    "gens_sdf_grad": ("grad_stream", _f32, "grad_row", False, sdf_grad_stash, False),
    "gens_sdf_value_f16": ("value_units", torch.float16, "value_w_out", False, None, True),
    "gens_sdf_value_bf16x3": ("bf16x3_value_pieces", torch.bfloat16, "grad_row", False, None, False),
    "gens_sdf_value": ("value_stream", _f32, "value_row", False, None, False),
}


def _sdf_route(plan, want_grad, precision, kernels):
    """(entry point, profile label) of a launch of sdf_mlp; no GPU involved.  In this order: the split-half kernel under precision "f16x2" if
    the plan has its stream (weights inside the half range; the gradient pass also needs kernels.sdf_grad_f16) -- whatever kernels.sdf_value /
    sdf_grad say; the three-term bfloat16 kernel under "bf16x3" if the plan has its pieces (3 and 5 levels); the float32 stream kernel under
    "transposed" or "bf16x3"; else the row-major gens_sdf_mlp, whose two device kernels (sdf_mlp_k<FE, true / false>) are priced separately."""
    kind = "grad" if want_grad else "value"
    generation = kernels.sdf_grad if want_grad else kernels.sdf_value
    if precision == "f16x2" and ((kernels.sdf_grad_f16 and getattr(plan, "grad_pieces", None) is not None) if want_grad else plan.value_ok):
        entry = f"gens_sdf_{kind}_f16"
    elif generation == "bf16x3" and getattr(plan, "bf16x3_pieces", None) is not None:
        entry = f"gens_sdf_{kind}_bf16x3"
    elif generation in ("transposed", "bf16x3"):
        entry = f"gens_sdf_{kind}"
    else:
        return "gens_sdf_mlp", f"gens_sdf_mlp:{kind}"
    return entry, entry


def sdf_mlp(plan, volumes, pts, index=None, want_grad=False, sdf_out=None, grad_out=None, precision="f32", count=None):
    """sdf (and d sdf/dx) of pts[index] written to sdf_out[index] / grad_out[index] (fresh, densely indexed outputs if
    no buffers are given).  volumes: packed VolumeSet with 3 or 5 levels.  No autograd graph is built (inference).
    precision: "f32" (float32-accurate products: three-term bfloat16 operands on gens_sdf_value_bf16x3 / gens_sdf_grad_bf16x3 at 3 and 5
    levels under kernels.sdf_value / sdf_grad "bf16x3", float32 MFMA otherwise) or "f16x2" (split-half operands, ~1e-6 relative; check
    plan.overflowed()) -- value-only launches on gens_sdf_value_f16, value + gradient launches on gens_sdf_grad_f16 (the "f32" kernels if the
    weights leave the half range or kernels.sdf_grad_f16 is off).
    count: optional (1,) int32 device tensor from compact_valid(): only the first `count` entries of `index` are evaluated."""
    assert isinstance(volumes, VolumeSet) and volumes.layout == L.LAYOUT_PACKED and volumes.n == plan.n_levels
    pts = _c(pts.detach().reshape(-1, 3).to(_f32))
    n = pts.shape[0] if index is None else index.shape[0]
    if sdf_out is None:
        sdf_out = torch.empty(pts.shape[0], 1, device=pts.device, dtype=_f32)
    if want_grad and grad_out is None:
        grad_out = torch.empty(pts.shape[0], 3, device=pts.device, dtype=_f32)
    idx = None if index is None else _c(index.to(torch.int64))
    fe = 20 * plan.n_levels
    flops = 2 * (27 * 128 + (128 + fe) * (4 * 128 + 101 + 1)) * (2 if want_grad else 1)
    nbytes = n * (12 + (16 if want_grad else 4) + (8 if idx is not None else 0))
    if isinstance(plan, SdfTrainStep):           # this training step's streams (gens_sdf_train_pack): the row-major layout, bias on the device
        entry, label = "gens_sdf_mlp_dev", "gens_sdf_mlp:grad" if want_grad else "gens_sdf_mlp:value"
    else:
        entry, label = _sdf_route(plan, want_grad, precision, kernels)
    if entry in _SDF_STREAMS:
        stream, dtype, row, scaled, stash, overflow = _SDF_STREAMS[entry]
        operands = (L.ptr(getattr(plan, stream), dtype), L.ptr(getattr(plan, row)), plan.b_last, plan.scale) + ((plan.grad_scale,) if scaled else ())
        tail = (L.ptr(grad_out), L.ptr(stash(pts.device), torch.uint8)) if want_grad else ()
        if overflow:
            tail += (L.ptr(plan.overflow, torch.int32),)
    else:       # the row-major kernel and its _dev form
        last = (L.ptr(plan.b_last), 1.0) if entry == "gens_sdf_mlp_dev" else (L.ptr(plan.w_last_scaled), plan.b_last, plan.scale)
        operands = (plan.wf_table, plan.wb_table, L.ptr(plan.w_last), *last)
        tail = (L.ptr(grad_out) if want_grad else None,)
    L.call(entry, volumes.table, volumes.dim_table, volumes.n, *operands, L.ptr(pts), L.ptr(idx, torch.int64), n, L.ptr(count, torch.int32),
           L.ptr(sdf_out), *tail, L.stream(), nbytes=nbytes, flops=n * flops, live=None if count is None else (count, n),
           label=label)
    if not getattr(plan, "finite", True):
        _poison(idx, count, sdf_out, grad_out if want_grad else None)
    return (sdf_out, grad_out) if want_grad else sdf_out


def _poison(idx, count, *outs):
    """NaN into the evaluated rows of `outs` (index map / device-side count as the kernels take them): a network with non-finite weights."""
    for out in outs:
        if out is None:
            continue
        if idx is None:
            out.fill_(float("nan"))
        else:
            live = idx if count is None else idx[torch.arange(idx.shape[0], device=idx.device) < count.to(idx.device)[0]]
            out[live] = float("nan")


# ------------------------------------------------------------------------------------------------------------------
# K17  the SDF network of a training step: value, gradient, `smooth`, and the loss backward   (sdf_network.py:98-154)
# ------------------------------------------------------------------------------------------------------------------
class SdfTrainStep:
    """One training / fine-tune step's view of the SDF network (gens_sdf_train_*): the effective (weight-normed) matrices are packed
    into MFMA B streams ONCE, then any number of point batches are evaluated against them.

        step = SdfTrainStep(weights, biases, volumes, packed)      # weights[l] (out_l, in_l) with autograd history, l = 0..6
        y, g, s = step(pts)                                         # (N,1), (N,3), (N,3); differentiable once more (loss.backward())
        g0 = step.first_order(pts0)                                 # d sdf / dx only, no graph (implicit_surface.py:305-310)

    `volumes`: the planar (1,4,X,Y,Z) tensors the gradient goes to; `packed`: their (X,Y,Z,4) texel copy the kernels read."""

    @staticmethod
    def supported(net, n_levels):
        return SdfMlpPlan.supported(net) and float(net.scale) == 1.0 and 1 <= n_levels <= 5 and net.init_feat_channels == 4 * n_levels

    def __init__(self, weights, biases, volumes, packed, raw=None, tv_masks=None):
        """weights / biases: the EFFECTIVE matrices with autograd history (torch._weight_norm's outputs) -- or, with raw = (weight_v list,
        weight_g list, bias list) of lin0..lin6, None: weight norm then happens inside the pack launch and its backward inside the
        gradient launch (gens_sdf_train_pack_wn / gens_sdf_train_wgrad), and the raw parameters are the autograd inputs.
        tv_masks: the mask pyramid; with it `step(pts, sel, tv=True)` also returns tv_regularization(volumes, masks) (implicit_surface.py:
        135-150) so that the dense TV gradient and the scattered look-up gradient of the volumes are formed in ONE buffer."""
        assert isinstance(packed, VolumeSet) and packed.layout == L.LAYOUT_PACKED and 1 <= packed.n <= 5
        self.volumes, self.packed = list(volumes), packed
        self.n_levels = packed.n
        self.raw = raw
        self.tv_masks = None if tv_masks is None else [_c(m.detach()) for m in tv_masks]
        dev = self.volumes[0].device if self.volumes else packed.tensors[0].device
        kin = 128 + 20 * self.n_levels
        self.kp = (kin + 1 + 7) // 8 * 8
        gf = [(27 + 1 + 7) // 8] + [self.kp // 8] * 5
        # backward n-tiles of layers 1..5: four hidden tiles + the conditioning tiles, padded to two or four (zero columns): the four waves of a
        # workgroup take one tile each or two share one (k17_sdf_train.hip: NT_B)
        n_cond = (20 * self.n_levels + 31) // 32
        ntb = [1] + [4 + (2 if n_cond <= 2 else 4)] * 5
        self.wf = [torch.empty(4 * g * 64 * 4, device=dev, dtype=_f32) for g in gf]
        self.wb = [torch.empty(nt * 16 * 64 * 4, device=dev, dtype=_f32) for nt in ntb]
        self.wf_table, self.wb_table = L.ptr_table(self.wf), L.ptr_table(self.wb)
        with torch.no_grad():
            if raw is None:
                assert len(weights) == 7 and len(biases) == 7
                self.tensors = [*weights, *biases]
                w = [_c(t.detach().to(_f32)) for t in weights[:6]]
                b = [_c(t.detach().to(_f32)) for t in biases[:6]]
                assert tuple(w[0].shape) == (128, 27) and tuple(w[2].shape) == (101, kin) and tuple(w[5].shape) == (128, kin)
                L.call("gens_sdf_train_pack", L.ptr_table(w), L.ptr_table(b), self.n_levels, self.wf_table, self.wb_table, L.stream())
                self.w_last = _c(weights[6].detach().to(_f32)[0].clone())
                self.b_last = _c(biases[6].detach().to(_f32)[:1].clone())
            else:
                vs, gs, bs = raw
                assert len(vs) == len(gs) == len(bs) == 7
                self.tensors = [*vs, *gs, *bs]
                self.v = [_c(t.detach().to(_f32)) for t in vs]
                self.g = [_c(t.detach().to(_f32).reshape(-1)) for t in gs]
                b = [_c(t.detach().to(_f32)) for t in bs]
                assert tuple(self.v[0].shape) == (128, 27) and tuple(self.v[2].shape) == (101, kin) and tuple(self.v[6].shape) == (129, kin)
                self.scale = [torch.empty(t.shape[0], device=dev, dtype=_f32) for t in self.v]
                self.w_last, self.b_last = torch.empty(kin, device=dev, dtype=_f32), torch.empty(1, device=dev, dtype=_f32)
                L.call("gens_sdf_train_pack_wn", L.ptr_table(self.v), L.ptr_table(self.g), L.ptr_table(b), self.n_levels, L.ptr_table(self.scale),
                       self.wf_table, self.wb_table, L.ptr(self.w_last), L.ptr(self.b_last), L.stream(), label="gens_sdf_train_pack")

    def _forward(self, pts, sel=None):
        """sel (StepPoints): evaluate pts[sel.idx[:count]] with the count left on the device and write rows sel.idx[i] of sel's dense
        outputs (their other rows already hold the reference's defaults); None: every row of pts, fresh outputs."""
        n = pts.shape[0]
        dev = pts.device
        stash = torch.empty(L.load().gens_sdf_train_stash_bytes(n, 0), device=dev, dtype=torch.uint8)
        if sel is None:
            y, g, s = (torch.empty(n, k, device=dev, dtype=_f32) for k in (1, 3, 3))
            idx = cnt = None
        else:
            y, g, s, idx, cnt = sel.y, sel.g, sel.s, sel.idx, sel.counts[0:1]
        fe = 20 * self.n_levels
        flops = 4 * 2 * (27 * 128 + (128 + fe) * (4 * 128 + 101 + 1))
        L.call("gens_sdf_train_fwd", self.packed.table, self.packed.dim_table, self.n_levels, self.wf_table, self.wb_table, L.ptr(self.w_last),
               L.ptr(self.b_last), L.ptr(pts), L.ptr(idx, torch.int64), n, L.ptr(cnt, torch.int32), L.ptr(stash, torch.uint8), L.ptr(y), L.ptr(g),
               L.ptr(s), L.stream(), nbytes=n * 40, flops=n * flops, live=None if cnt is None else (cnt, n))
        return y, g, s

    def __call__(self, pts, sel=None, tv=False):
        """-> (y, g, s) [, tv_reg when tv=True (needs tv_masks)]."""
        out = _SdfTrain.apply(_c(pts.detach().reshape(-1, 3).to(_f32)), self, sel, bool(tv), *self.tensors, *self.volumes)
        return out if tv else out[:3]

    @torch.no_grad()
    def first_order(self, pts):
        return self._forward(_c(pts.detach().reshape(-1, 3).to(_f32)))[1]


class _SdfTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pts, step, sel, tv, *tensors):
        # (NOT ctx.sel = sel: sel.y / sel.g / sel.s are this Function's OUTPUTS -- node -> sel -> output tensor -> grad_fn -> node is a cycle the
        # collector cannot break (the last edge lives in C++), so every training step would leave this node, the blending node behind sel.rgb and
        # everything they hold on the device for ever: 1.9 MB per step on the small test model, scripts/probe/eager_leak_probe.py)
        ctx.step = step
        ctx.sel_index = None if sel is None else (sel.idx, sel.counts[0:1])
        ctx.shapes = [t.shape for t in tensors]
        ctx.n_par = len(step.tensors)
        y, g, s = step._forward(pts, sel)
        tv_out = None
        if tv:
            assert step.tv_masks is not None, "SdfTrainStep(tv_masks=...) is needed for tv=True"
            nl = step.n_levels
            vols = [_c(v.detach()) for v in step.volumes]
            ctx.tv_dims = [d for v in vols for d in v.shape[-3:]]
            partial = torch.empty(L.load().gens_tv_levels_blocks(L.int_table(ctx.tv_dims), nl), 4, device=pts.device, dtype=_f32)
            tv_out = torch.empty(1 + nl, device=pts.device, dtype=_f32)
            L.call("gens_tv_levels_fwd", L.ptr_table(vols, align=16), L.ptr_table(step.tv_masks, align=16), L.int_table(ctx.tv_dims), nl, L.ptr(partial),
                   L.ptr(tv_out), L.stream(), nbytes=sum(20 * v[0, 0].numel() for v in vols))
            ctx.save_for_backward(pts, tv_out, *vols)
            return y, g, s, tv_out[0]
        ctx.save_for_backward(pts)
        return y, g, s, None

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, y_bar, g_bar, s_bar, tv_bar):
        step = ctx.step
        pts, *tv_saved = ctx.saved_tensors
        n, dev = pts.shape[0], pts.device
        idx, cnt = (None, None) if ctx.sel_index is None else ctx.sel_index
        nl = step.n_levels
        cf, fe, kin = 4 * nl, 20 * nl, 128 + 20 * nl
        fep = step.kp - 128
        npad = (n + 31) // 32 * 32
        f = lambda *shape: torch.empty(*shape, device=dev, dtype=_f32)  # noqa: E731
        lop, rh, re, r0 = f(npad, 4, 6, 128), f(5, npad, 4, 128), f(npad, 4, fep), f(npad, 4, 32)      # point-major operand rows
        f_hat, mu_f, lam_f, w6p = f(npad, cf), f(npad, cf), f(npad, cf), f(npad // 16, step.kp)     # (a row per 16-point workgroup of the launch)
        stash = torch.empty(L.load().gens_sdf_train_stash_bytes(n, 1), device=dev, dtype=torch.uint8)
        cot = [None if t is None else _c(t.to(_f32)) for t in (y_bar, g_bar, s_bar)]
        flops = 8 * 2 * (27 * 128 + (128 + fe) * (4 * 128 + 101 + 1))
        live = None if cnt is None else (cnt, n)
        L.call("gens_sdf_train_bwd", step.packed.table, step.packed.dim_table, nl, step.wf_table, step.wb_table, L.ptr(step.w_last), L.ptr(pts),
               L.ptr(idx, torch.int64), n, L.ptr(cnt, torch.int32), L.ptr(cot[0]), L.ptr(cot[1]), L.ptr(cot[2]), L.ptr(stash, torch.uint8), L.ptr(lop),
               L.ptr(rh), L.ptr(re), L.ptr(r0), L.ptr(f_hat), L.ptr(mu_f), L.ptr(lam_f), L.ptr(w6p), L.stream(),
               nbytes=n * (40 + 4 * (4 * 6 * 128 + 6 * 4 * 128 + 4 * fep + 4 * 32 + 3 * cf)), flops=n * flops, live=live)
        # weight gradients: eleven products over the 4 * npad operand rows in ONE launch (rows of padding points are zero on one side of
        # every product).  Per layer l = 1..5 the hidden columns (lop_l^T rh_l) and the conditioning columns + bias (lop_l^T re) are
        # neighbours in the unit list, so the second product finds lop_l's slab in L2 instead of reading it from HBM again; layer 0 last.
        k = 4 * npad
        fl = 4                                                            # bytes per float
        a_ptr, b_ptr, ldb, ms, ns = [], [], [], [], []
        for l in range(1, 6):
            a_ptr += [lop.data_ptr() + fl * 128 * l] * 2
            b_ptr += [rh.data_ptr() + fl * (l - 1) * k * 128, re.data_ptr()]
            ldb += [128, fep]
            ms += [128, 128]
            ns += [128, fep]
        a_ptr.append(lop.data_ptr())
        b_ptr.append(r0.data_ptr())
        ldb.append(32)
        ms.append(128)
        ns.append(32)
        n_prod = len(ms)
        mi, ni = L.int_table(ms), L.int_table(ns)
        ws = f(L.load().gens_gemm_tn_batch_workspace(n_prod, mi, ni, k))
        sizes = [m * n_ for m, n_ in zip(ms, ns)]
        cc = f(sum(sizes))
        tab = lambda v: C.cast((C.c_void_p * len(v))(*v), C.POINTER(C.c_void_p))  # noqa: E731
        if idx is None:
            L.call("gens_gemm_tn_batch", n_prod, tab(a_ptr), L.int_table([768] * n_prod), tab(b_ptr), L.int_table(ldb), mi, ni, k,
                   L.ptr(ws), L.ptr(cc), L.stream(), nbytes=fl * k * (768 + 32 + 5 * 128 + fep), flops=2 * k * sum(sizes))
        else:       # only the operand rows of the points that exist (32 points -> 128 rows per workgroup of the backward launch)
            L.call("gens_gemm_tn_batch_live", n_prod, tab(a_ptr), L.int_table([768] * n_prod), tab(b_ptr), L.int_table(ldb), mi, ni, k,
                   L.ptr(cnt, torch.int32), 32, 128, L.ptr(ws), L.ptr(cc), L.stream(), nbytes=fl * k * (768 + 32 + 5 * 128 + fep),
                   flops=2 * k * sum(sizes), live=live, label="gens_gemm_tn_batch")
        w6s = w6p.sum(0)
        n_par = ctx.n_par
        if step.raw is not None:
            # d loss / d (weight_v, weight_g, bias) of lin0..lin6 in ONE launch, weight norm's backward included; the 21 gradients are views
            # of one flat buffer (contiguous each: autograd installs them as .grad without a copy)
            sizes_v = [v.numel() for v in step.v]
            rows = [v.shape[0] for v in step.v]
            flat = f(sum(sizes_v) + 2 * sum(rows))
            dv, dg, db, off = [], [], [], 0
            for v in step.v:
                dv.append(flat[off:off + v.numel()].view(v.shape))
                off += v.numel()
            for r in rows:
                dg.append(flat[off:off + r])
                off += r
            for r in rows:
                db.append(flat[off:off + r])
                off += r
            L.call("gens_sdf_train_wgrad", L.ptr_table(step.v), L.ptr_table(step.g), nl, L.ptr(cc), L.ptr(w6s), L.ptr_table(dv), L.ptr_table(dg),
                   L.ptr_table(db), L.stream())
            g_par = [*dv, *[d.view(ctx.shapes[7 + k]) for k, d in enumerate(dg)], *db]
        else:
            parts, off = [], 0
            for m, n_ in zip(ms, ns):
                parts.append(cc[off:off + m * n_].view(m, n_))
                off += m * n_
            w0 = parts[10]
            g_w, g_b = [w0[:, :27]], [w0[:, 27]]
            for l in range(1, 6):
                rows = 101 if l == 2 else 128
                h, e_l = parts[2 * (l - 1)], parts[2 * (l - 1) + 1]
                g_w.append(torch.cat([h, e_l[:, :fe]], 1)[:rows])
                g_b.append(e_l[:rows, fe])
            w6 = torch.zeros(ctx.shapes[6], device=dev, dtype=_f32)
            w6[0] = w6s[:kin]
            b6 = torch.zeros(ctx.shapes[13], device=dev, dtype=_f32)
            b6[0] = w6s[kin]
            g_par = [*g_w, w6, *g_b, b6]
        # volume gradients: the dense TV gradient (when the step carries the regulariser) is WRITTEN first, the look-up's scatter adds into it
        g_vols = [None] * nl
        if any(ctx.needs_input_grad[4 + n_par:]):
            have_tv = bool(tv_saved) and tv_bar is not None
            if have_tv:
                tv_out, *vols = tv_saved
                g_vols = [torch.empty(s, device=dev, dtype=_f32) for s in ctx.shapes[n_par:]]
                L.call("gens_tv_levels_bwd", L.ptr_table(list(vols), align=16), L.ptr_table(step.tv_masks, align=16), L.int_table(ctx.tv_dims), nl,
                       L.ptr(tv_out), L.ptr(_c(tv_bar.detach().to(_f32).reshape(1))), L.ptr_table(g_vols, align=16), L.stream(),
                       nbytes=sum(36 * v[0, 0].numel() for v in vols))
            else:
                g_vols = [torch.zeros(s, device=dev, dtype=_f32) for s in ctx.shapes[n_par:]]
            L.call("gens_sdf_train_scatter", step.packed.dim_table, nl, L.ptr(pts), L.ptr(cot[1]), L.ptr(cot[2]), L.ptr(f_hat), L.ptr(mu_f),
                   L.ptr(lam_f), L.ptr(idx, torch.int64), n, L.ptr(cnt, torch.int32), L.ptr_table(g_vols), L.stream(), nbytes=n * (36 + 3 * 4 * cf),
                   live=live)
        return (None, None, None, None, *g_par, *g_vols)


__all__ = [n_ for n_ in dir() if not n_.startswith("__")]      # private helpers travel too: the package namespace is the old module's
