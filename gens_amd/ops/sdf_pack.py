"""The weight streams of the fused networks: the seven effective matrices of the SDF network (and the narrow layers of the blending
network) laid out as the MFMA operand streams their inference kernels consume.  Host code only: everything here runs on whatever device
the weights live on, a CPU included (tests/test_sdf_pack_cpu.py pins every stream bit for bit).

Part of gens_amd.ops (see ops/__init__.py); citations are relative to /root/reference."""
from .base import *  # noqa: F401,F403

_C = 100.0 / math.log(2.0)          # hidden units travel as c * softplus: columns fed by unscaled inputs (encodings, the one) carry c
_R2 = 1.0 / math.sqrt(2.0)          # layer 3's x = cat([h[:101], pe]) / sqrt(2)   (sdf_network.py:111-112)


def _pack_b_groups(w):
    """(J, K) matrix -> grouped fp32 MFMA B stream for gens_sdf_mlp: [ceil(J/32)][ceil(K/8)][64][4]; lane l of group
    (nt, g) holds w[32 nt + (l & 31)][8 g + 4 (l >> 5) + 0..3] (zero padded): one global_load_dwordx4 feeds 4 MFMAs."""
    j, k = w.shape
    nt, g = (j + 31) // 32, (k + 7) // 8
    wp = torch.zeros(nt * 32, g * 8, device=w.device, dtype=_f32)
    wp[:j, :k] = w
    return wp.view(nt, 32, g, 2, 4).permute(0, 2, 3, 1, 4).contiguous()


def _pack_b16(w, groups):
    """(J <= 16, K) matrix -> B stream of a narrow layer for two 16x16x4 fp32 MFMA tiles (k7_blend.hip::narrow_group): for every group
    (k0, S) of 4 S reduction columns, 64 lanes x S floats; lane l holds w[l % 16][k0 + S (l // 16) + 0..S-1] (zero padded)."""
    j, k = w.shape
    assert j <= 16
    kmax = max(k0 + 4 * s for k0, s in groups)
    wp = torch.zeros(16, kmax, device=w.device, dtype=_f32)
    wp[:j, :k] = w
    parts = []
    for k0, s in groups:
        blk = wp[:, k0:k0 + 4 * s].reshape(16, 4, s)           # [j][q][s]
        parts.append(blk.permute(1, 0, 2).reshape(-1))         # lane = q * 16 + j
    return torch.cat(parts).contiguous()


# ------------------------------------------------------------------------------------------------------------------
# the pieces every SDF stream is made of: slot tables, the gather, the forward layers, the reverse layers, the output row
# ------------------------------------------------------------------------------------------------------------------
def _slot_tables(n_levels, width):
    """Which input column every operand slot carries, for lane halves of `width` slots (8: k6v / k6gh / k6b, 4: k6t / k6g): three tables
    (blocks, half, width) of column numbers, -1 for the constant-one slot and -2 for a zero slot.  Hidden block B: the accumulator layout of
    the previous layer, slot s of half h = feature 2 width B + 8 (s >> 2) + 4 h + (s & 3).  Point encoding: half 0 pe[0:15], half 1
    pe[15:27]; the one sits in half 0's slot 15 (width 8) or right behind pe[15:27] in half 1 (width 4).  Volume features: half 0 the channels
    of the levels below the middle one and its first two, half 1 the levels above and its last two (an odd level count shares the middle level,
    two channels per half); five encodings per channel (column e * CF + channel, sdf_network.py:104-107), then the one (half 0)."""
    cf = 4 * n_levels
    nch, mid, odd = cf // 2, n_levels // 2, n_levels % 2
    hid = torch.tensor([[[2 * width * b + 8 * (s >> 2) + 4 * h + (s & 3) for s in range(width)] for h in range(2)] for b in range(64 // width)])
    pe = torch.full((16 // width, 2, width), -2, dtype=torch.long)
    for q in range(15):
        pe[q // width, 0, q % width] = q
        if q < 12:
            pe[q // width, 1, q % width] = 15 + q
    one_half, one_slot = (0, 15) if width == 8 else (1, 12)
    pe[one_slot // width, one_half, one_slot % width] = -1
    cond = torch.full(((5 * nch + 1 + width - 1) // width, 2, width), -2, dtype=torch.long)
    for h in range(2):
        nfull = 4 * mid                                       # whole levels of a half: the first / the last n_levels // 2
        for lc in range(nch):
            ch = (lc if h == 0 else 4 * (mid + odd) + lc) if lc < nfull else 4 * mid + 2 * h + (lc - nfull)
            for e in range(5):
                q = 5 * lc + e
                cond[q // width, h, q % width] = e * cf + ch
    cond[(5 * nch) // width, 0, (5 * nch) % width] = -1
    return hid, pe, cond


def _value_slots(n_levels):
    """Slot tables of k6v_sdf_value_f16.hip (and k6gh, k6b), (blocks, half, 8) each: _slot_tables at 8 slots per lane half.  Register r of
    accumulator tile t = slot r & 7 of hidden block 2 t + (r >> 3)."""
    return _slot_tables(n_levels, 8)


def _value_pairs(n_levels):
    """Slot tables of k6t_sdf_value.hip (and k6g), (groups, half, 4) each: _slot_tables at 4 slots per lane half.  An MFMA of group g, position
    i multiplies the weights of the two columns [g, 0, i] and [g, 1, i] with what the two lane halves hold; hidden group (t, g') = 4 t + g'."""
    return _slot_tables(n_levels, 4)


def _flat(table):
    """(blocks, half, width) -> (half, slot): the slots of a lane half in a row."""
    return table.permute(1, 0, 2).reshape(2, -1)


def _gather(mat, table, offset=0):
    """mat (32 NT, K + 2): the rows of NT output tiles; column K = what the constant-one slot multiplies, column K + 1 zeros (a table without
    negative entries needs neither).  table (B, 2, W): entry e >= 0 reads column offset + e.  -> (B, NT, 64, W): block, tile, lane = 32 half
    + m, slot."""
    nt, k = mat.shape[0] // 32, mat.shape[1] - 2
    cols = torch.where(table >= 0, table + offset, torch.where(table == -1, torch.full_like(table, k), torch.full_like(table, k + 1)))
    g = mat[:, cols.reshape(-1)].reshape(nt, 32, *table.shape)                    # [tile][m][block][half][slot]
    return g.permute(2, 0, 3, 1, 4).reshape(table.shape[0], nt, 64, table.shape[2])


def _rows128(w):
    """(J <= 128, K) -> (128, K), zero rows below."""
    out = torch.zeros(128, w.shape[1], device=w.device, dtype=_f32)
    out[:w.shape[0]] = w
    return out


def _forward_layers(ws, bs):
    """The forward operands of lin0..lin5, padded to 128 rows and scaled: per layer (hidden, skip, rest), each ready for _gather.
    hidden (128, 128): the columns fed by the (pre-scaled) hidden units, layer 3's times 1 / sqrt(2) and zero from column 101 on; None at
    layer 0.  skip (128, 27 + 2), layer 3 only: c / sqrt(2) times the point-encoding columns, nothing for the one.  rest (128, K + 2): c times
    the remaining input columns (layer 0: the point encoding, else the volume features), c times the bias for the one slot, zeros."""
    zero = torch.zeros(128, 1, device=ws[0].device, dtype=_f32)
    for l in range(6):
        w, b = _rows128(ws[l]), _rows128(bs[l][:, None])
        if l == 0:
            yield None, None, torch.cat([_C * w, _C * b, zero], 1)
            continue
        h, skip = w[:, :128].clone(), None
        if l == 3:
            skip = torch.cat([_C * _R2 * w[:, 101:128], zero, zero], 1)
            h = _R2 * h
            h[:, 101:] = 0.0
        yield h, skip, torch.cat([_C * w[:, 128:], _C * b, zero], 1)


def _forward_blocks(ws, bs, tables, parts, hid3=None, order="block"):
    """The forward half of a stream as a list of _gather results: layer 0's point-encoding blocks, then per layer 1..5 its "hid", "skip"
    (layer 3 only) and "cond" blocks in the sequence `parts`.  hid3: how many hidden blocks layer 3 reads (default: all).
    order: "block" -- every entry [block][tile]; "tile" -- one entry per layer, [tile][block] over all of the layer's blocks."""
    assert order in ("block", "tile")
    hid, pe, cond = tables
    pe_skip = torch.where(pe == -1, torch.full_like(pe, -2), pe)                  # the one slot of the point encoding carries nothing at the skip
    out = []
    for l, (h, skip, rest) in enumerate(_forward_layers(ws, bs)):
        if l == 0:
            layer = [_gather(rest, pe)]
        else:
            part = {"hid": _gather(h, hid[:hid3] if l == 3 else hid), "cond": _gather(rest, cond)}
            if l == 3:
                part["skip"] = _gather(skip, pe_skip)
            layer = [part[name] for name in parts if name in part]
        out += layer if order == "block" else [torch.cat(layer, 0).transpose(0, 1)]
    return out


def _slot_rows(src, flat, n_tiles):
    """Rows of a reverse-pass operand, ordered as the accumulator that receives them: accumulator row m of a tile <-> (lane half, register)
    by m = 8 (r >> 2) + 4 half + (r & 3).  -> (32 n_tiles, 128): row 32 c + m = src[:, column of slot 16 c + reg(m) of half(m)] (zero where
    the slot carries no column), so that lane half h, register r of tile c receives the gradient of that half's slot 16 c + r."""
    m = torch.arange(32, device=src.device)
    row_half, row_reg = (m >> 2) & 1, ((m >> 3) << 2) | (m & 3)
    mat = torch.zeros(32 * n_tiles, 128, device=src.device, dtype=_f32)
    for cc in range(n_tiles):
        slot = 16 * cc + row_reg
        col = torch.where(slot < flat.shape[1], flat[row_half, slot.clamp(max=flat.shape[1] - 1)], torch.full_like(slot, -2))
        live = col >= 0
        mat[32 * cc + m[live]] = src[:, col[live]].t()
    return mat


def _reverse_layers(ws, pe, cond, tc):
    """The reverse pass on the TRUE (unscaled) transposed matrices, layer 5 down to 1: per layer (l, hidden, cond_rows, pe_rows).
    hidden (128, 128) = W_l[:, :128]^T (rows: hidden inputs, columns: units of layer l; layer 3 as in the forward pass); cond_rows (32 tc, 128)
    and pe_rows (32, 128) = _slot_rows of the conditioning / point-encoding columns -- pe_rows at layer 3 (the skip) and at layer 1, where it is
    W_0^T, the layer that follows; None elsewhere."""
    pe_flat, cond_flat = _flat(pe), _flat(cond)
    for l in range(5, 0, -1):
        w = _rows128(ws[l])
        wt = w[:, :128].t().clone()
        if l == 3:
            wt = _R2 * wt
            wt[101:] = 0.0
        pe_src = _R2 * w[:, 101:128] if l == 3 else _rows128(ws[0]) if l == 1 else None
        yield l, wt, _slot_rows(w[:, 128:], cond_flat, tc), None if pe_src is None else _slot_rows(pe_src, pe_flat, 1)


def _output_row(w_last, cond, width):
    """lin6 as the kernels' last step reads it, (2, 64 + width) per lane half: the weights of the half's 64 accumulator registers (feature
    32 t + 8 (r >> 2) + 4 half + (r & 3) for register r of tile t) over c, then those of its first `width` conditioning slots (cond: the
    conditioning table; zero for the one, for empty slots and past the table)."""
    dev = w_last.device
    w_out = torch.zeros(2, 64 + width, device=dev, dtype=_f32)
    for hh in range(2):
        feat = torch.tensor([32 * t + 8 * (r >> 2) + 4 * hh + (r & 3) for t in range(4) for r in range(16)], device=dev)
        w_out[hh, :64] = w_last[feat] / _C
        tb = _flat(cond)[hh][:width]
        w_out[hh, 64:64 + tb.shape[0]] = torch.where(tb >= 0, w_last[(128 + tb).clamp(0, w_last.shape[0] - 1)], torch.zeros_like(tb, dtype=_f32))
    return w_out


# ------------------------------------------------------------------------------------------------------------------
# the four streams: the order in which each kernel consumes the blocks, and its tail
# ------------------------------------------------------------------------------------------------------------------
def _pack_value_stream(ws, bs, n_levels):
    """The float32 weight stream and output row of gens_sdf_value (k6t_sdf_value.hip): per group of four feature pairs and output tile
    T one float4 per lane (m, half) = the weights of row 32 T + m for the group's four columns of that half; columns fed by unscaled
    inputs carry 100 / ln 2 (pre-scaled hidden units), layer 3's hidden columns 1 / sqrt(2), its skip columns both.  Order: layer 0's
    point-encoding groups, then per layer the hidden groups (layer 3 reads features 0..103 only: 13 groups), (layer 3: the skip groups,) the
    conditioning groups; one zero group is appended because the kernel requests the next group before it knows there is none.
    ws[l] (out_l, in_l) and bs[l] are the effective float32 weights of lin0..lin6.  -> (stream (NG + 1, 4, 64, 4), w_out)."""
    dev = ws[0].device
    tables = [t.to(dev) for t in _value_pairs(n_levels)]
    out = _forward_blocks(ws, bs, tables, ("hid", "skip", "cond"), hid3=13)
    out.append(torch.zeros(1, 4, 64, 4, device=dev, dtype=_f32))
    return torch.cat(out, 0).contiguous(), _output_row(ws[6][0], tables[2], 4 * tables[2].shape[0])


def _pack_grad_stream(ws, bs, n_levels):
    """The weight stream and output row of gens_sdf_grad (k6g_sdf_grad.hip): the forward groups of _pack_value_stream, then the reverse
    pass on the TRUE (unscaled) transposed matrices, layer 5 down to 1: 16 groups (layer 2: 13) of W_l[:, :128]^T for the hidden-unit
    gradients, then per pair of conditioning tiles 8 groups (layer 2: 7) of 2 tiles x 8 pairs whose ROWS are ordered so that lane half h,
    register r of tile c receives the gradient of that half's slot 16 c + r, at layer 3 four groups of 1 tile x 16 pairs for the
    point-encoding slots, and after layer 1 the same four groups of W_0^T; two trailing zero groups (the kernel reads two groups ahead)."""
    dev = ws[0].device
    hid, pe, cond = tables = [t.to(dev) for t in _value_pairs(n_levels)]
    tc = ((10 * n_levels + 15) // 16 + 1) // 2 * 2           # conditioning-gradient tiles, in pairs (k6g_sdf_grad.hip: GradShapeT::TC)
    out = _forward_blocks(ws, bs, tables, ("hid", "skip", "cond"), hid3=13)
    for l, wt, cond_rows, pe_rows in _reverse_layers(ws, pe, cond, tc):
        out.append(_gather(wt, hid[:13] if l == 2 else hid))
        full = _gather(cond_rows, hid)                                    # (16 = (t, g), tc, 64, 4)
        for cc in range(0, tc, 2):
            for p in range(7 if l == 2 else 8):                           # a pair of groups x a pair of tiles
                a, b = full[2 * p], full[2 * p + 1]
                out.append(torch.stack([a[cc], b[cc], a[cc + 1], b[cc + 1]])[None])
        if pe_rows is not None:
            out.append(_gather(pe_rows, hid)[:, 0].reshape(4, 4, 64, 4))  # group t: the four float4 g = 0..3
    out.append(torch.zeros(2, 4, 64, 4, device=dev, dtype=_f32))
    return torch.cat(out, 0).contiguous(), _output_row(ws[6][0], cond, 16 * tc)


def _pack_value_units(ws, bs, n_levels):
    """The weight stream and the output row of gens_sdf_value_f16 (layout and scaling: k6v_sdf_value_f16.hip's header): the order of
    _pack_value_stream in units of one 16-deep K block (8 slots per lane half, layer 3 with all eight hidden blocks), padded with zeros to
    whole chunks of four units, every unit split into hi and lo halfs.  Returns (units (U, 4, 2, 64, 8) float16, w_out (2, 64 + 8 NC)
    float32, largest magnitude handed to half precision)."""
    dev = ws[0].device
    tables = [t.to(dev) for t in _value_slots(n_levels)]
    units = torch.cat(_forward_blocks(ws, bs, tables, ("hid", "skip", "cond")), 0)
    pad = (-units.shape[0]) % 4                                                  # whole chunks of four units
    if pad:
        units = torch.cat([units, torch.zeros(pad, *units.shape[1:], device=dev, dtype=_f32)], 0)
    hi = units.half()
    lo = (units - hi.float()).half()
    stream = torch.stack([hi, lo], 2).contiguous()                               # [unit][tile][hi, lo][lane][slot]
    return stream, _output_row(ws[6][0], tables[2], 8 * tables[2].shape[0]), float(units.abs().max())


def _pack_grad_pieces(ws, bs, n_levels, n_pieces=None, terms=2, hid3=None, order="block"):
    """The piece stream of gens_sdf_grad_f16 (k6gh_sdf_grad_f16.hip): 1 KB pieces = the A operand (hi or lo halfs) of one 32-row output
    tile and one 16-deep K block, lane (m, kh) holding row m's weights for the eight reduction slots of lane half kh (_value_slots).
    Forward: layer 0's two point-encoding K blocks, then per layer the conditioning K blocks, (layer 3: the point-encoding blocks,) the
    eight hidden blocks -- the scaling of _pack_value_units, 4 tiles x {hi, lo} per block.  Reverse, on the TRUE transposed matrices,
    layer 5 down to 1: per K block of G_l (layer 2: seven) the four hidden tiles, the conditioning tiles and at layer 3 the
    point-encoding tile, rows ordered as in _pack_grad_stream; then the eight blocks of G_0 for the point-encoding tile.  Padded with
    zeros to whole chunks of eight pieces.  -> (pieces (N, 64, 8) float16, largest magnitude handed to half precision).
    terms=3: the stream of gens_sdf_value_bf16x3 / gens_sdf_grad_bf16x3 (k6b_sdf_bf16x3.hip) -- the same order with three round-to-nearest
    bfloat16 terms (x0, x1, x2) per (block, tile) instead of (hi, lo): -> (pieces (N, 64, 8) bfloat16, largest magnitude).
    hid3: how many hidden K blocks forward layer 3 keeps (default: all eight).  The layer's hidden inputs end at unit 100, so block 7 (units
    112..127) is zeros by construction (_forward_layers); the bf16x3 kernels read seven (SdfMlpPlan asks the library), the split-half
    kernel reads all eight.
    order="tile": the value-only stream of the two-wave gens_sdf_value_bf16x3 kernel -- the forward pieces alone, the same bytes, within
    every layer [tile][block][term] instead of [block][tile][term], so that the kernel can finish (and activate) one output tile at a time."""
    assert order in ("block", "tile")
    dev = ws[0].device
    hid, pe, cond = tables = [t.to(dev) for t in _value_slots(n_levels)]
    out = _forward_blocks(ws, bs, tables, ("cond", "skip", "hid"), hid3=hid3, order=order)
    for l, wt, cond_rows, pe_rows in _reverse_layers(ws, pe, cond, (10 * n_levels + 15) // 16) if order == "block" else ():
        out.append(_gather(torch.cat([wt, cond_rows] + ([pe_rows] if l == 3 else []), 0), hid[:7] if l == 2 else hid))     # [block][tile]
        if l == 1:
            out.append(_gather(pe_rows, hid))                                     # G_0 for the point-encoding tile
    tiles = torch.cat([o.reshape(-1, 64, 8) for o in out], 0)                     # one row per (block, tile)
    if terms == 3:
        parts, rest = [], tiles
        for _ in range(3):                                                        # x - x0 and x - x0 - x1 are exact in float32
            parts.append(rest.bfloat16())
            rest = rest - parts[-1].float()
    else:
        hi = tiles.half()
        parts = [hi, (tiles - hi.float()).half()]
    pieces = torch.stack(parts, 1).reshape(-1, 64, 8)                             # [block][tile][hi, lo] / [x0, x1, x2]
    pad = (-pieces.shape[0]) % 8 if n_pieces is None else n_pieces - pieces.shape[0]      # (whole chunks of the kernel's ring)
    if pad:
        pieces = torch.cat([pieces, torch.zeros(pad, 64, 8, device=dev, dtype=pieces.dtype)], 0)
    return pieces.contiguous(), float(tiles.abs().max())


__all__ = [n_ for n_ in dir() if not n_.startswith("__")]      # private helpers travel too: the package namespace is the old module's
