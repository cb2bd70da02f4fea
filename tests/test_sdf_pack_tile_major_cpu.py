"""The two bf16x3 streams the plan ships, held on the CPU to the stream tests/golden/g22_sdf_pack.json pins (_pack_grad_pieces(terms=3): block
major, layer 3 with all eight hidden blocks).

  * hid3=7 drops forward layer 3's eighth hidden K block from the gradient stream: the dropped pieces are exactly that block's, every byte of
    them is zero, no other piece of the layer is all zero, and the rest of the stream is untouched.
  * order="tile" is the value-only stream of the two-wave value kernel's tile-major build (GENS_K6B_TILE_MAJOR=1): the forward pieces of the hid3=7 stream, byte for byte, permuted from
    [layer][block][tile][term] to [layer][tile][block][term], then zero padding to whole chunks of eight.

Seeded weights at 3 and 5 levels; no GPU."""
import pytest
import torch

from gens_amd import ops

TERMS, TILES = 3, 4


def _weights(n_levels, seed):
    g = torch.Generator().manual_seed(seed)
    k_in = 128 + 20 * n_levels
    dims = [(128, 27), (128, k_in), (101, k_in), (128, k_in), (128, k_in), (128, k_in), (1, k_in)]
    ws = [torch.randn(o, i, generator=g) * (1.5 / i ** 0.5) for o, i in dims]
    bs = [torch.randn(o, generator=g) * 0.1 for o, _ in dims]
    return ws, bs


def _layer_blocks(n_levels, hid3):
    """K blocks of forward layers 0..5: the point encoding; conditioning (+ the two skip blocks at layer 3) + hidden blocks."""
    nc = (5 * 2 * n_levels + 1 + 7) // 8
    return [2] + [nc + (2 + hid3 if l == 3 else 8) for l in range(1, 6)]


@pytest.fixture(scope="module", params=[3, 5])
def streams(request):
    n_levels = request.param
    ws, bs = _weights(n_levels, seed=290 + n_levels)
    full, vmax = ops._pack_grad_pieces(ws, bs, n_levels, terms=3)
    grad, vmax7 = ops._pack_grad_pieces(ws, bs, n_levels, terms=3, hid3=7)
    value, _ = ops._pack_grad_pieces(ws, bs, n_levels, terms=3, hid3=7, order="tile")
    assert full.dtype == grad.dtype == value.dtype == torch.bfloat16 and vmax == vmax7
    as_bytes = lambda t: t.contiguous().view(torch.uint8).reshape(t.shape[0], -1)  # noqa: E731
    return n_levels, as_bytes(full), as_bytes(grad), as_bytes(value)


def test_the_dropped_pieces_are_exactly_the_all_zero_ones(streams):
    n_levels, full, grad, _ = streams
    blocks8 = _layer_blocks(n_levels, 8)
    per_block = TILES * TERMS
    first = per_block * (sum(blocks8[:3]) + blocks8[3] - 1)          # layer 3's last block: hidden units 112..127
    dropped = torch.arange(first, first + per_block)
    keep = torch.ones(full.shape[0], dtype=torch.bool)
    keep[dropped] = False
    assert not full[dropped].any()
    lo, hi = per_block * sum(blocks8[:3]), per_block * sum(blocks8[:4])
    zero = ~(full[lo:hi] != 0).any(1)
    assert torch.equal(torch.nonzero(zero)[:, 0] + lo, dropped)      # ... and layer 3 has no other all-zero piece
    strip = lambda t: t[:int((t != 0).any(1).nonzero().max()) + 1]         # noqa: E731  (without the trailing padding)
    body = strip(full[keep])                                         # every other piece, forward and reverse, unchanged and in order
    assert torch.equal(strip(grad), body) and grad.shape[0] == (body.shape[0] + 7) // 8 * 8
    assert body.shape[0] > per_block * sum(_layer_blocks(n_levels, 7))


@pytest.mark.parametrize("hid3", [7, 8])
def test_tile_major_value_stream_is_a_permutation_of_the_forward_pieces(streams, hid3):
    n_levels, full, grad, value = streams
    if hid3 == 8:      # the order alone, on the pinned stream itself
        ws, bs = _weights(n_levels, seed=290 + n_levels)
        t, _ = ops._pack_grad_pieces(ws, bs, n_levels, terms=3, order="tile")
        value, grad = t.contiguous().view(torch.uint8).reshape(t.shape[0], -1), full
    blocks = _layer_blocks(n_levels, hid3)
    src, at = [], 0
    for kb in blocks:                                                # [layer][tile][block][term] <- [layer][block][tile][term]
        src += [at + (b * TILES + t) * TERMS + k for t in range(TILES) for b in range(kb) for k in range(TERMS)]
        at += kb * TILES * TERMS
    src = torch.tensor(src)
    assert at == TILES * TERMS * sum(blocks) and torch.equal(torch.sort(src).values, torch.arange(at))
    assert torch.equal(value[:at], grad[src])
    assert value.shape[0] == (at + 7) // 8 * 8 and not value[at:].any()
    assert not torch.equal(value[:at], grad[:at])                    # (a stream where the order shows)


def test_tile_major_stream_has_no_reverse_half_and_padding_is_taken_from_the_caller(streams):
    n_levels, _, grad, value = streams
    assert value.shape[0] < grad.shape[0]
    ws, bs = _weights(n_levels, seed=290 + n_levels)
    padded, _ = ops._pack_grad_pieces(ws, bs, n_levels, value.shape[0] + 16, terms=3, hid3=7, order="tile")
    assert padded.shape[0] == value.shape[0] + 16 and not padded[value.shape[0]:].float().any()
    assert torch.equal(padded[:value.shape[0]].view(torch.uint8).reshape(value.shape[0], -1), value)
    with pytest.raises(AssertionError):
        ops._pack_grad_pieces(ws, bs, n_levels, terms=3, order="tiles")


def test_the_library_and_the_packer_agree_on_the_sizes():
    """gens_sdf_bf16x3_layout is what SdfMlpPlan packs by: at three levels seven hidden blocks at layer 3, at five levels (whose gradient
    kernel has no register to spare) the pinned stream as it is; the shipped value kernels read the gradient stream's forward prefix (the
    tile-major order is a development build: make k6b_tile_major)."""
    import ctypes as C
    import os
    from gens_amd import lib as L
    shipped = not os.environ.get("GENS_HIP_LIB")      # (a development library states its own order and block count: held to its sizes only)
    for n_levels, tile_major, hid3 in ((3, 0, 7), (5, 0, 8)):
        out = (C.c_int * 3)()
        assert L.load().gens_sdf_bf16x3_layout(n_levels, out) == 0
        if not shipped:
            tile_major, hid3 = out[1], out[2]
            assert tile_major in (0, 1) and hid3 in (7, 8)
        fwd = TILES * TERMS * sum(_layer_blocks(n_levels, hid3))
        assert list(out) == [(fwd + 7) // 8 * 8, tile_major, hid3], list(out)
        assert L.load().gens_sdf_bf16x3_pieces(n_levels) > out[0]
    out = (C.c_int * 3)()
    assert L.load().gens_sdf_bf16x3_layout(4, out) == -2 and b"3 or 5" in L.load().gens_last_error()
    assert L.load().gens_sdf_bf16x3_layout(3, None) == -1
