"""Host logic of gens_blend_views_bf16x3 (no GPU): the weight stream of gens_amd.ops._pack_blend_b, decoded by the layout the kernel assumes
(k7b_blend_bf16x3.hip: groups of three 1 KB pieces; a bf16 group is the three bfloat16 planes of (M tile T, K block b), lane (m, qk) holding
for j = 0..7 the weight of output feature 16 T + 4 (m & 3) + (m >> 2) and input slot 4 (8 b + j) + qk, slot 2 w in the low half of word w;
the first and last groups are float32 fragments in gens_blend_views_t's float4 layout) and applied in the kernel's order, with its K
permutation and its zero padding, must reproduce BlendingNetwork.forward (models/modules/blending_network.py:69-118 of the reference)."""
import pytest
import torch

from gens_amd.models.modules.blending_network import BlendingNetwork
from gens_amd.ops import _pack_blend_b, _pack_blend_t

from .test_blend_stream_cpu import quad_bias, quad_row

LANE = torch.arange(64)
M, QK = LANE & 15, LANE >> 4
ROW_IN_TILE = 4 * (M & 3) + (M >> 2)


def bf16_terms(piece):
    """(64, 4) int32 -> (64, 8) float64: the bfloat16 in the low half of word w is slot 2 w, the one in the high half slot 2 w + 1"""
    lo = (piece << 16).view(torch.float32)
    hi = (piece & -65536).view(torch.float32)
    return torch.stack([lo, hi], -1).reshape(64, 8).double()


class Stream:
    def __init__(self, stream):
        self.s, self.pos = stream, 0

    def group(self):
        self.pos += 1
        return self.s[self.pos - 1]

    def product(self, m_tiles, n_blocks):
        """-> dense (16 m_tiles, 32 n_blocks) float64 matrix of the next bf16 product: the float64 sum of its three planes"""
        w = torch.zeros(16 * m_tiles, 32 * n_blocks, dtype=torch.float64)
        for t in range(m_tiles):
            for b in range(n_blocks):
                g = self.group()
                frag = bf16_terms(g[0]) + bf16_terms(g[1]) + bf16_terms(g[2])
                for j in range(8):
                    w[16 * t + ROW_IN_TILE, 32 * b + 4 * j + QK] = frag[:, j]
        return w


def f32_fragment(piece, n_quads):
    """(64, 4) int32 piece holding a float4 per lane -> dense (16, 4 n_quads) float64 matrix"""
    frag = piece.view(torch.float32).double()
    w = torch.zeros(16, 16, dtype=torch.float64)
    for j in range(4):
        w[ROW_IN_TILE, 4 * j + QK] = frag[:, j]
    assert float(w[:, 4 * n_quads:].abs().max()) == 0.0 if n_quads < 4 else True
    return w[:, :4 * n_quads]


def make_layers(n_levels):
    torch.manual_seed(n_levels)
    net = BlendingNetwork(d_feature=4 * n_levels).double()
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.05 * torch.randn_like(p))
    g = lambda mod: (mod.weight.detach().float(), mod.bias.detach().float())  # noqa: E731
    layers = dict(rd1=g(net.ray_dir_fc[0]), rd2=g(net.ray_dir_fc[2]), b1=g(net.base_fc[0]), b2=g(net.base_fc[2]), v1=g(net.vis_fc[0]),
                  v2=g(net.vis_fc[2]), u1=g(net.vis_fc2[0]), u2=g(net.vis_fc2[2]), r1=g(net.rgb_fc[0]), r2=g(net.rgb_fc[2]), r3=g(net.rgb_fc[4]))
    return net, layers


@pytest.mark.parametrize("n_levels", [1, 3, 5])
def test_three_planes_sum_to_the_float32_weights_exactly(n_levels):
    """Every packed weight and bias: x0 + x1 + x2 (float64) == the float32 value, bit for bit; the padding is zero in every plane."""
    f = 3 + 4 * n_levels
    xq = n_levels + 1
    _net, layers = make_layers(n_levels)
    st = Stream(_pack_blend_b(layers, f))
    st.group()
    b1, b1b = layers["b1"][0].double(), layers["b1"][1].double()
    nb = (2 * xq + 7) // 8
    mv = st.product(4, nb)
    assert torch.equal(mv[:, :f], b1[:, :f]) and torch.equal(mv[:, 4 * xq:4 * xq + f], b1[:, f:2 * f])
    assert float(mv[:, f:4 * xq].abs().max()) == 0.0 and float(mv[:, 4 * xq + f:].abs().max()) == 0.0
    x = st.product(4, 1)
    assert torch.equal(x[:, :f], b1[:, 2 * f:]) and torch.equal(x[:, f], b1b) and float(x[:, f + 1:].abs().max()) == 0.0
    assert torch.equal(st.product(2, 2), layers["b2"][0].double())
    assert torch.equal(st.product(2, 1), layers["v1"][0].double())
    assert torch.equal(st.product(2, 1), layers["v2"][0][:32].double())
    assert torch.equal(st.product(2, 1), layers["u1"][0].double())
    assert torch.equal(st.product(1, 1), layers["r1"][0][:, :32].double())
    # every term is a bfloat16 by construction (16 bits per slot); the smaller terms are residuals: |x1| <= ulp_bf16(x0) / 2
    planes = _pack_blend_b(layers, f)[1:-3]
    t0, t1, t2 = (torch.stack([bf16_terms(g[k]) for g in planes]) for k in range(3))
    assert bool((t1.abs() <= t0.abs() * 2.0 ** -8).all()) and bool((t2.abs() <= t0.abs() * 2.0 ** -16).all())


@pytest.mark.parametrize("n_levels", [1, 3, 5])
def test_blend_bf16x3_stream_reproduces_the_network(n_levels):
    f = 3 + 4 * n_levels
    xq = n_levels + 1
    net, layers = make_layers(n_levels)
    stream = _pack_blend_b(layers, f)
    tab = _pack_blend_t(layers, f)[1].double()          # the tables are gens_blend_views_t's
    assert stream.dtype == torch.int32 and stream.shape[1:] == (3, 64, 4)
    n, s_views = 9, 4
    rgb_feat = torch.rand(n, s_views, f, dtype=torch.float64)
    ray_diff = torch.randn(n, s_views, 4, dtype=torch.float64) * 0.3
    mask = (torch.rand(n, s_views) > 0.2).double()
    with torch.no_grad():
        want = net(rgb_feat, ray_diff, mask)

    st = Stream(stream)
    elu = torch.nn.functional.elu
    one = torch.ones(n, s_views, 1, dtype=torch.float64)
    zero = torch.zeros_like(one)
    pad = lambda t, k: torch.cat([t, t.new_zeros(*t.shape[:-1], k - t.shape[-1])], -1)  # noqa: E731  (zero padding to k slots)
    xt = (xq + 3) // 4
    head = st.group()                                                                                 # [ray_dir_fc.0 | ray_dir_fc.2 tiles]
    d = elu(ray_diff @ f32_fragment(head[0], 1).T + quad_bias(tab, 0, 1))                             # ray_dir_fc.0
    rd2 = torch.cat([f32_fragment(head[1 + t], 4) for t in range(xt)], 0)
    assert xt == 2 or float(head[2].abs().max()) == 0
    x = torch.cat([rgb_feat, one], -1)                                                                # slot F = the one
    x = x + elu(d @ rd2.T + quad_bias(tab, 1, xt))[..., :4 * xq]
    e = torch.exp(net.s.detach().abs() * (ray_diff[..., 3:4] - 1))
    w = (e - e.min(dim=1, keepdim=True)[0]) * mask[..., None]
    w = w / (w.sum(dim=1, keepdim=True) + 1e-8)
    mean = (x * w).sum(dim=1, keepdim=True)
    var = (w * (x - mean) ** 2).sum(dim=1, keepdim=True)
    nb = (2 * xq + 7) // 8
    per_point = pad(torch.cat([mean, var], -1), 32 * nb) @ st.product(4, nb).T                        # once per point
    h1 = elu(per_point + pad(x, 32) @ st.product(4, 1).T)                                             # + x's columns and the bias slot
    h = elu(h1 @ st.product(2, 2).T + quad_bias(tab, 2, 2))
    g1 = elu((h * w) @ st.product(2, 1).T + quad_bias(tab, 3, 2))
    vis = torch.sigmoid(elu(g1 @ quad_row(tab, 7, 32) + float(layers["v2"][1][32]))) * mask
    h = h + elu(g1 @ st.product(2, 1).T + quad_bias(tab, 4, 2))
    g2 = elu((h * vis[..., None]) @ st.product(2, 1).T + quad_bias(tab, 5, 2))
    vis2 = torch.sigmoid(g2 @ quad_row(tab, 8, 32) + float(layers["u2"][1][0])) * mask
    c1 = h @ st.product(1, 1).T                                                                       # rgb_fc.0: x's 32 columns in bf16 ...
    last = st.group()                                                                                 # [rgb_fc.0 quads 8, 9 | rgb_fc.2 | 0]
    r_tail = torch.cat([vis2[..., None], ray_diff[..., 0:3], ray_diff[..., 3:4], one, zero, zero], -1)
    c1 = elu(c1 + r_tail @ f32_fragment(last[0], 2).T)                                                # ... quads 8 and 9 in float32
    c2 = elu(c1 @ f32_fragment(last[1], 4).T + quad_bias(tab, 6, 1))
    assert float(last[2].abs().max()) == 0
    score = c2[..., :8] @ quad_row(tab, 9, 8) + float(layers["r3"][1][0])
    score = score.masked_fill(mask == 0, -1e9)
    got = (rgb_feat[..., :3] * torch.softmax(score, dim=1)[..., None]).sum(dim=1)
    assert st.pos + 2 == stream.shape[0] and int(stream[-2:].abs().max()) == 0
    assert (got - want).abs().max() < 2e-6            # the stream is the float32 rounding of the float64 test network
