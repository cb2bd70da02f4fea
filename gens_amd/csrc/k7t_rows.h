// What the two transposed blending kernels share (k7t_blend.hip on v_mfma_f32_16x16x4_f32, k7b_blend_bf16x3.hip on
// v_mfma_f32_16x16x32_bf16 with three-term operands): the row layout of a wavefront -- 64 (point, view) rows as four N tiles of 16
// columns, the S views of a point in G adjacent lanes -- the reductions over views and lane groups, the activation, and phase 0, in which
// one lane per row gathers it into LDS.  See k7t_blend.hip's header for the dataflow.
#pragma once
#include "k4_common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define KT_NT 4                 // N tiles per wave (16 columns each): 16 points x 4 views
#define KT_XS 29                // row stride of the gathered-feature tile (floats): odd, so the per-column reads spread over the banks

enum { KT_RD1_B = 0, KT_RD2_B, KT_B2_B, KT_V1_B, KT_V2_B, KT_U1_B, KT_R2_B, KT_V2_LAST, KT_U2, KT_R3, KT_TAB_ENTRIES };

__device__ __forceinline__ float elu1t(float x) { return __builtin_amdgcn_fmed3f(x, hw_exp(x) - 1.0f, 0.0f); }   // see k7_blend.hip::elu1
template <int G>
__device__ __forceinline__ float group_sum(float v) {     // sum over the G adjacent lanes of a point (= its views), in every lane
    v += dpp_move<0xB1, 0xF>(v, v);                       // quad_perm:[1,0,3,2]
    if (G == 4) v += dpp_move<0x4E, 0xF>(v, v);           // quad_perm:[2,3,0,1]
    return v;
}
template <int G>
__device__ __forceinline__ float group_min(float v) {
    v = fminf(v, dpp_move<0xB1, 0xF>(v, v));
    if (G == 4) v = fminf(v, dpp_move<0x4E, 0xF>(v, v));
    return v;
}
template <int G>
__device__ __forceinline__ float group_max(float v) {
    v = fmaxf(v, dpp_move<0xB1, 0xF>(v, v));
    if (G == 4) v = fmaxf(v, dpp_move<0x4E, 0xF>(v, v));
    return v;
}
__device__ __forceinline__ float lanes_q_sum(float v) {   // sum over the four lane groups q of a column
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

// phase 0: lane `lane` gathers (point, view) row `lane` of the wave whose first point is `first` -- X[64 * KT_XS]: rgb (3), features
// (4 NLEV), one; RD[64 * 5]: ray difference (4); R[64]: mask -- and writes the row's in-frustum flag
template <int NLEV, int S>
__device__ __forceinline__ void blend_gather_row(const MapSet& fs, const float4* __restrict__ imgs, const float* __restrict__ w2c,
                                                 const float* __restrict__ intr, const float* __restrict__ c2w, const float* __restrict__ pts,
                                                 const int64_t* __restrict__ index, int64_t first, int64_t n, uint8_t* __restrict__ vis_out,
                                                 int lane, float* X, float* RD, float* R) {
    constexpr int F = 3 + 4 * NLEV;
    constexpr int G = S == 2 ? 2 : 4;        // lanes per point (S = 3: one dead lane)
    const int pl = lane / G, sv = (lane % G) + 1;
    const bool live = first + pl < n && sv <= S;          // (S = 3: the fourth lane of a quad carries no view)
    const int64_t src = live ? (index ? index[first + pl] : first + pl) : 0;
    float x = 0.f, y = 0.f, z = 0.f;
    if (live) { x = pts[3 * src]; y = pts[3 * src + 1]; z = pts[3 * src + 2]; }
    bool inside = true;
    float* xr = X + lane * KT_XS;
    const int svc = sv <= S ? sv : S;                       // camera read by the dead lane (never used)
    const SrcBase pb = project_src_base(w2c + 16 * svc, intr + 16 * svc, x, y, z);
#pragma unroll
    for (int l = 0; l < NLEV; ++l) {
        const int h = fs.h[l], w = fs.w[l];
        const SrcProj p = project_src_level(pb, exp2f(-(float)l), h, w, fs.cw[l], fs.ch[l], fs.rcw[l], fs.rch[l]);
        inside = inside && p.inside;
        float4 f = f4_zero(), c = f4_zero();
        if (live) {
            const Taps2 t = bilinear_taps(p.ix, p.iy, h, w);
            f = sample_texel(fs.data[l] + (int64_t)svc * h * w, h, w, 1, 0, t);
            if (l == 0) c = sample_texel(imgs + (int64_t)svc * h * w, h, w, 1, 0, t);
        }
        xr[3 + 4 * l] = f.x; xr[4 + 4 * l] = f.y; xr[5 + 4 * l] = f.z; xr[6 + 4 * l] = f.w;
        if (l == 0) { xr[0] = c.x; xr[1] = c.y; xr[2] = c.z; }
    }
    xr[F] = 1.0f;
    // (not-a-number inputs must come out as not-a-number: the median form of the ELU would drop them, so the row's mask carries a
    // poison term 0 * (sum of its inputs) -- the mask multiplies the view weights, the visibilities and gates the score)
    float acc_in = x + y + z;
#pragma unroll
    for (int k = 0; k < F; ++k) acc_in += xr[k];
    R[lane] = ((live && inside) ? 1.0f : 0.0f) + 0.0f * acc_in;
    if (live && vis_out) vis_out[src * S + (sv - 1)] = inside ? 1 : 0;
    // compute_angle (projector.py:278-291), hardware sqrt / rcp as in k7_blend.hip
    float rx = c2w[3] - x, ry = c2w[7] - y, rz = c2w[11] - z;
    const float rn = hw_rcp(__builtin_amdgcn_sqrtf(rx * rx + ry * ry + rz * rz) + 1e-6f);
    rx *= rn; ry *= rn; rz *= rn;
    const float* cs = c2w + 16 * svc;
    float sx = cs[3] - x, sy = cs[7] - y, sz = cs[11] - z;
    const float sn = hw_rcp(__builtin_amdgcn_sqrtf(sx * sx + sy * sy + sz * sz) + 1e-6f);
    sx *= sn; sy *= sn; sz *= sn;
    const float dx = rx - sx, dy = ry - sy, dz = rz - sz;
    const float dn = hw_rcp(fmaxf(__builtin_amdgcn_sqrtf(dx * dx + dy * dy + dz * dz), 1e-6f));
    float* rd = RD + lane * 5;
    rd[0] = live ? dx * dn : 0.0f;
    rd[1] = live ? dy * dn : 0.0f;
    rd[2] = live ? dz * dn : 0.0f;
    rd[3] = live ? rx * sx + ry * sy + rz * sz : 0.0f;
}
