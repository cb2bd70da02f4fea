// K7b: K7t (k7t_blend.hip: source-view look-up + the whole BlendingNetwork for two, three or four source views, transposed, all eleven
// layers in registers) with its large products on the bf16 matrix pipe, float32-accurate -- the remedy of k6b_sdf_bf16x3.hip:
//
//   * every float32 operand is x = x0 + x1 + x2, three round-to-nearest bf16 terms (split3.h); a product is the six terms
//     x2 y0, x1 y1, x0 y2, x1 y0, x0 y1, x0 y0 on v_mfma_f32_16x16x32_bf16, smallest first, float32 accumulation: 6 x 16 cycles per
//     16 x 16 x 32 block against 8 x 32 of v_mfma_f32_16x16x4_f32.  The weights (A operand) are split on the host into three planes,
//     a lane's 16-byte load is one A fragment of 8 bf16; the activations (B operand) are split in registers.
//   * rows, lanes, quad layout, phase 0, the reductions over views, the per-point mean / variance product, the bias slots, the
//     single-output dot products and the index / n_dev semantics are K7t's (k7t_rows.h).  The C/D layout of 16x16x32_bf16 is that of
//     16x16x4_f32 (column = lane & 15, row = 4 (lane >> 4) + register) and its B operand wants k = 8 (lane >> 4) + j in a lane: the four
//     registers of TWO accumulator tiles 2 t, 2 t + 1 of lane group q are the lane's eight slots j = 4 (T & 1) + i of K block t.  In
//     quad layout that slot is feature 4 (8 t + j) + q: a K block is eight K quads, and the host orders each matrix's reduction index so
//     (gens_amd.ops._pack_blend_b).  No LDS between layers.  K is padded to whole blocks with zeros.
//   * the products whose K is half a block or less stay on v_mfma_f32_16x16x4_f32 (the C/D layouts agree, so the two kinds accumulate
//     into the same tile): ray_dir_fc.0 (K = 4), ray_dir_fc.2 and rgb_fc.2 (K = 16) and the last two quads of rgb_fc.0 (vis, ray
//     difference, the bias's one).  At K = 16 the bf16 form is 6 x 16 cycles of which half multiply padding, plus the split of the
//     operand (9 vector instructions per pair of values), against 4 x 32 cycles with no split; the kernel's vector pipe, which carries
//     the splits and the activations, is the busier one (profiles/r14_blend_bf16x3.txt: 3 680 vector instructions against 8.4 k matrix
//     cycles per wave).  For the same reason the residuals of a split and the ELU's scaling and -1 go through the packed float32
//     instructions (split3_pair<true>, elu4b: the same values), and vis_fc2.0, which reads x * vis with vis ONE factor per row, is
//     computed as vis * (W x): x is split once for vis_fc2.0 and rgb_fc.0.
//   * the weight stream is one sequence of GROUPS of three 1 KB pieces (64 lanes x 16 bytes): a bf16 group is the three planes of one
//     (M tile, K block); the first group is the float32 fragments [ray_dir_fc.0 | ray_dir_fc.2 tile 0 | tile 1] and the last one
//     [rgb_fc.0 quads 8, 9 | rgb_fc.2 | 0] in K7t's float4 layout.  Every lane loads its 48 bytes of a group two groups ahead.
//   * THREE waves per SIMD (KB_OCC, <= 168 registers, no scratch): the kernel is bound by the vector pipe and its dataflow is one register
//     chain, so a third resident wave fills issue slots the two leave empty (profiles/r26_blend_three_waves.txt: vector issue 63 -> 75 % of the
//     SIMD cycles, 2 716 -> 2 336 us per launch of 3.9 M points x 4 views, the same output bits).  DIET in the kernel: the
//     values phase 0 left in LDS and that are used late -- the colour, the ray difference's rgb_fc.0 quads, the mask -- are read again
//     where they are used and not carried from the prologue.  -DGENS_K7B_OCC=2 is the build before it, instruction for instruction.
#include "k7t_rows.h"
#include "split3.h"

// resident waves per SIMD the kernel is bounded for (__launch_bounds__(64, w): w workgroups of one wave per SIMD): 3 wants <= 168 registers,
// 2 <= 256.  Per instantiation, so that one that would spill at 3 can stay at 2; today none does.
#ifndef GENS_K7B_OCC
#define GENS_K7B_OCC 3
#endif
#define KB_OCC(NLEV_, S_) (GENS_K7B_OCC)

struct BlendBWeights {
    const u32x4* stream;        // groups in consumption order: 3 pieces x 64 lanes x 16 bytes each
    const float* tab;           // K7t's table: per lane group q [entry][q][8] floats (accumulator-layout biases, dot-product rows)
    float v2_last_b, u2_b, r3_b, s_abs;
};

// elu1t of two values and of an accumulator tile with the scaling and the -1 on the packed float32 instructions (the same values)
__device__ __forceinline__ f32x2v elu2b(f32x2v x) {
    const f32x2v t = x * 1.44269504088896340736f;
    const f32x2v e = (f32x2v){__builtin_amdgcn_exp2f(t[0]), __builtin_amdgcn_exp2f(t[1])} - 1.0f;
    return (f32x2v){__builtin_amdgcn_fmed3f(x[0], e[0], 0.0f), __builtin_amdgcn_fmed3f(x[1], e[1], 0.0f)};
}
__device__ __forceinline__ f32x4 elu4b(f32x4 x) {
    const f32x2v lo = elu2b((f32x2v){x[0], x[1]}), hi = elu2b((f32x2v){x[2], x[3]});
    return (f32x4){lo[0], lo[1], hi[0], hi[1]};
}

template <int NLEV, int S>
__global__ __launch_bounds__(64, KB_OCC(NLEV, S)) void blend_b_k(BlendBWeights W, MapSet fs, const float4* __restrict__ imgs, const float* __restrict__ w2c,
                                                   const float* __restrict__ intr, const float* __restrict__ c2w, const float* __restrict__ pts,
                                                   const int64_t* __restrict__ index, int64_t n_max, const int32_t* __restrict__ n_dev,
                                                   float* __restrict__ rgb_out, uint8_t* __restrict__ vis_out) {
    constexpr int XQ = NLEV + 1;             // K quads of a feature vector: F + 1 = 4 (NLEV + 1) slots, the last one carries the constant one
    constexpr int XT = (XQ + 3) / 4;         // accumulator tiles of a feature vector
    constexpr int NB_MV = (2 * XQ + 7) / 8;  // K blocks of [mean | variance]
    constexpr int G = S == 2 ? 2 : 4;        // lanes per point (S = 3: one dead lane)
    constexpr int PPT = 16 / G;              // points per N tile
    constexpr int PPW = 64 / G;              // points per wave
    constexpr int NPT = PPW / 16;            // N tiles of POINTS of the per-point product (mean / variance columns)
    static_assert(S >= 2 && S <= 4, "two to four source views");
    static_assert(4 * XQ <= KT_XS && XQ <= 8, "feature tile too narrow");
    // DIET: the build for three waves per SIMD, <= 168 registers: rgbc, rdsh, rd3one and (for its late uses) mask are not carried through
    // the network but read again from X, RD and R, which phase 0 writes and nothing overwrites (ds_bpermute moves registers only)
    constexpr bool DIET = KB_OCC(NLEV, S) >= 3;
    __shared__ float X[64 * KT_XS];          // gathered rows: rgb (3), features (4 NLEV), one
    __shared__ float RD[64 * 5];             // ray difference (4)
    __shared__ float R[64];                  // mask
    const int lane = threadIdx.x;
    const int np = lane & 15, q = lane >> 4;
    const int64_t n = n_dev ? min(n_max, (int64_t)n_dev[0]) : n_max;
    const int64_t first = (int64_t)blockIdx.x * PPW;
    if (first >= n) return;

    // weights: scalar base, three groups of three 16-byte registers rotate (this group's, the next two in flight)
    const u32x4* wp = W.stream;
    u32x4 wb[3][3];
    int par = 0;
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int k = 0; k < 3; ++k) wb[g][k] = wp[lane + 64 * (3 * g + k)];
    wp += 384;

    // ---------------------------------------------------------------- phase 0: one lane per (point, view) row gathers it
    blend_gather_row<NLEV, S>(fs, imgs, w2c, intr, c2w, pts, index, first, n, vis_out, lane, X, RD, R);
    __syncthreads();

    // ---------------------------------------------------------------- this lane's operand slots of the four N tiles
    float xq[KT_NT][XQ];        // x in quad layout (slot F = the one)
    float rgbc[KT_NT];          // colour channel q of the column (q < 3)
    float rdq[KT_NT], dotv[KT_NT], mask[KT_NT], rd3one[KT_NT], rdsh[KT_NT];
#pragma unroll
    for (int j = 0; j < KT_NT; ++j) {
        const int row = 16 * j + np;
#pragma unroll
        for (int kq = 0; kq < XQ; ++kq) xq[j][kq] = X[row * KT_XS + 4 * kq + q];
        rdq[j] = RD[row * 5 + q];
        dotv[j] = RD[row * 5 + 3];
        mask[j] = R[row];
        if constexpr (!DIET) {
            rgbc[j] = xq[j][0];
            rdsh[j] = q ? RD[row * 5 + q - 1] : 0.0f;                      // rgb_fc.0's quad [vis, rd0, rd1, rd2] (vis filled in later)
            rd3one[j] = q == 0 ? dotv[j] : (q == 1 ? 1.0f : 0.0f);        // ... and [rd3, one, 0, 0]
        }
    }
    // DIET: this lane's row of N tile j_ for a late read (opaque lane: a new address to the compiler, or it keeps the prologue's value alive)
#define KB_ROW_O(j_) (16 * (j_) + (lane_o & 15))
    const float* tab = W.tab + q * 8;
#define KB_TAB(E, K) tab[(E) * 32 + (K)]
#define KB_BIAS(E, T) ((f32x4){KB_TAB(E, 4 * (T)), KB_TAB(E, 4 * (T) + 1), KB_TAB(E, 4 * (T) + 2), KB_TAB(E, 4 * (T) + 3)})

    // the next group of the stream becomes a0_ / a1_ / a2_ (planes x0, x1, x2, or three float32 fragments); requested two groups ahead
#define KB_NEXT()                                                                                        \
    const u32x4 a0_ = wb[par][0], a1_ = wb[par][1], a2_ = wb[par][2];                                    \
    _Pragma("unroll") for (int k_ = 0; k_ < 3; ++k_) wb[(par + 2) % 3][k_] = wp[lane + 64 * k_];          \
    wp += 192;                                                                                           \
    par = (par + 1) % 3;
#define KB_MFMA(A_, B_, C_) __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, (A_)), __builtin_bit_cast(bf16x8, (B_)), (C_), 0, 0, 0)
    // one bf16 group: K block BLK_ of one M tile for the NT_ N tiles whose accumulators are ACC_(j), whose first C operand is C0_(j)
    // and whose operands are the Split3Blocks B_(j, BLK_): weight term x activation term, smallest first
#define KB_GROUP(NT_, ACC_, C0_, B_, BLK_)                                                               \
    {                                                                                                    \
        KB_NEXT()                                                                                        \
        _Pragma("unroll") for (int j_ = 0; j_ < (NT_); ++j_) ACC_(j_) = KB_MFMA(a2_, B_(j_, (BLK_)).p[0], C0_(j_));  \
        _Pragma("unroll") for (int j_ = 0; j_ < (NT_); ++j_) ACC_(j_) = KB_MFMA(a1_, B_(j_, (BLK_)).p[1], ACC_(j_)); \
        _Pragma("unroll") for (int j_ = 0; j_ < (NT_); ++j_) ACC_(j_) = KB_MFMA(a0_, B_(j_, (BLK_)).p[2], ACC_(j_)); \
        _Pragma("unroll") for (int j_ = 0; j_ < (NT_); ++j_) ACC_(j_) = KB_MFMA(a1_, B_(j_, (BLK_)).p[0], ACC_(j_)); \
        _Pragma("unroll") for (int j_ = 0; j_ < (NT_); ++j_) ACC_(j_) = KB_MFMA(a0_, B_(j_, (BLK_)).p[1], ACC_(j_)); \
        _Pragma("unroll") for (int j_ = 0; j_ < (NT_); ++j_) ACC_(j_) = KB_MFMA(a0_, B_(j_, (BLK_)).p[0], ACC_(j_)); \
    }
    // a whole bf16 product: M tiles MT_, K blocks NB_, accumulators ACC_T_(j); the FIRST MFMA of a chain reads its C operand from
    // INIT_T_(j) -- the bias vector of the tile, shared by the four N tiles -- instead of from a copy of it in the accumulator
#define KB_PRODUCT(NT_, MT_, NB_, B_)                                                                    \
    _Pragma("unroll") for (int T_ = 0; T_ < (MT_); ++T_)                                                 \
        _Pragma("unroll") for (int b_ = 0; b_ < (NB_); ++b_) {                                           \
            if (b_ == 0) KB_GROUP(NT_, ACC_T_, INIT_T_, B_, 0)                                           \
            else KB_GROUP(NT_, ACC_T_, ACC_T_, B_, b_)                                                   \
        }
    // NQ_ (<= 4) K quads of a float32 fragment A_ (K7t's float4 layout) onto the KT_NT accumulators ACC_(j); operands B_(j, quad)
#define KB_F32(A_, NQ_, ACC_, C0_, B_)                                                                   \
    {                                                                                                    \
        const f32x4 af_ = __builtin_bit_cast(f32x4, (A_));                                               \
        _Pragma("unroll") for (int k_ = 0; k_ < (NQ_); ++k_)                                             \
            _Pragma("unroll") for (int j_ = 0; j_ < KT_NT; ++j_)                                         \
                ACC_(j_) = k_ == 0 ? __builtin_amdgcn_mfma_f32_16x16x4f32(af_[0], B_(j_, 0), C0_(j_), 0, 0, 0)          \
                                   : __builtin_amdgcn_mfma_f32_16x16x4f32(af_[k_], B_(j_, k_), ACC_(j_), 0, 0, 0);      \
    }
    // eight values V_(0) .. V_(7) -> the three-term K block BLK_ (slot j of the lane = word j / 2, half j % 2)
#define KB_SPLIT8(BLK_, V_)                                                                              \
    _Pragma("unroll") for (int w_ = 0; w_ < 4; ++w_) {                                                   \
        const Split3Word sw_ = split3_pair<true>(V_(2 * w_), V_(2 * w_ + 1));                                  \
        _Pragma("unroll") for (int k_ = 0; k_ < SPLIT3_TERMS; ++k_) (BLK_).p[k_][w_] = sw_.w[k_];        \
    }

    // ---------------------------------------------------------------- ray_dir_fc (blending_network.py:36-39, 87), float32 MFMAs
    {
        KB_NEXT()                                                     // [ray_dir_fc.0 | ray_dir_fc.2 tile 0 | tile 1]
        f32x4 D[KT_NT];
        const f32x4 b = KB_BIAS(KT_RD1_B, 0);
#define ACC_D_(j) D[j]
#define INIT_B_(j) b
#define B_RD(j, k) rdq[j]
        KB_F32(a0_, 1, ACC_D_, INIT_B_, B_RD)
#undef INIT_B_
#pragma unroll
        for (int j = 0; j < KT_NT; ++j) D[j] = elu4b(D[j]);
        f32x4 E[XT][KT_NT];
#define B_D(j, k) D[j][k]
#pragma unroll
        for (int T = 0; T < XT; ++T) {
            const f32x4 bias = KB_BIAS(KT_RD2_B, T);
#define ACC_E_(j) E[T][j]
#define INIT_B_(j) bias
            KB_F32((T == 0 ? a1_ : a2_), 4, ACC_E_, INIT_B_, B_D)
#undef ACC_E_
#undef INIT_B_
        }
#undef ACC_D_
#pragma unroll
        for (int j = 0; j < KT_NT; ++j) {
#pragma unroll
            for (int T = 0; T < XT; ++T) E[T][j] = elu4b(E[T][j]);
#pragma unroll
            for (int kq = 0; kq < XQ; ++kq) xq[j][kq] += E[kq >> 2][j][kq & 3];             // x = rgb_feat + direction_feat (:89); the one's row is zero
        }
    }

    // ---------------------------------------------------------------- view weights, weighted mean / variance (:93-101)
    float wn[KT_NT];
    Split3Block pmv[NPT][NB_MV];             // [mean | variance] of the wave's points as the operands of NPT N tiles of 16 points
    const bool dead = S == 3 && (np & 3) == 3;
    {
        float pc[NPT][8 * NB_MV];            // quads 0 .. XQ - 1: mean, XQ .. 2 XQ - 1: variance, then zeros
        // point p = 16 t + np of point tile t is row tile p / PPT, column G (p % PPT) (its first view), same lane group
        const int src = (G * (np % PPT) + 16 * q) * 4;          // byte address for ds_bpermute
#pragma unroll
        for (int t = 0; t < NPT; ++t)
#pragma unroll
            for (int k = 0; k < 8 * NB_MV; ++k) pc[t][k] = 0.0f;
#pragma unroll
        for (int j = 0; j < KT_NT; ++j) {
            const float e = hw_exp(W.s_abs * (dotv[j] - 1.0f));
            const float mn = group_min<G>(dead ? __builtin_inff() : e);
            const float wr = dead ? 0.0f : (e - mn) * mask[j];
            wn[j] = wr / (group_sum<G>(wr) + 1e-8f);
#pragma unroll
            for (int kq = 0; kq < XQ; ++kq) {
                const float mean = group_sum<G>(wn[j] * xq[j][kq]);
                const float d = xq[j][kq] - mean;
                const float var = group_sum<G>(wn[j] * (d * d));
                const float tm = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, mean)));
                const float tv = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, var)));
#pragma unroll
                for (int t = 0; t < NPT; ++t) {
                    const bool sel = (16 * t + np) / PPT == j;
                    pc[t][kq] = sel ? tm : pc[t][kq];
                    pc[t][XQ + kq] = sel ? tv : pc[t][XQ + kq];
                }
            }
        }
#pragma unroll
        for (int t = 0; t < NPT; ++t)
#pragma unroll
            for (int b = 0; b < NB_MV; ++b) {
#define V_PC(k) pc[t][8 * b + (k)]
                KB_SPLIT8(pmv[t][b], V_PC)
#undef V_PC
            }
    }

    // ---------------------------------------------------------------- base_fc (:103-104)
    Split3Block hb[KT_NT][2];     // the running product's operand: base_fc.0's 64 activated outputs, later one block of 32 values
    {
        f32x4 H1[4][KT_NT];        // base_fc.0's 64 outputs per N tile
        {
            f32x4 P[NPT][4];       // the mean / variance columns, once per POINT (N tiles of 16 points)
            const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#define INIT_T_(j) zero4
#define ACC_T_(j) P[j][T_]
#define B_PMV(j, b) pmv[j][b]
            KB_PRODUCT(NPT, 4, NB_MV, B_PMV)
#undef ACC_T_
#undef INIT_T_
            // back to the rows: column n' of row tile j is point PPT j + n' / G = column (PPT j) % 16 + n' / G of point tile (PPT j) / 16
#pragma unroll
            for (int j = 0; j < KT_NT; ++j) {
                const int src = (((PPT * j) & 15) + np / G + 16 * q) * 4;
#pragma unroll
                for (int T = 0; T < 4; ++T)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float v = P[(PPT * j) >> 4][T][i];
                        asm volatile("" : "+v"(v));      // (hipcc 7.2 otherwise replaces the four moves of a tile by ONE and splats its result)
                        H1[T][j][i] = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, v)));
                    }
            }
        }
        Split3Block xb[KT_NT];     // x: XQ quads, zeros up to the block's eight
#pragma unroll
        for (int j = 0; j < KT_NT; ++j) {
#define V_X(k) ((k) < XQ ? xq[j][(k) < XQ ? (k) : 0] : 0.0f)
            KB_SPLIT8(xb[j], V_X)
#undef V_X
        }
#define ACC_T_(j) H1[T_][j]
#define INIT_T_(j) H1[T_][j]
#define B_XB(j, b) xb[j]
        KB_PRODUCT(KT_NT, 4, 1, B_XB)              // + x's columns and the bias (slot F)
#undef ACC_T_
#undef INIT_T_
#pragma unroll
        for (int j = 0; j < KT_NT; ++j)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                H1[2 * b][j] = elu4b(H1[2 * b][j]);
                H1[2 * b + 1][j] = elu4b(H1[2 * b + 1][j]);
#define V_H1(k) H1[2 * b + ((k) >> 2)][j][(k) & 3]
                KB_SPLIT8(hb[j][b], V_H1)
#undef V_H1
            }
    }
#define B_HB(j, b) hb[j][b]
    f32x4 XH[2][KT_NT];           // the 32-wide hidden state x
    {
#define ACC_T_(j) XH[T_][j]
#define INIT_T_(j) KB_BIAS(KT_B2_B, T_)
        KB_PRODUCT(KT_NT, 2, 2, B_HB)
#undef ACC_T_
#undef INIT_T_
#pragma unroll
        for (int T = 0; T < 2; ++T)
#pragma unroll
            for (int j = 0; j < KT_NT; ++j) XH[T][j] = elu4b(XH[T][j]);
    }

    f32x4 G1[2][KT_NT];           // the hidden layer of vis_fc, then of vis_fc2
    // dot product of G1 with a 32-float row given in quad layout, summed over the lane groups: every lane of the column gets it
#define KB_DOT32(ENTRY, OUT)                                                                                          \
    _Pragma("unroll") for (int j = 0; j < KT_NT; ++j) {                                                               \
        float s_ = 0.0f;                                                                                              \
        _Pragma("unroll") for (int k = 0; k < 8; ++k) s_ = __builtin_fmaf(G1[k >> 2][j][k & 3], KB_TAB(ENTRY, k), s_); \
        OUT[j] = lanes_q_sum(s_);                                                                                     \
    }

    // ---------------------------------------------------------------- vis_fc on x * weight (:106-109)
    float vis[KT_NT];
#pragma unroll
    for (int j = 0; j < KT_NT; ++j) {
#define V_XS(k) (XH[(k) >> 2][j][(k) & 3] * wn[j])
        KB_SPLIT8(hb[j][0], V_XS)
#undef V_XS
    }
#define ACC_T_(j) G1[T_][j]
#define INIT_T_(j) KB_BIAS(KT_V1_B, T_)
    KB_PRODUCT(KT_NT, 2, 1, B_HB)
#undef INIT_T_
#undef ACC_T_
#pragma unroll
    for (int T = 0; T < 2; ++T)
#pragma unroll
        for (int j = 0; j < KT_NT; ++j) G1[T][j] = elu4b(G1[T][j]);
    KB_DOT32(KT_V2_LAST, vis)                                      // the 33rd output of vis_fc.2 reads the same hidden layer
    {
        f32x4 V2[2][KT_NT];
#pragma unroll
        for (int j = 0; j < KT_NT; ++j) {
#define V_G1(k) G1[(k) >> 2][j][(k) & 3]
            KB_SPLIT8(hb[j][0], V_G1)
#undef V_G1
        }
#define ACC_T_(j) V2[T_][j]
#define INIT_T_(j) KB_BIAS(KT_V2_B, T_)
        KB_PRODUCT(KT_NT, 2, 1, B_HB)
#undef ACC_T_
#undef INIT_T_
#pragma unroll
        for (int T = 0; T < 2; ++T)
#pragma unroll
            for (int j = 0; j < KT_NT; ++j) XH[T][j] += elu4b(V2[T][j]);                    // x = x + x_res
    }
    if constexpr (DIET) {
        int lane_o = lane;
        asm volatile("" : "+v"(lane_o));
#pragma unroll
        for (int j = 0; j < KT_NT; ++j) mask[j] = R[KB_ROW_O(j)];
    }
#pragma unroll
    for (int j = 0; j < KT_NT; ++j) vis[j] = hw_sigmoid(elu1t(vis[j] + W.v2_last_b)) * mask[j];

    // ---------------------------------------------------------------- vis_fc2 on x * vis (:110)
    // vis is one factor per row, so W (vis x) = vis (W x): x is split ONCE for vis_fc2.0 and rgb_fc.0, and vis scales the product
    float vis2[KT_NT];
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < KT_NT; ++j) {
#define V_XH(k) XH[(k) >> 2][j][(k) & 3]
        KB_SPLIT8(hb[j][0], V_XH)
#undef V_XH
    }
#define ACC_T_(j) G1[T_][j]
#define INIT_T_(j) zero4
    KB_PRODUCT(KT_NT, 2, 1, B_HB)
#undef INIT_T_
#undef ACC_T_
#pragma unroll
    for (int T = 0; T < 2; ++T) {
        const f32x4 bias = KB_BIAS(KT_U1_B, T);
#pragma unroll
        for (int j = 0; j < KT_NT; ++j) {
#pragma unroll
            for (int i = 0; i < 4; ++i) G1[T][j][i] = __builtin_fmaf(G1[T][j][i], vis[j], bias[i]);
            G1[T][j] = elu4b(G1[T][j]);
        }
    }
    KB_DOT32(KT_U2, vis2)
#pragma unroll
    for (int j = 0; j < KT_NT; ++j) vis2[j] = hw_sigmoid(vis2[j] + W.u2_b) * mask[j];

    // ---------------------------------------------------------------- rgb_fc on cat([x, vis, ray_diff]) (:113-115)
    float score[KT_NT];
    {
        f32x4 C1[KT_NT], C2[KT_NT];
        if constexpr (DIET) {
            int lane_o = lane;
            asm volatile("" : "+v"(lane_o));
            const int q_o = lane_o >> 4;
#pragma unroll
            for (int j = 0; j < KT_NT; ++j) {
                const float* rd = RD + KB_ROW_O(j) * 5;
                rdsh[j] = q_o ? rd[q_o - 1] : 0.0f;
                rd3one[j] = q_o == 0 ? rd[3] : (q_o == 1 ? 1.0f : 0.0f);
            }
        }
#define INIT_T_(j) zero4                                                                     // (bias: the one of quad 9)
#define ACC_T_(j) C1[j]
        KB_PRODUCT(KT_NT, 1, 1, B_HB)                                                        // x's 32 columns
#undef INIT_T_
        {
            KB_NEXT()                                                                        // [rgb_fc.0 quads 8, 9 | rgb_fc.2 | 0]
            (void)a2_;
#define B_R1(j, k) ((k) == 0 ? (q == 0 ? vis2[j] : rdsh[j]) : rd3one[j])
            KB_F32(a0_, 2, ACC_T_, ACC_T_, B_R1)
#undef ACC_T_
#pragma unroll
            for (int j = 0; j < KT_NT; ++j) C1[j] = elu4b(C1[j]);
            const f32x4 b2 = KB_BIAS(KT_R2_B, 0);
#define ACC_T_(j) C2[j]
#define INIT_T_(j) b2
#define B_C1(j, k) C1[j][k]
            KB_F32(a1_, 4, ACC_T_, INIT_T_, B_C1)
#undef ACC_T_
#undef INIT_T_
        }
#pragma unroll
        for (int j = 0; j < KT_NT; ++j) {
            const f32x2v c2 = elu2b((f32x2v){C2[j][0], C2[j][1]});
            const float s = c2[0] * KB_TAB(KT_R3, 0) + c2[1] * KB_TAB(KT_R3, 1);      // features 0..7 = registers 0, 1 of the four groups
            score[j] = (mask[j] == 0.0f ? -1e9f : lanes_q_sum(s) + W.r3_b) + 0.0f * mask[j];              // masked_fill(mask == 0, -1e9)  (:115); NaN mask = poisoned row
            if (dead) score[j] = -__builtin_inff();                                                       // no such view: weight exactly 0 in the soft-max
        }
    }

    // ---------------------------------------------------------------- softmax over views, colour (:116-117)
    if constexpr (DIET) {
        int lane_o = lane;
        asm volatile("" : "+v"(lane_o));
#pragma unroll
        for (int j = 0; j < KT_NT; ++j) rgbc[j] = X[KB_ROW_O(j) * KT_XS + (lane_o >> 4)];
    }
#pragma unroll
    for (int j = 0; j < KT_NT; ++j) {
        const float mx = group_max<G>(score[j]);
        const float e = hw_exp(score[j] - mx);
        const float den = group_sum<G>(e);
        const float col = group_sum<G>(rgbc[j] * e) / den;
        const int64_t pt = first + PPT * j + np / G;
        if ((np % G) == 0 && q < 3 && pt < n) {
            const int64_t dst = index ? index[pt] : pt;
            rgb_out[3 * dst + q] = col;
        }
    }
#undef KB_TAB
#undef KB_BIAS
#undef KB_NEXT
#undef KB_MFMA
#undef KB_GROUP
#undef KB_PRODUCT
#undef KB_F32
#undef KB_SPLIT8
#undef KB_DOT32
#undef KB_ROW_O
}

// What the device says about one instantiation at the launcher's block size: registers per lane, scratch bytes per lane, static LDS bytes,
// resident workgroups (of one wave) per CU.
template <int S>
static const void* blend_b_fn(int n_levels) {
    switch (n_levels) {
        case 1: return (const void*)blend_b_k<1, S>;
        case 2: return (const void*)blend_b_k<2, S>;
        case 3: return (const void*)blend_b_k<3, S>;
        case 4: return (const void*)blend_b_k<4, S>;
        default: return (const void*)blend_b_k<5, S>;
    }
}

extern "C" int gens_blend_bf16x3_residency(int n_levels, int nv, int out[4]) {
    GENS_CHECK_ARG(n_levels >= 1 && n_levels <= 5, GENS_ELIMIT, "gens_blend_bf16x3_residency: built for 1 to 5 feature levels, got %d", n_levels);
    GENS_CHECK_ARG(nv >= 3 && nv <= 5, GENS_ELIMIT, "gens_blend_bf16x3_residency: built for two to four source views (nv = 3..5), got nv=%d", nv);
    GENS_CHECK_ARG(out, GENS_EINVAL, "gens_blend_bf16x3_residency: null output");
    const void* fn = nv == 3 ? blend_b_fn<2>(n_levels) : nv == 4 ? blend_b_fn<3>(n_levels) : blend_b_fn<4>(n_levels);
    hipFuncAttributes attr;
    int blocks = 0;
    hipError_t err = hipFuncGetAttributes(&attr, fn);
    if (err == hipSuccess) err = hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, fn, 64, 0);
    if (err != hipSuccess) {
        (void)hipGetLastError();
        gens_set_error("gens_blend_bf16x3_residency: %s", hipGetErrorString(err));
        return (int)err;
    }
    out[0] = attr.numRegs;
    out[1] = (int)attr.localSizeBytes;
    out[2] = (int)attr.sharedSizeBytes;
    out[3] = blocks;
    return 0;
}

int gens_fill_maps(const char* who, MapSet* ms, const float* const* feats, const int* hw, int n_levels);

// number of 3 KB groups of the weight stream (without the two zero groups the kernel reads ahead); the same for every view count
extern "C" int gens_blend_bf16x3_groups(int n_levels) {
    if (n_levels < 1 || n_levels > 5) return 0;
    const int xq = n_levels + 1;
    return 1 + 4 * ((2 * xq + 7) / 8) + 4 + 2 * 2 + 2 + 2 + 2 + 1 + 1;
}

template <int S>
static void blend_b_launch(int n_levels, unsigned grid, hipStream_t st, const BlendBWeights& W, const MapSet& fs, const float* imgs, const float* w2c,
                           const float* intr, const float* c2w, const float* pts, const int64_t* index, int64_t n, const int32_t* n_device,
                           float* rgb_out, uint8_t* vis_out) {
#define BLEND_LAUNCH(NL) blend_b_k<NL, S><<<grid, 64, 0, st>>>(W, fs, (const float4*)imgs, w2c, intr, c2w, pts, index, n, n_device, rgb_out, vis_out)
    switch (n_levels) {
        case 1: BLEND_LAUNCH(1); break;
        case 2: BLEND_LAUNCH(2); break;
        case 3: BLEND_LAUNCH(3); break;
        case 4: BLEND_LAUNCH(4); break;
        default: BLEND_LAUNCH(5); break;
    }
#undef BLEND_LAUNCH
}

extern "C" int gens_blend_views_bf16x3(const float* const* feats, const int* hw, int n_levels, const float* imgs, const float* w2c, const float* intr,
                                       const float* c2w, int nv, const void* wstream, const float* tab, const float* scalars, const float* pts,
                                       const int64_t* index, int64_t n, const int32_t* n_device, float* rgb_out, uint8_t* vis_out, void* stream) {
    MapSet fs;
    GENS_CHECK_ARG(feats && wstream && tab && scalars, GENS_EINVAL, "gens_blend_views_bf16x3: null table");
    if (int e = gens_fill_maps("gens_blend_views_bf16x3", &fs, feats, hw, n_levels)) return e;
    GENS_CHECK_ARG(n_levels <= 5, GENS_ELIMIT, "gens_blend_views_bf16x3: at most 5 feature levels (d_feature <= 20), got %d", n_levels);
    GENS_CHECK_ARG(nv >= 3 && nv <= 5, GENS_ELIMIT, "gens_blend_views_bf16x3: built for two to four source views (nv = 3..5), got nv=%d (use gens_blend_views)", nv);
    GENS_CHECK_ARG(imgs && w2c && intr && c2w, GENS_EINVAL, "gens_blend_views_bf16x3: null camera / image pointer");
    GENS_CHECK_ARG(((uintptr_t)wstream & 15) == 0, GENS_EINVAL, "gens_blend_views_bf16x3: the weight stream must be 16-byte aligned");
    GENS_CHECK_ARG(n >= 0 && (n == 0 || (pts && rgb_out)), GENS_EINVAL, "gens_blend_views_bf16x3: null pts / output");
    if (n == 0) return 0;
    BlendBWeights W;
    W.stream = (const u32x4*)wstream;
    W.tab = tab;
    W.v2_last_b = scalars[0]; W.u2_b = scalars[1]; W.r3_b = scalars[2]; W.s_abs = scalars[3];
    hipStream_t st = (hipStream_t)stream;
    if (nv == 3) blend_b_launch<2>(n_levels, gens_blocks(n, 32), st, W, fs, imgs, w2c, intr, c2w, pts, index, n, n_device, rgb_out, vis_out);
    else if (nv == 4) blend_b_launch<3>(n_levels, gens_blocks(n, 16), st, W, fs, imgs, w2c, intr, c2w, pts, index, n, n_device, rgb_out, vis_out);
    else blend_b_launch<4>(n_levels, gens_blocks(n, 16), st, W, fs, imgs, w2c, intr, c2w, pts, index, n, n_device, rgb_out, vis_out);
    return gens_launch_status("gens_blend_views_bf16x3");
}
