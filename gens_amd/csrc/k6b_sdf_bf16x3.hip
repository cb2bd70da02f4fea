// K6b: the SDF network on the bf16 matrix cores with THREE-TERM split operands -- value only (the sampling passes of
// the reference's models/modules/implicit_surface.py:125, 329-352) and value AND gradient d sdf / dx (render_core's 128 samples per ray:
// implicit_surface.py:179-191 -> sdf_network.py:98-154), float32-accurate, the default "f32" arithmetic at three and five volume levels.
//
//   * every float32 operand is x = x0 + x1 + x2, three round-to-nearest bf16 terms (v_cvt_pk_bf16_f32; x - x0 and x - x0 - x1 are exact
//     in float32): 24+ bits of significand and float32's exponent range -- nothing can overflow, no flag, no re-run.  A product is the six
//     terms x2 y0, x1 y1, x0 y2, x1 y0, x0 y1, x0 y0 on v_mfma_f32_32x32x16_bf16 (smallest first, float32 accumulation; each bf16 x bf16
//     product is exact in float32); the three dropped terms are below ~2^-26 relative.  6 x 32 cycles per 32 x 32 x 16 block against
//     8 x 64 of v_mfma_f32_32x32x2_f32.
//   * the dataflow of k6gh_sdf_grad_f16.hip: one wavefront owns 32 points and all 128 hidden units; the weights are the A operand, the
//     activations the B operand; the activated accumulators of a layer, split, ARE the B operands of the next one (registers 8 s .. 8 s + 7
//     of a tile are K step s; the host packs the reduction index in that order).  The reverse pass is the same chain on the transposed
//     matrices, G_{l-1} = (W_l^T G_l) * softplus'(a_{l-1}), split the same way.  The weight stream (1 KB pieces: one term of the A operand
//     of one output tile and one 16-deep K block) goes global -> LDS once per workgroup of four waves, by LDS-direct buffer loads into a
//     ring of four 8 KB chunks filled three chunks ahead.
//   * the value kernel is the forward half of the same code (GRAD = false): every accumulator receives the same MFMAs in the same order on
//     the same operands as in the gradient kernel, so the two return the SAME float32 sdf for the same point.  At five levels it reads the
//     forward prefix of the gradient kernel's stream.
//   * at three levels forward layer 3 reads seven hidden K blocks, not eight: its hidden inputs end at unit 100 (the skip connection fills
//     the row), so the weights of block 7 (units 112..127) are zeros by construction and the stream leaves them out (GB_HID3) -- 24 MFMAs
//     per wave, and with them layer 2's softplus and split of those sixteen units, which nothing reads any more.
//   * at three levels the value kernel is built for TWO waves per SIMD (two workgroups per CU, each with its own ring): one wave's MFMAs
//     issue while the other does its softplus and split, which a single wave between its sched_barrier fences cannot overlap.  That takes
//     <= 256 registers without scratch (a spill would also count in the vmcnt of the chunk boundaries): see DIET in the kernel.
//   * that kernel can also walk a forward layer TILE BY TILE (GENS_K6B_TILE_MAJOR=1, TM in the kernel; make k6b_tile_major): all K blocks
//     of output tile t -- conditioning, at layer 3 the point encoding, hidden -- as ONE segment, softplus of acc[t] in place, then tile
//     t + 1; the splits into H follow the fourth tile, because H is the operand of all four.  A wave then alternates four times per layer
//     between ~72 MFMAs and a quarter of the vector work, instead of 288 MFMAs and one block of vector work, so that its partner on the SIMD
//     finds more places to run the opposite phase.  Per accumulator the MFMAs, their operands and their order are unchanged, and so is every
//     result bit.  The stream is the kernel's own (gens_amd.ops._pack_grad_pieces(order="tile"): [layer][tile][block][term], the layer
//     offsets of the gradient stream); the conditioning blocks that wait in LDS come back once per tile and x is encoded again once per
//     tile at layer 3 (96 + 64 registers for H and acc stay, as does the LDS).  NOT the shipped order: measured against block-major it
//     did not move the step by the project's rule (profiles/r29_sdf_value_tile_major.txt).
//   * softplus and softplus' (float32), the trilinear look-up and its Jacobians, the stash of layer 2's softplus' and the chain rule to x
//     are k6gh's; the gradients need no scaling (bf16 has float32's range).
#include "common.h"
#include "split3.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4v __attribute__((ext_vector_type(4)));

#define GB_WAVES 4
#define GB_PIECE 1024                       // bytes of one piece: 64 lanes x 8 bf16
#define GB_TERMS SPLIT3_TERMS               // pieces per (K block, output tile): x0, x1, x2 (split3.h)
#define GB_CH 8                             // pieces per chunk of the ring
#define GB_RING 4
#define GB_GT 2                             // output tiles per group of A operands (the two-wave build: one)
// resident waves per SIMD: two for the value kernel at three levels, on half the register file (the "diet" in the kernel); the gradient
// kernels (160 KB of LDS) and the five-level value kernel (28 more conditioning registers) stay at one
#define GB_OCC(NLEV_, GRAD_) (!(GRAD_) && (NLEV_) == 3 ? 2 : 1)
#define GB_NCL 2                            // the two-wave build: conditioning K blocks that wait in LDS between the layers
#define GB_CL_BYTES (GB_NCL * GB_TERMS * GB_PIECE)      // ... per wave, behind the ring
#define GB_VALUE_LDS_BYTES(NLEV_) (GB_W_BYTES + (GB_OCC(NLEV_, false) == 2 ? GB_WAVES * GB_CL_BYTES : 0))
#define GB_LPW (GB_CH / GB_WAVES)           // LDS-direct loads per wave and chunk
#define GB_W_BYTES (GB_RING * GB_CH * GB_PIECE)
#define GB_D_BYTES (2 * 16 * 64 * 16)       // softplus' of layers 0 and 1 of one wave
#define GB_LDS_BYTES (GB_W_BYTES + GB_WAVES * GB_D_BYTES)
#define GB_JL_OFF 16384                     // stash slot: [0, 16 KB) softplus' of layer 2, then 32 rows x 256 B of Jacobians, then the lock
#define GB_LOCK_OFF (GB_JL_OFF + 32 * 256)
#define GB_SLOT_BYTES (GB_LOCK_OFF + 256)
#define GB_SLOTS 2048                       // (XCC 3 bits, SE 2, CU 4, wave 2)
#define GB_C 144.26950408889634f            // 100 / ln 2: hidden units travel as c * softplus (k6_sdfmlp.hip::softplus_t)

// Where a wave issues its refill of the weight ring (GB_BOUNDARY and GB_FILL in the kernel):
//   1  in the gaps behind the first MFMAs after the chunk boundary, one piece per gap (the shipped placement)
//   0  at the boundary itself, back to back in front of those MFMAs (what profiles/r25_k6b_stamps.txt stamped; kept for that A/B)
// The MFMAs, their operands and their order are the same in both, and so is every result bit (profiles/r25_sdf_ring_boundaries.txt).
#ifndef GENS_K6B_PLACE
#define GENS_K6B_PLACE 1
#endif
// The five-level gradient kernel keeps placement 0: it holds 508 of 512 registers, and with the refill between its MFMAs it spills.
#define GB_PLACE(NLEV_, GRAD_) ((GRAD_) && (NLEV_) == 5 ? 0 : GENS_K6B_PLACE)

// The order in which a forward layer of the two-wave value kernel walks its products (GB_TILE_MAJOR, TM in the kernel):
//   0  block by block, all four tiles per K block and one softplus of all 64 accumulators per layer, on the forward prefix of the gradient
//      stream (the order of every other instantiation, and the shipped one)
//   1  tile by tile: all K blocks of output tile t, its softplus, then tile t + 1 -- four short matrix / vector alternations per layer, on a
//      value-only stream packed [layer][tile][block][term].  Built, measured and NOT shipped: the step did not move by the project's rule
//      (profiles/r29_sdf_value_tile_major.txt); kept for that A/B: make -C gens_amd/csrc k6b_tile_major
// Every accumulator receives the same MFMAs on the same operands in the same order in both, and so every result bit is the same.
#ifndef GENS_K6B_TILE_MAJOR
#define GENS_K6B_TILE_MAJOR 0
#endif
#define GB_TILE_MAJOR(NLEV_, GRAD_) (GENS_K6B_TILE_MAJOR && GB_OCC(NLEV_, GRAD_) == 2)
// Hidden K blocks that forward layer 3 reads.  Its hidden inputs end at unit 100 (the skip connection takes the rest of the row), so block 7
// (units 112..127) multiplies weights that are zero by construction: seven blocks at three levels, in both kernels.  8 rebuilds the stream with
// that block for the A/B.  The five-level kernels keep all eight: their gradient kernel holds 508 of 512 registers, and without the block its
// register allocation comes out with 12 bytes of scratch per lane (the two five-level kernels share one stream).
#ifndef GENS_K6B_HID3
#define GENS_K6B_HID3 7
#endif
#define GB_HID3(NLEV_) ((NLEV_) == 3 ? GENS_K6B_HID3 : 8)

// Cycle stamps of the gradient kernel's phases (build with -DGENS_K6B_STAMPS: make -C gens_amd/csrc stamps; scripts/probe/k6b_stamps_probe.py
// reads them): never in the shipped library.  GB_STAMP(K_) ends a stretch of kind K_: 0 products (MFMAs, their LDS reads, whatever sits in
// their gaps), 1 a boundary's vmcnt wait, 2 its barrier, 3 its refill issues, 4 a forward layer's softplus and split, 5 a reverse layer's
// product with softplus' and split, 6 the chain rule to x.  Every wave adds its cycles per kind into k6b_stamps[wave][K_], the number of
// stamps of that kind into [wave][8 + K_], the cost of one stamp (two back to back) into [wave][7] and one into [wave][15].
#ifdef GENS_K6B_STAMPS
__device__ unsigned long long k6b_stamps[GB_WAVES][16];
#define GB_STAMP_READ(T_)                                                                  \
    __builtin_amdgcn_sched_barrier(0);                                                     \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(T_)::"memory");             \
    __builtin_amdgcn_sched_barrier(0);
#define GB_STAMP_INIT()                                                                    \
    unsigned long long st_sum[8] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull}, st_last, st_now; \
    int st_cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};                                              \
    GB_STAMP_READ(st_last)                                                                 \
    GB_STAMP_READ(st_now)                                                                  \
    st_sum[7] = st_now - st_last;                                                          \
    st_last = st_now;
#define GB_STAMP(K_)                                                                       \
    {                                                                                      \
        GB_STAMP_READ(st_now)                                                              \
        st_sum[K_] += st_now - st_last;                                                    \
        st_last = st_now;                                                                  \
        ++st_cnt[K_];                                                                      \
    }
#define GB_STAMP_WRITE()                                                                   \
    if (lane == 0) {                                                                       \
        _Pragma("unroll") for (int k_ = 0; k_ < 8; ++k_) {                                 \
            atomicAdd(&k6b_stamps[wave][k_], st_sum[k_]);                                  \
            atomicAdd(&k6b_stamps[wave][8 + k_], k_ < 7 ? (unsigned long long)st_cnt[k_] : 1ull); \
        }                                                                                  \
    }
#else
#define GB_STAMP_INIT()
#define GB_STAMP(K_)
#define GB_STAMP_WRITE()
#endif

#define GB_PUT(BLK_, W_, A_, B_)                                            \
    {                                                                       \
        const Split3Word sw__ = split3_pair((A_), (B_));                    \
        _Pragma("unroll") for (int k__ = 0; k__ < GB_TERMS; ++k__) (BLK_).p[k__][(W_)] = sw__.w[k__]; \
    }

// The point encoding of this lane as B-operand blocks.  Expands inside sdf_bf16x3_k and reads its locals x[3] (the point), scale and half
// (the lane's half of the K slots); with ONLY_ = -1 it also adds the three inputs to the kernel's nan_sum.  Two modes:
//   ONLY_ = -1    both K blocks -> P_[0], P_[1]                   (the prologue of every build)
//   ONLY_ = 0, 1  that K block alone -> P_[0], nan_sum untouched  (the two-wave build at layer 3, which encodes x again)
// A macro and not a function: as a lambda the one-wave builds no longer compiled to the instructions they had.
#define GB_ENCODE_POINT(P_, ONLY_)                                          \
    {                                                                       \
        float qe_[16];                                                      \
        _Pragma("unroll") for (int ke_ = 0; ke_ < 16; ++ke_) qe_[ke_] = 0.0f; \
        _Pragma("unroll") for (int ae_ = 0; ae_ < 3; ++ae_) {               \
            const float v = x[ae_] * scale;                                 \
            float s0, c0, s1, c1;                                           \
            hw_sincos(v * (half ? 4.0f : 1.0f), s0, c0);                    \
            hw_sincos(v * (half ? 8.0f : 2.0f), s1, c1);                    \
            if (half == 0) {                                                \
                qe_[ae_] = v; qe_[3 + ae_] = s0; qe_[6 + ae_] = c0; qe_[9 + ae_] = s1; qe_[12 + ae_] = c1; \
            } else {                                                        \
                qe_[ae_] = s0; qe_[3 + ae_] = c0; qe_[6 + ae_] = s1; qe_[9 + ae_] = c1; \
            }                                                               \
            if ((ONLY_) < 0) nan_sum += x[ae_];                             \
        }                                                                   \
        if (half == 0) qe_[15] = 1.0f;                                      \
        _Pragma("unroll") for (int ke_ = 0; ke_ < 16; ke_ += 2)             \
            if ((ONLY_) < 0 || (ONLY_) == (ke_ >> 3)) GB_PUT((P_)[(ONLY_) < 0 ? ke_ >> 3 : 0], (ke_ & 7) >> 1, qe_[ke_], qe_[ke_ + 1]) \
    }

// value of one packed (X, Y, Z, 4) volume at x and its derivative with respect to x (zero padding, align_corners=True)
__device__ __forceinline__ float4 sample_volume4b(const float4* __restrict__ v, int Xd, int Yd, int Zd, const float x[3], bool live, float4& jx,
                                                  float4& jy, float4& jz) {
    float w0[3], w1[3];
    int i0[3];
    bool in0[3], in1[3];
    const int sz[3] = {Xd, Yd, Zd};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float pos = (x[a] + 1.0f) / 2.0f * (float)(sz[a] - 1);
        const float f = fminf(fmaxf(floorf(pos), -2.0f), (float)sz[a] + 1.0f);
        i0[a] = (int)f;
        w0[a] = (f + 1.0f) - pos;
        w1[a] = pos - f;
        in0[a] = i0[a] >= 0 && i0[a] < sz[a];
        in1[a] = i0[a] + 1 >= 0 && i0[a] + 1 < sz[a];
    }
    float4 acc = f4_zero();
    jx = f4_zero(); jy = f4_zero(); jz = f4_zero();
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int a = c >> 2, b = (c >> 1) & 1, d = c & 1;
        const bool ok = live && (a ? in1[0] : in0[0]) && (b ? in1[1] : in0[1]) && (d ? in1[2] : in0[2]);
        const int cx = min(max(i0[0] + a, 0), Xd - 1), cy = min(max(i0[1] + b, 0), Yd - 1), cz = min(max(i0[2] + d, 0), Zd - 1);
        float4 t = v[((int64_t)cx * Yd + cy) * Zd + cz];
        if (!ok) t = f4_zero();
        const float wx = a ? w1[0] : w0[0], wy = b ? w1[1] : w0[1], wz = d ? w1[2] : w0[2];
        acc = f4_madd(acc, t, wx * wy * wz);
        jx = f4_madd(jx, t, (a ? 1.0f : -1.0f) * wy * wz);
        jy = f4_madd(jy, t, wx * (b ? 1.0f : -1.0f) * wz);
        jz = f4_madd(jz, t, wx * wy * (d ? 1.0f : -1.0f));
    }
    const float sx = (float)(Xd - 1) / 2.0f, sy = (float)(Yd - 1) / 2.0f, sz_ = (float)(Zd - 1) / 2.0f;
    jx.x *= sx; jx.y *= sx; jx.z *= sx; jx.w *= sx;
    jy.x *= sy; jy.y *= sy; jy.z *= sy; jy.w *= sy;
    jz.x *= sz_; jz.y *= sz_; jz.z *= sz_; jz.w *= sz_;
    return acc;
}

// The piece stream, in the order the kernels consume it (gens_amd.ops._pack_grad_pieces(..., terms=3)): k6gh's order with three pieces
// (x0, x1, x2) per (K block, output tile) instead of (hi, lo), and forward layer 3 with GB_HID3 hidden blocks.  The block-major value kernels
// read the forward part only; the tile-major one reads a stream of its own (order="tile"): the same pieces, the same layer offsets fwd(l),
// [tile][block][term] within a layer.
template <int NLEV>
struct GradShapeB {
    static constexpr int CF = 4 * NLEV;
    static constexpr int NCH = CF / 2;                     // channels per lane half
    static constexpr int NC = (5 * NCH + 1 + 7) / 8;       // conditioning K blocks: 5 encodings per channel + the constant-one slot
    static constexpr int TC = (5 * NCH + 15) / 16;         // accumulator tiles of the conditioning gradient (16 slots of a half per tile)
    static constexpr int BLK = 4 * GB_TERMS;               // pieces of one forward K block
    static constexpr int HID3 = GB_HID3(NLEV);            // hidden K blocks of forward layer 3
    static constexpr int blocks(int l) { return l == 0 ? 2 : l == 3 ? NC + 2 + HID3 : NC + 8; }      // K blocks of forward layer l
    static constexpr int fwd(int l) { return l == 0 ? 0 : BLK * (2 + (l - 1) * (NC + 8) + (l > 3 ? 2 + HID3 - 8 : 0)); }      // first piece of forward layer l
    static constexpr int FWD_PIECES = fwd(5) + BLK * blocks(5);
    static constexpr int rev_tiles(int l) { return 4 + TC + (l == 3 ? 1 : 0); }
    static constexpr int rev_blocks(int l) { return l == 2 ? 7 : 8; }
    static constexpr int rev(int l) {      // first piece of reverse layer l = 5 .. 1; rev(0): the G_0 blocks
        int p = FWD_PIECES;
        for (int k = 5; k > l; --k) p += GB_TERMS * rev_tiles(k) * rev_blocks(k);
        return p;
    }
    static constexpr int PIECES = rev(0) + 8 * GB_TERMS;
    static constexpr int NCHUNK = (PIECES + GB_CH - 1) / GB_CH;
    static constexpr int NCHUNK_FWD = (FWD_PIECES + GB_CH - 1) / GB_CH;
};

template <int NLEV, bool GRAD>
__global__ __launch_bounds__(64 * GB_WAVES, GB_OCC(NLEV, GRAD)) void sdf_bf16x3_k(LevelSet vols, const char* __restrict__ pieces, const float* w_out, float b_last,
                                                                 float scale, float inv_scale, const float* __restrict__ pts,
                                                                 const int64_t* __restrict__ index, int64_t n_max, const int32_t* __restrict__ n_dev,
                                                                 float* __restrict__ sdf_out, float* __restrict__ grad_out,
                                                                 char* __restrict__ stash_all) {
    typedef GradShapeB<NLEV> S;
    constexpr int NCH = S::NCH, NC = S::NC, TC = S::TC, MID = NLEV / 2;
    constexpr int NCHUNK = GRAD ? S::NCHUNK : S::NCHUNK_FWD;
    // DIET: the build for two waves per SIMD, <= 256 registers: A operands one tile ahead (GT = 1), the point encoded again at layer 3 and
    // the last GB_NCL conditioning blocks read back from LDS at every layer; the MFMAs, their operands and their order per accumulator are
    // those of the one-wave build
    constexpr bool DIET = GB_OCC(NLEV, GRAD) == 2;
    constexpr int GT = DIET ? 1 : GB_GT;
    constexpr int PLACE = GB_PLACE(NLEV, GRAD);
    // TM: the forward layers tile by tile on the tile-major value stream (GB_TILE_MAJOR above)
    constexpr bool TM = GB_TILE_MAJOR(NLEV, GRAD);
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n_pt = lane & 31, half = lane >> 5;
    const int64_t n = n_dev ? min(n_max, (int64_t)n_dev[0]) : n_max;
    const int64_t m0 = (int64_t)blockIdx.x * (32 * GB_WAVES);
    if (m0 >= n) return;
    float4* const DS = (float4*)(lds + GB_W_BYTES + wave * GB_D_BYTES);       // [layer][accumulator register / 4][lane]  (GRAD only)

    // chunk c of the stream -> ring slot c % GB_RING: wave w brings pieces w, w + 4, .. (LDS-direct buffer loads: the piece's offset in
    // the stream is a scalar, 16 lane the one vector offset, lane i lands at the piece's base in LDS + 16 i)
    const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc((void*)pieces, 0, NCHUNK * GB_CH * GB_PIECE, 0x00020000);
    const uint32_t lane16 = (uint32_t)lane * 16u;
    auto stage1 = [&](int c, int p) {      // this wave's p-th piece of chunk c
        char* dst = lds + (c % GB_RING) * (GB_CH * GB_PIECE);
        const int piece = wave + GB_WAVES * p;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(prs, (__attribute__((address_space(3))) void*)(dst + piece * GB_PIECE), 16, lane16,
                                                 (uint32_t)(c * (GB_CH * GB_PIECE) + piece * GB_PIECE), 0, 0);
    };
    auto stage = [&](int c) {
#pragma unroll
        for (int p = 0; p < GB_LPW; ++p) stage1(c, p);
    };
#pragma unroll
    for (int c = 0; c < GB_RING - 1; ++c) stage(c);

    // this wave's slot of the stash (one workgroup per CU -- the LDS allocation sees to it -- so (CU, wave) is unique; the lock word
    // makes that a performance assumption instead of a correctness one)
    uint32_t* lock = nullptr;
    uint32_t lock_seen = 0u;
    __amdgpu_buffer_rsrc_t stash;
    if constexpr (GRAD) {
        uint32_t hw_id, xcc_id;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));          // [11:8] CU, [15:13] SE (scripts/probe/hwid_probe.py)
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_id));
        const uint32_t slot = ((((xcc_id & 7u) << 2 | ((hw_id >> 13) & 3u)) << 4 | ((hw_id >> 8) & 15u)) << 2) | (uint32_t)wave;
        char* const stash_slot = stash_all + (size_t)slot * GB_SLOT_BYTES;
        lock = (uint32_t*)(stash_slot + GB_LOCK_OFF);
        lock_seen = lane == 0 ? atomicCAS(lock, 0u, 1u) : 0u;      // (asked for here, looked at before the first store into the slot)
        stash = __builtin_amdgcn_make_buffer_rsrc((void*)stash_slot, 0, GB_LOCK_OFF, 0x00020000);
    }
    const uint32_t stash_lane = (uint32_t)lane * 16u, jl_lane = GB_JL_OFF + (uint32_t)lane * 4u;

    // ------------------------------------------------------------------ prologue: this lane's B-operand slots
    const int64_t row = m0 + 32 * wave + n_pt;
    const bool live = row < n;
    const int64_t src = live ? (index ? index[row] : row) : 0;
    float x[3] = {0.f, 0.f, 0.f};
    if (live) { x[0] = pts[3 * src]; x[1] = pts[3 * src + 1]; x[2] = pts[3 * src + 2]; }
    float nan_sum = 0.0f;      // not-a-number inputs must come out as not-a-number: see the poison term below

    Split3Block P[2];     // point encoding: half 0 = x, octaves 0 and 1, ONE; half 1 = octaves 2 and 3, zeros
    GB_ENCODE_POINT(P, -1)

    Split3Block C[NC];    // volume features: 5 encodings of this half's NCH channels, then ONE (half 0), then zeros
    const float* wo = w_out + half * (64 + 16 * TC);
    float s_cond = 0.0f;
    float f[NCH];        // the raw features: the chain rule at the end re-derives the encodings from them
    {
        float jl[3 * NCH];
#pragma unroll
        for (int j = 0; j <= MID; ++j) {     // whole levels of this half (j < MID); level MID is shared, two channels each
            const int l = j < MID ? (half ? MID + 1 + j : j) : MID;
            float4 jx, jy, jz;
            const float4 t = sample_volume4b((const float4*)vols.data[l], vols.dx[l], vols.dy[l], vols.dz[l], x, live, jx, jy, jz);
            float tv[4] = {t.x, t.y, t.z, t.w}, ax[4] = {jx.x, jx.y, jx.z, jx.w}, ay[4] = {jy.x, jy.y, jy.z, jy.w}, az[4] = {jz.x, jz.y, jz.z, jz.w};
            if (j == MID && half) {
                tv[0] = tv[2]; tv[1] = tv[3]; ax[0] = ax[2]; ax[1] = ax[3]; ay[0] = ay[2]; ay[1] = ay[3]; az[0] = az[2]; az[1] = az[3];
            }
#pragma unroll
            for (int c = 0; c < (j < MID ? 4 : 2); ++c) {
                const int ch = 4 * j + c;
                f[ch] = tv[c];
                jl[3 * ch] = ax[c]; jl[3 * ch + 1] = ay[c]; jl[3 * ch + 2] = az[c];
            }
        }
        if constexpr (GRAD) {
            if (lane == 0) gens_lock_slot(lock, lock_seen);
#pragma unroll
            for (int k = 0; k < 3 * NCH; ++k) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, jl[k]), stash, jl_lane + (uint32_t)k * 256u, 0, 0);
        }
        float e[8 * NC];
#pragma unroll
        for (int k = 5 * NCH; k < 8 * NC; ++k) e[k] = (k == 5 * NCH && half == 0) ? 1.0f : 0.0f;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            e[5 * j] = f[j];
            hw_sincos(f[j], e[5 * j + 1], e[5 * j + 2]);
            hw_sincos(2.0f * f[j], e[5 * j + 3], e[5 * j + 4]);
            nan_sum += f[j];
#pragma unroll
            for (int q = 0; q < 5; ++q) s_cond = __builtin_fmaf(e[5 * j + q], wo[64 + 5 * j + q], s_cond);       // layer 6 reads the conditioning features too
        }
        if constexpr (DIET) {      // finished HERE: left to itself the compiler sinks the two sums to layer 3 and carries e[] and w_out to them
            asm volatile("" : "+v"(s_cond));
            asm volatile("" : "+v"(nan_sum));
        }
#pragma unroll
        for (int k = 0; k < 8 * NC; k += 2) GB_PUT(C[k >> 3], (k & 7) >> 1, e[k], e[k + 1])
    }

    // [block][term][lane], this wave's own; the other builds allocate no such area and get no pointer to one
    u32x4* const CL = DIET ? (u32x4*)(lds + GB_W_BYTES + wave * GB_CL_BYTES) : nullptr;
    if constexpr (DIET) {
#pragma unroll
        for (int b = 0; b < GB_NCL; ++b)
#pragma unroll
            for (int k = 0; k < GB_TERMS; ++k) CL[(b * GB_TERMS + k) * 64 + lane] = C[NC - GB_NCL + b].p[k];
    }

    f32x16 acc[4];                 // the product being accumulated
    Split3Block H[8];              // the operand of the running product: activations, then G_l (block 2 t + (r >> 3), slot r & 7 <- tile t, register r)
    f32x16 D3[4], D4[4];           // softplus' of layers 3, 4 (GRAD)
    f32x16 gc[TC], gp;             // d sdf / d (this lane's conditioning slots), d sdf / d (its point-encoding slots)
    u32x4 abuf[2][GB_TERMS * GT];      // A operands: this group's and the next one's
    int par = 0;                   // (compile-time after unrolling, like every index below)
    int dirty = GRAD ? 1 : 0;      // stores are outstanding: the next chunk boundary waits for everything
    int pend = -1, pend_i = 0;     // the chunk whose refill the last boundary left to the MFMA gaps, and this wave's next piece of it
    GB_STAMP_INIT()

    // chunk boundary: this wave's share of chunk C_ has landed (its later chunks may still be in flight), every wave says so, and the
    // ring slot everyone has just finished reading is refilled three chunks ahead
    //
    // The refill is not issued at the boundary (PLACE 1): the boundary leaves it pending (pend, pend_i) and the MFMAs that follow
    // issue it one piece per MFMA gap (GB_FILL).  INVARIANT: when boundary c begins its wait, this wave has issued all its pieces of every
    // chunk <= min(c + GB_RING - 2, NCHUNK - 1) and of no later one -- a refill still pending then (two boundaries with no MFMA between them:
    // the first two loads of a segment) is issued there, in front of the wait -- so the vmcnt immediates below count exactly the later__
    // chunks of GB_LPW loads that may stay in flight, and after the wait this wave's pieces of chunk c have landed.  (Stash loads and stores
    // in flight only make the wait longer: buffer loads return in order, and `dirty` waits for everything.)
#define GB_PEND_FLUSH()                                                                                  \
    while (pend >= 0) {                                                                                  \
        stage1(pend, pend_i);                                                                            \
        if (++pend_i == GB_LPW) pend = -1;                                                               \
    }
#define GB_BOUNDARY(C_)                                                                                  \
    {                                                                                                    \
        const int c__ = (C_);                                                                            \
        const int later__ = (c__ + GB_RING - 2 < NCHUNK - 1 ? c__ + GB_RING - 2 : NCHUNK - 1) - c__;     \
        GB_PEND_FLUSH()                                                                                  \
        GB_STAMP(0)                                                                                      \
        if (dirty || later__ <= 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                      \
        else if (later__ == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(GB_LPW) : "memory");             \
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * GB_LPW) : "memory");                           \
        dirty = 0;                                                                                       \
        GB_STAMP(1)                                                                                      \
        __builtin_amdgcn_s_barrier();                                                                    \
        asm volatile("" ::: "memory");                                                                   \
        GB_STAMP(2)                                                                                      \
        if (c__ + GB_RING - 1 < NCHUNK) {                                                                \
            if (PLACE == 0) {                                                                            \
                stage(c__ + GB_RING - 1);                                                                \
                GB_STAMP(3)                                                                              \
            } else {                                                                                     \
                pend = c__ + GB_RING - 1;                                                                \
                pend_i = 0;                                                                              \
            }                                                                                            \
        }                                                                                                \
    }
    // pieces P0_ .. P0_ + CNT_ -> A register set SET_
#define GB_LOAD(SET_, P0_, CNT_)                                                                         \
    _Pragma("unroll") for (int j_ = 0; j_ < GB_TERMS * GT; ++j_) if (j_ < (CNT_)) {                      \
        const int p_ = (P0_) + j_;                                                                       \
        if (p_ % GB_CH == 0) GB_BOUNDARY(p_ / GB_CH)                                                     \
        abuf[SET_][j_] = *((const u32x4*)(lds + ((p_ / GB_CH) % GB_RING) * (GB_CH * GB_PIECE) + (p_ % GB_CH) * GB_PIECE) + lane); \
    }
    // the gap behind one MFMA: one piece of a pending refill -- an LDS-direct issue is the one long filler a gap has room for
#define GB_FILL()                                                                                        \
    if (pend >= 0) {                                                                                     \
        __builtin_amdgcn_sched_barrier(0);                                                               \
        stage1(pend, pend_i);                                                                            \
        if (++pend_i == GB_LPW) pend = -1;                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                               \
    }
#define GB_MFMA_(ACC_, A_, B_) ACC_ = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, (A_)), __builtin_bit_cast(bf16x8, (B_)), ACC_, 0, 0, 0)
#define GB_MFMA(ACC_, A_, B_) { GB_MFMA_(ACC_, A_, B_); GB_FILL() }
    // accumulator of output tile T_ of a reverse K block: hidden tiles, conditioning tiles, the point-encoding tile
#define GB_RACC(T_) (*((T_) < 4 ? &acc[(T_) < 4 ? (T_) : 0] : (T_) < 4 + TC ? &gc[(T_) < 4 + TC && (T_) >= 4 ? (T_) - 4 : 0] : &gp))
    // the six products of one operand pair, smallest first: weight term WA_ x activation term WB_
#define GB_TERM(WA_, WB_, REV_, B_)                                                                      \
    _Pragma("unroll") for (int t_ = 0; t_ < GT; ++t_) if (t_ < nt_) {                                    \
        if (REV_) GB_MFMA(GB_RACC(t0_ + t_), abuf[par][GB_TERMS * t_ + (WA_)], B_(i_).p[(WB_)])          \
        else GB_MFMA(acc[(t0_ + t_) & 3], abuf[par][GB_TERMS * t_ + (WA_)], B_(i_).p[(WB_)])             \
    }
    // the B operand of K block I_ of a segment: one of the kernel's three operand arrays, or (GB_OP_CPH) their concatenation as a tile-major
    // forward layer l reads it -- layer 0 the point encoding, the others C, at layer 3 the point-encoding block in P[0] (GB_PREP_TM), then H
    // (GB_OP_CPH and GB_PREP_TM expand inside the tile-major layer loop only and read its loop variable l and the kernel's lane, x, CL, NC)
#define GB_OP_P(I_) P[I_]
#define GB_OP_C(I_) C[I_]
#define GB_OP_H(I_) H[I_]
#define GB_OP_CPH(I_) (*(l == 0 ? &P[(I_) & 1] : (I_) < NC ? &C[(I_) < NC ? (I_) : 0] : l == 3 && (I_) < NC + 2 ? &P[0] : &H[((I_) - NC - (l == 3 ? 2 : 0)) & 7]))
    // what a tile-major segment does in front of K block I_: at block 0 the conditioning blocks that wait in LDS come back, at layer 3's two
    // point-encoding blocks x is encoded again (as the block-major two-wave build does once per layer, here once per tile)
#define GB_PREP_NONE(I_)
#define GB_PREP_TM(I_)                                                                                   \
    if (l > 0 && (I_) == 0) {      /* (opaque lane: a new address to the compiler, or it keeps the blocks of the tile before) */ \
        int lane_o = lane;                                                                               \
        asm volatile("" : "+v"(lane_o));                                                                 \
        _Pragma("unroll") for (int b_ = 0; b_ < GB_NCL; ++b_)                                            \
            _Pragma("unroll") for (int k_ = 0; k_ < GB_TERMS; ++k_) C[NC - GB_NCL + b_].p[k_] = CL[(b_ * GB_TERMS + k_) * 64 + lane_o]; \
    }                                                                                                    \
    if (l == 3 && (I_) >= NC && (I_) < NC + 2) {      /* (opaque x, or the compiler keeps the first copy) */ \
        _Pragma("unroll") for (int a_ = 0; a_ < 3; ++a_) asm volatile("" : "+v"(x[a_]));                 \
        GB_ENCODE_POINT(P, (I_) - NC)                                                                    \
    }
    // CNT_ K blocks of NT_ output tiles TB_ .. TB_ + NT_ - 1 from piece P0_ on, B operands B_(0 .. CNT_ - 1), PREP_(i) in front of block i;
    // REV_: the accumulators of a reverse block.  The A operands arrive in groups of GT tiles (three terms each), one group ahead of the
    // MFMAs that read them.  Within a group the accumulators alternate.
    // A tile base other than 0 goes with NT_ = 1 (one tile per segment: the tile-major calls); the offset of the next group's pieces counts
    // tiles from 0 and does not know TB_.
#define GB_SEGMENT(P0_, CNT_, NT_, TB_, B_, PREP_, REV_)                                                 \
    {                                                                                                    \
        constexpr int ng__ = ((NT_) + GT - 1) / GT;      /* (CNT_ and NT_ are constant expressions at every call) */ \
        GB_LOAD(par, (P0_), GB_TERMS * ((NT_) < GT ? (NT_) : GT))                                        \
        _Pragma("unroll") for (int q_ = 0; q_ < (CNT_) * ng__; ++q_) {                                   \
            const int i_ = q_ / ng__, t0_ = (TB_) + (q_ % ng__) * GT, nt_ = (TB_) + (NT_) - t0_ < GT ? (TB_) + (NT_) - t0_ : GT; \
            if (q_ + 1 < (CNT_) * ng__) {                                                                \
                const int i2_ = (q_ + 1) / ng__, t2_ = ((q_ + 1) % ng__) * GT, n2_ = (NT_) - t2_ < GT ? (NT_) - t2_ : GT; \
                GB_LOAD(par ^ 1, (P0_) + GB_TERMS * ((NT_) * i2_ + t2_), GB_TERMS * n2_)                  \
            }                                                                                            \
            PREP_(i_)                                                                                    \
            __builtin_amdgcn_sched_barrier(0);                                                           \
            GB_TERM(2, 0, REV_, B_) GB_TERM(1, 1, REV_, B_) GB_TERM(0, 2, REV_, B_)                      \
            GB_TERM(1, 0, REV_, B_) GB_TERM(0, 1, REV_, B_) GB_TERM(0, 0, REV_, B_)                      \
            __builtin_amdgcn_sched_barrier(0);                                                           \
            par ^= 1;                                                                                    \
        }                                                                                                \
    }
#define GB_ZERO()                                             \
    _Pragma("unroll") for (int t_ = 0; t_ < 4; ++t_)          \
        _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) acc[t_][r_] = 0.0f;
    // h~ = c softplus(a) = log2(1 + 2^t) and softplus' = 2^t / (1 + 2^t) of one accumulator tile (k6g_sdf_grad.hip: no compare masks, 16
    // independent instructions of one kind back to back)
#define GB_SOFTPLUS_TILE(T_, HT_, DT_)                                                                     \
    {                                                                                                      \
        f32x16 e__, u__, r__;                                                                              \
        _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) e__[r_] = __builtin_amdgcn_exp2f(__builtin_amdgcn_fmed3f((T_)[r_], 126.0f, -3.0e38f)); \
        _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) u__[r_] = 1.0f + e__[r_];                        \
        if (GRAD) { _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) r__[r_] = __builtin_amdgcn_rcpf(u__[r_]); } \
        _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) u__[r_] = __builtin_amdgcn_logf(u__[r_]);        \
        if (GRAD) { _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) (DT_)[r_] = e__[r_] * r__[r_]; }     \
        _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) (HT_)[r_] = __builtin_amdgcn_fmed3f((T_)[r_], u__[r_], 3.0e38f); \
    }
    // the 16 values of tile T_ -> K blocks 2 T_, 2 T_ + 1 of H
#define GB_SPLIT_TILE(T_, V_)                                                                              \
    _Pragma("unroll") for (int r_ = 0; r_ < 16; r_ += 2) GB_PUT(H[2 * (T_) + (r_ >> 3)], (r_ & 7) >> 1, (V_)[r_], (V_)[r_ + 1])

    // ------------------------------------------------------------------ forward
    float s_val = s_cond;
    if constexpr (TM) {
        // tile by tile: the matrix pipe has tile t + 1 of this wave, or whatever the other wave of the SIMD is at, while softplus runs on
        // tile t; the splits wait for the fourth tile, because H is the operand of all four
#pragma unroll
        for (int l = 0; l < 6; ++l) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
                if (l == 0) {
                    GB_SEGMENT(S::fwd(0) + GB_TERMS * 2 * t, 2, 1, t, GB_OP_CPH, GB_PREP_TM, false);
                } else if (l == 3) {
                    GB_SEGMENT(S::fwd(3) + GB_TERMS * (NC + 2 + S::HID3) * t, NC + 2 + S::HID3, 1, t, GB_OP_CPH, GB_PREP_TM, false);
                } else {
                    GB_SEGMENT(S::fwd(l) + GB_TERMS * (NC + 8) * t, NC + 8, 1, t, GB_OP_CPH, GB_PREP_TM, false);
                }
                GB_STAMP(0)
                f32x16 d;
                GB_SOFTPLUS_TILE(acc[t], acc[t], d);
                GB_STAMP(4)
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (l < 5) {
                    GB_SPLIT_TILE(t, acc[t]);
                } else {    // layer 6 is one row: the value is a dot product
#pragma unroll
                    for (int r = 0; r < 16; ++r) s_val = __builtin_fmaf(acc[t][r], wo[16 * t + r], s_val);
                }
            }
            GB_STAMP(4)
        }
    } else {
        GB_ZERO();
        GB_SEGMENT(S::fwd(0), 2, 4, 0, GB_OP_P, GB_PREP_NONE, false);
#pragma unroll
        for (int l = 0; l < 6; ++l) {
            if (l > 0) {
                GB_ZERO();
                if constexpr (DIET) {      // (opaque lane: a new address to the compiler, or it keeps the blocks of the layer before)
                    int lane_o = lane;
                    asm volatile("" : "+v"(lane_o));
#pragma unroll
                    for (int b = 0; b < GB_NCL; ++b)
#pragma unroll
                        for (int k = 0; k < GB_TERMS; ++k) C[NC - GB_NCL + b].p[k] = CL[(b * GB_TERMS + k) * 64 + lane_o];
                }
                GB_SEGMENT(S::fwd(l), NC, 4, 0, GB_OP_C, GB_PREP_NONE, false);
                if (l == 3) {
                    if constexpr (!DIET) {
                        GB_SEGMENT(S::fwd(3) + S::BLK * NC, 2, 4, 0, GB_OP_P, GB_PREP_NONE, false);
                    } else {
                        // x is encoded again, one K block at a time (the same instructions on the same x: the same bits), instead of 24 registers
                        // held from the prologue to here; opaque, or the compiler keeps the first copy
#pragma unroll
                        for (int pb = 0; pb < 2; ++pb) {
#pragma unroll
                            for (int a = 0; a < 3; ++a) asm volatile("" : "+v"(x[a]));
                            GB_ENCODE_POINT(P, pb)
                            GB_SEGMENT(S::fwd(3) + S::BLK * (NC + pb), 1, 4, 0, GB_OP_P, GB_PREP_NONE, false);
                        }
                    }
                }
                GB_SEGMENT(S::fwd(l) + S::BLK * (NC + (l == 3 ? 2 : 0)), (l == 3 ? S::HID3 : 8), 4, 0, GB_OP_H, GB_PREP_NONE, false);
            }
            GB_STAMP(0)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                f32x16 h, d;
                if (l == 3) {
                    GB_SOFTPLUS_TILE(acc[t], h, D3[t]);
                } else if (l == 4) {
                    GB_SOFTPLUS_TILE(acc[t], h, D4[t]);
                } else {
                    GB_SOFTPLUS_TILE(acc[t], h, d);
                }
                if constexpr (GRAD) {
                    if (l < 2) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) DS[(l * 16 + 4 * t + q) * 64 + lane] = make_float4(d[4 * q], d[4 * q + 1], d[4 * q + 2], d[4 * q + 3]);
                    }
                    if (l == 2) {
#pragma unroll
                        for (int q = 0; q < 4; ++q)      // (the register's offset in the VECTOR offset: see k6g_sdf_grad.hip)
                            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, (f32x4v){d[4 * q], d[4 * q + 1], d[4 * q + 2], d[4 * q + 3]}), stash,
                                                                   stash_lane + (uint32_t)(4 * t + q) * 1024u, 0, 0);
                        dirty = 1;
                    }
                }
                if (l < 5) {
                    GB_SPLIT_TILE(t, h);
                } else {    // layer 6 is one row: the value is a dot product, and G_5 = w_last * softplus' starts the reverse pass
                    f32x16 g;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float w = wo[16 * t + r];                      // w_last / c in this lane's accumulator order
                        s_val = __builtin_fmaf(h[r], w, s_val);
                        if (GRAD) g[r] = (w * GB_C) * d[r];
                    }
                    if constexpr (GRAD) GB_SPLIT_TILE(t, g);
                }
            }
            GB_STAMP(4)
        }
    }
    // not-a-number inputs must come out as not-a-number (the reference's layers propagate them; the max / median forms of the activation drop
    // them): a poison term 0 * (sum of the inputs), NaN iff one of them is NaN or infinite
    s_val += 0.0f * nan_sum;
    s_val += __shfl_xor(s_val, 32, 64);

    if constexpr (!GRAD) {
        if constexpr (!DIET) {
            if (half == 0 && live) sdf_out[src] = (s_val + b_last) * inv_scale;
        } else {      // the row is looked up again (opaque lane number), not carried in two registers through the layers
            int lane_o = lane;
            asm volatile("" : "+v"(lane_o));
            const int64_t row_o = m0 + 32 * wave + (lane_o & 31);
            if (lane_o < 32 && row_o < n) sdf_out[index ? index[row_o] : row_o] = (s_val + b_last) * inv_scale;
        }
    } else {
        // ------------------------------------------------------------------ reverse pass
#pragma unroll
        for (int c = 0; c < TC; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) gc[c][r] = (16 * c + r < 5 * NCH) ? wo[64 + 16 * c + r] : 0.0f;      // layer 6 reads the features directly
#pragma unroll
        for (int r = 0; r < 16; ++r) gp[r] = 0.0f;
#pragma unroll
        for (int l = 5; l >= 1; --l) {
            GB_ZERO();
            if (l == 3) {      // softplus' of layer 2 comes back into the registers layer 4's has left (requested before the products that hide the trip)
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const f32x4v v = __builtin_bit_cast(f32x4v, __builtin_amdgcn_raw_buffer_load_b128(stash, stash_lane + (uint32_t)(4 * t + q) * 1024u, 0, 0));
                        D4[t][4 * q] = v[0]; D4[t][4 * q + 1] = v[1]; D4[t][4 * q + 2] = v[2]; D4[t][4 * q + 3] = v[3];
                    }
            }
            if (l == 3) {
                GB_SEGMENT(S::rev(3), 8, 4 + TC + 1, 0, GB_OP_H, GB_PREP_NONE, true);
            } else if (l == 2) {
                GB_SEGMENT(S::rev(2), 7, 4 + TC, 0, GB_OP_H, GB_PREP_NONE, true);
            } else {
                GB_SEGMENT(S::rev(l), 8, 4 + TC, 0, GB_OP_H, GB_PREP_NONE, true);
            }
            // G_{l-1} = (W_l^T G_l) * softplus'(a_{l-1})
            GB_STAMP(0)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                f32x16 g;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float4 d;
                    if (l == 5) d = make_float4(D4[t][4 * q], D4[t][4 * q + 1], D4[t][4 * q + 2], D4[t][4 * q + 3]);
                    if (l == 4) d = make_float4(D3[t][4 * q], D3[t][4 * q + 1], D3[t][4 * q + 2], D3[t][4 * q + 3]);
                    if (l == 3) d = make_float4(D4[t][4 * q], D4[t][4 * q + 1], D4[t][4 * q + 2], D4[t][4 * q + 3]);
                    if (l == 2) d = DS[(16 + 4 * t + q) * 64 + lane];
                    if (l == 1) d = DS[(4 * t + q) * 64 + lane];
                    g[4 * q] = acc[t][4 * q] * d.x;
                    g[4 * q + 1] = acc[t][4 * q + 1] * d.y;
                    g[4 * q + 2] = acc[t][4 * q + 2] * d.z;
                    g[4 * q + 3] = acc[t][4 * q + 3] * d.w;
                }
                GB_SPLIT_TILE(t, g);
            }
            GB_STAMP(5)
        }
        {   // layer 0 reads the point encoding only: the six products in five independent chains, added smallest first at the end
            GB_ZERO();
            GB_LOAD(par, S::rev(0), GB_TERMS)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (i + 1 < 8) { GB_LOAD(par ^ 1, S::rev(0) + GB_TERMS * (i + 1), GB_TERMS) }
                __builtin_amdgcn_sched_barrier(0);
                GB_MFMA(acc[0], abuf[par][2], H[i].p[0])
                GB_MFMA(acc[1], abuf[par][1], H[i].p[1])
                GB_MFMA(acc[2], abuf[par][1], H[i].p[0])
                GB_MFMA(acc[0], abuf[par][0], H[i].p[2])
                GB_MFMA(acc[3], abuf[par][0], H[i].p[1])
                GB_MFMA(gp, abuf[par][0], H[i].p[0])
                __builtin_amdgcn_sched_barrier(0);
                par ^= 1;
            }
            GB_STAMP(0)
#pragma unroll
            for (int r = 0; r < 16; ++r) gp[r] += (acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r]);
        }

        // ------------------------------------------------------------------ chain rule to x, lane-local (sdf_network.py:131-154)
        {
            float g[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) asm volatile("" : "+v"(x[a]));      // (opaque: or the compiler keeps the prologue's encodings alive instead)
#pragma unroll
            for (int j = 0; j < NCH; ++j) asm volatile("" : "+v"(f[j]));
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float v = x[a] * scale;
                float s0, c0, s1, c1;
                hw_sincos(v * (half ? 4.0f : 1.0f), s0, c0);
                hw_sincos(v * (half ? 8.0f : 2.0f), s1, c1);
                // half 0 slots: x, sin / cos of octaves 0 and 1; half 1: sin / cos of octaves 2 and 3
                g[a] = half ? 4.0f * (gp[a] * c0 - gp[3 + a] * s0) + 8.0f * (gp[6 + a] * c1 - gp[9 + a] * s1)
                            : gp[a] + (gp[3 + a] * c0 - gp[6 + a] * s0) + 2.0f * (gp[9 + a] * c1 - gp[12 + a] * s1);
                g[a] *= scale;
            }
            {
                float acc_in = x[0] + x[1] + x[2];
#pragma unroll
                for (int j = 0; j < NCH; ++j) acc_in += f[j];
#pragma unroll
                for (int a = 0; a < 3; ++a) g[a] += 0.0f * acc_in;
            }
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                const int q = 5 * j;
                float s1, c1, s2, c2;
                hw_sincos(f[j], s1, c1);
                hw_sincos(2.0f * f[j], s2, c2);
                const float df = gc[q >> 4][q & 15] + gc[(q + 1) >> 4][(q + 1) & 15] * c1 - gc[(q + 2) >> 4][(q + 2) & 15] * s1 +
                                 2.0f * (gc[(q + 3) >> 4][(q + 3) & 15] * c2 - gc[(q + 4) >> 4][(q + 4) & 15] * s2);
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const float jl = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(stash, jl_lane + (uint32_t)(3 * j + a) * 256u, 0, 0));
                    g[a] = __builtin_fmaf(df, jl, g[a]);
                }
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) g[a] += __shfl_xor(g[a], 32, 64);
            if (half == 0 && live) {
                sdf_out[src] = (s_val + b_last) * inv_scale;
                grad_out[3 * src] = g[0] * inv_scale;
                grad_out[3 * src + 1] = g[1] * inv_scale;
                grad_out[3 * src + 2] = g[2] * inv_scale;
            }
        }
        GB_STAMP(6)
        GB_STAMP_WRITE()
        if (lane == 0) atomicExch(lock, 0u);
    }
#undef GB_PEND_FLUSH
#undef GB_BOUNDARY
#undef GB_LOAD
#undef GB_FILL
#undef GB_MFMA_
#undef GB_MFMA
#undef GB_RACC
#undef GB_TERM
#undef GB_OP_P
#undef GB_OP_C
#undef GB_OP_H
#undef GB_OP_CPH
#undef GB_PREP_NONE
#undef GB_PREP_TM
#undef GB_SEGMENT
#undef GB_ZERO
#undef GB_SOFTPLUS_TILE
#undef GB_SPLIT_TILE
}

int gens_fill_levels(const char* who, LevelSet* ls, const float* const* data, const int* dims, int n_levels);

extern "C" int gens_sdf_bf16x3_pieces(int n_levels) {
    return n_levels == 3 ? GradShapeB<3>::NCHUNK * GB_CH : n_levels == 5 ? GradShapeB<5>::NCHUNK * GB_CH : 0;
}

// What the packer has to know about this build (the orders are compile-time switches: GENS_K6B_TILE_MAJOR, GENS_K6B_HID3).
extern "C" int gens_sdf_bf16x3_layout(int n_levels, int out[3]) {
    GENS_CHECK_ARG(n_levels == 3 || n_levels == 5, GENS_ELIMIT, "gens_sdf_bf16x3_layout: built for 3 or 5 volume levels, got %d", n_levels);
    GENS_CHECK_ARG(out, GENS_EINVAL, "gens_sdf_bf16x3_layout: null output");
    out[0] = (n_levels == 3 ? GradShapeB<3>::NCHUNK_FWD : GradShapeB<5>::NCHUNK_FWD) * GB_CH;
    out[1] = n_levels == 3 ? GB_TILE_MAJOR(3, false) : GB_TILE_MAJOR(5, false);
    out[2] = n_levels == 3 ? GB_HID3(3) : GB_HID3(5);
    return 0;
}

static GensLdsOptIn g_grad_lds3, g_grad_lds5;     // the gradient kernels' 160 KB of LDS, granted once per device

extern "C" int64_t gens_sdf_grad_f16_stash_bytes(void);      // the stash is k6gh's: the same slots, the same layout

static int check_bf16x3_args(const char* who, int n_levels, const void* pieces, const float* w_out, float scale, const float* pts, int64_t n,
                             const float* sdf_out) {
    GENS_CHECK_ARG(n_levels == 3 || n_levels == 5, GENS_ELIMIT, "%s: built for 3 or 5 volume levels, got %d", who, n_levels);
    GENS_CHECK_ARG(pieces && w_out, GENS_EINVAL, "%s: null weight stream", who);
    GENS_CHECK_ARG(((uintptr_t)pieces & 15) == 0, GENS_EINVAL, "%s: the weight stream must be 16-byte aligned", who);
    GENS_CHECK_ARG(n >= 0 && (n == 0 || (pts && sdf_out)), GENS_EINVAL, "%s: null pts / output", who);
    GENS_CHECK_ARG(scale != 0.0f, GENS_EINVAL, "%s: scale must be non-zero", who);
    return 0;
}

extern "C" int gens_sdf_value_bf16x3(const float* const* vols_packed, const int* dims, int n_levels, const void* pieces, const float* w_out,
                                     float b_last, float scale, const float* pts, const int64_t* index, int64_t n, const int32_t* n_device,
                                     float* sdf_out, void* stream) {
    LevelSet vs;
    if (int e = gens_fill_levels("gens_sdf_value_bf16x3", &vs, vols_packed, dims, n_levels)) return e;
    if (int e = check_bf16x3_args("gens_sdf_value_bf16x3", n_levels, pieces, w_out, scale, pts, n, sdf_out)) return e;
    if (n == 0) return 0;
    const unsigned grid = gens_blocks(n, 32 * GB_WAVES);
    if (n_levels == 3)
        sdf_bf16x3_k<3, false><<<grid, 64 * GB_WAVES, GB_VALUE_LDS_BYTES(3), (hipStream_t)stream>>>(vs, (const char*)pieces, w_out, b_last, scale, 1.0f / scale, pts,
                                                                                          index, n, n_device, sdf_out, nullptr, nullptr);
    else
        sdf_bf16x3_k<5, false><<<grid, 64 * GB_WAVES, GB_VALUE_LDS_BYTES(5), (hipStream_t)stream>>>(vs, (const char*)pieces, w_out, b_last, scale, 1.0f / scale, pts,
                                                                                          index, n, n_device, sdf_out, nullptr, nullptr);
    return gens_launch_status("gens_sdf_value_bf16x3");
}

extern "C" int gens_sdf_grad_bf16x3(const float* const* vols_packed, const int* dims, int n_levels, const void* pieces, const float* w_out,
                                    float b_last, float scale, const float* pts, const int64_t* index, int64_t n, const int32_t* n_device,
                                    float* sdf_out, float* grad_out, void* stash, void* stream) {
    LevelSet vs;
    if (int e = gens_fill_levels("gens_sdf_grad_bf16x3", &vs, vols_packed, dims, n_levels)) return e;
    if (int e = check_bf16x3_args("gens_sdf_grad_bf16x3", n_levels, pieces, w_out, scale, pts, n, sdf_out)) return e;
    GENS_CHECK_ARG(n == 0 || grad_out, GENS_EINVAL, "gens_sdf_grad_bf16x3: null gradient output");
    GENS_CHECK_ARG(stash && ((uintptr_t)stash & 15) == 0, GENS_EINVAL,
                   "gens_sdf_grad_bf16x3: null or misaligned stash (gens_sdf_grad_f16_stash_bytes() bytes, zeroed once)");
    GENS_CHECK_ARG(gens_sdf_grad_f16_stash_bytes() == (int64_t)GB_SLOTS * GB_SLOT_BYTES, GENS_EINVAL, "gens_sdf_grad_bf16x3: stash layout differs from k6gh's");
    if (n == 0) return 0;
    if (int e = n_levels == 3 ? gens_lds_opt_in(g_grad_lds3, (const void*)sdf_bf16x3_k<3, true>, GB_LDS_BYTES, "gens_sdf_grad_bf16x3")
                              : gens_lds_opt_in(g_grad_lds5, (const void*)sdf_bf16x3_k<5, true>, GB_LDS_BYTES, "gens_sdf_grad_bf16x3"))
        return e;
    const unsigned grid = gens_blocks(n, 32 * GB_WAVES);
    if (n_levels == 3)
        sdf_bf16x3_k<3, true><<<grid, 64 * GB_WAVES, GB_LDS_BYTES, (hipStream_t)stream>>>(vs, (const char*)pieces, w_out, b_last, scale, 1.0f / scale, pts,
                                                                                           index, n, n_device, sdf_out, grad_out, (char*)stash);
    else
        sdf_bf16x3_k<5, true><<<grid, 64 * GB_WAVES, GB_LDS_BYTES, (hipStream_t)stream>>>(vs, (const char*)pieces, w_out, b_last, scale, 1.0f / scale, pts,
                                                                                           index, n, n_device, sdf_out, grad_out, (char*)stash);
    return gens_launch_status("gens_sdf_grad_bf16x3");
}

// What the device says about one instantiation at the launcher's own block and LDS sizes: registers per lane, scratch bytes per lane, dynamic
// LDS bytes, resident workgroups per CU.
extern "C" int gens_sdf_bf16x3_residency(int n_levels, int grad, int out[4]) {
    GENS_CHECK_ARG(n_levels == 3 || n_levels == 5, GENS_ELIMIT, "gens_sdf_bf16x3_residency: built for 3 or 5 volume levels, got %d", n_levels);
    GENS_CHECK_ARG(out, GENS_EINVAL, "gens_sdf_bf16x3_residency: null output");
    const void* fn = grad ? (n_levels == 3 ? (const void*)sdf_bf16x3_k<3, true> : (const void*)sdf_bf16x3_k<5, true>)
                          : (n_levels == 3 ? (const void*)sdf_bf16x3_k<3, false> : (const void*)sdf_bf16x3_k<5, false>);
    const int lds = grad ? GB_LDS_BYTES : n_levels == 3 ? GB_VALUE_LDS_BYTES(3) : GB_VALUE_LDS_BYTES(5);
    if (grad)
        if (int e = gens_lds_opt_in(n_levels == 3 ? g_grad_lds3 : g_grad_lds5, fn, GB_LDS_BYTES, "gens_sdf_bf16x3_residency")) return e;
    hipFuncAttributes attr;
    int blocks = 0;
    hipError_t err = hipFuncGetAttributes(&attr, fn);
    if (err == hipSuccess) err = hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, fn, 64 * GB_WAVES, lds);
    if (err != hipSuccess) {
        (void)hipGetLastError();
        gens_set_error("gens_sdf_bf16x3_residency: %s", hipGetErrorString(err));
        return (int)err;
    }
    out[0] = attr.numRegs;
    out[1] = (int)attr.localSizeBytes;
    out[2] = lds;
    out[3] = blocks;
    return 0;
}

#ifdef GENS_K6B_STAMPS
extern "C" int gens_debug_k6b_stamps(unsigned long long* out, int reset) {
    if (reset) {
        unsigned long long z[GB_WAVES * 16] = {0};
        return hipMemcpyToSymbol(HIP_SYMBOL(k6b_stamps), z, sizeof(z)) == hipSuccess ? 0 : 1;
    }
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(k6b_stamps), sizeof(unsigned long long) * GB_WAVES * 16) == hipSuccess ? 0 : 1;
}
#endif
