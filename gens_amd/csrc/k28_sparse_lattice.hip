// K28: the two-level lattice of extract_geometry (implicit_surface.py:407-427) -- the SDF network evaluated near the iso-surface only.
// (The definitions K29 shares -- dimensions, limits, the deciding brick, the ACTIVE and the leak rule -- are lattice.h's.)
// res points per axis, bricks of `brick` cells; C = ceil((res - 1) / brick) + 1 coarse points per axis, coarse index i = fine index
// min(i * brick, res - 1); (C - 1)^3 bricks, brick b between the coarse points b and b + 1 of every axis.  Six streaming launches around the
// caller's evaluator (ops.sparse_lattice):
//   coarse_points_k   the coarse lattice points, (n, 3) for the evaluator
//   classify_k        one thread per brick: 8 corners of uc -> one byte (active: a corner non-finite, within margin of t, or the corners disagree)
//   brick_points_k    the points of the listed point bricks, brick^3 each, (n, 3) for the evaluator
//   fill_k            every fine point <- the lowest corner of its brick, four points along z per thread, one 16-byte store
//   scatter_k         u[owned point] = -sdf for the evaluated bricks
//   leaks_k           lattice edges that cross t with an endpoint in an inactive brick -> one int64
// POINT BRICKS: fine index i belongs to point brick i / brick on each axis, P = ceil(res / brick) of them per axis.  P == C - 1 unless
// (res - 1) % brick == 0; then the plane res - 1 is a point brick of its own (P == C), which the caller lists whenever the brick below it
// is active -- so every list entry stands for exactly brick^3 evaluator rows, and a row whose index passes res - 1 is a clamped
// duplicate that the scatter drops.  The brick that DECIDES for fine index i is min(i / brick, C - 2).
// Coordinates are linspace_at's, K11's formula: the points are bit-equal to gens_lattice_points' at the same fine indices.
// All indices are 32-bit (res^3 < 2^31, checked): the per-thread decode is a handful of 32-bit divisions, no 64-bit arithmetic.
// coarse_points_k, classify_k and brick_points_k also serve K29's entry points (gens_brick_coarse_points, gens_brick_active,
// gens_brick_points) under K29's limits, where res^3 may pass 2^31: they index only the coarse grid (C^3), the point-brick grid (P^3) and
// the rows of one call (fewer than 2^31 / 3) in 32 bits and a fine index per AXIS, never a flat fine index, so they are correct under both.
#include "lattice.h"

#define SPARSE_BLOCK 256

__global__ __launch_bounds__(SPARSE_BLOCK) void coarse_points_k(SparseBox b, SparseDims d, uint32_t first, uint32_t count, float* __restrict__ pts) {
    const uint32_t t = blockIdx.x * SPARSE_BLOCK + threadIdx.x;
    if (t >= count) return;
    const uint32_t i = first + t, c = (uint32_t)d.coarse;
    const uint32_t xy = i / c, kz = i - xy * c, ix = xy / c, jy = xy - ix * c;
    const int last = d.res - 1;
    float* p = pts + (size_t)3 * t;
    p[0] = linspace_at(b.lo[0], b.hi[0], d.res, (int)min(ix * (uint32_t)d.brick, (uint32_t)last));
    p[1] = linspace_at(b.lo[1], b.hi[1], d.res, (int)min(jy * (uint32_t)d.brick, (uint32_t)last));
    p[2] = linspace_at(b.lo[2], b.hi[2], d.res, (int)min(kz * (uint32_t)d.brick, (uint32_t)last));
}

__global__ __launch_bounds__(SPARSE_BLOCK) void classify_k(const float* __restrict__ uc, int c, float t, float margin, uint32_t n,
                                                           uint8_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * SPARSE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t nb = (uint32_t)c - 1u;
    const uint32_t xy = i / nb, bz = i - xy * nb, bx = xy / nb, by = xy - bx * nb;
    flags[i] = brick_is_active(uc, (uint32_t)c, bx, by, bz, t, margin) ? 1 : 0;
}

__global__ __launch_bounds__(SPARSE_BLOCK) void brick_points_k(SparseBox bx, SparseDims d, const int64_t* __restrict__ list, uint32_t first, uint32_t rows,
                                                               float* __restrict__ pts) {
    const uint32_t t = blockIdx.x * SPARSE_BLOCK + threadIdx.x;
    if (t >= rows) return;
    int fx = 0, fy = 0, fz = 0;
    (void)brick_row(d, list, first, t, fx, fy, fz);         // (a bad entry: the first lattice point, a row no caller keeps)
    const int last = d.res - 1;
    float* p = pts + (size_t)3 * t;
    p[0] = linspace_at(bx.lo[0], bx.hi[0], d.res, min(fx, last));
    p[1] = linspace_at(bx.lo[1], bx.hi[1], d.res, min(fy, last));
    p[2] = linspace_at(bx.lo[2], bx.hi[2], d.res, min(fz, last));
}

__global__ __launch_bounds__(SPARSE_BLOCK) void scatter_k(const float* __restrict__ sdf, SparseDims d, const int64_t* __restrict__ list, uint32_t first,
                                                          uint32_t rows, float* __restrict__ u) {
    const uint32_t t = blockIdx.x * SPARSE_BLOCK + threadIdx.x;
    if (t >= rows) return;
    int fx, fy, fz;
    if (!brick_row(d, list, first, t, fx, fy, fz)) return;
    if (fx >= d.res || fy >= d.res || fz >= d.res) return;                                // a clamped duplicate: its owner wrote the value
    u[((uint32_t)fx * (uint32_t)d.res + (uint32_t)fy) * (uint32_t)d.res + (uint32_t)fz] = -sdf[t];
}

__global__ __launch_bounds__(SPARSE_BLOCK) void fill_k(const float* __restrict__ uc, SparseDims d, uint32_t n, float* __restrict__ u) {
    const uint32_t q = blockIdx.x * SPARSE_BLOCK + threadIdx.x, i0 = q * 4u;
    if (i0 >= n) return;
    const uint32_t r = (uint32_t)d.res, b = (uint32_t)d.brick, c = (uint32_t)d.coarse, lb = c - 2u;
    const uint32_t xy = i0 / r;
    uint32_t kz = i0 - xy * r, ix = xy / r, jy = xy - ix * r;
    uint32_t row = (deciding_brick(ix, b, lb) * c + deciding_brick(jy, b, lb)) * c;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v[e] = uc[row + deciding_brick(kz, b, lb)];
        if (++kz == r) {                                   // the next lattice row (past the last point: never stored)
            kz = 0;
            if (++jy == r) { jy = 0; ++ix; }
            row = (deciding_brick(min(ix, r - 1u), b, lb) * c + deciding_brick(jy, b, lb)) * c;
        }
    }
    if (i0 + 4u <= n) {
        *reinterpret_cast<float4*>(u + i0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (uint32_t e = 0; i0 + e < n; ++e) u[i0 + e] = v[e];
    }
}

__global__ __launch_bounds__(SPARSE_BLOCK) void leaks_k(const float* __restrict__ u, SparseDims d, const uint8_t* __restrict__ flags, float t, uint32_t n,
                                                        unsigned long long* __restrict__ leaks) {
    const uint32_t i = blockIdx.x * SPARSE_BLOCK + threadIdx.x;
    uint32_t mine = 0;
    if (i < n) {
        const uint32_t r = (uint32_t)d.res;
        const uint32_t xy = i / r, kz = i - xy * r, ix = xy / r, jy = xy - ix * r;
        const bool below = u[i] < t;
        const uint32_t step[3] = {r * r, r, 1u}, at[3] = {ix, jy, kz};
        uint32_t m = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a)
            if (at[a] + 1u < r && (u[i + step[a]] < t) != below) m |= 1u << a;
        if (m) mine = leaking_edges(flags, d, ix, jy, kz, m);       // crossing edges are rare: the flags are read for those only
    }
    // one atomic per wave that found something: a thread counts 0 to 3 edges: one ballot per bit of that
    const unsigned long long b0 = __ballot(mine & 1u), b1 = __ballot(mine & 2u);
    if ((threadIdx.x & 63) == 0 && (b0 | b1)) atomicAdd(leaks, (unsigned long long)(__popcll(b0) + 2 * __popcll(b1)));
}

// The launchers of the three kernels both families share: `who` is the entry point, `limits` its set of limits.
static int launch_coarse_points(const char* who, LatticeLimits limits, const float* bmin3_host, const float* bmax3_host, int res, int brick, int64_t first,
                                int64_t count, float* pts, void* stream) {
    if (int e = lattice_check(who, res, brick, limits)) return e;
    SparseBox b;
    if (int e = sparse_box(who, bmin3_host, bmax3_host, b)) return e;
    const SparseDims d = sparse_dims(res, brick);
    const int64_t n = (int64_t)d.coarse * d.coarse * d.coarse;
    GENS_CHECK_ARG(first >= 0 && count >= 0 && first <= n && count <= n - first, GENS_EINVAL, "%s: range [%lld, %lld + %lld) beyond the %d^3 coarse points",
                   who, (long long)first, (long long)first, (long long)count, d.coarse);
    GENS_CHECK_ARG(limits == LATTICE_K28 || count < ((int64_t)1 << 31) / 3, GENS_ELIMIT, "%s: %lld points: fewer than 2^31 / 3 per call", who,
                   (long long)count);
    if (count == 0) return 0;
    GENS_CHECK_ARG(pts, GENS_EINVAL, "%s: null pointer (pts)", who);
    coarse_points_k<<<gens_blocks(count, SPARSE_BLOCK), SPARSE_BLOCK, 0, (hipStream_t)stream>>>(b, d, (uint32_t)first, (uint32_t)count, pts);
    return gens_launch_status(who);
}

static int launch_classify(const char* who, LatticeLimits limits, const float* uc, int res, int brick, float t, float margin, uint8_t* flags, void* stream) {
    if (int e = lattice_check(who, res, brick, limits)) return e;
    GENS_CHECK_ARG(uc && flags, GENS_EINVAL, "%s: null pointer", who);
    GENS_CHECK_ARG(margin >= 0.0f, GENS_EINVAL, "%s: margin = %g, must be >= 0 (and no NaN)", who, (double)margin);
    const SparseDims d = sparse_dims(res, brick);
    const int64_t n = (int64_t)(d.coarse - 1) * (d.coarse - 1) * (d.coarse - 1);
    classify_k<<<gens_blocks(n, SPARSE_BLOCK), SPARSE_BLOCK, 0, (hipStream_t)stream>>>(uc, d.coarse, t, margin, (uint32_t)n, flags);
    return gens_launch_status(who);
}

static int launch_brick_points(const char* who, LatticeLimits limits, const float* bmin3_host, const float* bmax3_host, int res, int brick,
                               const int64_t* list, int64_t n_list, int64_t first, int64_t count, float* pts, void* stream) {
    if (int e = lattice_check(who, res, brick, limits)) return e;
    SparseBox b;
    if (int e = sparse_box(who, bmin3_host, bmax3_host, b)) return e;
    if (int e = lattice_range(who, limits, brick, list, n_list, first, count, true)) return e;
    if (count == 0) return 0;
    GENS_CHECK_ARG(pts, GENS_EINVAL, "%s: null pointer (pts)", who);
    const int64_t rows = count * brick * brick * brick;
    brick_points_k<<<gens_blocks(rows, SPARSE_BLOCK), SPARSE_BLOCK, 0, (hipStream_t)stream>>>(b, sparse_dims(res, brick), list, (uint32_t)first, (uint32_t)rows,
                                                                                            pts);
    return gens_launch_status(who);
}

extern "C" int gens_sparse_coarse_points(const float* bmin3_host, const float* bmax3_host, int res, int brick, int64_t first, int64_t count,
                                         float* pts, void* stream) {
    return launch_coarse_points("gens_sparse_coarse_points", LATTICE_K28, bmin3_host, bmax3_host, res, brick, first, count, pts, stream);
}

extern "C" int gens_brick_coarse_points(const float* bmin3_host, const float* bmax3_host, int res, int brick, int64_t first, int64_t count,
                                        float* pts, void* stream) {
    return launch_coarse_points("gens_brick_coarse_points", LATTICE_K29, bmin3_host, bmax3_host, res, brick, first, count, pts, stream);
}

extern "C" int gens_sparse_classify(const float* uc, int res, int brick, float t, float margin, uint8_t* flags, void* stream) {
    return launch_classify("gens_sparse_classify", LATTICE_K28, uc, res, brick, t, margin, flags, stream);
}

extern "C" int gens_brick_active(const float* uc, int res, int brick, float t, float margin, uint8_t* flags, void* stream) {
    return launch_classify("gens_brick_active", LATTICE_K29, uc, res, brick, t, margin, flags, stream);
}

extern "C" int gens_sparse_brick_points(const float* bmin3_host, const float* bmax3_host, int res, int brick, const int64_t* list, int64_t n_list,
                                        int64_t first, int64_t count, float* pts, void* stream) {
    return launch_brick_points("gens_sparse_brick_points", LATTICE_K28, bmin3_host, bmax3_host, res, brick, list, n_list, first, count, pts, stream);
}

extern "C" int gens_brick_points(const float* bmin3_host, const float* bmax3_host, int res, int brick, const int64_t* list, int64_t n_list, int64_t first,
                                 int64_t count, float* pts, void* stream) {
    return launch_brick_points("gens_brick_points", LATTICE_K29, bmin3_host, bmax3_host, res, brick, list, n_list, first, count, pts, stream);
}

extern "C" int gens_sparse_fill(const float* uc, int res, int brick, float* u, void* stream) {
    const char* who = "gens_sparse_fill";
    if (int e = lattice_check(who, res, brick, LATTICE_K28)) return e;
    GENS_CHECK_ARG(uc && u, GENS_EINVAL, "%s: null pointer", who);
    GENS_CHECK_ARG(((uintptr_t)u & 15) == 0 && ((uintptr_t)uc & 3) == 0, GENS_EINVAL, "%s: misaligned pointer (u: 16 bytes; uc: 4 bytes)", who);
    const SparseDims d = sparse_dims(res, brick);
    const int64_t n = (int64_t)res * res * res;
    fill_k<<<gens_blocks((n + 3) / 4, SPARSE_BLOCK), SPARSE_BLOCK, 0, (hipStream_t)stream>>>(uc, d, (uint32_t)n, u);
    return gens_launch_status(who);
}

extern "C" int gens_sparse_scatter(const float* sdf, int res, int brick, const int64_t* list, int64_t n_list, int64_t first, int64_t count, float* u,
                                   void* stream) {
    const char* who = "gens_sparse_scatter";
    if (int e = lattice_check(who, res, brick, LATTICE_K28)) return e;
    if (int e = lattice_range(who, LATTICE_K28, brick, list, n_list, first, count, true)) return e;
    if (count == 0) return 0;
    GENS_CHECK_ARG(sdf && u, GENS_EINVAL, "%s: null pointer", who);
    const int64_t rows = count * brick * brick * brick;
    scatter_k<<<gens_blocks(rows, SPARSE_BLOCK), SPARSE_BLOCK, 0, (hipStream_t)stream>>>(sdf, sparse_dims(res, brick), list, (uint32_t)first, (uint32_t)rows, u);
    return gens_launch_status(who);
}

extern "C" int gens_sparse_leaks(const float* u, int res, int brick, const uint8_t* flags, float t, int64_t* leaks, void* stream) {
    const char* who = "gens_sparse_leaks";
    if (int e = lattice_check(who, res, brick, LATTICE_K28)) return e;
    GENS_CHECK_ARG(u && flags && leaks, GENS_EINVAL, "%s: null pointer", who);
    GENS_CHECK_ARG(((uintptr_t)leaks & 7) == 0 && ((uintptr_t)u & 3) == 0, GENS_EINVAL, "%s: misaligned pointer (u: 4 bytes; leaks: 8 bytes)", who);
    const SparseDims d = sparse_dims(res, brick);
    const int64_t n = (int64_t)res * res * res;
    hipStream_t s = (hipStream_t)stream;
    if (hipError_t e = hipMemsetAsync(leaks, 0, sizeof(int64_t), s)) {
        (void)hipGetLastError();
        gens_set_error("%s: clearing the count: %s", who, hipGetErrorString(e));
        return (int)e;
    }
    leaks_k<<<gens_blocks(n, SPARSE_BLOCK), SPARSE_BLOCK, 0, s>>>(u, d, flags, t, (uint32_t)n, (unsigned long long*)leaks);
    return gens_launch_status(who);
}
