// The lattice and marching-cubes family: K12 (k12_mcubes.hip), K28 (k28_sparse_lattice.hip, whose header comment defines the terms of the
// two-level lattice) and K29 (k29_brick_mcubes.hip).  K29 promises K12's mesh of K28's lattice, vertex for vertex, so every rule the three
// share is written here once: the lattice's dimensions and limits, the deciding brick, the ACTIVE rule, the leak rule, and marching cubes'
// per-point decisions, vertex and vertex id.
#pragma once
#include "common.h"

struct SparseBox { float lo[3], hi[3]; };

struct SparseDims {
    int res, brick, coarse, pbricks;      // R, B, C, P
};

static inline SparseDims sparse_dims(int res, int brick) {
    SparseDims d;
    d.res = res;
    d.brick = brick;
    d.coarse = (int)(((int64_t)res + brick - 2) / brick) + 1;
    d.pbricks = (int)(((int64_t)res + brick - 1) / brick);
    return d;
}

static int sparse_box(const char* who, const float* bmin3_host, const float* bmax3_host, SparseBox& b) {
    GENS_CHECK_ARG(bmin3_host && bmax3_host, GENS_EINVAL, "%s: null pointer (bounds)", who);
    for (int a = 0; a < 3; ++a) { b.lo[a] = bmin3_host[a]; b.hi[a] = bmax3_host[a]; }
    return 0;
}

// The two sets of limits the entry points come in: K28's (gens_sparse_*: flat FINE indices are 32-bit) and K29's (gens_brick_*: only the
// coarse and the point-brick grids are indexed in 32 bits, and a brick's points are a workgroup's threads).
enum LatticeLimits { LATTICE_K28, LATTICE_K29 };
#define BRICK_MAX 8

// The checks every entry point shares; -> 0 or the error code.  All in 64 bits: res and brick are whatever the caller passed.
static int lattice_check(const char* who, int res, int brick, LatticeLimits limits) {
    const int64_t lim = (int64_t)1 << 31;
    GENS_CHECK_ARG(res >= 2, GENS_EINVAL, "%s: res = %d, at least 2 points per axis", who, res);
    if (limits == LATTICE_K28) {
        GENS_CHECK_ARG(brick >= 1, GENS_EINVAL, "%s: brick = %d, at least one cell", who, brick);
        GENS_CHECK_ARG((int64_t)res * res * res < lim, GENS_ELIMIT, "%s: res = %d, res^3 must stay below 2^31 (32-bit point indices)", who, res);
        return 0;
    }
    GENS_CHECK_ARG(brick >= 2 && brick <= BRICK_MAX, GENS_EINVAL, "%s: brick = %d, 2 to %d cells", who, brick, BRICK_MAX);
    const SparseDims d = sparse_dims(res, brick);
    GENS_CHECK_ARG((int64_t)d.coarse * d.coarse * d.coarse < lim && (int64_t)d.pbricks * d.pbricks * d.pbricks < lim, GENS_ELIMIT,
                   "%s: res = %d, brick = %d: C^3 = %d^3 coarse points and P^3 = %d^3 point bricks must stay below 2^31", who, res, brick, d.coarse,
                   d.pbricks);
    return 0;
}

// The list range of the per-brick entry points -> 0 or the error code.  rows: the range is expanded to brick^3 rows of 3 floats per entry.
static int lattice_range(const char* who, LatticeLimits limits, int brick, const int64_t* list, int64_t n_list, int64_t first, int64_t count, bool rows) {
    GENS_CHECK_ARG(n_list >= 0 && first >= 0 && count >= 0 && first <= n_list && count <= n_list - first, GENS_EINVAL,
                   "%s: range [%lld, %lld + %lld) beyond the list of %lld bricks", who, (long long)first, (long long)first, (long long)count,
                   (long long)n_list);
    const int64_t lim = (int64_t)1 << 31;
    if (limits == LATTICE_K28) {
        GENS_CHECK_ARG(brick <= 1024 && count < lim, GENS_ELIMIT, "%s: brick = %d (at most 1024), %lld bricks (fewer than 2^31)", who, brick,
                       (long long)count);
        GENS_CHECK_ARG(first < lim && count * brick * brick * brick < lim / 3, GENS_ELIMIT,
                       "%s: %lld bricks of %d^3 points: fewer than 2^31 / 3 rows per call", who, (long long)count, brick);
    } else {
        GENS_CHECK_ARG(first < lim && count < lim && (!rows || count < lim / 3 / (brick * brick * brick)), GENS_ELIMIT,
                       "%s: %lld bricks: fewer than 2^31 per call, and than 2^31 / 3 rows", who, (long long)count);
    }
    GENS_CHECK_ARG(count == 0 || list, GENS_EINVAL, "%s: null pointer (list)", who);
    return 0;
}

// the deciding brick's coordinate of fine index i
__device__ __forceinline__ uint32_t deciding_brick(uint32_t i, uint32_t brick, uint32_t last_brick) { return min(i / brick, last_brick); }

// Row t of a range of listed point bricks -> its UNCLAMPED fine indices; false if the list entry is no point brick (the row is skipped).
__device__ __forceinline__ bool brick_row(const SparseDims& d, const int64_t* __restrict__ list, uint32_t first, uint32_t t, int& fx, int& fy, int& fz) {
    const uint32_t b = (uint32_t)d.brick, b3 = b * b * b, p = (uint32_t)d.pbricks;
    const uint32_t k = t / b3, l = t - k * b3;
    const int64_t entry = list[first + k];
    if (entry < 0 || entry >= (int64_t)p * p * p) return false;
    const uint32_t e = (uint32_t)entry;
    const uint32_t exy = e / p, ez = e - exy * p, ex = exy / p, ey = exy - ex * p;
    const uint32_t lxy = l / b, lz = l - lxy * b, lx = lxy / b, ly = lxy - lx * b;
    fx = (int)(ex * b + lx);
    fy = (int)(ey * b + ly);
    fz = (int)(ez * b + lz);
    return true;
}

// The ACTIVE rule of brick (bx, by, bz) on the coarse values uc (c^3): a corner non-finite or within margin of t, or the corners disagree.
__device__ __forceinline__ bool brick_is_active(const float* __restrict__ uc, uint32_t c, uint32_t bx, uint32_t by, uint32_t bz, float t, float margin) {
    bool near = false, any_below = false, all_below = true;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float v = uc[((bx + (k >> 2)) * c + by + ((k >> 1) & 1)) * c + bz + (k & 1)];
        near = near || !isfinite(v) || fabsf(v - t) <= margin;
        const bool below = v < t;                     // (a NaN is not below; it made the brick active already)
        any_below = any_below || below;
        all_below = all_below && below;
    }
    return near || (any_below && !all_below);
}

// The LEAK rule at fine point (fx, fy, fz), whose owned edges with bit a of m (!= 0) set cross the threshold: how many of those edges have
// an endpoint decided by a brick whose flag ((C - 1)^3 of them) is clear.
__device__ __forceinline__ uint32_t leaking_edges(const uint8_t* __restrict__ flags, const SparseDims& d, uint32_t fx, uint32_t fy, uint32_t fz, uint32_t m) {
    const uint32_t b = (uint32_t)d.brick, nb = (uint32_t)d.coarse - 1u, lb = nb - 1u;
    const bool own = flags[(deciding_brick(fx, b, lb) * nb + deciding_brick(fy, b, lb)) * nb + deciding_brick(fz, b, lb)] != 0;
    uint32_t leaks = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!(m & (1u << a))) continue;
        const uint32_t qx = fx + (a == 0), qy = fy + (a == 1), qz = fz + (a == 2);
        const bool other = flags[(deciding_brick(qx, b, lb) * nb + deciding_brick(qy, b, lb)) * nb + deciding_brick(qz, b, lb)] != 0;
        if (!own || !other) ++leaks;
    }
    return leaks;
}

// Marching cubes: edge of a cell in Bourke's numbering -> (offset of the lattice point that owns it, axis)
[[maybe_unused]] static __device__ __constant__ int c_edge_owner[12][4] = {{0, 0, 0, 0}, {1, 0, 0, 1}, {0, 1, 0, 0}, {0, 0, 0, 1}, {0, 0, 1, 0}, {1, 0, 1, 1},
                                                                           {0, 1, 1, 0}, {0, 0, 1, 1}, {0, 0, 0, 2}, {1, 0, 0, 2}, {1, 1, 0, 2}, {0, 1, 0, 2}};

// Marching cubes' decisions at one lattice point, from b0 .. b7 = (value < iso) at the corners of its cell in Bourke order and hx, hy, hz =
// the point has a +x, +y, +z neighbour (a corner that does not exist is never looked at: pass anything) -> the mask of its owned edges
// (+x, +y, +z) that cross, and in `cs` the cell's case index, 0 where the point is no cell's origin.  The caller reads tri_count[cs].
__device__ __forceinline__ uint32_t mc_decide(bool b0, bool b1, bool b2, bool b3, bool b4, bool b5, bool b6, bool b7, bool hx, bool hy, bool hz, uint32_t& cs) {
    uint32_t m = 0;
    if (hx && b1 != b0) m |= 1u;
    if (hy && b3 != b0) m |= 2u;
    if (hz && b4 != b0) m |= 4u;
    cs = 0;
    if (hx && hy && hz)
        cs = (b0 ? 1u : 0u) | (b1 ? 2u : 0u) | (b2 ? 4u : 0u) | (b3 ? 8u : 0u) | (b4 ? 16u : 0u) | (b5 ? 32u : 0u) | (b6 ? 64u : 0u) | (b7 ? 128u : 0u);
    return m;
}

// The vertex on the edge from lattice point (i, j, k), value a, to its neighbour along axis ax, value q: linear in float64, index coordinates.
__device__ __forceinline__ void mc_vertex(double* __restrict__ v, double i, double j, double k, int ax, float a, float q, float iso) {
    const double lvl = (double)iso, t = (lvl - (double)a) / ((double)q - (double)a);
    v[0] = i + (ax == 0 ? t : 0.0);
    v[1] = j + (ax == 1 ? t : 0.0);
    v[2] = k + (ax == 2 ? t : 0.0);
}

// The id of the vertex on a cell's edge e: its owner's first vertex + the owner's crossing edges of a lower axis.
template <typename T>
__device__ __forceinline__ T mc_vertex_id(T owner_first, uint32_t owner_vmask, int e) {
    return owner_first + (T)__popc(owner_vmask & ((1u << c_edge_owner[e][3]) - 1u));
}
