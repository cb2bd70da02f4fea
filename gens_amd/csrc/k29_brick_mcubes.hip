// K29: marching cubes on the bricks of the two-level lattice (its terms: k28_sparse_lattice.hip's header comment; its definitions and the
// rules shared with K12 and K28: lattice.h) -- the mesh of ops.marching_cubes(u_s, t), u_s the lattice
// ops.sparse_lattice would build, without u_s: device memory and work follow the surface, and the limit is C^3 < 2^31 on the COARSE
// lattice instead of R^3 < 2^31.  The coarse points, the ACTIVE flags and the points of the listed bricks are K28's kernels under that limit
// (gens_brick_coarse_points, gens_brick_active, gens_brick_points: k28_sparse_lattice.hip); here:
//   brick_emit_flags_k                       a deciding brick EMITS if a brick of X + {0,1}^3 is active: every mixed-sign cell and every
//                                            crossing edge of u_s starts at a point such a brick decides
//   brick_mc_classify_k                      one workgroup per listed point brick: its (B + 1)^3 corner values staged in LDS (an evaluated
//                                            point brick's stored value, else the fill from uc), then K12's decisions per point (mc_decide):
//                                            vmask, case, the in-brick exclusive vertex rank; per brick the vertex, triangle and leak counts
//   brick_mc_emit_k                          vertices (K12's: mc_vertex) at the brick's offset + rank, triangles through the slot map
//                                            of the listed bricks, one int64 sort key per vertex (3 flat(p) + axis) and triangle (flat(cell))
// The listed unit is the POINT brick (B^3 points, fine index e * B + l per axis; an index past R - 1 is no point), so the plane R - 1 of
// (R - 1) % B == 0 is a brick of its own here as in K28.  Per-axis indices and everything counted over the coarse or point-brick grids are
// 32-bit; flat fine-lattice indices (the keys) are 64-bit.
#include "lattice.h"

#define BRICK_POINTS_BLOCK 256
#define BRICK_CORNERS ((BRICK_MAX + 1) * (BRICK_MAX + 1) * (BRICK_MAX + 1))

__global__ __launch_bounds__(BRICK_POINTS_BLOCK) void brick_emit_flags_k(const uint8_t* __restrict__ active, uint32_t nb, uint32_t n, uint8_t* __restrict__ emit) {
    const uint32_t i = blockIdx.x * BRICK_POINTS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t xy = i / nb, bz = i - xy * nb, bx = xy / nb, by = xy - bx * nb;
    bool any = false;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t x = min(bx + (k >> 2), nb - 1u), y = min(by + ((k >> 1) & 1), nb - 1u), z = min(bz + (k & 1), nb - 1u);   // (clipped: a brick seen twice)
        any = any || active[(x * nb + y) * nb + z] != 0;
    }
    emit[i] = any ? 1 : 0;
}

// What the two per-brick kernels read of the two-level lattice.
struct BrickField {
    const float* uc;            // (C^3) u at the coarse points
    const float* store;         // (evaluated point bricks, B^3) u in brick-local C order
    const int32_t* pslot;       // (P^3) a point brick's row of `store`, -1: not evaluated
    const uint8_t* active;      // ((C - 1)^3) K28's flags of the deciding bricks
};

// The listed point brick of this workgroup -> its coordinates; false for an entry outside the P^3 grid (the whole workgroup agrees).
__device__ __forceinline__ bool listed_brick(const SparseDims& d, const int64_t* __restrict__ list, uint32_t& ex, uint32_t& ey, uint32_t& ez) {
    const uint32_t p = (uint32_t)d.pbricks;
    const int64_t entry = list[blockIdx.x];
    if (entry < 0 || entry >= (int64_t)p * p * p) return false;
    const uint32_t e = (uint32_t)entry, exy = e / p;
    ez = e - exy * p;
    ex = exy / p;
    ey = exy - ex * p;
    return true;
}

// u_s at the (B + 1)^3 points from the brick's first point on -> s_u in C order [cx, cy, cz]; 0 where an index passes R - 1 (never compared).
__device__ __forceinline__ void stage_corners(const SparseDims& d, const BrickField& f, uint32_t ex, uint32_t ey, uint32_t ez, float* s_u) {
    const uint32_t b = (uint32_t)d.brick, b1 = b + 1u, n = b1 * b1 * b1, r = (uint32_t)d.res, c = (uint32_t)d.coarse, p = (uint32_t)d.pbricks, lb = c - 2u;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        const uint32_t cxy = i / b1, cz = i - cxy * b1, cx = cxy / b1, cy = cxy - cx * b1;
        const uint32_t fx = ex * b + cx, fy = ey * b + cy, fz = ez * b + cz;
        float v = 0.0f;
        if (fx < r && fy < r && fz < r) {
            const uint32_t qx = ex + (cx == b), qy = ey + (cy == b), qz = ez + (cz == b);          // the point brick that owns it (<= P - 1: f <= R - 1)
            const int32_t slot = f.pslot[(qx * p + qy) * p + qz];
            if (slot >= 0) {
                const uint32_t lx = cx == b ? 0u : cx, ly = cy == b ? 0u : cy, lz = cz == b ? 0u : cz;
                v = f.store[(size_t)slot * (b * b * b) + (lx * b + ly) * b + lz];
            } else {
                v = f.uc[(deciding_brick(fx, b, lb) * c + deciding_brick(fy, b, lb)) * c + deciding_brick(fz, b, lb)];
            }
        }
        s_u[i] = v;
    }
}

// Exclusive scan of v over the workgroup (whole waves; at most 8 of them) and its total.  One __syncthreads inside: every thread calls it.
__device__ __forceinline__ uint32_t block_scan_exclusive(uint32_t v, uint32_t* s_wave, uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(inc, o);
        if (lane >= (uint32_t)o) inc += up;
    }
    if (lane == 63u) s_wave[w] = inc;
    __syncthreads();
    uint32_t base = 0, all = 0;
    for (uint32_t i = 0; i < nw; ++i) {
        const uint32_t s = s_wave[i];
        if (i < w) base += s;
        all += s;
    }
    total = all;
    return base + inc - v;
}

__global__ __launch_bounds__(512) void brick_mc_classify_k(SparseDims d, BrickField f, const int64_t* __restrict__ list, float iso,
                                                           const uint8_t* __restrict__ tri_count, uint8_t* __restrict__ vmask,
                                                           uint8_t* __restrict__ cases, uint16_t* __restrict__ rank, int32_t* __restrict__ counts) {
    __shared__ float s_u[BRICK_CORNERS];
    __shared__ uint32_t s_wave[8];
    __shared__ uint32_t s_leaks;
    const uint32_t b = (uint32_t)d.brick, b1 = b + 1u, b3 = b * b * b, l = threadIdx.x, r = (uint32_t)d.res;
    const size_t at0 = (size_t)blockIdx.x * b3;
    uint32_t ex = 0, ey = 0, ez = 0;
    if (!listed_brick(d, list, ex, ey, ez)) {               // no brick: nothing of it is emitted
        if (l < b3) { vmask[at0 + l] = 0; cases[at0 + l] = 0; rank[at0 + l] = 0; }
        if (l < 3u) counts[(size_t)l * gridDim.x + blockIdx.x] = 0;
        return;
    }
    if (l == 0) s_leaks = 0;
    stage_corners(d, f, ex, ey, ez, s_u);
    __syncthreads();
    uint32_t m = 0, cs = 0, nt = 0, leaks = 0;
    if (l < b3) {
        const uint32_t lxy = l / b, lz = l - lxy * b, lx = lxy / b, ly = lxy - lx * b;
        const uint32_t fx = ex * b + lx, fy = ey * b + ly, fz = ez * b + lz;
        if (fx < r && fy < r && fz < r) {
            const uint32_t at = (lx * b1 + ly) * b1 + lz, sx = b1 * b1, sy = b1;
            const bool hx = fx + 1u < r, hy = fy + 1u < r, hz = fz + 1u < r;
            // corners in Bourke order; one that does not exist is not read
            const bool b0 = s_u[at] < iso, c1 = hx ? s_u[at + sx] < iso : false, c3 = hy ? s_u[at + sy] < iso : false, c4 = hz ? s_u[at + 1u] < iso : false;
            bool c2 = false, c5 = false, c6 = false, c7 = false;
            if (hx && hy && hz) { c2 = s_u[at + sx + sy] < iso; c5 = s_u[at + sx + 1u] < iso; c6 = s_u[at + sx + sy + 1u] < iso; c7 = s_u[at + sy + 1u] < iso; }
            m = mc_decide(b0, c1, c2, c3, c4, c5, c6, c7, hx, hy, hz, cs);
            nt = tri_count[cs];                             // (case 0, no cell included: no triangle)
            if (m) leaks = leaking_edges(f.active, d, fx, fy, fz, m);
        }
        vmask[at0 + l] = (uint8_t)m;
        cases[at0 + l] = (uint8_t)cs;
    }
    if (leaks) atomicAdd(&s_leaks, leaks);
    // vertices (at most 3 B^3 = 1536) in the low half, triangles (at most 5 B^3 = 2560) in the high half: one scan
    uint32_t total = 0;
    const uint32_t before = block_scan_exclusive((uint32_t)__popc(m) | (nt << 16), s_wave, total);
    if (l < b3) rank[at0 + l] = (uint16_t)(before & 0xffffu);
    if (l == 0) {                                           // (after the scan's barrier: every leak has been added)
        const size_t n = gridDim.x;                         // three rows of n_list: each is scanned along its own memory
        counts[blockIdx.x] = (int32_t)(total & 0xffffu);
        counts[n + blockIdx.x] = (int32_t)(total >> 16);
        counts[2 * n + blockIdx.x] = (int32_t)s_leaks;
    }
}

__global__ __launch_bounds__(512) void brick_mc_emit_k(SparseDims d, BrickField f, const int64_t* __restrict__ list, const int32_t* __restrict__ eslot,
                                                       float iso, const int8_t* __restrict__ tri_table, int table_stride,
                                                       const uint8_t* __restrict__ tri_count, const uint8_t* __restrict__ vmask,
                                                       const uint8_t* __restrict__ cases, const uint16_t* __restrict__ rank,
                                                       const int64_t* __restrict__ voff, const int64_t* __restrict__ toff, double* __restrict__ vertices,
                                                       int32_t* __restrict__ triangles, int64_t* __restrict__ vkey, int64_t* __restrict__ tkey) {
    __shared__ float s_u[BRICK_CORNERS];
    __shared__ uint32_t s_wave[8];
    const uint32_t b = (uint32_t)d.brick, b1 = b + 1u, b3 = b * b * b, l = threadIdx.x, r = (uint32_t)d.res, p = (uint32_t)d.pbricks;
    const size_t at0 = (size_t)blockIdx.x * b3;
    uint32_t ex = 0, ey = 0, ez = 0;
    if (!listed_brick(d, list, ex, ey, ez)) return;         // (its counts are zero)
    stage_corners(d, f, ex, ey, ez, s_u);
    const uint32_t m = l < b3 ? vmask[at0 + l] : 0u, cs = l < b3 ? cases[at0 + l] : 0u;
    const uint32_t nt = tri_count[cs];                      // (case 0: no triangle)
    uint32_t total = 0;
    const uint32_t t_before = block_scan_exclusive(nt, s_wave, total);     // (its barrier also publishes s_u)
    if (!m && !nt) return;
    const uint32_t lxy = l / b, lz = l - lxy * b, lx = lxy / b, ly = lxy - lx * b;
    const uint32_t fx = ex * b + lx, fy = ey * b + ly, fz = ez * b + lz;
    const int64_t flat = ((int64_t)fx * r + fy) * r + fz;
    if (m) {
        const uint32_t at = (lx * b1 + ly) * b1 + lz;
        const uint32_t step[3] = {b1 * b1, b1, 1u};
        const float a = s_u[at];
        int64_t o = voff[blockIdx.x] + rank[at0 + l];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            if (!(m & (1u << ax))) continue;
            mc_vertex(vertices + 3 * o, (double)fx, (double)fy, (double)fz, ax, a, s_u[at + step[ax]], iso);
            vkey[o] = 3 * flat + ax;
            ++o;
        }
    }
    if (nt) {
        const int8_t* row = tri_table + (int)cs * table_stride;
        const int64_t t0 = toff[blockIdx.x] + t_before;
        int32_t* out = triangles + 3 * t0;
        for (uint32_t t = 0; t < 3u * nt; ++t) {
            const int e = row[t];
            const uint32_t cx = lx + (uint32_t)c_edge_owner[e][0], cy = ly + (uint32_t)c_edge_owner[e][1], cz = lz + (uint32_t)c_edge_owner[e][2];
            // the owner's point brick (the cell exists, so every index is <= R - 1 and the brick <= P - 1) and its place in it
            const uint32_t qx = ex + (cx == b), qy = ey + (cy == b), qz = ez + (cz == b);
            const int32_t slot = eslot[(qx * p + qy) * p + qz];
            int32_t id = -1;                                // an owner in no listed brick: cannot be; never an index out of range
            if (slot >= 0) {
                const size_t q = (size_t)slot * b3 + ((cx == b ? 0u : cx) * b + (cy == b ? 0u : cy)) * b + (cz == b ? 0u : cz);
                id = (int32_t)mc_vertex_id(voff[slot] + (int64_t)rank[q], vmask[q], e);
            }
            out[t] = id;
        }
        for (uint32_t t = 0; t < nt; ++t) tkey[t0 + t] = flat;
    }
}

extern "C" int gens_brick_emit_flags(const uint8_t* active, int res, int brick, uint8_t* emit, void* stream) {
    const char* who = "gens_brick_emit_flags";
    if (int e = lattice_check(who, res, brick, LATTICE_K29)) return e;
    GENS_CHECK_ARG(active && emit, GENS_EINVAL, "%s: null pointer", who);
    const SparseDims d = sparse_dims(res, brick);
    const int64_t n = (int64_t)(d.coarse - 1) * (d.coarse - 1) * (d.coarse - 1);
    brick_emit_flags_k<<<gens_blocks(n, BRICK_POINTS_BLOCK), BRICK_POINTS_BLOCK, 0, (hipStream_t)stream>>>(active, (uint32_t)d.coarse - 1u, (uint32_t)n, emit);
    return gens_launch_status(who);
}

// whole waves that hold the B^3 points of a brick: one at B <= 4, 512 threads at B = 8
static inline unsigned brick_threads(int brick) { return (unsigned)((brick * brick * brick + 63) / 64 * 64); }

extern "C" int gens_brick_mc_classify(const float* uc, const float* store, const int32_t* pslot, const uint8_t* active, int res, int brick,
                                      const int64_t* list, int64_t n_list, float iso, const uint8_t* tri_count, uint8_t* vmask, uint8_t* cases,
                                      uint16_t* rank, int32_t* counts, void* stream) {
    const char* who = "gens_brick_mc_classify";
    if (int e = lattice_check(who, res, brick, LATTICE_K29)) return e;
    if (int e = lattice_range(who, LATTICE_K29, brick, list, n_list, 0, n_list, false)) return e;
    if (n_list == 0) return 0;
    GENS_CHECK_ARG(uc && store && pslot && active && tri_count && vmask && cases && rank && counts, GENS_EINVAL, "%s: null pointer", who);
    GENS_CHECK_ARG(((uintptr_t)rank & 1) == 0 && ((uintptr_t)counts & 3) == 0 && ((uintptr_t)pslot & 3) == 0, GENS_EINVAL,
                   "%s: misaligned pointer (rank: 2 bytes; counts, pslot: 4 bytes)", who);
    const BrickField f = {uc, store, pslot, active};
    brick_mc_classify_k<<<(unsigned)n_list, brick_threads(brick), 0, (hipStream_t)stream>>>(sparse_dims(res, brick), f, list, iso, tri_count, vmask, cases, rank,
                                                                                          counts);
    return gens_launch_status(who);
}

extern "C" int gens_brick_mc_emit(const float* uc, const float* store, const int32_t* pslot, const int32_t* eslot, int res, int brick,
                                  const int64_t* list, int64_t n_list, float iso, const int8_t* tri_table, int table_stride, const uint8_t* tri_count,
                                  const uint8_t* vmask, const uint8_t* cases, const uint16_t* rank, const int64_t* voff, const int64_t* toff,
                                  double* vertices, int32_t* triangles, int64_t* vkey, int64_t* tkey, void* stream) {
    const char* who = "gens_brick_mc_emit";
    if (int e = lattice_check(who, res, brick, LATTICE_K29)) return e;
    if (int e = lattice_range(who, LATTICE_K29, brick, list, n_list, 0, n_list, false)) return e;
    GENS_CHECK_ARG(table_stride >= 15, GENS_EINVAL, "%s: table stride %d", who, table_stride);
    if (n_list == 0) return 0;
    GENS_CHECK_ARG(uc && store && pslot && eslot && tri_table && tri_count && vmask && cases && rank && voff && toff && vertices && triangles && vkey && tkey,
                   GENS_EINVAL, "%s: null pointer", who);
    GENS_CHECK_ARG(((uintptr_t)rank & 1) == 0 && (((uintptr_t)pslot | (uintptr_t)eslot | (uintptr_t)triangles) & 3) == 0 &&
                       (((uintptr_t)voff | (uintptr_t)toff | (uintptr_t)vertices | (uintptr_t)vkey | (uintptr_t)tkey) & 7) == 0,
                   GENS_EINVAL, "%s: misaligned pointer (rank: 2 bytes; pslot, eslot, triangles: 4 bytes; voff, toff, vertices, vkey, tkey: 8 bytes)", who);
    const BrickField f = {uc, store, pslot, nullptr};
    brick_mc_emit_k<<<(unsigned)n_list, brick_threads(brick), 0, (hipStream_t)stream>>>(sparse_dims(res, brick), f, list, eslot, iso, tri_table, table_stride,
                                                                                      tri_count, vmask, cases, rank, voff, toff, vertices, triangles, vkey, tkey);
    return gens_launch_status(who);
}
