// K27: the largest connected component of a bit volume (utils/tools.py:34-50, clean_volume: skimage.measure.label + regionprops + argmax,
// a host function in the reference).  Bits in, bits out (gens_pack_mask_bits' format), one int32 parent per voxel of scratch.  Six launches,
// each one a phase that needs every workgroup of the one before it to have finished -- nothing waits inside a launch:
//   vcc_init_k      parent[i] = first voxel of i's run of set bits along z (a run is connected whatever the connectivity; runs end at row ends).
//   vcc_hook_k      every set voxel links its run to the runs of the 4 (connectivity 3) or 2 (connectivity 1) rows that precede it in C order:
//                   min-index union (gens_union_min: the larger ROOT is hooked under the smaller with a compare-exchange, parents only decrease).
//                   A voxel that continues a run only looks at what its predecessor's window did not cover.
//   vcc_flatten_k   parent[i] = root for every set voxel that is no root; a root's slot becomes ROOT_MARK (negative: told from any index).
//                   Whatever order the hooks landed in, the root is the component's smallest linear index.
//   vcc_count_k     sizes: root slot += members, added per WAVE and per distinct root (ballot on equal roots), and a wave carries the root it
//                   met first across its eight 64-voxel groups -- the largest component is most of the band, one add per voxel would queue there.
//   vcc_winner_k    the number of components, and atomicMax over (size << 32 | ~root): largest size, ties to the smallest root.  Integer
//                   max and sums: the order of arrival does not matter.
//   vcc_keep_k      the winner's voxels as bits, the roots before the winner's (its label number - 1), and the results.
#include "common.h"

#define CC_BLOCK 256
#define CC_GROUPS 8                               // 64-voxel groups per wave in vcc_count_k
#define CC_ROOT_MARK ((int32_t)0x80000000)        // a root's slot after vcc_flatten_k: ROOT_MARK + size once counted (sizes < 2^31: stays negative)
#define CC_HEAD_BYTES 16                          // scratch: the winner key (uint64) and padding, then the parents

__device__ __forceinline__ bool cc_bit(const uint32_t* __restrict__ bits, int32_t i) { return (bits[i >> 5] >> (i & 31)) & 1u; }

// Bits z - 1, z, z + 1 of the row that starts at voxel `base`, as bits 0, 1, 2 (positions outside the row: 0).
__device__ __forceinline__ uint32_t cc_window(const uint32_t* __restrict__ bits, int32_t base, int z, int nz) {
    const int z_lo = max(z - 1, 0), nb = min(z + 1, nz - 1) - z_lo + 1;
    const uint32_t j = (uint32_t)(base + z_lo), w = j >> 5, sh = j & 31u;
    uint64_t win = bits[w];
    if (sh + (uint32_t)nb > 32u) win |= (uint64_t)bits[w + 1] << 32;        // (bit j + nb - 1 is a voxel, so its word exists)
    const uint32_t v = (uint32_t)(win >> sh) & ((1u << nb) - 1u);
    return z == 0 ? v << 1 : v;
}

__global__ __launch_bounds__(CC_BLOCK) void vcc_init_k(const uint32_t* __restrict__ bits, int nz, int64_t n, int32_t* __restrict__ parent) {
    const int64_t t = (int64_t)blockIdx.x * CC_BLOCK + threadIdx.x;
    if (t >= n) return;
    const int32_t i = (int32_t)t;
    if (!cc_bit(bits, i)) return;                                           // (the slots of clear voxels are never read)
    const int32_t row = i - i % nz;
    int32_t s = i;
    for (;;) {                                                              // walk down word by word to the zero bit below i, or the row's start
        const int32_t lo = (s >> 5) << 5;
        const uint32_t sh = (uint32_t)(s & 31);
        const uint32_t zeros = ~bits[s >> 5] & (uint32_t)((2ull << sh) - 1ull);
        if (zeros) {
            s = lo + (32 - __clz(zeros));
            break;
        }
        if (lo <= row) {
            s = row;
            break;
        }
        s = lo - 1;
    }
    parent[i] = max(s, row);
}

template <int CONN>
__global__ __launch_bounds__(CC_BLOCK) void vcc_hook_k(const uint32_t* __restrict__ bits, int ny, int nz, int64_t n, int32_t* parent) {
    const int64_t t = (int64_t)blockIdx.x * CC_BLOCK + threadIdx.x;
    if (t >= n) return;
    const int32_t i = (int32_t)t;
    if (!cc_bit(bits, i)) return;
    const int z = i % nz, y = (i / nz) % ny, x = i / (nz * ny);
    const bool starts = z == 0 || !cc_bit(bits, i - 1);                     // first voxel of its run
    // The runs of an earlier row that touch this voxel.  b set: a, b, c are one run, and if this voxel continues a run its predecessor's
    // window (z - 2 .. z) has linked it already.  Induction along the run: all of a, b, c are linked to it after this voxel.
    auto link_row = [&](int32_t base) {
        const uint32_t w = cc_window(bits, base, z, nz);
        const bool a = w & 1u, b = w & 2u, c = w & 4u;
        if (CONN == 3) {
            if (starts) {
                if (b) gens_union_min(parent, i, base + z);
                else {
                    if (a) gens_union_min(parent, i, base + z - 1);
                    if (c) gens_union_min(parent, i, base + z + 1);
                }
            } else if (c && !b) gens_union_min(parent, i, base + z + 1);
        } else if (b && (starts || !a)) gens_union_min(parent, i, base + z);
    };
    const int32_t row = i - z;
    if (y > 0) link_row(row - nz);
    if (x > 0) {
        const int32_t below = row - ny * nz;
        link_row(below);
        if (CONN == 3) {
            if (y > 0) link_row(below - nz);
            if (y + 1 < ny) link_row(below + nz);
        }
    }
}

__global__ __launch_bounds__(CC_BLOCK) void vcc_flatten_k(const uint32_t* __restrict__ bits, int64_t n, int32_t* parent) {
    const int64_t t = (int64_t)blockIdx.x * CC_BLOCK + threadIdx.x;
    if (t >= n) return;
    const int32_t i = (int32_t)t;
    if (!cc_bit(bits, i)) return;
    // Other threads of this launch rewrite slots while this one walks: a non-root's slot goes from an ancestor to the root, a root's from itself
    // to ROOT_MARK.  Every value a walk can read is an ancestor or the mark, so it ends at the root either way (strictly decreasing indices).
    int32_t x = i, p = parent_load(parent + x);
    while (p != x && p >= 0) {
        x = p;
        p = parent_load(parent + x);
    }
    __hip_atomic_store(parent + i, x == i ? CC_ROOT_MARK : x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(CC_BLOCK) void vcc_count_k(const uint32_t* __restrict__ bits, int64_t n, int32_t* parent) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (CC_BLOCK / 64) + (threadIdx.x >> 6);
    int32_t held = -1, held_n = 0;                                          // wave-uniform: the root this wave carries, and its members so far
    for (int g = 0; g < CC_GROUPS; ++g) {
        const int64_t t = (wave * CC_GROUPS + g) * 64 + lane;
        int32_t r = -1;
        if (t < n && cc_bit(bits, (int32_t)t)) {
            const int32_t p = parent[t];                                    // a non-root's slot is not written in this launch; a root's stays negative
            r = p < 0 ? (int32_t)t : p;
        }
        unsigned long long todo = __ballot(r >= 0);
        if (held >= 0) {
            const unsigned long long same = __ballot(r == held);
            held_n += __popcll(same);
            todo &= ~same;
        }
        while (todo) {                                                      // one add per distinct root of the group
            const int32_t r0 = __builtin_amdgcn_readlane(r, __ffsll((long long)todo) - 1);
            const unsigned long long same = __ballot(r == r0);
            if (held < 0) {
                held = r0;
                held_n = __popcll(same);
            } else if (lane == 0) atomicAdd(parent + r0, __popcll(same));
            todo &= ~same;
        }
    }
    if (held >= 0 && lane == 0) atomicAdd(parent + held, held_n);
}

__global__ __launch_bounds__(CC_BLOCK) void vcc_winner_k(const uint32_t* __restrict__ bits, int64_t n, const int32_t* __restrict__ parent,
                                                        unsigned long long* __restrict__ key, unsigned long long* __restrict__ results) {
    const int64_t t = (int64_t)blockIdx.x * CC_BLOCK + threadIdx.x;
    unsigned long long k = 0;
    if (t < n && cc_bit(bits, (int32_t)t)) {
        const int32_t p = parent[t];
        if (p < 0) k = ((unsigned long long)(uint32_t)(p - CC_ROOT_MARK) << 32) | (uint32_t)(0x7FFFFFFF - (int32_t)t);
    }
    const unsigned long long roots = __ballot(k != 0);
    if (!roots) return;
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(k, off);
        k = o > k ? o : k;
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMax(key, k);
        atomicAdd(results, (unsigned long long)__popcll(roots));
    }
}

__global__ __launch_bounds__(CC_BLOCK) void vcc_keep_k(const uint32_t* __restrict__ bits, int64_t n, const int32_t* __restrict__ parent,
                                                      const unsigned long long* __restrict__ key, uint32_t* __restrict__ out, long long* __restrict__ results) {
    const int64_t t = (int64_t)blockIdx.x * CC_BLOCK + threadIdx.x;
    const unsigned long long k = *key;
    const int32_t win = k ? 0x7FFFFFFF - (int32_t)(uint32_t)k : -1;
    bool keep = false, before = false;
    if (t < n && cc_bit(bits, (int32_t)t)) {
        const int32_t p = parent[t];
        keep = (p < 0 ? (int32_t)t : p) == win;
        before = p < 0 && (int32_t)t < win;
    }
    const unsigned long long b = __ballot(keep), c = __ballot(before);
    const int lane = threadIdx.x & 63;
    if (lane == 0 && t < n) out[t >> 5] = (uint32_t)b;
    if (lane == 32 && t < n) out[t >> 5] = (uint32_t)(b >> 32);
    if (lane == 0 && c) atomicAdd((unsigned long long*)results + 3, (unsigned long long)__popcll(c));
    if (t == 0) {
        results[1] = (long long)(k >> 32);
        results[2] = win;
        if (k) atomicAdd((unsigned long long*)results + 3, 1ull);
    }
}

__global__ __launch_bounds__(CC_BLOCK) void unpack_bits_k(const uint32_t* __restrict__ bits, int64_t n, float* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * CC_BLOCK + threadIdx.x;
    if (t < n) out[t] = ((bits[t >> 5] >> (t & 31)) & 1u) ? 1.0f : 0.0f;
}

extern "C" int64_t gens_components_scratch_bytes(int nx, int ny, int nz) {
    if (nx < 1 || ny < 1 || nz < 1) return 0;
    if ((int64_t)nx * ny >= ((int64_t)1 << 31) || (int64_t)nx * ny * nz >= ((int64_t)1 << 31)) return 0;
    return CC_HEAD_BYTES + 4 * ((int64_t)nx * ny * nz);
}

extern "C" int gens_largest_component(const uint32_t* bits_in, int nx, int ny, int nz, int connectivity, uint32_t* bits_out, void* scratch,
                                      int64_t* results, void* stream) {
    GENS_CHECK_ARG(bits_in && bits_out && scratch && results, GENS_EINVAL, "gens_largest_component: null pointer");
    GENS_CHECK_ARG(nx >= 1 && ny >= 1 && nz >= 1, GENS_EINVAL, "gens_largest_component: extents (%d, %d, %d) must be positive", nx, ny, nz);
    GENS_CHECK_ARG((int64_t)nx * ny < ((int64_t)1 << 31) && (int64_t)nx * ny * nz < ((int64_t)1 << 31), GENS_ELIMIT,
                   "gens_largest_component: (%d, %d, %d) has 2^31 voxels or more (32-bit voxel indices)", nx, ny, nz);
    GENS_CHECK_ARG(connectivity == 1 || connectivity == 3, GENS_EINVAL, "gens_largest_component: connectivity = %d, 1 (6 neighbours) or 3 (26)",
                   connectivity);
    GENS_CHECK_ARG(((uintptr_t)bits_in & 3) == 0 && ((uintptr_t)bits_out & 3) == 0 && ((uintptr_t)scratch & 7) == 0 && ((uintptr_t)results & 7) == 0,
                   GENS_EINVAL, "gens_largest_component: misaligned pointer (bits: 4 bytes; scratch, results: 8 bytes)");
    GENS_CHECK_ARG(bits_in != bits_out, GENS_EINVAL, "gens_largest_component: bits_out must not be bits_in");
    const int64_t n = (int64_t)nx * ny * nz;
    unsigned long long* key = (unsigned long long*)scratch;
    int32_t* parent = (int32_t*)((char*)scratch + CC_HEAD_BYTES);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(results, 0, 4 * sizeof(int64_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(key, 0, CC_HEAD_BYTES, s);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        gens_set_error("gens_largest_component: clearing the results: %s", hipGetErrorString(e));
        return (int)e;
    }
    const unsigned blocks = gens_blocks(n, CC_BLOCK);
    vcc_init_k<<<blocks, CC_BLOCK, 0, s>>>(bits_in, nz, n, parent);
    if (int err = gens_launch_status("gens_largest_component (init)")) return err;
    if (connectivity == 3)
        vcc_hook_k<3><<<blocks, CC_BLOCK, 0, s>>>(bits_in, ny, nz, n, parent);
    else
        vcc_hook_k<1><<<blocks, CC_BLOCK, 0, s>>>(bits_in, ny, nz, n, parent);
    if (int err = gens_launch_status("gens_largest_component (hook)")) return err;
    vcc_flatten_k<<<blocks, CC_BLOCK, 0, s>>>(bits_in, n, parent);
    if (int err = gens_launch_status("gens_largest_component (flatten)")) return err;
    vcc_count_k<<<gens_blocks(n, CC_BLOCK * CC_GROUPS), CC_BLOCK, 0, s>>>(bits_in, n, parent);
    if (int err = gens_launch_status("gens_largest_component (count)")) return err;
    vcc_winner_k<<<blocks, CC_BLOCK, 0, s>>>(bits_in, n, parent, key, (unsigned long long*)results);
    if (int err = gens_launch_status("gens_largest_component (winner)")) return err;
    vcc_keep_k<<<blocks, CC_BLOCK, 0, s>>>(bits_in, n, parent, key, bits_out, (long long*)results);
    return gens_launch_status("gens_largest_component");
}

extern "C" int gens_unpack_mask_bits(const uint32_t* bits, int64_t n, float* mask, void* stream) {
    GENS_CHECK_ARG(bits && mask, GENS_EINVAL, "gens_unpack_mask_bits: null pointer");
    GENS_CHECK_ARG(n >= 1, GENS_EINVAL, "gens_unpack_mask_bits: n = %lld", (long long)n);
    GENS_CHECK_ARG(((uintptr_t)bits & 3) == 0 && ((uintptr_t)mask & 3) == 0, GENS_EINVAL, "gens_unpack_mask_bits: misaligned pointer");
    unpack_bits_k<<<gens_blocks(n, CC_BLOCK), CC_BLOCK, 0, (hipStream_t)stream>>>(bits, n, mask);
    return gens_launch_status("gens_unpack_mask_bits");
}
