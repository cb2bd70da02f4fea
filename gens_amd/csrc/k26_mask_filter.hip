// K26: GenS.filter_volume (gens.py:87-122) -- the mask pyramid restricted to a one-voxel dilation of the band |sdf| < thresh inside the unit
// sphere.  Two launches for all levels (gens_filter_masks; gens_filter_band and gens_filter_levels run one each, for a caller that edits the
// band in between: K27's largest component):
//   filter_band_k    one thread per level-0 voxel: the band decision, left as BITS (a wave's ballot = two words along z, gens_pack_mask_bits'
//                    format) -- the 256^3 lattice becomes 2 MB that the second launch reads from L2 -- and the band count.
//   filter_levels_k  one thread per voxel of EVERY level: the 3 x 3 x 3 maximum around the level-0 voxel (x << l, y << l, z << l) from nine
//                    three-bit windows of those words, the float product with the input mask, the product's bits, the dilated count.
// Algorithmic bytes: u once, every mask once in and once out, the bit words.  The reference's chain (threshold, sphere, max_pool3d, permute,
// nearest halvings, products) makes about ten passes over the level-0 lattice.
#include "common.h"

#define FILTER_BLOCK 256

__global__ __launch_bounds__(FILTER_BLOCK) void filter_band_k(const float* __restrict__ u, float thresh, int d, int n, uint32_t* __restrict__ band,
                                                              unsigned long long* __restrict__ counts) {
    const int i = (int)(blockIdx.x * FILTER_BLOCK + threadIdx.x);
    bool in_band = false;
    if (i < n) {
        const int kz = i % d, jy = (i / d) % d, ix = i / (d * d);
        const float x = linspace_at(-1.0f, 1.0f, d, ix), y = linspace_at(-1.0f, 1.0f, d, jy), z = linspace_at(-1.0f, 1.0f, d, kz);
        const float norm = sqrtf(x * x + y * y + z * z);          // (-ffp-contract=off: three products, two sums, one correctly rounded root)
        in_band = (fabsf(u[i]) < thresh) && (norm < 1.0f);        // a NaN compares false
    }
    const unsigned long long b = __ballot(in_band);
    const int lane = threadIdx.x & 63;
    if (lane == 0 && i < n) {
        band[i >> 5] = (uint32_t)b;
        if (b) atomicAdd(counts, (unsigned long long)__popcll(b));
    }
    if (lane == 32 && i < n) band[i >> 5] = (uint32_t)(b >> 32);
}

struct FilterLevels {
    const float* in[GENS_MAX_LEVELS];
    float* out[GENS_MAX_LEVELS];
    uint32_t* bits[GENS_MAX_LEVELS];
    int d[GENS_MAX_LEVELS];
    unsigned first_block[GENS_MAX_LEVELS + 1];       // level l owns blocks first_block[l] .. first_block[l + 1] - 1 (its voxels start on a wave)
    int n;
};

__global__ __launch_bounds__(FILTER_BLOCK) void filter_levels_k(FilterLevels lv, const uint32_t* __restrict__ band,
                                                                unsigned long long* __restrict__ counts) {
    int l = 0;
    while (l + 1 < lv.n && blockIdx.x >= lv.first_block[l + 1]) ++l;
    const int d = lv.d[l], d0 = lv.d[0], n = d * d * d;
    const int i = (int)((blockIdx.x - lv.first_block[l]) * FILTER_BLOCK + threadIdx.x);
    bool dil = false, set = false;
    if (i < n) {
        const int cz = (i % d) << l, cy = ((i / d) % d) << l, cx = (i / (d * d)) << l;
        const int z_lo = max(cz - 1, 0), nb = min(cz + 1, d0 - 1) - z_lo + 1;        // the row's window: bits z_lo .. z_lo + nb - 1, nb = 2 or 3 (1 when d0 == 1)
        uint32_t any = 0;
        for (int ax = max(cx - 1, 0); ax <= min(cx + 1, d0 - 1); ++ax)
            for (int ay = max(cy - 1, 0); ay <= min(cy + 1, d0 - 1); ++ay) {
                const uint32_t j = (uint32_t)((ax * d0 + ay) * d0 + z_lo);
                const uint32_t w = j >> 5, sh = j & 31u;
                uint64_t win = band[w];
                if (sh + (uint32_t)nb > 32u) win |= (uint64_t)band[w + 1] << 32;       // (bit j + nb - 1 exists, so does its word)
                any |= (uint32_t)(win >> sh);
            }
        dil = (any & ((1u << nb) - 1u)) != 0u;
        const float v = lv.in[l][i] * (dil ? 1.0f : 0.0f);
        lv.out[l][i] = v;
        set = v > 0.0f;
    }
    const unsigned long long b = __ballot(set);
    const int lane = threadIdx.x & 63;
    if (lane == 0 && i < n) lv.bits[l][i >> 5] = (uint32_t)b;
    if (lane == 32 && i < n) lv.bits[l][i >> 5] = (uint32_t)(b >> 32);
    if (l == 0) {
        const unsigned long long c = __ballot(dil);
        if (lane == 0 && c) atomicAdd(counts + 1, (unsigned long long)__popcll(c));
    }
}

// The argument checks and the level table of the second launch; -> 0 or the error code.
static int filter_levels_table(const char* who, const float* const* masks_in, float* const* masks_out, uint32_t* const* bits_out, const int* dims,
                               int n_levels, FilterLevels& lv, unsigned& blocks) {
    GENS_CHECK_ARG(n_levels >= 1, GENS_EINVAL, "%s: n_levels = %d", who, n_levels);
    GENS_CHECK_ARG(n_levels <= GENS_MAX_LEVELS, GENS_ELIMIT, "%s: %d levels, at most GENS_MAX_LEVELS = %d", who, n_levels, GENS_MAX_LEVELS);
    GENS_CHECK_ARG(masks_in && masks_out && bits_out && dims, GENS_EINVAL, "%s: null pointer", who);
    const int d0 = dims[0];
    GENS_CHECK_ARG(d0 >= 1 && d0 <= 1024, GENS_EINVAL, "%s: dims[0] = %d, 1 to 1024 (32-bit voxel indices)", who, d0);
    GENS_CHECK_ARG(d0 % (1 << (n_levels - 1)) == 0, GENS_EINVAL, "%s: dims[0] = %d is no multiple of 2^(n_levels - 1) = %d", who, d0,
                   1 << (n_levels - 1));
    lv.n = n_levels;
    blocks = 0;
    for (int l = 0; l < n_levels; ++l) {
        GENS_CHECK_ARG(dims[l] == d0 >> l, GENS_EINVAL, "%s: dims[%d] = %d, expected dims[0] >> %d = %d", who, l, dims[l], l, d0 >> l);
        GENS_CHECK_ARG(masks_in[l] && masks_out[l] && bits_out[l], GENS_EINVAL, "%s: null pointer at level %d", who, l);
        GENS_CHECK_ARG(((uintptr_t)masks_in[l] & 3) == 0 && ((uintptr_t)masks_out[l] & 3) == 0 && ((uintptr_t)bits_out[l] & 3) == 0, GENS_EINVAL,
                       "%s: misaligned pointer at level %d", who, l);
        lv.in[l] = masks_in[l];
        lv.out[l] = masks_out[l];
        lv.bits[l] = bits_out[l];
        lv.d[l] = dims[l];
        lv.first_block[l] = blocks;
        blocks += gens_blocks((int64_t)dims[l] * dims[l] * dims[l], FILTER_BLOCK);
    }
    lv.first_block[n_levels] = blocks;
    return 0;
}

static int filter_clear(const char* who, int64_t* counts, int n, hipStream_t s) {
    if (hipError_t e = hipMemsetAsync(counts, 0, n * sizeof(int64_t), s)) {
        (void)hipGetLastError();
        gens_set_error("%s: clearing the counts: %s", who, hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}

extern "C" int gens_filter_masks(const float* u, float thresh, const float* const* masks_in, float* const* masks_out, uint32_t* const* bits_out,
                                 const int* dims, int n_levels, uint32_t* band_words, int64_t* counts, void* stream) {
    const char* who = "gens_filter_masks";
    FilterLevels lv;
    unsigned blocks;
    if (int e = filter_levels_table(who, masks_in, masks_out, bits_out, dims, n_levels, lv, blocks)) return e;
    GENS_CHECK_ARG(u && band_words && counts, GENS_EINVAL, "%s: null pointer", who);
    GENS_CHECK_ARG(((uintptr_t)u & 3) == 0 && ((uintptr_t)band_words & 3) == 0 && ((uintptr_t)counts & 7) == 0, GENS_EINVAL,
                   "%s: misaligned pointer (u, band_words: 4 bytes; counts: 8 bytes)", who);
    const int d0 = dims[0], n0 = d0 * d0 * d0;
    hipStream_t s = (hipStream_t)stream;
    if (int e = filter_clear(who, counts, 2, s)) return e;
    filter_band_k<<<gens_blocks(n0, FILTER_BLOCK), FILTER_BLOCK, 0, s>>>(u, thresh, d0, n0, band_words, (unsigned long long*)counts);
    if (int e = gens_launch_status("gens_filter_masks (band)")) return e;
    filter_levels_k<<<blocks, FILTER_BLOCK, 0, s>>>(lv, band_words, (unsigned long long*)counts);
    return gens_launch_status(who);
}

extern "C" int gens_filter_band(const float* u, float thresh, int d0, uint32_t* band_words, int64_t* counts, void* stream) {
    const char* who = "gens_filter_band";
    GENS_CHECK_ARG(u && band_words && counts, GENS_EINVAL, "%s: null pointer", who);
    GENS_CHECK_ARG(d0 >= 1 && d0 <= 1024, GENS_EINVAL, "%s: d0 = %d, 1 to 1024 (32-bit voxel indices)", who, d0);
    GENS_CHECK_ARG(((uintptr_t)u & 3) == 0 && ((uintptr_t)band_words & 3) == 0 && ((uintptr_t)counts & 7) == 0, GENS_EINVAL,
                   "%s: misaligned pointer (u, band_words: 4 bytes; counts: 8 bytes)", who);
    const int n0 = d0 * d0 * d0;
    hipStream_t s = (hipStream_t)stream;
    if (int e = filter_clear(who, counts, 1, s)) return e;
    filter_band_k<<<gens_blocks(n0, FILTER_BLOCK), FILTER_BLOCK, 0, s>>>(u, thresh, d0, n0, band_words, (unsigned long long*)counts);
    return gens_launch_status(who);
}

extern "C" int gens_filter_levels(const float* const* masks_in, float* const* masks_out, uint32_t* const* bits_out, const int* dims, int n_levels,
                                  const uint32_t* band_words, int64_t* counts, void* stream) {
    const char* who = "gens_filter_levels";
    FilterLevels lv;
    unsigned blocks;
    if (int e = filter_levels_table(who, masks_in, masks_out, bits_out, dims, n_levels, lv, blocks)) return e;
    GENS_CHECK_ARG(band_words && counts, GENS_EINVAL, "%s: null pointer", who);
    GENS_CHECK_ARG(((uintptr_t)band_words & 3) == 0 && ((uintptr_t)counts & 7) == 0, GENS_EINVAL,
                   "%s: misaligned pointer (band_words: 4 bytes; counts: 8 bytes)", who);
    hipStream_t s = (hipStream_t)stream;
    if (int e = filter_clear(who, counts + 1, 1, s)) return e;
    filter_levels_k<<<blocks, FILTER_BLOCK, 0, s>>>(lv, band_words, (unsigned long long*)counts);
    return gens_launch_status(who);
}
