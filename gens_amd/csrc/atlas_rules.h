// The atlas layout of K34 (include/gens_hip.h, K34, steps 1 and 2) as K34 (gens_texture_pack / gens_texture_uv) and K35 (gens_mesh_shade)
// share it: one definition of where a triangle's texels are.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#define K34_MIN_TEXELS 3
#define K34_MAX_TEXELS 64

// Local texel (i', j') of triangle f -> its pixel (x, y): tile f >> 1 at column q % cols and row q / cols, half f & 1 turned by a half turn.
__device__ __forceinline__ void k34_pixel(int S, int cols, int64_t f, int ip, int jp, int64_t& x, int64_t& y) {
    const int64_t q = f >> 1;
    const bool turned = (f & 1) != 0;
    const int i = turned ? S - ip : ip, j = turned ? S - 1 - jp : jp;
    x = (q % cols) * (S + 1) + i;
    y = (q / cols) * S + j;
}

// The atlas of n_faces triangles: cols = ceil(sqrt(n_tiles)) in exact integers, rows = ceil(n_tiles / cols).
static inline void k34_layout(int64_t n_faces, int texels, int64_t& cols, int64_t& rows) {
    const int64_t tiles = (n_faces + 1) / 2;
    int64_t c = (int64_t)sqrt((double)tiles);
    while (c * c < tiles) ++c;
    while (c > 0 && (c - 1) * (c - 1) >= tiles) --c;
    cols = c;
    rows = c ? (tiles + c - 1) / c : 0;
}
