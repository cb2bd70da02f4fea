// The per-point pack rules K30 (gens_vertex_pack), K31 (gens_surface_pack), K34 (gens_texture_pack) and K35 (gens_mesh_shade) share: one
// definition, the same bits in all of them.
#pragma once
#include <math.h>
#include <stdint.h>

#pragma clang fp contract(off)

// g / sqrt((gx^2 + gy^2) + gz^2) in float64, rounded once per component; (0, 0, 0) where a component is not finite or the norm is 0.
// (float32 squares are exact in double and cannot overflow it, so no float32 square root or rescaling enters the result)
__device__ __forceinline__ void gens_unit_normal64(double gx, double gy, double gz, float& nx, float& ny, float& nz) {
    const double norm = sqrt((gx * gx + gy * gy) + gz * gz);
    nx = ny = nz = 0.f;
    if (isfinite(gx) && isfinite(gy) && isfinite(gz) && norm > 0.0) {
        nx = (float)(gx / norm);
        ny = (float)(gy / norm);
        nz = (float)(gz / norm);
    }
}
__device__ __forceinline__ void gens_unit_normal(float fx, float fy, float fz, float& nx, float& ny, float& nz) {
    gens_unit_normal64((double)fx, (double)fy, (double)fz, nx, ny, nz);
}

// rot @ v per component as validate forms it in float32: (v0 * rot[k][0] + v1 * rot[k][1]) + v2 * rot[k][2]
__device__ __forceinline__ float gens_rot_row(const float* __restrict__ rot, int k, float v0, float v1, float v2) {
    return (v0 * rot[3 * k] + v1 * rot[3 * k + 1]) + v2 * rot[3 * k + 2];
}

// The depth of a hit at parameter t of the ray d: t (rot d)_z (the reference's z_val * cos, implicit_surface.py:298).
__device__ __forceinline__ float gens_pack_depth(const float* __restrict__ rot, float t, float dx, float dy, float dz) {
    return t * gens_rot_row(rot, 2, dx, dy, dz);
}

// Component k of the normal image of a unit normal: min(max((rot n)_k 128 + 128, 0), 255).
__device__ __forceinline__ float gens_normal_img(const float* __restrict__ rot, int k, float nx, float ny, float nz) {
    return fminf(fmaxf(gens_rot_row(rot, k, nx, ny, nz) * 128.f + 128.f, 0.f), 255.f);
}

// validate's img_fine convention (implicit_surface.py:455): trunc(min(max(c * 256, 0), 255)); 0 for a component that is not finite.
__device__ __forceinline__ uint8_t gens_color8(float c) {
    uint8_t q = 0;
    if (isfinite(c)) q = (uint8_t)(int)fminf(fmaxf(c * 256.f, 0.f), 255.f);       // (c * 256 is exact or overflows to an infinity the clamp takes)
    return q;
}

// 1 if any of the n_src in-frustum flags of a row is set.
__device__ __forceinline__ uint8_t gens_any_flag(const uint8_t* __restrict__ row, int n_src) {
    unsigned any = 0;
    for (int s = 0; s < n_src; ++s) any |= row[s];
    return any ? 1 : 0;
}
