// K30: per-vertex attributes of an extracted mesh (ImplicitSurface.vertex_attributes): the two streaming steps around the network launches.
//
//   points:  the lattice-index vertices K12 / K29 leave on the device (float64) -> points in the model's frame (float32), the float32
//            rounding of exactly the float64 vertices extract_geometry returns: v / (R - 1.0) * span + lo per component in float64, in that
//            order, un-fused, rounded once.  One thread per component: consecutive lanes read and write consecutive words.
//   pack:    what gens_sdf_grad* and gens_blend_views* leave for the same points -> a unit shading normal (float32), an 8-bit colour in
//            validate's img_fine convention and a `seen` flag.  One thread per vertex; the rows are 12, 3 and S bytes long, so a wave's
//            accesses stay inside the contiguous span of its 64 rows.
//
// No arithmetic here may contract: the definitions are IEEE double operations with one rounding each (the file is compiled with
// -ffp-contract=off like the rest of the library; the pragma keeps that true whatever the flags).
#include <math.h>

#include "common.h"
#include "pack_rules.h"

#pragma clang fp contract(off)

struct Vec3d {
    double x, y, z;
};

__global__ __launch_bounds__(256) void vertex_points_k(const double* __restrict__ v, int64_t n3, double denom, Vec3d span, Vec3d lo, float* __restrict__ pts) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n3) return;
    const int a = (int)(e % 3);
    const double s = a == 0 ? span.x : a == 1 ? span.y : span.z;
    const double l = a == 0 ? lo.x : a == 1 ? lo.y : lo.z;
    pts[e] = (float)(v[e] / denom * s + l);
}

// grad / color: either may be null (the outputs that depend on it are then not touched).
__global__ __launch_bounds__(256) void vertex_pack_k(const float* __restrict__ grad, const float* __restrict__ color, const uint8_t* __restrict__ vis, int n_src,
                                                     int64_t n, float* __restrict__ normals, uint8_t* __restrict__ colors, uint8_t* __restrict__ seen) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (grad) {
        float nx, ny, nz;
        gens_unit_normal(grad[3 * i], grad[3 * i + 1], grad[3 * i + 2], nx, ny, nz);
        normals[3 * i] = nx;
        normals[3 * i + 1] = ny;
        normals[3 * i + 2] = nz;
    }
    if (color) {
        for (int a = 0; a < 3; ++a) colors[3 * i + a] = gens_color8(color[3 * i + a]);
        seen[i] = gens_any_flag(vis + i * n_src, n_src);
    }
}

// ------------------------------------------------------------------------------------------------ entry points
extern "C" int gens_vertex_points(const double* vertices, int64_t n, int resolution, double span_x, double span_y, double span_z, double lo_x,
                                  double lo_y, double lo_z, float* points, void* stream) {
    GENS_CHECK_ARG(n >= 0 && resolution >= 2, GENS_EINVAL, "gens_vertex_points: %lld vertices at resolution %d (n >= 0, resolution >= 2)", (long long)n,
                   resolution);
    GENS_CHECK_ARG(n < ((int64_t)1 << 31), GENS_ELIMIT, "gens_vertex_points: %lld vertices (below 2^31)", (long long)n);
    if (n == 0) return 0;
    GENS_CHECK_ARG(vertices && points, GENS_EINVAL, "gens_vertex_points: null pointer");
    const Vec3d span = {span_x, span_y, span_z}, lo = {lo_x, lo_y, lo_z};
    vertex_points_k<<<gens_blocks(3 * n, 256), 256, 0, (hipStream_t)stream>>>(vertices, 3 * n, resolution - 1.0, span, lo, points);
    return gens_launch_status("gens_vertex_points");
}

extern "C" int gens_vertex_pack(const float* grad, const float* color, const uint8_t* vis, int n_src, int64_t n, float* normals, uint8_t* colors,
                                uint8_t* seen, void* stream) {
    GENS_CHECK_ARG(n >= 0, GENS_EINVAL, "gens_vertex_pack: %lld vertices", (long long)n);
    GENS_CHECK_ARG(n < ((int64_t)1 << 31), GENS_ELIMIT, "gens_vertex_pack: %lld vertices (below 2^31)", (long long)n);
    if (n == 0) return 0;
    GENS_CHECK_ARG(grad || color, GENS_EINVAL, "gens_vertex_pack: null pointer (neither a gradient nor a colour)");
    GENS_CHECK_ARG(!grad || normals, GENS_EINVAL, "gens_vertex_pack: null pointer (a gradient without normals to write)");
    GENS_CHECK_ARG(!color || (vis && colors && seen), GENS_EINVAL, "gens_vertex_pack: null pointer (a colour needs the flags, colours and seen)");
    GENS_CHECK_ARG(!color || (n_src >= 1 && n_src <= 255), GENS_EINVAL, "gens_vertex_pack: %d source views (1 to 255)", n_src);
    vertex_pack_k<<<gens_blocks(n, 256), 256, 0, (hipStream_t)stream>>>(grad, color, vis, n_src, n, normals, colors, seen);
    return gens_launch_status("gens_vertex_pack");
}
