// K34: texture atlases for triangle meshes (ops.texture_points / texture_snap / texture_pack / texture_uv, ImplicitSurface.texture_mesh,
// extract_geometry(texture=)).  The definition is the comment of K34 in include/gens_hip.h; tests/mesh_texture_reference.py restates it in
// numpy and the kernels equal that restatement bit for bit.
//
//   points:  one thread per sample s = f P + k of a chunk [s0, s1) -> the sample's point on the plane of triangle f (float32) and, if asked,
//            the triangle's longest edge.  The P threads of a triangle read the same three indices and 36 bytes of corners (one cache line or
//            two per wave) and write consecutive 12-byte rows.
//   snap:    one thread per sample -> one Newton step of the point towards sdf + threshold = 0, or the point kept.
//   keep:    one thread per sample -> the point, value and gradient of the step's origin back where the step did not lower |g|.
//   pack:    one thread per sample -> the three bytes of its texel and its `seen` flag at the texel's pixel address.  No two samples share a
//            pixel, so the stores are plain byte stores; a wave's samples are runs of a tile's rows, so its stores fall into a few short spans.
//   uv:      one thread per triangle -> its three corner coordinates.
//
// Streaming kernels, 64-bit sample indices, named scalars only (no indexed arrays): no scratch.  All arithmetic of the definition is float64,
// every operation rounded on its own (no contraction), results rounded once to float32.
#include <math.h>

#include "atlas_rules.h"
#include "common.h"
#include "pack_rules.h"

#pragma clang fp contract(off)

// Sample number k of a triangle -> its local texel (i', j'): j' is the outer index, row j' holds S - j' texels and begins at
// j' S - j' (j' - 1) / 2.  The float estimate is corrected in integers, so the result is exact.
__device__ __forceinline__ void k34_local(int S, int k, int& ip, int& jp) {
    const int m = 2 * S + 1;
    int j = (int)(((float)m - sqrtf((float)(m * m - 8 * k))) * 0.5f);
    j = j < 0 ? 0 : j > S - 1 ? S - 1 : j;
    while (j > 0 && j * S - j * (j - 1) / 2 > k) --j;
    while (j < S - 1 && (j + 1) * S - (j + 1) * j / 2 <= k) ++j;
    ip = k - (j * S - j * (j - 1) / 2);
    jp = j;
}

__device__ __forceinline__ double k34_edge2(double ax, double ay, double az, double bx, double by, double bz) {
    const double dx = bx - ax, dy = by - ay, dz = bz - az;
    return (dx * dx + dy * dy) + dz * dz;
}

__global__ __launch_bounds__(256) void texture_points_k(const float* __restrict__ points, int n_vert, const int32_t* __restrict__ triangles, int S,
                                                        int64_t s0, int64_t n, float* __restrict__ out, float* __restrict__ edge) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int64_t P = (int64_t)S * (S + 1) / 2, s = s0 + r, f = s / P;
    int ip, jp;
    k34_local(S, (int)(s - f * P), ip, jp);
    const int32_t i0 = triangles[3 * f], i1 = triangles[3 * f + 1], i2 = triangles[3 * f + 2];
    float px = NAN, py = NAN, pz = NAN, longest = NAN;
    if (i0 >= 0 && i0 < n_vert && i1 >= 0 && i1 < n_vert && i2 >= 0 && i2 < n_vert) {     // (else NaN; nothing is read through the index)
        const float* __restrict__ pa = points + 3 * (int64_t)i0;
        const float* __restrict__ pb = points + 3 * (int64_t)i1;
        const float* __restrict__ pc = points + 3 * (int64_t)i2;
        const double ax = pa[0], ay = pa[1], az = pa[2], bx = pb[0], by = pb[1], bz = pb[2], cx = pc[0], cy = pc[1], cz = pc[2];
        const double den = (double)(S - 2), a = (double)ip / den, b = (double)jp / den;
        px = (float)((ax + a * (bx - ax)) + b * (cx - ax));
        py = (float)((ay + a * (by - ay)) + b * (cy - ay));
        pz = (float)((az + a * (bz - az)) + b * (cz - az));
        if (edge) {                                                 // (e > m is false for a NaN: the rule's own comparisons, not fmax)
            const double e_bc = k34_edge2(bx, by, bz, cx, cy, cz), e_ca = k34_edge2(cx, cy, cz, ax, ay, az);
            double m = k34_edge2(ax, ay, az, bx, by, bz);
            m = e_bc > m ? e_bc : m;
            m = e_ca > m ? e_ca : m;
            longest = (float)sqrt(m);
        }
    }
    out[3 * r] = px, out[3 * r + 1] = py, out[3 * r + 2] = pz;
    if (edge) edge[r] = longest;
}

__global__ __launch_bounds__(256) void texture_snap_k(float* __restrict__ points, const float* __restrict__ value, const float* __restrict__ grad,
                                                      const float* __restrict__ limit, double max_move, double threshold, int64_t n,
                                                      uint8_t* __restrict__ taken) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const double g = (double)value[r] + threshold;
    const double gx = grad[3 * r], gy = grad[3 * r + 1], gz = grad[3 * r + 2];
    const double n2 = (gx * gx + gy * gy) + gz * gz;
    const double mm = limit ? (double)limit[r] : max_move;
    uint8_t took = 0;
    if (isfinite(g) && isfinite(n2) && n2 > 0.0) {                  // (n2 is finite exactly when the three components are)
        const double t = g / n2;
        const double sx = t * gx, sy = t * gy, sz = t * gz;
        const double len2 = (sx * sx + sy * sy) + sz * sz;
        if (len2 <= mm * mm) {                                      // (a NaN limit fails the comparison: the point is kept)
            points[3 * r] = (float)((double)points[3 * r] - sx);
            points[3 * r + 1] = (float)((double)points[3 * r + 1] - sy);
            points[3 * r + 2] = (float)((double)points[3 * r + 2] - sz);
            took = 1;
        }
    }
    taken[r] = took;
}

// The snap's guard: a point whose |g| is larger than at the point it came from (or not a number) goes back there, with that point's value and
// gradient, so that the next round starts from the better point's state.
__global__ __launch_bounds__(256) void texture_keep_k(float* __restrict__ points, float* __restrict__ value, float* __restrict__ grad,
                                                      const float* __restrict__ prev_points, const float* __restrict__ prev_value,
                                                      const float* __restrict__ prev_grad, double threshold, int64_t n, uint8_t* __restrict__ reverted) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const double now = fabs((double)value[r] + threshold), before = fabs((double)prev_value[r] + threshold);
    uint8_t back = 0;
    if (!(now <= before)) {                                         // (a NaN on either side fails the comparison)
        points[3 * r] = prev_points[3 * r], points[3 * r + 1] = prev_points[3 * r + 1], points[3 * r + 2] = prev_points[3 * r + 2];
        grad[3 * r] = prev_grad[3 * r], grad[3 * r + 1] = prev_grad[3 * r + 1], grad[3 * r + 2] = prev_grad[3 * r + 2];
        value[r] = prev_value[r];
        back = 1;
    }
    reverted[r] = back;
}

__global__ __launch_bounds__(256) void texture_pack_k(const float* __restrict__ color, const uint8_t* __restrict__ vis, int n_src, int S, int cols,
                                                      int64_t W, int64_t s0, int64_t n, uint8_t* __restrict__ atlas, uint8_t* __restrict__ seen) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int64_t P = (int64_t)S * (S + 1) / 2, s = s0 + r, f = s / P;
    int ip, jp;
    k34_local(S, (int)(s - f * P), ip, jp);
    int64_t x, y;
    k34_pixel(S, cols, f, ip, jp, x, y);
    const int64_t pix = y * W + x;
    const uint8_t c0 = gens_color8(color[3 * r]), c1 = gens_color8(color[3 * r + 1]), c2 = gens_color8(color[3 * r + 2]);
    atlas[3 * pix] = c0, atlas[3 * pix + 1] = c1, atlas[3 * pix + 2] = c2;
    seen[pix] = gens_any_flag(vis + r * n_src, n_src);
}

__global__ __launch_bounds__(256) void texture_uv_k(int64_t n_faces, int S, int cols, double W, double H, float* __restrict__ uv) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= n_faces) return;
    int64_t x, y;
    k34_pixel(S, cols, f, 0, 0, x, y);
    uv[6 * f] = (float)(((double)x + 0.5) / W), uv[6 * f + 1] = (float)(1.0 - ((double)y + 0.5) / H);
    k34_pixel(S, cols, f, S - 2, 0, x, y);
    uv[6 * f + 2] = (float)(((double)x + 0.5) / W), uv[6 * f + 3] = (float)(1.0 - ((double)y + 0.5) / H);
    k34_pixel(S, cols, f, 0, S - 2, x, y);
    uv[6 * f + 4] = (float)(((double)x + 0.5) / W), uv[6 * f + 5] = (float)(1.0 - ((double)y + 0.5) / H);
}

// ------------------------------------------------------------------------------------------------ entry points
#define K34_LIMIT ((int64_t)1 << 31)

#define K34_CHECK_SHAPE(who)                                                                                                                         \
    GENS_CHECK_ARG(texels >= K34_MIN_TEXELS && texels <= K34_MAX_TEXELS, GENS_EINVAL, who ": texels = %d (%d to %d)", texels, K34_MIN_TEXELS,         \
                   K34_MAX_TEXELS);                                                                                                                  \
    GENS_CHECK_ARG(n_faces >= 0, GENS_EINVAL, who ": %lld triangles", (long long)n_faces);                                                           \
    GENS_CHECK_ARG(n_faces < K34_LIMIT, GENS_ELIMIT, who ": %lld triangles (below 2^31)", (long long)n_faces)

#define K34_CHECK_CHUNK(who)                                                                                                                         \
    const int64_t per_face = (int64_t)texels * (texels + 1) / 2, n = s1 - s0;                                                                        \
    GENS_CHECK_ARG(s0 >= 0 && s1 >= s0 && s1 <= n_faces * per_face, GENS_EINVAL, who ": samples %lld .. %lld of %lld triangles x %lld samples",       \
                   (long long)s0, (long long)s1, (long long)n_faces, (long long)per_face);                                                           \
    GENS_CHECK_ARG(n < K34_LIMIT, GENS_ELIMIT, who ": %lld samples in one launch (below 2^31)", (long long)n)

extern "C" int gens_texture_points(const float* points, int64_t n_vertices, const int32_t* triangles, int64_t n_faces, int texels, int64_t s0,
                                   int64_t s1, float* out, float* edge, void* stream) {
    K34_CHECK_SHAPE("gens_texture_points");
    GENS_CHECK_ARG(n_vertices >= 0, GENS_EINVAL, "gens_texture_points: %lld vertices", (long long)n_vertices);
    GENS_CHECK_ARG(n_vertices < K34_LIMIT, GENS_ELIMIT, "gens_texture_points: %lld vertices (below 2^31)", (long long)n_vertices);
    K34_CHECK_CHUNK("gens_texture_points");
    if (n == 0) return 0;
    GENS_CHECK_ARG(triangles && out, GENS_EINVAL, "gens_texture_points: null pointer");
    GENS_CHECK_ARG(points || n_vertices == 0, GENS_EINVAL, "gens_texture_points: null pointer (points, with %lld vertices)", (long long)n_vertices);
    texture_points_k<<<gens_blocks(n, 256), 256, 0, (hipStream_t)stream>>>(points, (int)n_vertices, triangles, texels, s0, n, out, edge);
    return gens_launch_status("gens_texture_points");
}

extern "C" int gens_texture_snap(float* points, const float* value, const float* grad, const float* limit, double max_move, float threshold,
                                 int64_t n, uint8_t* taken, void* stream) {
    GENS_CHECK_ARG(n >= 0, GENS_EINVAL, "gens_texture_snap: %lld samples", (long long)n);
    GENS_CHECK_ARG(n < K34_LIMIT, GENS_ELIMIT, "gens_texture_snap: %lld samples in one launch (below 2^31)", (long long)n);
    GENS_CHECK_ARG(isfinite(threshold), GENS_EINVAL, "gens_texture_snap: threshold = %g (finite)", (double)threshold);
    GENS_CHECK_ARG(limit || max_move > 0.0, GENS_EINVAL, "gens_texture_snap: max_move = %g (positive, or a limit per sample)", max_move);
    if (n == 0) return 0;
    GENS_CHECK_ARG(points && value && grad && taken, GENS_EINVAL, "gens_texture_snap: null pointer");
    texture_snap_k<<<gens_blocks(n, 256), 256, 0, (hipStream_t)stream>>>(points, value, grad, limit, max_move, (double)threshold, n, taken);
    return gens_launch_status("gens_texture_snap");
}

extern "C" int gens_texture_keep_better(float* points, float* value, float* grad, const float* prev_points, const float* prev_value,
                                        const float* prev_grad, float threshold, int64_t n, uint8_t* reverted, void* stream) {
    GENS_CHECK_ARG(n >= 0, GENS_EINVAL, "gens_texture_keep_better: %lld samples", (long long)n);
    GENS_CHECK_ARG(n < K34_LIMIT, GENS_ELIMIT, "gens_texture_keep_better: %lld samples in one launch (below 2^31)", (long long)n);
    GENS_CHECK_ARG(isfinite(threshold), GENS_EINVAL, "gens_texture_keep_better: threshold = %g (finite)", (double)threshold);
    if (n == 0) return 0;
    GENS_CHECK_ARG(points && value && grad && prev_points && prev_value && prev_grad && reverted, GENS_EINVAL, "gens_texture_keep_better: null pointer");
    texture_keep_k<<<gens_blocks(n, 256), 256, 0, (hipStream_t)stream>>>(points, value, grad, prev_points, prev_value, prev_grad, (double)threshold, n,
                                                                         reverted);
    return gens_launch_status("gens_texture_keep_better");
}

extern "C" int gens_texture_pack(const float* color, const uint8_t* vis, int n_src, int64_t n_faces, int texels, int64_t s0, int64_t s1,
                                 uint8_t* atlas, uint8_t* seen, void* stream) {
    K34_CHECK_SHAPE("gens_texture_pack");
    GENS_CHECK_ARG(n_src >= 1 && n_src <= 255, GENS_EINVAL, "gens_texture_pack: %d source views (1 to 255)", n_src);
    K34_CHECK_CHUNK("gens_texture_pack");
    if (n == 0) return 0;
    GENS_CHECK_ARG(color && vis && atlas && seen, GENS_EINVAL, "gens_texture_pack: null pointer");
    int64_t cols, rows;
    k34_layout(n_faces, texels, cols, rows);
    texture_pack_k<<<gens_blocks(n, 256), 256, 0, (hipStream_t)stream>>>(color, vis, n_src, texels, (int)cols, cols * (texels + 1), s0, n, atlas, seen);
    return gens_launch_status("gens_texture_pack");
}

extern "C" int gens_texture_uv(int64_t n_faces, int texels, float* uv, void* stream) {
    K34_CHECK_SHAPE("gens_texture_uv");
    if (n_faces == 0) return 0;
    GENS_CHECK_ARG(uv, GENS_EINVAL, "gens_texture_uv: null pointer");
    int64_t cols, rows;
    k34_layout(n_faces, texels, cols, rows);
    texture_uv_k<<<gens_blocks(n_faces, 256), 256, 0, (hipStream_t)stream>>>(n_faces, texels, (int)cols, (double)(cols * (texels + 1)), (double)(rows * texels),
                                                                           uv);
    return gens_launch_status("gens_texture_uv");
}
