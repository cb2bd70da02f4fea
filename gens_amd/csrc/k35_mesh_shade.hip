// K35: depth, normal and colour maps of a triangle mesh at the first hits of rays (ops.shade_mesh_hits / render_mesh,
// ImplicitSurface.render_mesh, validate(mesh_render=)).  The definition is the comment of K35 in include/gens_hip.h;
// tests/mesh_render_reference.py restates it in numpy and the kernel equals that restatement bit for bit.
//
//   shade:  one thread per ray -> hit, barycentrics, depth, normal, normal image, colour, seen.  A thread reads its (face, t), the face's
//           three indices, 72 bytes of corners and, as asked, 36 bytes of vertex normals, 9 + 3 bytes of vertex colours and flags or at
//           most four atlas texels; neighbouring rays hit neighbouring faces, so a wave's gathers fall into a few cache lines.
//
// A streaming kernel, 64-bit ray indices, no LDS, no atomics, named scalars only (no indexed arrays): no scratch.  All arithmetic of the
// definition is float64, every operation rounded on its own (no contraction), results rounded once.
#include <math.h>

#include "atlas_rules.h"
#include "common.h"
#include "pack_rules.h"

#pragma clang fp contract(off)

__device__ __forceinline__ double k35_dot(double ux, double uy, double uz, double vx, double vy, double vz) {
    return (ux * vx + uy * vy) + uz * vz;
}

__device__ __forceinline__ uint8_t k35_round8(double x) {
    const double q = floor(x + 0.5);
    return (uint8_t)(int)(q < 0.0 ? 0.0 : q > 255.0 ? 255.0 : q);
}

// One tap of the atlas look-up: weight w at the local texel (ip, jp) of face f.  A tap whose weight is not > 0 is not read.
__device__ __forceinline__ void k35_tap(const gens_mesh_shade_args& a, int cols, int64_t f, int ip, int jp, double w, bool want_img, double& c0,
                                        double& c1, double& c2, bool& seen) {
    c0 = c1 = c2 = 0.0;
    if (!(w > 0.0)) return;
    int64_t x, y;
    k34_pixel(a.texels, cols, f, ip, jp, x, y);
    const int64_t pix = y * a.atlas_w + x;
    if (want_img) {
        c0 = w * (double)a.atlas[3 * pix];
        c1 = w * (double)a.atlas[3 * pix + 1];
        c2 = w * (double)a.atlas[3 * pix + 2];
    }
    if (a.seen) seen = seen && a.atlas_seen[pix] != 0;
}

__global__ __launch_bounds__(256) void mesh_shade_k(gens_mesh_shade_args a, int cols) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.n) return;
    const bool want_normal = a.normal || a.normal_img, want_color = a.img || a.seen;
    const bool want_bary = a.bary || want_color || (want_normal && a.shading == 1);

    // 1. hit
    const int64_t f = a.face[r];
    const float tf = a.t[r];
    bool hit = f >= 0 && f < a.n_faces && isfinite(tf) && tf > 0.f;
    int64_t i0 = 0, i1 = 0, i2 = 0;
    if (hit) {
        i0 = a.triangles[3 * f], i1 = a.triangles[3 * f + 1], i2 = a.triangles[3 * f + 2];
        hit = i0 >= 0 && i0 < a.n_vertices && i1 >= 0 && i1 < a.n_vertices && i2 >= 0 && i2 < a.n_vertices;
    }
    double ax = 0, ay = 0, az = 0, bx = 0, by = 0, bz = 0, cx = 0, cy = 0, cz = 0;
    if (hit) {
        const double* __restrict__ pa = a.vertices + 3 * i0;
        const double* __restrict__ pb = a.vertices + 3 * i1;
        const double* __restrict__ pc = a.vertices + 3 * i2;
        ax = pa[0], ay = pa[1], az = pa[2], bx = pb[0], by = pb[1], bz = pb[2], cx = pc[0], cy = pc[1], cz = pc[2];
        hit = isfinite(ax) && isfinite(ay) && isfinite(az) && isfinite(bx) && isfinite(by) && isfinite(bz) && isfinite(cx) && isfinite(cy) &&
              isfinite(cz);
    }
    if (a.hit) a.hit[r] = hit ? 1 : 0;

    float dx = 0.f, dy = 0.f, dz = 0.f;
    if (hit && (a.depth || want_bary)) dx = a.rays_d[3 * r], dy = a.rays_d[3 * r + 1], dz = a.rays_d[3 * r + 2];

    // 2. depth
    if (a.depth) a.depth[r] = hit ? gens_pack_depth(a.rot, tf, dx, dy, dz) : 0.f;

    // 3. barycentrics
    const double e1x = bx - ax, e1y = by - ay, e1z = bz - az, e2x = cx - ax, e2y = cy - ay, e2z = cz - az;
    double wa = 0.0, wb = 0.0, wc = 0.0;
    if (hit && want_bary) {
        const double t = (double)tf;
        const double px = (double)a.rays_o[3 * r] + t * (double)dx, py = (double)a.rays_o[3 * r + 1] + t * (double)dy,
                     pz = (double)a.rays_o[3 * r + 2] + t * (double)dz;
        const double wx = px - ax, wy = py - ay, wz = pz - az;
        const double d11 = k35_dot(e1x, e1y, e1z, e1x, e1y, e1z), d12 = k35_dot(e1x, e1y, e1z, e2x, e2y, e2z),
                     d22 = k35_dot(e2x, e2y, e2z, e2x, e2y, e2z);
        const double w1 = k35_dot(wx, wy, wz, e1x, e1y, e1z), w2 = k35_dot(wx, wy, wz, e2x, e2y, e2z);
        const double den = d11 * d22 - d12 * d12;
        double b = (d22 * w1 - d12 * w2) / den, c = (d11 * w2 - d12 * w1) / den;
        wa = 1.0;
        if (den > 0.0 && isfinite(b) && isfinite(c)) {
            b = b > 0.0 ? b : 0.0;
            c = c > 0.0 ? c : 0.0;
            const double s = b + c;
            if (s > 1.0) b = b / s, c = c / s;
            const double rest = (1.0 - b) - c;
            wa = rest > 0.0 ? rest : 0.0, wb = b, wc = c;
        }
    }
    if (a.bary) a.bary[3 * r] = (float)wa, a.bary[3 * r + 1] = (float)wb, a.bary[3 * r + 2] = (float)wc;

    // 4. normal
    if (want_normal) {
        float nx = 0.f, ny = 0.f, nz = 0.f;
        if (hit) {
            double gx, gy, gz;
            if (a.shading == 1) {
                const float* __restrict__ na = a.vertex_normals + 3 * i0;
                const float* __restrict__ nb = a.vertex_normals + 3 * i1;
                const float* __restrict__ nc = a.vertex_normals + 3 * i2;
                gx = (wa * (double)na[0] + wb * (double)nb[0]) + wc * (double)nc[0];
                gy = (wa * (double)na[1] + wb * (double)nb[1]) + wc * (double)nc[1];
                gz = (wa * (double)na[2] + wb * (double)nb[2]) + wc * (double)nc[2];
            } else {
                gx = e1y * e2z - e1z * e2y, gy = e1z * e2x - e1x * e2z, gz = e1x * e2y - e1y * e2x;
                if (a.orient) gx = -gx, gy = -gy, gz = -gz;
            }
            gens_unit_normal64(gx, gy, gz, nx, ny, nz);
        }
        if (a.normal) a.normal[3 * r] = nx, a.normal[3 * r + 1] = ny, a.normal[3 * r + 2] = nz;
        if (a.normal_img) {
            a.normal_img[3 * r] = hit ? gens_normal_img(a.rot, 0, nx, ny, nz) : 0.f;
            a.normal_img[3 * r + 1] = hit ? gens_normal_img(a.rot, 1, nx, ny, nz) : 0.f;
            a.normal_img[3 * r + 2] = hit ? gens_normal_img(a.rot, 2, nx, ny, nz) : 0.f;
        }
    }

    // 5. / 6. colour
    if (want_color) {
        double x0 = 0.0, x1 = 0.0, x2 = 0.0;
        bool seen = hit;
        if (hit && a.atlas) {
            const double scale = (double)(a.texels - 2);
            const double x = wb * scale, y = wc * scale;
            const double fi = floor(x), fj = floor(y);
            const double fx = x - fi, fy = y - fj, gx = 1.0 - fx, gy = 1.0 - fy;
            const int ip = (int)fi, jp = (int)fj;               // (0 <= b, c <= 1: 0 <= ip, jp <= S - 2, and a tap at S - 1 has a weight > 0 only below it)
            const bool want_img = a.img != nullptr;
            double p0, p1, p2, q0, q1, q2, r0, r1, r2, s0, s1, s2;
            k35_tap(a, cols, f, ip, jp, gx * gy, want_img, p0, p1, p2, seen);
            k35_tap(a, cols, f, ip + 1, jp, fx * gy, want_img, q0, q1, q2, seen);
            k35_tap(a, cols, f, ip, jp + 1, gx * fy, want_img, r0, r1, r2, seen);
            k35_tap(a, cols, f, ip + 1, jp + 1, fx * fy, want_img, s0, s1, s2, seen);
            x0 = ((p0 + q0) + r0) + s0, x1 = ((p1 + q1) + r1) + s1, x2 = ((p2 + q2) + r2) + s2;
        } else if (hit) {
            if (a.img) {
                const uint8_t* __restrict__ ca = a.vertex_colors + 3 * i0;
                const uint8_t* __restrict__ cb = a.vertex_colors + 3 * i1;
                const uint8_t* __restrict__ cc = a.vertex_colors + 3 * i2;
                x0 = (wa * (double)ca[0] + wb * (double)cb[0]) + wc * (double)cc[0];
                x1 = (wa * (double)ca[1] + wb * (double)cb[1]) + wc * (double)cc[1];
                x2 = (wa * (double)ca[2] + wb * (double)cb[2]) + wc * (double)cc[2];
            }
            if (a.seen) {
                if (wa > 0.0) seen = seen && a.vertex_seen[i0] != 0;
                if (wb > 0.0) seen = seen && a.vertex_seen[i1] != 0;
                if (wc > 0.0) seen = seen && a.vertex_seen[i2] != 0;
            }
        }
        if (a.img) a.img[3 * r] = k35_round8(x0), a.img[3 * r + 1] = k35_round8(x1), a.img[3 * r + 2] = k35_round8(x2);
        if (a.seen) a.seen[r] = seen ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------------ entry point
#define K35_LIMIT ((int64_t)1 << 31)

extern "C" int gens_mesh_shade(const gens_mesh_shade_args* a, void* stream) {
    const char* who = "gens_mesh_shade";
    GENS_CHECK_ARG(a, GENS_EINVAL, "%s: null pointer (the arguments)", who);
    GENS_CHECK_ARG(a->n >= 0 && a->n_vertices >= 0 && a->n_faces >= 0, GENS_EINVAL, "%s: %lld rays, %lld vertices, %lld triangles", who,
                   (long long)a->n, (long long)a->n_vertices, (long long)a->n_faces);
    GENS_CHECK_ARG(a->n < K35_LIMIT && a->n_vertices < K35_LIMIT && a->n_faces < K35_LIMIT, GENS_ELIMIT,
                   "%s: %lld rays, %lld vertices, %lld triangles (each below 2^31)", who, (long long)a->n, (long long)a->n_vertices,
                   (long long)a->n_faces);
    GENS_CHECK_ARG(a->shading == 0 || a->shading == 1, GENS_EINVAL, "%s: shading = %d (0 flat, 1 smooth)", who, a->shading);
    GENS_CHECK_ARG(a->orient == 0 || a->orient == 1, GENS_EINVAL, "%s: orient = %d (0 as wound, 1 reversed)", who, a->orient);
    int64_t cols = 0, rows = 0;
    GENS_CHECK_ARG(a->atlas || !a->atlas_seen, GENS_EINVAL, "%s: atlas_seen without an atlas", who);
    if (a->atlas) {
        GENS_CHECK_ARG(a->texels >= K34_MIN_TEXELS && a->texels <= K34_MAX_TEXELS, GENS_EINVAL, "%s: texels = %d (%d to %d)", who, a->texels,
                       K34_MIN_TEXELS, K34_MAX_TEXELS);
        k34_layout(a->n_faces, a->texels, cols, rows);
        GENS_CHECK_ARG(a->atlas_h == rows * a->texels && a->atlas_w == cols * (a->texels + 1), GENS_EINVAL,
                       "%s: an atlas of %lld x %lld, expected %lld x %lld for %lld triangles with texels = %d", who, (long long)a->atlas_h,
                       (long long)a->atlas_w, (long long)(rows * a->texels), (long long)(cols * (a->texels + 1)), (long long)a->n_faces, a->texels);
    }
    GENS_CHECK_ARG(a->shading == 0 || a->vertex_normals, GENS_EINVAL, "%s: smooth shading without vertex normals", who);
    GENS_CHECK_ARG(!(a->img || a->seen) || a->atlas || a->vertex_colors, GENS_EINVAL, "%s: img or seen without vertex colours or an atlas", who);
    GENS_CHECK_ARG(!a->seen || (a->atlas ? a->atlas_seen != nullptr : a->vertex_seen != nullptr), GENS_EINVAL,
                   "%s: seen without the seen plane of the colour's source", who);
    const bool want_normal = a->normal || a->normal_img, want_color = a->img || a->seen;
    if (a->n == 0 || !(a->hit || a->bary || a->depth || want_normal || want_color)) return 0;
    const bool want_bary = a->bary || want_color || (want_normal && a->shading == 1);
    GENS_CHECK_ARG(a->face && a->t, GENS_EINVAL, "%s: null pointer (face, t)", who);
    GENS_CHECK_ARG(a->triangles || a->n_faces == 0, GENS_EINVAL, "%s: null pointer (triangles, with %lld of them)", who, (long long)a->n_faces);
    GENS_CHECK_ARG(a->vertices || a->n_vertices == 0, GENS_EINVAL, "%s: null pointer (vertices, with %lld of them)", who, (long long)a->n_vertices);
    GENS_CHECK_ARG(a->rays_d || !(a->depth || want_bary), GENS_EINVAL, "%s: null pointer (rays_d: the depth and the barycentrics need it)", who);
    GENS_CHECK_ARG(a->rays_o || !want_bary, GENS_EINVAL, "%s: null pointer (rays_o: the barycentrics need it)", who);
    GENS_CHECK_ARG(a->rot || !(a->depth || a->normal_img), GENS_EINVAL, "%s: null pointer (rot: the depth and the normal image need it)", who);
    mesh_shade_k<<<gens_blocks(a->n, 256), 256, 0, (hipStream_t)stream>>>(*a, (int)cols);
    return gens_launch_status(who);
}
