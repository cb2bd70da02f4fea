// K32: fusion of per-view depth maps into a consistency-filtered point cloud (ops.fuse_depth_maps, ops.fused_points,
// ImplicitSurface.fuse_surface).  The definition is the comment of K32 in include/gens_hip.h; tests/depth_fusion_reference.py restates it in
// numpy and the kernels equal that restatement bit for bit.
//
//   fuse:    one thread per reference pixel (r, y, x); the listed source views are looped inside the thread: lift the pixel, project it into
//            the source, read the source's depth bilinearly, lift that, project it back, compare -> votes, keep, fused depth.
//   points:  one thread per entry of a compacted list of kept pixels -> the world point, and the pixel's normal and colour where given.
//
// A workgroup covers 16 x 16 pixels of ONE view, a wave an 8 x 8 tile of them: the view r, its camera row and its row of `pairs` are
// wave-uniform, so the compiler reads them (and the source's row cams[s]) with scalar loads -- 24 + 24 constants per (wave, source), not per
// lane.  The four bilinear taps are the only per-lane reads: neighbouring pixels of an 8 x 8 tile project to neighbouring pixels of the
// source, so a wave's 256 taps fall on about ten rows of one or two 128-byte lines each where a 64 x 1 row of pixels would touch the same
// number of lines for an eighth of the rows' reuse (the L1 looks up one line per clock).  All arithmetic is float64,
// every operation rounded on its own (no contraction), in the order the definition writes; the divisions are the correctly rounded ones.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

struct FuseArgs {
    const float* depth;
    const double* cams;
    const int32_t* pairs;
    const float* normal;
    int nv, h, w, k, tiles_x, tiles_y, min_views;
    double pix_tol2, rel_tol, normal_cos;
    uint8_t *votes, *keep;
    double* fused;
};

__device__ __forceinline__ bool usable(float d) { return isfinite(d) && d > 0.f; }

// row i of B [x, y, 1]: (B[i][0] x + B[i][1] y) + B[i][2]
__device__ __forceinline__ double ray_row(const double* __restrict__ b, int i, double x, double y) { return (b[3 * i] * x + b[3 * i + 1] * y) + b[3 * i + 2]; }
// row i of P [X, 1]: ((P[i][0] X0 + P[i][1] X1) + P[i][2] X2) + P[i][3]
__device__ __forceinline__ double proj_row(const double* __restrict__ p, int i, double x0, double x1, double x2) {
    return ((p[4 * i] * x0 + p[4 * i + 1] * x1) + p[4 * i + 2] * x2) + p[4 * i + 3];
}

__global__ __launch_bounds__(256) void fuse_depth_maps_k(FuseArgs a) {
    // (r, tile row, tile column) of this workgroup: scalar arithmetic on blockIdx
    const unsigned per_view = (unsigned)a.tiles_x * (unsigned)a.tiles_y;
    const int r = (int)(blockIdx.x / per_view);
    const unsigned t = blockIdx.x - (unsigned)r * per_view;
    const int ty = (int)(t / (unsigned)a.tiles_x), tx = (int)(t - (unsigned)ty * (unsigned)a.tiles_x);
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int x = tx * 16 + (wave & 1) * 8 + (lane & 7), y = ty * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (x >= a.w || y >= a.h) return;
    const int hw = a.h * a.w;
    const int pix = r * hw + y * a.w + x;                      // nv h w < 2^31 (an argument check)
    const double* __restrict__ cr = a.cams + 24 * (int64_t)r;
    const float df = a.depth[pix];
    int n = 0;
    double dsum = 0.0;
    const double d = (double)df, xd = (double)x, yd = (double)y;
    if (usable(df)) {
        double X[3];
        for (int i = 0; i < 3; ++i) X[i] = cr[21 + i] + d * ray_row(cr + 12, i, xd, yd);
        const float* __restrict__ nr = a.normal ? a.normal + 3 * (int64_t)pix : nullptr;
        for (int j = 0; j < a.k; ++j) {
            const int s = a.pairs[(int64_t)r * a.k + j];
            if (s < 0 || s >= a.nv) continue;                  // -1 pads a row (the host refuses anything else outside the views)
            const double* __restrict__ cs = a.cams + 24 * (int64_t)s;
            const double qz = proj_row(cs, 2, X[0], X[1], X[2]);
            if (!(qz > 0.0)) continue;
            const double xs = proj_row(cs, 0, X[0], X[1], X[2]) / qz, ys = proj_row(cs, 1, X[0], X[1], X[2]) / qz;
            const double x0 = floor(xs), y0 = floor(ys);
            if (!(0.0 <= x0 && x0 + 1.0 <= (double)(a.w - 1) && 0.0 <= y0 && y0 + 1.0 <= (double)(a.h - 1))) continue;
            const int base = s * hw + (int)y0 * a.w + (int)x0;
            const float t00 = a.depth[base], t01 = a.depth[base + 1], t10 = a.depth[base + a.w], t11 = a.depth[base + a.w + 1];
            if (!(usable(t00) && usable(t01) && usable(t10) && usable(t11))) continue;
            const double fx = xs - x0, fy = ys - y0, gx = 1.0 - fx, gy = 1.0 - fy;
            const double ds = ((double)t00 * gx + (double)t01 * fx) * gy + ((double)t10 * gx + (double)t11 * fx) * fy;
            double Xs[3];
            for (int i = 0; i < 3; ++i) Xs[i] = cs[21 + i] + ds * ray_row(cs + 12, i, xs, ys);
            const double bz = proj_row(cr, 2, Xs[0], Xs[1], Xs[2]);
            if (!(bz > 0.0)) continue;
            const double ex = proj_row(cr, 0, Xs[0], Xs[1], Xs[2]) / bz - xd, ey = proj_row(cr, 1, Xs[0], Xs[1], Xs[2]) / bz - yd;
            if (!(ex * ex + ey * ey < a.pix_tol2)) continue;
            if (!(fabs(bz - d) / d < a.rel_tol)) continue;
            if (nr) {
                const int xn = (int)floor(xs + 0.5), yn = (int)floor(ys + 0.5);     // inside the four taps: 0 <= x0 <= xn <= x0 + 1 <= w - 1
                const float* __restrict__ ns = a.normal + 3 * (int64_t)(s * hw + yn * a.w + xn);
                const double dot = ((double)nr[0] * (double)ns[0] + (double)nr[1] * (double)ns[1]) + (double)nr[2] * (double)ns[2];
                if (!(dot >= a.normal_cos)) continue;
            }
            n += 1;
            dsum += bz;
        }
    }
    const bool kept = n >= a.min_views;
    a.votes[pix] = (uint8_t)(n < 255 ? n : 255);
    a.keep[pix] = kept ? 1 : 0;
    a.fused[pix] = kept ? (d + dsum) / (double)(n + 1) : 0.0;
}

__global__ __launch_bounds__(256) void fused_points_k(const double* __restrict__ fused, const double* __restrict__ cams, const int64_t* __restrict__ list,
                                                      int m, int hw, int w, int n_pix, const float* __restrict__ normal, const uint8_t* __restrict__ img,
                                                      double* __restrict__ points, float* __restrict__ normals, uint8_t* __restrict__ colors) {
    const int j = (int)(blockIdx.x * 256u + threadIdx.x);
    if (j >= m) return;
    const int64_t p64 = list[j];
    const bool ok = p64 >= 0 && p64 < n_pix;                   // (an entry outside the maps: a zero row, nothing read)
    const int pix = ok ? (int)p64 : 0;
    const int r = pix / hw, rem = pix - r * hw, y = rem / w, x = rem - y * w;
    const double* __restrict__ c = cams + 24 * (int64_t)r;
    const double f = ok ? fused[pix] : 0.0;
    for (int i = 0; i < 3; ++i) {
        points[3 * (int64_t)j + i] = ok ? c[21 + i] + f * ray_row(c + 12, i, (double)x, (double)y) : 0.0;
        if (normals) normals[3 * (int64_t)j + i] = ok ? normal[3 * (int64_t)pix + i] : 0.f;
        if (colors) colors[3 * (int64_t)j + i] = ok ? img[3 * (int64_t)pix + i] : 0;
    }
}

// ------------------------------------------------------------------------------------------------ entry points
static int check_maps(const char* who, int nv, int h, int w, int64_t* n_pix) {
    GENS_CHECK_ARG(nv >= 0 && h >= 0 && w >= 0, GENS_EINVAL, "%s: %d maps of %d x %d pixels", who, nv, h, w);
    const int64_t hw = (int64_t)h * w;                          // < 2^62
    GENS_CHECK_ARG(hw < ((int64_t)1 << 31) && (int64_t)nv * hw < ((int64_t)1 << 31), GENS_ELIMIT, "%s: %d maps of %d x %d pixels (nv h w below 2^31)", who,
                   nv, h, w);
    *n_pix = (int64_t)nv * hw;
    return 0;
}

extern "C" int gens_fuse_depth_maps(const float* depth, const double* cams, const int32_t* pairs, const float* normal, int nv, int h, int w, int k,
                                    double pix_tol, double rel_tol, int min_views, double normal_cos, uint8_t* votes, uint8_t* keep, double* fused,
                                    void* stream) {
    int64_t n_pix = 0;
    if (int rc = check_maps("gens_fuse_depth_maps", nv, h, w, &n_pix)) return rc;
    GENS_CHECK_ARG(k >= 0, GENS_EINVAL, "gens_fuse_depth_maps: %d source views per row of pairs", k);
    GENS_CHECK_ARG(pix_tol >= 0.0 && isfinite(pix_tol), GENS_EINVAL, "gens_fuse_depth_maps: pix_tol = %g (finite, at least 0)", pix_tol);
    GENS_CHECK_ARG(rel_tol >= 0.0 && isfinite(rel_tol), GENS_EINVAL, "gens_fuse_depth_maps: rel_tol = %g (finite, at least 0)", rel_tol);
    GENS_CHECK_ARG(min_views >= 1, GENS_EINVAL, "gens_fuse_depth_maps: min_views = %d (at least 1)", min_views);
    GENS_CHECK_ARG(!normal || normal_cos == normal_cos, GENS_EINVAL, "gens_fuse_depth_maps: normal_cos is not a number");
    if (n_pix == 0) return 0;
    GENS_CHECK_ARG(depth && cams && votes && keep && fused, GENS_EINVAL, "gens_fuse_depth_maps: null pointer");
    GENS_CHECK_ARG(pairs || k == 0, GENS_EINVAL, "gens_fuse_depth_maps: null pointer (pairs, with %d source views per row)", k);
    FuseArgs a;
    a.depth = depth, a.cams = cams, a.pairs = pairs, a.normal = normal;
    a.nv = nv, a.h = h, a.w = w, a.k = k, a.tiles_x = (w + 15) / 16, a.tiles_y = (h + 15) / 16, a.min_views = min_views;
    a.pix_tol2 = pix_tol * pix_tol, a.rel_tol = rel_tol, a.normal_cos = normal_cos;
    a.votes = votes, a.keep = keep, a.fused = fused;
    const int64_t blocks = (int64_t)nv * a.tiles_x * a.tiles_y;       // <= nv h w
    fuse_depth_maps_k<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(a);
    return gens_launch_status("gens_fuse_depth_maps");
}

extern "C" int gens_fused_points(const double* fused, const double* cams, const int64_t* list, int64_t n_list, int nv, int h, int w, const float* normal,
                                 const uint8_t* img, double* points, float* normals, uint8_t* colors, void* stream) {
    int64_t n_pix = 0;
    if (int rc = check_maps("gens_fused_points", nv, h, w, &n_pix)) return rc;
    GENS_CHECK_ARG(n_list >= 0, GENS_EINVAL, "gens_fused_points: a list of %lld pixels", (long long)n_list);
    GENS_CHECK_ARG(n_list < ((int64_t)1 << 31), GENS_ELIMIT, "gens_fused_points: a list of %lld pixels (below 2^31)", (long long)n_list);
    GENS_CHECK_ARG(!normal == !normals && !img == !colors, GENS_EINVAL,
                   "gens_fused_points: null pointer (a normal / colour map comes with its output, and an output with its map)");
    if (n_list == 0) return 0;
    GENS_CHECK_ARG(n_pix > 0, GENS_EINVAL, "gens_fused_points: a list of %lld pixels of empty maps", (long long)n_list);
    GENS_CHECK_ARG(fused && cams && list && points, GENS_EINVAL, "gens_fused_points: null pointer");
    fused_points_k<<<gens_blocks(n_list, 256), 256, 0, (hipStream_t)stream>>>(fused, cams, list, (int)n_list, h * w, w, (int)n_pix, normal, img, points,
                                                                            normals, colors);
    return gens_launch_status("gens_fused_points");
}
