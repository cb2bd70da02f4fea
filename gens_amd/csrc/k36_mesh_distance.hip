// K36: exact point-to-mesh distance (ops.closest_point_on_mesh, ops.mesh_distance, io.compare_meshes, python -m gens_amd.compare_meshes,
// ImplicitSurface.extract_geometry(simplify_error=)).  The definition is the comment of K36 in include/gens_hip.h;
// tests/mesh_distance_reference.py restates it in numpy as brute force over all faces and the kernel equals that restatement bit for bit.
//
//   closest: one thread per query, 256 per workgroup (ray_first_hit_k's shape).  The thread finds its cell of K23's grid (clamped into the
//            grid) and visits the cells at Chebyshev distance r = 0, 1, 2, ... from it, every listed face through face_d2 below, keeping the
//            lexicographically smallest (d2, face).  After ring r every face it has not seen lies wholly beyond one of the sides of the block
//            [c - r, c + r]^3 that are not on the grid's border (ring_bound); it stops once best d2 < bound^2 STRICTLY -- an unseen face can
//            then have neither a smaller d2 nor an equal one, so the answer is the brute-force one whatever the walk -- or once bound^2 >
//            max_dist^2, or once the block covers the grid.
//
// A face is listed in several cells and is evaluated once per listing the walk meets: harmless, d2 is a pure function of (query, face), and
// remembering faces would cost registers the gathers need more.  The 72 bytes of a face's corners are three scattered 24-byte reads; the
// lanes of a wave walk neighbouring cells, so the lines are shared in L1 / L2, and waves in flight hide the rest.  All state is named scalars
// (no indexed arrays): no scratch.  All arithmetic is float64, every operation rounded on its own (no contraction), in the order the
// definition writes; the divisions are the correctly rounded ones; there is no square root.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

#define K36_GRID_MAX_AXIS 512           // K23's limit (k23_mesh_cull.hip: GRID_MAX_AXIS)
#define K36_SHRINK (1.0 - 0x1p-40)      // the ring bound's margin: relative ...
#define K36_SLACK 0x1p-30               // ... and absolute, in cells (see ring_bound)
#define K36_MAX_RATIO 0x1p32            // (|lo| + 512 cell) / cell below this: what the margin's derivation assumes

struct Closest {
    double d2, px, py, pz;
    int region;
};

// |q - p0 - t e|^2 at the t in [0, 1] nearest to q along the segment p0 + t e (t = 0 for a segment of zero length, or where t is not > 0)
#define K36_SEGMENT(P0X, P0Y, P0Z, EX, EY, EZ, WX, WY, WZ, FIRST)                                   \
    {                                                                                               \
        const double l = (EX * EX + EY * EY) + EZ * EZ;                                             \
        double t = 0.0;                                                                             \
        if (l > 0.0) t = ((WX * EX + WY * EY) + WZ * EZ) / l;                                       \
        if (!(t > 0.0)) t = 0.0;                                                                    \
        if (t > 1.0) t = 1.0;                                                                       \
        const double sx = P0X + t * EX, sy = P0Y + t * EY, sz = P0Z + t * EZ;                       \
        const double ux = qx - sx, uy = qy - sy, uz = qz - sz;                                      \
        const double s2 = (ux * ux + uy * uy) + uz * uz;                                            \
        if (FIRST || s2 < r.d2) r.d2 = s2, r.px = sx, r.py = sy, r.pz = sz;                         \
    }

// The rule (a) of the header: Ericson's region walk, product by product.
__device__ __forceinline__ Closest face_d2(double qx, double qy, double qz, double ax, double ay, double az, double bx, double by, double bz,
                                           double cx, double cy, double cz) {
    Closest r;
    const double abx = bx - ax, aby = by - ay, abz = bz - az;
    const double acx = cx - ax, acy = cy - ay, acz = cz - az;
    const double apx = qx - ax, apy = qy - ay, apz = qz - az;
    const double nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
    int region = 7;
    double px = ax, py = ay, pz = az;
    if (!(nx == 0.0 && ny == 0.0 && nz == 0.0)) {
        const double d1 = (abx * apx + aby * apy) + abz * apz, d2 = (acx * apx + acy * apy) + acz * apz;
        const double bpx = qx - bx, bpy = qy - by, bpz = qz - bz;
        const double d3 = (abx * bpx + aby * bpy) + abz * bpz, d4 = (acx * bpx + acy * bpy) + acz * bpz;
        const double cpx = qx - cx, cpy = qy - cy, cpz = qz - cz;
        const double d5 = (abx * cpx + aby * cpy) + abz * cpz, d6 = (acx * cpx + acy * cpy) + acz * cpz;
        const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
        const double e = d4 - d3, g = d5 - d6;
        if (d1 <= 0.0 && d2 <= 0.0) {
            region = 1;
        } else if (d3 >= 0.0 && d4 <= d3) {
            region = 2, px = bx, py = by, pz = bz;
        } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
            const double den = d1 - d3;
            if (den > 0.0) {
                const double v = d1 / den;
                region = 4, px = ax + v * abx, py = ay + v * aby, pz = az + v * abz;
            }
        } else if (d6 >= 0.0 && d5 <= d6) {
            region = 3, px = cx, py = cy, pz = cz;
        } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
            const double den = d2 - d6;
            if (den > 0.0) {
                const double w = d2 / den;
                region = 6, px = ax + w * acx, py = ay + w * acy, pz = az + w * acz;
            }
        } else if (va <= 0.0 && e >= 0.0 && g >= 0.0) {
            const double den = e + g;
            if (den > 0.0) {
                const double w = e / den;
                region = 5, px = bx + w * (cx - bx), py = by + w * (cy - by), pz = bz + w * (cz - bz);
            }
        } else if (va >= 0.0 && vb >= 0.0 && vc >= 0.0) {
            const double den = (va + vb) + vc;
            if (den > 0.0) {
                const double v = vb / den, w = vc / den;
                region = 0, px = (ax + v * abx) + w * acx, py = (ay + v * aby) + w * acy, pz = (az + v * abz) + w * acz;
            }
        }
    }
    r.region = region;
    if (region != 7) {
        const double ux = qx - px, uy = qy - py, uz = qz - pz;
        r.d2 = (ux * ux + uy * uy) + uz * uz, r.px = px, r.py = py, r.pz = pz;
    } else {                            // the degenerate path: the nearest of the segments ab, bc, ca, the first on ties
        const double bcx = cx - bx, bcy = cy - by, bcz = cz - bz;
        const double cax = ax - cx, cay = ay - cy, caz = az - cz;
        const double bpx = qx - bx, bpy = qy - by, bpz = qz - bz;
        const double cpx = qx - cx, cpy = qy - cy, cpz = qz - cz;
        K36_SEGMENT(ax, ay, az, abx, aby, abz, apx, apy, apz, true)
        K36_SEGMENT(bx, by, bz, bcx, bcy, bcz, bpx, bpy, bpz, false)
        K36_SEGMENT(cx, cy, cz, cax, cay, caz, cpx, cpy, cpz, false)
    }
    return r;
}

// The lower bound, in cells, on the distance along one axis from the query (at p cells from the grid's corner) to anything beyond the sides
// lo_side, hi_side (cells) of the block; a side on the grid's border has nothing beyond it.  Shrunk by the margin of the header.
__device__ __forceinline__ double axis_bound(double p, int lo_side, int hi_side, int n) {
    double b = INFINITY;
    if (lo_side > 0) b = fmin(b, fmax((p - (double)lo_side) * K36_SHRINK - K36_SLACK, 0.0));
    if (hi_side < n) b = fmin(b, fmax(((double)hi_side - p) * K36_SHRINK - K36_SLACK, 0.0));
    return b;
}

__global__ __launch_bounds__(256) void mesh_closest_k(gens_mesh_grid g, const double* __restrict__ queries, int64_t n, double cap2,
                                                      double* __restrict__ dist2, int32_t* __restrict__ face, double* __restrict__ point,
                                                      uint8_t* __restrict__ region) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double qx = queries[3 * i], qy = queries[3 * i + 1], qz = queries[3 * i + 2];
    double best = INFINITY, bpx = NAN, bpy = NAN, bpz = NAN;
    int best_f = -1, best_r = 255;
    if (!(isfinite(qx) && isfinite(qy) && isfinite(qz))) {
        best = NAN;
    } else {
        const double cell = (double)g.cell, inv = 1.0 / cell;
        const double px = (qx - (double)g.lo_x) * inv, py = (qy - (double)g.lo_y) * inv, pz = (qz - (double)g.lo_z) * inv;
        const int nx = g.nx, ny = g.ny, nz = g.nz;
        const int ci = (int)fmin(fmax(floor(px), 0.0), (double)(nx - 1)), cj = (int)fmin(fmax(floor(py), 0.0), (double)(ny - 1)),
                  ck = (int)fmin(fmax(floor(pz), 0.0), (double)(nz - 1));
        const int64_t n_faces = g.n_faces;
        const int32_t listed = g.cell_start[(int64_t)nx * ny * nz];
        const int rings = max(nx, max(ny, nz));
        // at most max(nx, ny, nz) rings whatever the input: ring max - 1 reaches every border from any cell, and the block then covers the grid
        for (int r = 0; r < rings; ++r) {
            const int i0 = max(ci - r, 0), i1 = min(ci + r, nx - 1), j0 = max(cj - r, 0), j1 = min(cj + r, ny - 1);
            const int k0 = max(ck - r, 0), k1 = min(ck + r, nz - 1);
            for (int ii = i0; ii <= i1; ++ii)
                for (int jj = j0; jj <= j1; ++jj) {
                    // a column of the block: all of it where (ii, jj) is on the ring, else its two ends (one where r = 0, none outside the grid)
                    const bool whole = ii - ci == r || ci - ii == r || jj - cj == r || cj - jj == r;
                    const int step = whole ? 1 : 2 * r;
                    for (int kk = whole ? k0 : ck - r; kk <= (whole ? k1 : ck + r); kk += step) {
                        if (kk < 0 || kk >= nz) continue;
                        const int64_t c = ((int64_t)ii * ny + jj) * nz + kk;
                        int32_t s = g.cell_start[c], e = g.cell_start[c + 1];
                        s = s < 0 ? 0 : s, e = e > listed ? listed : e;
                        for (int32_t m = s; m < e; ++m) {
                            const int32_t f = g.cell_faces[m];
                            if (f < 0 || f >= n_faces) continue;                  // (a planted id: skipped, never read through)
                            const int32_t* __restrict__ tri = g.triangles + 3 * (int64_t)f;
                            const double* __restrict__ A = g.vertices + 3 * (int64_t)tri[0];
                            const double* __restrict__ B = g.vertices + 3 * (int64_t)tri[1];
                            const double* __restrict__ Cc = g.vertices + 3 * (int64_t)tri[2];
                            const Closest t = face_d2(qx, qy, qz, A[0], A[1], A[2], B[0], B[1], B[2], Cc[0], Cc[1], Cc[2]);
                            if (t.d2 < best || (t.d2 == best && f < best_f)) {    // (a NaN d2 is never taken)
                                best = t.d2, best_f = f, best_r = t.region;
                                bpx = t.px, bpy = t.py, bpz = t.pz;
                            }
                        }
                    }
                }
            if (i0 == 0 && i1 == nx - 1 && j0 == 0 && j1 == ny - 1 && k0 == 0 && k1 == nz - 1) break;       // the block covers the grid
            const double bc = fmin(axis_bound(px, ci - r, ci + r + 1, nx), fmin(axis_bound(py, cj - r, cj + r + 1, ny), axis_bound(pz, ck - r, ck + r + 1, nz)));
            const double bw = bc * cell;
            const double b2 = bw * bw;
            if (best < b2 || b2 > cap2) break;
        }
        if (!(best <= cap2)) best = INFINITY, best_f = -1, best_r = 255, bpx = bpy = bpz = NAN;
    }
    dist2[i] = best;
    face[i] = best_f;
    if (point) point[3 * i] = bpx, point[3 * i + 1] = bpy, point[3 * i + 2] = bpz;
    if (region) region[i] = (uint8_t)best_r;
}

__global__ __launch_bounds__(256) void mesh_closest_none_k(int64_t n, const double* __restrict__ queries, double* __restrict__ dist2,
                                                           int32_t* __restrict__ face, double* __restrict__ point, uint8_t* __restrict__ region) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool fin = isfinite(queries[3 * i]) && isfinite(queries[3 * i + 1]) && isfinite(queries[3 * i + 2]);
    dist2[i] = fin ? INFINITY : NAN;
    face[i] = -1;
    if (point) point[3 * i] = NAN, point[3 * i + 1] = NAN, point[3 * i + 2] = NAN;
    if (region) region[i] = 255;
}

// ------------------------------------------------------------------------------------------------ entry point
extern "C" int gens_mesh_closest_point(const gens_mesh_grid* g, const double* queries, int64_t n_queries, double max_dist, double* dist2,
                                       int32_t* face, double* point, uint8_t* region, void* stream) {
    const char* who = "gens_mesh_closest_point";
    GENS_CHECK_ARG(g, GENS_EINVAL, "%s: null grid", who);
    GENS_CHECK_ARG(n_queries >= 0, GENS_EINVAL, "%s: %lld queries", who, (long long)n_queries);
    GENS_CHECK_ARG(n_queries < ((int64_t)1 << 31), GENS_ELIMIT, "%s: %lld queries (below 2^31)", who, (long long)n_queries);
    GENS_CHECK_ARG(max_dist > 0.0, GENS_EINVAL, "%s: max_dist %g (must be positive; +inf for no cap)", who, max_dist);      // (NaN fails)
    GENS_CHECK_ARG(g->n_faces >= 0, GENS_EINVAL, "%s: %lld faces", who, (long long)g->n_faces);
    GENS_CHECK_ARG(g->n_faces < ((int64_t)1 << 31), GENS_ELIMIT, "%s: %lld faces (below 2^31)", who, (long long)g->n_faces);
    GENS_CHECK_ARG(g->nx >= 1 && g->nx <= K36_GRID_MAX_AXIS && g->ny >= 1 && g->ny <= K36_GRID_MAX_AXIS && g->nz >= 1 && g->nz <= K36_GRID_MAX_AXIS,
                   GENS_ELIMIT, "%s: grid %dx%dx%d (1 .. %d cells per axis)", who, g->nx, g->ny, g->nz, K36_GRID_MAX_AXIS);
    GENS_CHECK_ARG(g->cell > 0.0f && isfinite(g->cell) && isfinite(g->lo_x) && isfinite(g->lo_y) && isfinite(g->lo_z), GENS_ELIMIT, "%s: bad grid box",
                   who);
    GENS_CHECK_ARG((fmax(fabs((double)g->lo_x), fmax(fabs((double)g->lo_y), fabs((double)g->lo_z))) + 512.0 * (double)g->cell) / (double)g->cell <
                       K36_MAX_RATIO,
                   GENS_ELIMIT, "%s: the grid's corner is more than 2^32 cells from the origin (the stop bound's margin assumes less)", who);
    if (n_queries == 0) return 0;
    GENS_CHECK_ARG(queries && dist2 && face, GENS_EINVAL, "%s: null pointer (queries, dist2 or face)", who);
    if (g->n_faces == 0) {              // nothing to walk: +inf / -1 (NaN for a query that is not finite), the grid's pointers are not read
        mesh_closest_none_k<<<gens_blocks(n_queries, 256), 256, 0, (hipStream_t)stream>>>(n_queries, queries, dist2, face, point, region);
        return gens_launch_status(who);
    }
    GENS_CHECK_ARG(g->vertices && g->triangles && g->cell_start && g->cell_faces, GENS_EINVAL, "%s: null pointer (in the grid)", who);
    const double cap2 = max_dist * max_dist;
    mesh_closest_k<<<gens_blocks(n_queries, 256), 256, 0, (hipStream_t)stream>>>(*g, queries, n_queries, cap2, dist2, face, point, region);
    return gens_launch_status(who);
}
