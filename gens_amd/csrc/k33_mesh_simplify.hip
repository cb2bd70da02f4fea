// K33: mesh simplification by vertex clustering with quadric-optimal representatives (ops.simplify_mesh, io.simplify_mesh,
// ImplicitSurface.extract_geometry(simplify=)).  The definition is the comment of K33 in include/gens_hip.h; tests/mesh_simplify_reference.py
// restates it in numpy and the kernels equal that restatement bit for bit.
//
//   keys:       one thread per vertex -> the int64 key of its cell (-1 where the cell is outside 0 .. 2^21 - 1 on an axis, or not a number).
//   triangles:  one thread per triangle -> the cluster ranks of its three vertices, whether it survives, and the ranks sorted.
//   solve:      one thread per output cluster.  The thread walks the cluster's segment of triangle entries (ascending triangle index) and its
//               segment of members (ascending vertex index) IN ORDER -- the order is part of the definition, so nothing is split across lanes --
//               gathers each surviving triangle's three vertices (72 bytes), accumulates the quadric (6 + 3 sums) and the members' mean in
//               registers, solves the 3 x 3 system by its adjugate, and walks the members a second time for the source vertex.
//
// The segments of neighbouring clusters are unrelated in memory (entries sorted by cluster point at triangles anywhere in the mesh), so the
// gathers are the cost; a cluster holds a handful of vertices and a dozen entries, and a wave's 64 clusters keep 64 gathers in flight.  All
// state is named scalars (no indexed arrays): no scratch.  All arithmetic is float64, every operation rounded on its own (no contraction), in
// the order the definition writes; the divisions are the correctly rounded ones; there is no square root.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

#define K33_AXIS_CELLS ((int64_t)1 << 21)

__global__ __launch_bounds__(256) void cluster_keys_k(const double* __restrict__ vertices, int n, double ox, double oy, double oz, double cell,
                                                      int64_t* __restrict__ keys) {
    const int v = (int)(blockIdx.x * 256u + threadIdx.x);
    if (v >= n) return;
    const double cx = floor((vertices[3 * (int64_t)v] - ox) / cell), cy = floor((vertices[3 * (int64_t)v + 1] - oy) / cell),
                 cz = floor((vertices[3 * (int64_t)v + 2] - oz) / cell);
    const double top = (double)K33_AXIS_CELLS;
    const bool ok = cx >= 0.0 && cx < top && cy >= 0.0 && cy < top && cz >= 0.0 && cz < top;     // (a NaN fails every comparison)
    keys[v] = ok ? (((int64_t)cz << 42) + ((int64_t)cy << 21)) + (int64_t)cx : (int64_t)-1;
}

__global__ __launch_bounds__(256) void cluster_triangles_k(const int32_t* __restrict__ triangles, int n_tri, const int32_t* __restrict__ vertex_cluster,
                                                           int n_vert, int32_t* __restrict__ ranks, uint8_t* __restrict__ survive,
                                                           int32_t* __restrict__ triple) {
    const int t = (int)(blockIdx.x * 256u + threadIdx.x);
    if (t >= n_tri) return;
    const int32_t i0 = triangles[3 * (int64_t)t], i1 = triangles[3 * (int64_t)t + 1], i2 = triangles[3 * (int64_t)t + 2];
    const bool in0 = i0 >= 0 && i0 < n_vert, in1 = i1 >= 0 && i1 < n_vert, in2 = i2 >= 0 && i2 < n_vert;
    const int32_t a = in0 ? vertex_cluster[i0] : -1, b = in1 ? vertex_cluster[i1] : -1, c = in2 ? vertex_cluster[i2] : -1;
    const bool ok = a >= 0 && b >= 0 && c >= 0 && a != b && b != c && a != c;
    int32_t lo = a < b ? a : b, hi = a < b ? b : a, mid;
    if (c < lo) mid = lo, lo = c;
    else if (c > hi) mid = hi, hi = c;
    else mid = c;
    ranks[3 * (int64_t)t] = a, ranks[3 * (int64_t)t + 1] = b, ranks[3 * (int64_t)t + 2] = c;
    survive[t] = ok ? 1 : 0;
    triple[3 * (int64_t)t] = lo, triple[3 * (int64_t)t + 1] = mid, triple[3 * (int64_t)t + 2] = hi;
}

struct SolveArgs {
    const double* vertices;
    const int32_t* triangles;
    const uint8_t* survive;
    const int64_t* cluster_keys;
    const int32_t *entries, *entry_start, *members, *member_start, *out_clusters;
    int n_vert, n_tri, n_clusters, n_out;
    double ox, oy, oz, cell, reg;
    double* out_vertices;
    int32_t* source;
    uint8_t* fell_back;
};

__global__ __launch_bounds__(256) void cluster_solve_k(SolveArgs a) {
    const int j = (int)(blockIdx.x * 256u + threadIdx.x);
    if (j >= a.n_out) return;
    const int32_t c = a.out_clusters[j];
    double x0 = 0.0, x1 = 0.0, x2 = 0.0;
    double px = 0.0, py = 0.0, pz = 0.0;
    int32_t src = -1;
    bool fell = true;
    if (c >= 0 && c < a.n_clusters) {                               // (a rank outside the clusters: a zero row, source -1, nothing read)
        const int64_t key = a.cluster_keys[c];
        const double ccx = (double)(key & (K33_AXIS_CELLS - 1)), ccy = (double)((key >> 21) & (K33_AXIS_CELLS - 1)),
                     ccz = (double)((key >> 42) & (K33_AXIS_CELLS - 1));
        const double cell = a.cell;
        const double tx = a.ox + (ccx + 0.5) * cell, ty = a.oy + (ccy + 0.5) * cell, tz = a.oz + (ccz + 0.5) * cell;
        // --- the quadric: every surviving triangle of the entry segment, in order
        double A00 = 0.0, A01 = 0.0, A02 = 0.0, A11 = 0.0, A12 = 0.0, A22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
        int e0 = a.entry_start[c], e1 = a.entry_start[c + 1];
        const int n_ent = 3 * a.n_tri;                              // 3 T < 2^31 (an argument check)
        e0 = e0 < 0 ? 0 : e0, e1 = e1 > n_ent ? n_ent : e1;
        for (int e = e0; e < e1; ++e) {
            const int32_t ent = a.entries[e];
            if (ent < 0 || ent >= n_ent) continue;
            const int t = ent / 3;
            if (!a.survive[t]) continue;
            const int32_t i0 = a.triangles[3 * (int64_t)t], i1 = a.triangles[3 * (int64_t)t + 1], i2 = a.triangles[3 * (int64_t)t + 2];
            if (i0 < 0 || i0 >= a.n_vert || i1 < 0 || i1 >= a.n_vert || i2 < 0 || i2 >= a.n_vert) continue;
            const double* __restrict__ p0 = a.vertices + 3 * (int64_t)i0;
            const double* __restrict__ p1 = a.vertices + 3 * (int64_t)i1;
            const double* __restrict__ p2 = a.vertices + 3 * (int64_t)i2;
            const double q0x = (p0[0] - tx) / cell, q0y = (p0[1] - ty) / cell, q0z = (p0[2] - tz) / cell;
            const double q1x = (p1[0] - tx) / cell, q1y = (p1[1] - ty) / cell, q1z = (p1[2] - tz) / cell;
            const double q2x = (p2[0] - tx) / cell, q2y = (p2[1] - ty) / cell, q2z = (p2[2] - tz) / cell;
            const double ux = q1x - q0x, uy = q1y - q0y, uz = q1z - q0z;
            const double vx = q2x - q0x, vy = q2y - q0y, vz = q2z - q0z;
            const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
            const double d = -((nx * q0x + ny * q0y) + nz * q0z);
            A00 += nx * nx, A01 += nx * ny, A02 += nx * nz, A11 += ny * ny, A12 += ny * nz, A22 += nz * nz;
            b0 += nx * d, b1 += ny * d, b2 += nz * d;
        }
        // --- the members' mean
        int m0 = a.member_start[c], m1 = a.member_start[c + 1];
        m0 = m0 < 0 ? 0 : m0, m1 = m1 > a.n_vert ? a.n_vert : m1;
        double sx = 0.0, sy = 0.0, sz = 0.0;
        int count = 0;
        for (int m = m0; m < m1; ++m) {
            const int32_t v = a.members[m];
            if (v < 0 || v >= a.n_vert) continue;
            const double* __restrict__ p = a.vertices + 3 * (int64_t)v;
            sx += (p[0] - tx) / cell, sy += (p[1] - ty) / cell, sz += (p[2] - tz) / cell;
            count += 1;
        }
        const double cnt = (double)count;
        const double mx = sx / cnt, my = sy / cnt, mz = sz / cnt;   // (an output cluster has a member: a triangle references it)
        // --- the representative
        x0 = mx, x1 = my, x2 = mz;
        const double tr = (A00 + A11) + A22;
        if (tr > 0.0) {
            const double lam = a.reg * tr;
            const double M00 = A00 + lam, M11 = A11 + lam, M22 = A22 + lam, M01 = A01, M02 = A02, M12 = A12;
            const double r0 = lam * mx - b0, r1 = lam * my - b1, r2 = lam * mz - b2;
            const double c00 = M11 * M22 - M12 * M12, c01 = M02 * M12 - M01 * M22, c02 = M01 * M12 - M02 * M11;
            const double c11 = M00 * M22 - M02 * M02, c12 = M01 * M02 - M00 * M12, c22 = M00 * M11 - M01 * M01;
            const double det = (M00 * c00 + M01 * c01) + M02 * c02;
            const double y0 = ((c00 * r0 + c01 * r1) + c02 * r2) / det, y1 = ((c01 * r0 + c11 * r1) + c12 * r2) / det,
                         y2 = ((c02 * r0 + c12 * r1) + c22 * r2) / det;
            if (det > 0.0 && fabs(y0) <= 0.5 && fabs(y1) <= 0.5 && fabs(y2) <= 0.5) x0 = y0, x1 = y1, x2 = y2, fell = false;
        }
        px = tx + x0 * cell, py = ty + x1 * cell, pz = tz + x2 * cell;
        // --- the source: the member nearest to x, the first on ties
        double best = 0.0;
        for (int m = m0; m < m1; ++m) {
            const int32_t v = a.members[m];
            if (v < 0 || v >= a.n_vert) continue;
            const double* __restrict__ p = a.vertices + 3 * (int64_t)v;
            const double dx = (p[0] - tx) / cell - x0, dy = (p[1] - ty) / cell - x1, dz = (p[2] - tz) / cell - x2;
            const double dist = (dx * dx + dy * dy) + dz * dz;
            if (src < 0 || dist < best) best = dist, src = v;
        }
    }
    a.out_vertices[3 * (int64_t)j] = px, a.out_vertices[3 * (int64_t)j + 1] = py, a.out_vertices[3 * (int64_t)j + 2] = pz;
    a.source[j] = src;
    a.fell_back[j] = fell ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ entry points
#define K33_LIMIT ((int64_t)1 << 31)

extern "C" int gens_cluster_keys(const double* vertices, int64_t n_vertices, double origin_x, double origin_y, double origin_z, double cell,
                                 int64_t* keys, void* stream) {
    GENS_CHECK_ARG(n_vertices >= 0, GENS_EINVAL, "gens_cluster_keys: %lld vertices", (long long)n_vertices);
    GENS_CHECK_ARG(n_vertices < K33_LIMIT, GENS_ELIMIT, "gens_cluster_keys: %lld vertices (below 2^31)", (long long)n_vertices);
    GENS_CHECK_ARG(cell > 0.0 && isfinite(cell), GENS_EINVAL, "gens_cluster_keys: cell = %g (positive and finite)", cell);
    GENS_CHECK_ARG(isfinite(origin_x) && isfinite(origin_y) && isfinite(origin_z), GENS_EINVAL, "gens_cluster_keys: origin (%g, %g, %g) is not finite",
                   origin_x, origin_y, origin_z);
    if (n_vertices == 0) return 0;
    GENS_CHECK_ARG(vertices && keys, GENS_EINVAL, "gens_cluster_keys: null pointer");
    cluster_keys_k<<<gens_blocks(n_vertices, 256), 256, 0, (hipStream_t)stream>>>(vertices, (int)n_vertices, origin_x, origin_y, origin_z, cell, keys);
    return gens_launch_status("gens_cluster_keys");
}

extern "C" int gens_cluster_triangles(const int32_t* triangles, int64_t n_triangles, const int32_t* vertex_cluster, int64_t n_vertices, int32_t* ranks,
                                      uint8_t* survive, int32_t* triple, void* stream) {
    GENS_CHECK_ARG(n_triangles >= 0 && n_vertices >= 0, GENS_EINVAL, "gens_cluster_triangles: %lld triangles on %lld vertices", (long long)n_triangles,
                   (long long)n_vertices);
    GENS_CHECK_ARG(n_vertices < K33_LIMIT && n_triangles < K33_LIMIT / 3 + 1 && 3 * n_triangles < K33_LIMIT, GENS_ELIMIT,
                   "gens_cluster_triangles: %lld triangles on %lld vertices (V and 3 T below 2^31)", (long long)n_triangles, (long long)n_vertices);
    if (n_triangles == 0) return 0;
    GENS_CHECK_ARG(triangles && ranks && survive && triple, GENS_EINVAL, "gens_cluster_triangles: null pointer");
    GENS_CHECK_ARG(vertex_cluster || n_vertices == 0, GENS_EINVAL, "gens_cluster_triangles: null pointer (vertex_cluster, with %lld vertices)",
                   (long long)n_vertices);
    cluster_triangles_k<<<gens_blocks(n_triangles, 256), 256, 0, (hipStream_t)stream>>>(triangles, (int)n_triangles, vertex_cluster, (int)n_vertices, ranks,
                                                                                      survive, triple);
    return gens_launch_status("gens_cluster_triangles");
}

extern "C" int gens_cluster_solve(const gens_cluster_solve_args* g, void* stream) {
    GENS_CHECK_ARG(g, GENS_EINVAL, "gens_cluster_solve: null pointer (args)");
    GENS_CHECK_ARG(g->n_vertices >= 0 && g->n_triangles >= 0 && g->n_clusters >= 0 && g->n_out >= 0, GENS_EINVAL,
                   "gens_cluster_solve: %lld vertices, %lld triangles, %lld clusters, %lld output clusters", (long long)g->n_vertices,
                   (long long)g->n_triangles, (long long)g->n_clusters, (long long)g->n_out);
    GENS_CHECK_ARG(g->n_vertices < K33_LIMIT && g->n_triangles < K33_LIMIT / 3 + 1 && 3 * g->n_triangles < K33_LIMIT, GENS_ELIMIT,
                   "gens_cluster_solve: %lld triangles on %lld vertices (V and 3 T below 2^31)", (long long)g->n_triangles, (long long)g->n_vertices);
    GENS_CHECK_ARG(g->n_clusters <= g->n_vertices && g->n_out <= g->n_clusters, GENS_EINVAL,
                   "gens_cluster_solve: %lld output clusters of %lld clusters of %lld vertices (each at most the next)", (long long)g->n_out,
                   (long long)g->n_clusters, (long long)g->n_vertices);
    GENS_CHECK_ARG(g->cell > 0.0 && isfinite(g->cell), GENS_EINVAL, "gens_cluster_solve: cell = %g (positive and finite)", g->cell);
    GENS_CHECK_ARG(g->reg > 0.0 && isfinite(g->reg), GENS_EINVAL, "gens_cluster_solve: reg = %g (positive and finite)", g->reg);
    GENS_CHECK_ARG(isfinite(g->origin[0]) && isfinite(g->origin[1]) && isfinite(g->origin[2]), GENS_EINVAL,
                   "gens_cluster_solve: origin (%g, %g, %g) is not finite", g->origin[0], g->origin[1], g->origin[2]);
    if (g->n_out == 0) return 0;
    GENS_CHECK_ARG(g->vertices && g->cluster_keys && g->entry_start && g->members && g->member_start && g->out_clusters && g->out_vertices && g->source &&
                       g->fell_back,
                   GENS_EINVAL, "gens_cluster_solve: null pointer");
    GENS_CHECK_ARG(g->n_triangles == 0 || (g->triangles && g->survive && g->entries), GENS_EINVAL,
                   "gens_cluster_solve: null pointer (triangles, survive or entries, with %lld triangles)", (long long)g->n_triangles);
    SolveArgs a;
    a.vertices = g->vertices, a.triangles = g->triangles, a.survive = g->survive, a.cluster_keys = g->cluster_keys;
    a.entries = g->entries, a.entry_start = g->entry_start, a.members = g->members, a.member_start = g->member_start, a.out_clusters = g->out_clusters;
    a.n_vert = (int)g->n_vertices, a.n_tri = (int)g->n_triangles, a.n_clusters = (int)g->n_clusters, a.n_out = (int)g->n_out;
    a.ox = g->origin[0], a.oy = g->origin[1], a.oz = g->origin[2], a.cell = g->cell, a.reg = g->reg;
    a.out_vertices = g->out_vertices, a.source = g->source, a.fell_back = g->fell_back;
    cluster_solve_k<<<gens_blocks(g->n_out, 256), 256, 0, (hipStream_t)stream>>>(a);
    return gens_launch_status("gens_cluster_solve");
}
