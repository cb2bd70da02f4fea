// K39: mesh fairing -- Laplacian / Taubin smoothing of a triangle mesh with uniform or cotangent weights, the vertex Laplacian itself and the
// dihedral roughness of the edges (ops.smooth_mesh, ops.mesh_laplacian, ops.mesh_roughness, io.smooth_mesh, python -m gens_amd.smooth_mesh,
// ImplicitSurface.extract_geometry(smooth=)).  The rules are the comment of K39 in include/gens_hip.h; tests/mesh_smooth_reference.py restates
// them in numpy with dicts and loops.
//
// One thread per item (half-edge, edge, vertex), 256 per workgroup.  The neighbour lists come from one torch sort of K37's edges; the run of
// an edge's half-edges is K37's.  A segment (the uses of an edge, the neighbours of a vertex) is walked by ONE thread in stored order, so every
// float64 sum has one order: no atomics at all, the same bits on every run.  A step reads one buffer and writes another.  Every index read
// from memory is checked against its range before it is used as an address; what fails the check is skipped.  float64, every operation
// rounded on its own (no contraction).
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

__device__ __forceinline__ bool k39_face_valid(int32_t a, int32_t b, int32_t c, int64_t n_vertices) {
    return a >= 0 && b >= 0 && c >= 0 && a < n_vertices && b < n_vertices && c < n_vertices && a != b && b != c && c != a;
}

// ------------------------------------------------------------------------------------------------ weights
__global__ __launch_bounds__(256) void corner_cot_k(const double* __restrict__ vert, const int32_t* __restrict__ tri, int64_t n_vertices,
                                                    int64_t n_half, double* __restrict__ cot) {
    const int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (h >= n_half) return;
    const int64_t t = h / 3;
    const int k = (int)(h - 3 * t);
    const int32_t a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
    double out = 0.0;
    if (k39_face_valid(a, b, c, n_vertices)) {
        const int32_t iq = k == 0 ? a : k == 1 ? b : c, ir = k == 0 ? b : k == 1 ? c : a, ip = k == 0 ? c : k == 1 ? a : b;
        const double* __restrict__ P = vert + 3 * (int64_t)ip;
        const double* __restrict__ Q = vert + 3 * (int64_t)iq;
        const double* __restrict__ R = vert + 3 * (int64_t)ir;
        const double ux = Q[0] - P[0], uy = Q[1] - P[1], uz = Q[2] - P[2];
        const double vx = R[0] - P[0], vy = R[1] - P[1], vz = R[2] - P[2];
        const double d = (ux * vx + uy * vy) + uz * vz;
        const double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
        const double len = sqrt((cx * cx + cy * cy) + cz * cz);
        if (len > 0.0) {
            const double q = d / len;
            if (isfinite(q)) out = q;
        }
    }
    cot[h] = out;
}

__global__ __launch_bounds__(256) void edge_weights_k(const double* __restrict__ cot, const int32_t* __restrict__ edge_start,
                                                      const int32_t* __restrict__ order, int64_t n_edges, int64_t n_half,
                                                      double* __restrict__ weight) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges) return;
    int64_t s = edge_start[e], end = edge_start[e + 1];
    s = s < 0 ? 0 : s, end = end > n_half ? n_half : end;
    double w = 0.0;
    for (int64_t j = s; j < end; ++j) {
        const int32_t h = order[j];
        if (h < 0 || h >= n_half) continue;             // (a planted id: skipped, never read through)
        w = w + cot[h];
    }
    weight[e] = w > 0.0 ? w : 0.0;                      // (negatives and NaN: 0, so that every step is a convex combination)
}

// ------------------------------------------------------------------------------------------------ the Laplacian and a step
// in and out differ (the entry point refuses the same pointer), so a neighbour's position is never one that this launch wrote
__global__ __launch_bounds__(256) void laplacian_step_k(const double* __restrict__ in, int64_t n_vertices, const int32_t* __restrict__ nbr_start,
                                                        const int32_t* __restrict__ nbr_vertex, const int32_t* __restrict__ nbr_edge,
                                                        int64_t n_nbr, const double* __restrict__ weight, int64_t n_edges,
                                                        const uint8_t* __restrict__ pinned, double factor, double* __restrict__ out,
                                                        double* __restrict__ delta, double* __restrict__ weight_sum) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_vertices) return;
    int64_t s = nbr_start[i], end = nbr_start[i + 1];
    s = s < 0 ? 0 : s, end = end > n_nbr ? n_nbr : end;
    const double px = in[3 * i], py = in[3 * i + 1], pz = in[3 * i + 2];
    double sx = 0.0, sy = 0.0, sz = 0.0, wsum = 0.0;
    for (int64_t j = s; j < end; ++j) {
        const int32_t nb = nbr_vertex[j];
        if (nb < 0 || nb >= n_vertices) continue;
        double w = 1.0;
        if (weight) {
            const int32_t e = nbr_edge[j];
            if (e < 0 || e >= n_edges) continue;
            w = weight[e];
        }
        const double* __restrict__ q = in + 3 * (int64_t)nb;
        wsum = wsum + w;
        sx = sx + w * (q[0] - px), sy = sy + w * (q[1] - py), sz = sz + w * (q[2] - pz);
    }
    const bool has = wsum > 0.0 && isfinite(wsum);
    const double dx = has ? sx / wsum : 0.0, dy = has ? sy / wsum : 0.0, dz = has ? sz / wsum : 0.0;
    if (delta) delta[3 * i] = dx, delta[3 * i + 1] = dy, delta[3 * i + 2] = dz;
    if (weight_sum) weight_sum[i] = wsum;
    if (out) {
        const bool stay = !has || (pinned && pinned[i] != 0);           // (a vertex that stays keeps its bits, a -0.0 included)
        out[3 * i] = stay ? px : px + factor * dx;
        out[3 * i + 1] = stay ? py : py + factor * dy;
        out[3 * i + 2] = stay ? pz : pz + factor * dz;
    }
}

// ------------------------------------------------------------------------------------------------ dihedral roughness
__global__ __launch_bounds__(256) void dihedral_k(const double* __restrict__ face_normal, int64_t n_faces, const int32_t* __restrict__ edge_halfedges,
                                                  const uint8_t* __restrict__ edge_class, int64_t n_edges, double* __restrict__ angle) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges) return;
    double out = NAN;
    const int32_t h0 = edge_halfedges[2 * e], h1 = edge_halfedges[2 * e + 1];
    if (edge_class[e] == 2 && h0 >= 0 && h1 >= 0 && h0 < 3 * n_faces && h1 < 3 * n_faces) {
        const double* __restrict__ a = face_normal + 3 * (int64_t)(h0 / 3);
        const double* __restrict__ b = face_normal + 3 * (int64_t)(h1 / 3);
        const double ax = a[0], ay = a[1], az = a[2], bx = b[0], by = b[1], bz = b[2];
        if ((ax != 0.0 || ay != 0.0 || az != 0.0) && (bx != 0.0 || by != 0.0 || bz != 0.0)) {
            const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
            out = atan2(sqrt((cx * cx + cy * cy) + cz * cz), (ax * bx + ay * by) + az * bz);
        }
    }
    angle[e] = out;
}

// ------------------------------------------------------------------------------------------------ entry points
#define K39_LIMIT ((int64_t)1 << 31)

extern "C" int gens_mesh_corner_cot(const double* vertices, const int32_t* triangles, int64_t n_vertices, int64_t n_faces, double* cot,
                                    void* stream) {
    const char* who = "gens_mesh_corner_cot";
    GENS_CHECK_ARG(n_faces >= 0 && n_vertices >= 0, GENS_EINVAL, "%s: %lld faces over %lld vertices", who, (long long)n_faces, (long long)n_vertices);
    GENS_CHECK_ARG(n_vertices < K39_LIMIT && n_faces < K39_LIMIT / 3 + 1 && 3 * n_faces < K39_LIMIT, GENS_ELIMIT,
                   "%s: %lld faces over %lld vertices (V and 3 T below 2^31)", who, (long long)n_faces, (long long)n_vertices);
    if (n_faces == 0) return 0;
    GENS_CHECK_ARG(triangles && cot && (vertices || n_vertices == 0), GENS_EINVAL, "%s: null pointer", who);
    corner_cot_k<<<gens_blocks(3 * n_faces, 256), 256, 0, (hipStream_t)stream>>>(vertices, triangles, n_vertices, 3 * n_faces, cot);
    return gens_launch_status(who);
}

extern "C" int gens_mesh_edge_weights(const double* cot, const int32_t* edge_start, const int32_t* halfedge_order, int64_t n_edges,
                                      int64_t n_halfedges, double* weight, void* stream) {
    const char* who = "gens_mesh_edge_weights";
    GENS_CHECK_ARG(n_edges >= 0 && n_halfedges >= 0, GENS_EINVAL, "%s: %lld edges over %lld half-edges", who, (long long)n_edges,
                   (long long)n_halfedges);
    GENS_CHECK_ARG(n_halfedges < K39_LIMIT, GENS_ELIMIT, "%s: %lld half-edges (3 T below 2^31)", who, (long long)n_halfedges);
    GENS_CHECK_ARG(n_halfedges % 3 == 0, GENS_EINVAL, "%s: %lld half-edges (three per face)", who, (long long)n_halfedges);
    GENS_CHECK_ARG(n_edges <= n_halfedges, GENS_EINVAL, "%s: %lld edges over %lld half-edges (an edge has a use)", who, (long long)n_edges,
                   (long long)n_halfedges);
    if (n_edges == 0) return 0;
    GENS_CHECK_ARG(cot && edge_start && halfedge_order && weight, GENS_EINVAL, "%s: null pointer", who);
    edge_weights_k<<<gens_blocks(n_edges, 256), 256, 0, (hipStream_t)stream>>>(cot, edge_start, halfedge_order, n_edges, n_halfedges, weight);
    return gens_launch_status(who);
}

extern "C" int gens_mesh_laplacian_step(const double* in, int64_t n_vertices, const int32_t* nbr_start, const int32_t* nbr_vertex,
                                        const int32_t* nbr_edge, int64_t n_neighbours, const double* weight, int64_t n_edges,
                                        const uint8_t* pinned, double factor, double* out, double* delta, double* weight_sum, void* stream) {
    const char* who = "gens_mesh_laplacian_step";
    GENS_CHECK_ARG(n_vertices >= 0 && n_neighbours >= 0 && n_edges >= 0, GENS_EINVAL, "%s: %lld vertices, %lld neighbours, %lld edges", who,
                   (long long)n_vertices, (long long)n_neighbours, (long long)n_edges);
    GENS_CHECK_ARG(n_vertices < K39_LIMIT && n_neighbours < K39_LIMIT, GENS_ELIMIT, "%s: %lld vertices, %lld neighbours (V and 2 E below 2^31)", who,
                   (long long)n_vertices, (long long)n_neighbours);
    GENS_CHECK_ARG(n_neighbours == 2 * n_edges, GENS_EINVAL, "%s: %lld neighbours over %lld edges (an edge has two ends)", who,
                   (long long)n_neighbours, (long long)n_edges);
    GENS_CHECK_ARG(factor == factor && factor >= -2.0 && factor <= 1.0, GENS_EINVAL, "%s: factor %g (-2 to 1)", who, factor);
    if (n_vertices == 0) return 0;
    GENS_CHECK_ARG(in && nbr_start, GENS_EINVAL, "%s: null pointer", who);
    if (n_neighbours > 0) GENS_CHECK_ARG(nbr_vertex && nbr_edge, GENS_EINVAL, "%s: null pointer (neighbours)", who);
    GENS_CHECK_ARG(out || delta || weight_sum, GENS_EINVAL, "%s: no output", who);
    GENS_CHECK_ARG(out != in && delta != in && weight_sum != (const double*)in, GENS_EINVAL,
                   "%s: a step reads one buffer and writes another (out == in)", who);
    GENS_CHECK_ARG((!out || (out != delta && out != weight_sum)) && (!delta || delta != weight_sum), GENS_EINVAL,
                   "%s: two outputs share a buffer", who);
    laplacian_step_k<<<gens_blocks(n_vertices, 256), 256, 0, (hipStream_t)stream>>>(in, n_vertices, nbr_start, nbr_vertex, nbr_edge, n_neighbours,
                                                                                   weight, n_edges, pinned, factor, out, delta, weight_sum);
    return gens_launch_status(who);
}

extern "C" int gens_mesh_dihedral(const double* face_normal, int64_t n_faces, const int32_t* edge_halfedges, const uint8_t* edge_class,
                                  int64_t n_edges, double* angle, void* stream) {
    const char* who = "gens_mesh_dihedral";
    GENS_CHECK_ARG(n_faces >= 0 && n_edges >= 0, GENS_EINVAL, "%s: %lld edges over %lld faces", who, (long long)n_edges, (long long)n_faces);
    GENS_CHECK_ARG(n_faces < K39_LIMIT / 3 + 1 && 3 * n_faces < K39_LIMIT, GENS_ELIMIT, "%s: %lld faces (3 T below 2^31)", who, (long long)n_faces);
    GENS_CHECK_ARG(n_edges <= 3 * n_faces, GENS_EINVAL, "%s: %lld edges over %lld faces (an edge has a use)", who, (long long)n_edges,
                   (long long)n_faces);
    if (n_edges == 0) return 0;
    GENS_CHECK_ARG(face_normal && edge_halfedges && edge_class && angle, GENS_EINVAL, "%s: null pointer", who);
    dihedral_k<<<gens_blocks(n_edges, 256), 256, 0, (hipStream_t)stream>>>(face_normal, n_faces, edge_halfedges, edge_class, n_edges, angle);
    return gens_launch_status(who);
}
