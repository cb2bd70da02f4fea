// K37: the undirected edge table of a triangle mesh, its classification, the vertex fans, Baerentzen-Aanaes pseudonormals and the sign of
// K36's distance (ops.mesh_topology, ops.signed_distance_to_mesh, ops.mesh_distance(signed=True), io.mesh_report,
// python -m gens_amd.mesh_report, ImplicitSurface.extract_geometry(topology=)).  The definitions are the comment of K37 in
// include/gens_hip.h; tests/mesh_topology_reference.py restates them in numpy with dicts and loops.
//
// One thread per item (half-edge, edge, vertex, face, query), 256 per workgroup.  The sorts (half-edges by edge key, corners by vertex), the
// run lengths and their prefix sums stay in torch, as K33's do; the kernels here write the keys and walk the sorted segments.  A segment is
// walked by ONE thread in stored order -- a stable sort leaves a segment's half-edges / corners in ascending id -- so every count, every
// "first two" and every float64 sum has one order: no atomics on doubles, the same bits on every run.  The union of corners into fans goes
// through K23's gens_face_cc_hook / gens_face_cc_compress (roots are smallest members, so labels do not depend on the atomics' order).
// Every index read from memory is checked against its range before it is used as an address; what fails the check is skipped.
// All state is named scalars: no scratch.  float64, every operation rounded on its own (no contraction).
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

#define K37_SENTINEL INT64_MAX          // the key of a half-edge of an invalid face: sorts after every (lo << 32) | hi
#define K37_NO_SIGN_FLAGS 0x1E          // vertex flag bits 1 .. 4: on a boundary, non-manifold or flipped edge, or pinched

__device__ __forceinline__ bool face_valid(int32_t a, int32_t b, int32_t c, int64_t n_vertices) {
    return a >= 0 && b >= 0 && c >= 0 && a < n_vertices && b < n_vertices && c < n_vertices && a != b && b != c && c != a;
}

// ------------------------------------------------------------------------------------------------ edge keys
__global__ __launch_bounds__(256) void edge_keys_k(const int32_t* __restrict__ tri, int64_t n_half, int64_t n_vertices, int64_t* __restrict__ key,
                                                   uint8_t* __restrict__ forward) {
    const int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (h >= n_half) return;
    const int64_t t = h / 3;
    const int k = (int)(h - 3 * t);
    const int32_t a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
    int64_t out = K37_SENTINEL;
    uint8_t fwd = 0;
    if (face_valid(a, b, c, n_vertices)) {
        const int32_t from = k == 0 ? a : k == 1 ? b : c, to = k == 0 ? b : k == 1 ? c : a;
        const int32_t lo = from < to ? from : to, hi = from < to ? to : from;
        out = ((int64_t)lo << 32) | (int64_t)hi;
        fwd = from < to ? 1 : 0;
    }
    key[h] = out;
    forward[h] = fwd;
}

// ------------------------------------------------------------------------------------------------ edge classes
__global__ __launch_bounds__(256) void fill_i32_k(int32_t* __restrict__ p, int64_t n, int32_t value) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = value;
}

__global__ __launch_bounds__(256) void edge_classify_k(const int64_t* __restrict__ edge_key, const int32_t* __restrict__ seg_start,
                                                       const int32_t* __restrict__ order, const uint8_t* __restrict__ forward, int64_t n_edges,
                                                       int64_t n_half, int32_t* __restrict__ edges, int32_t* __restrict__ edge_count,
                                                       int32_t* __restrict__ edge_forward, int32_t* __restrict__ edge_halfedges,
                                                       uint8_t* __restrict__ edge_class, int32_t* __restrict__ edge_of_halfedge) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges) return;
    const int64_t key = edge_key[e];
    int64_t s = seg_start[e], end = seg_start[e + 1];
    s = s < 0 ? 0 : s, end = end > n_half ? n_half : end;
    int32_t count = 0, fwd = 0, h0 = -1, h1 = -1;
    for (int64_t j = s; j < end; ++j) {
        const int32_t h = order[j];
        if (h < 0 || h >= n_half) continue;             // (a planted id: skipped, never read through)
        edge_of_halfedge[h] = (int32_t)e;
        fwd += forward[h] ? 1 : 0;
        if (count == 0) h0 = h;
        if (count == 1) h1 = h;
        ++count;
    }
    edges[2 * e] = (int32_t)(key >> 32);
    edges[2 * e + 1] = (int32_t)(key & 0xffffffffll);
    edge_count[e] = count;
    edge_forward[e] = fwd;
    edge_halfedges[2 * e] = h0;
    edge_halfedges[2 * e + 1] = h1;
    edge_class[e] = count == 0 ? 0 : count == 1 ? 1 : count > 2 ? 4 : fwd == 1 ? 2 : 3;
}

// ------------------------------------------------------------------------------------------------ fans
// the corner id that face t has at vertex v, -1 if none
__device__ __forceinline__ int32_t corner_at(const int32_t* __restrict__ tri, int64_t t, int32_t v) {
    return tri[3 * t] == v ? (int32_t)(3 * t) : tri[3 * t + 1] == v ? (int32_t)(3 * t + 1) : tri[3 * t + 2] == v ? (int32_t)(3 * t + 2) : -1;
}

__global__ __launch_bounds__(256) void fan_pairs_k(const int32_t* __restrict__ tri, int64_t n_faces, const int32_t* __restrict__ edges,
                                                   const int32_t* __restrict__ edge_halfedges, const uint8_t* __restrict__ edge_class,
                                                   int64_t n_edges, int32_t* __restrict__ pairs) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges) return;
    int32_t p0 = -1, p1 = -1, p2 = -1, p3 = -1;
    const uint8_t cls = edge_class[e];
    const int32_t h0 = edge_halfedges[2 * e], h1 = edge_halfedges[2 * e + 1];
    if ((cls == 2 || cls == 3) && h0 >= 0 && h1 >= 0 && h0 < 3 * n_faces && h1 < 3 * n_faces) {
        const int64_t t0 = h0 / 3, t1 = h1 / 3;
        const int32_t lo = edges[2 * e], hi = edges[2 * e + 1];
        p0 = corner_at(tri, t0, lo), p1 = corner_at(tri, t1, lo);
        p2 = corner_at(tri, t0, hi), p3 = corner_at(tri, t1, hi);
    }
    // a pair with a corner that was not found joins nothing (gens_face_cc_hook skips ids below zero)
    pairs[4 * e] = p0, pairs[4 * e + 1] = p0 < 0 ? -1 : p1;
    pairs[4 * e + 2] = p2, pairs[4 * e + 3] = p2 < 0 ? -1 : p3;
}

// ------------------------------------------------------------------------------------------------ vertex classes
__global__ __launch_bounds__(256) void vertex_classify_k(const int32_t* __restrict__ corner_order, const int32_t* __restrict__ corner_start,
                                                         const int32_t* __restrict__ corner_label, const int32_t* __restrict__ edge_of_halfedge,
                                                         const uint8_t* __restrict__ edge_class, int64_t n_vertices, int64_t n_half, int64_t n_edges,
                                                         int32_t* __restrict__ valence, int32_t* __restrict__ fans, uint8_t* __restrict__ flags) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_vertices) return;
    int64_t s = corner_start[v], end = corner_start[v + 1];
    s = s < 0 ? 0 : s, end = end > n_half ? n_half : end;
    int32_t val = 0, roots = 0;
    unsigned bits = 0;
    for (int64_t j = s; j < end; ++j) {
        const int32_t c = corner_order[j];
        if (c < 0 || c >= n_half) continue;
        ++val;
        roots += corner_label[c] == c ? 1 : 0;          // a fan's label is its smallest corner, which lies in this segment: one root per fan
        const int32_t t3 = c - c % 3, k = c % 3;
        const int32_t e_out = edge_of_halfedge[c], e_in = edge_of_halfedge[t3 + (k + 2) % 3];
        if (e_out >= 0 && e_out < n_edges) {
            const uint8_t cls = edge_class[e_out];
            bits |= cls == 1 ? 2u : cls == 4 ? 4u : cls == 3 ? 8u : 0u;
        }
        if (e_in >= 0 && e_in < n_edges) {
            const uint8_t cls = edge_class[e_in];
            bits |= cls == 1 ? 2u : cls == 4 ? 4u : cls == 3 ? 8u : 0u;
        }
    }
    if (val > 0) bits |= 1u;
    if (roots > 1) bits |= 16u;
    valence[v] = val;
    fans[v] = roots;
    flags[v] = (uint8_t)bits;
}

// ------------------------------------------------------------------------------------------------ pseudonormals
__global__ __launch_bounds__(256) void face_normals_k(const double* __restrict__ vert, const int32_t* __restrict__ tri, int64_t n_vertices,
                                                      int64_t n_faces, double* __restrict__ face_normal) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_faces) return;
    const int32_t ia = tri[3 * t], ib = tri[3 * t + 1], ic = tri[3 * t + 2];
    double nx = 0.0, ny = 0.0, nz = 0.0;
    if (face_valid(ia, ib, ic, n_vertices)) {
        const double* __restrict__ A = vert + 3 * (int64_t)ia;
        const double* __restrict__ B = vert + 3 * (int64_t)ib;
        const double* __restrict__ Cc = vert + 3 * (int64_t)ic;
        const double ux = B[0] - A[0], uy = B[1] - A[1], uz = B[2] - A[2];
        const double vx = Cc[0] - A[0], vy = Cc[1] - A[1], vz = Cc[2] - A[2];
        const double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
        const double len = sqrt((cx * cx + cy * cy) + cz * cz);
        if (len > 0.0 && isfinite(len)) nx = cx / len, ny = cy / len, nz = cz / len;
    }
    face_normal[3 * t] = nx, face_normal[3 * t + 1] = ny, face_normal[3 * t + 2] = nz;
}

__global__ __launch_bounds__(256) void edge_normals_k(const int32_t* __restrict__ seg_start, const int32_t* __restrict__ order, int64_t n_edges,
                                                      int64_t n_half, const double* __restrict__ face_normal, double* __restrict__ edge_normal) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges) return;
    int64_t s = seg_start[e], end = seg_start[e + 1];
    s = s < 0 ? 0 : s, end = end > n_half ? n_half : end;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int64_t j = s; j < end; ++j) {
        const int32_t h = order[j];
        if (h < 0 || h >= n_half) continue;
        const double* __restrict__ n = face_normal + 3 * (int64_t)(h / 3);
        sx = sx + n[0], sy = sy + n[1], sz = sz + n[2];
    }
    edge_normal[3 * e] = sx, edge_normal[3 * e + 1] = sy, edge_normal[3 * e + 2] = sz;
}

__global__ __launch_bounds__(256) void vertex_normals_k(const double* __restrict__ vert, const int32_t* __restrict__ tri, int64_t n_vertices,
                                                        int64_t n_half, const int32_t* __restrict__ corner_start,
                                                        const int32_t* __restrict__ corner_order, const double* __restrict__ face_normal,
                                                        double* __restrict__ vertex_normal) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_vertices) return;
    int64_t s = corner_start[v], end = corner_start[v + 1];
    s = s < 0 ? 0 : s, end = end > n_half ? n_half : end;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int64_t j = s; j < end; ++j) {
        const int32_t c = corner_order[j];
        if (c < 0 || c >= n_half) continue;
        const int32_t t3 = c - c % 3, k = c % 3;
        const int32_t i0 = tri[c], i1 = tri[t3 + (k + 1) % 3], i2 = tri[t3 + (k + 2) % 3];
        if (!face_valid(i0, i1, i2, n_vertices)) continue;
        const double* __restrict__ P = vert + 3 * (int64_t)i0;
        const double* __restrict__ Q = vert + 3 * (int64_t)i1;
        const double* __restrict__ R = vert + 3 * (int64_t)i2;
        const double ux = Q[0] - P[0], uy = Q[1] - P[1], uz = Q[2] - P[2];
        const double vx = R[0] - P[0], vy = R[1] - P[1], vz = R[2] - P[2];
        const double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
        const double angle = atan2(sqrt((cx * cx + cy * cy) + cz * cz), (ux * vx + uy * vy) + uz * vz);
        const double* __restrict__ n = face_normal + 3 * (int64_t)(c / 3);
        if (!isfinite(angle)) continue;
        sx = sx + angle * n[0], sy = sy + angle * n[1], sz = sz + angle * n[2];
    }
    vertex_normal[3 * v] = sx, vertex_normal[3 * v + 1] = sy, vertex_normal[3 * v + 2] = sz;
}

// ------------------------------------------------------------------------------------------------ the sign
struct SignMesh {
    const int32_t* triangles;
    const double *face_normal, *edge_normal, *vertex_normal;
    const int32_t* edge_of_halfedge;
    const uint8_t *edge_class, *vertex_flags;
    int64_t n_faces, n_vertices, n_edges;
};

__global__ __launch_bounds__(256) void distance_sign_k(SignMesh m, const double* __restrict__ queries, int64_t n, const double* __restrict__ dist2,
                                                       const int32_t* __restrict__ face, const double* __restrict__ point,
                                                       const uint8_t* __restrict__ region, double* __restrict__ signed_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double d2 = dist2[i];
    const int32_t f = face[i];
    const int r = region[i];
    double out = NAN;
    if (f >= 0 && f < m.n_faces && d2 >= 0.0 && isfinite(d2)) {
        if (d2 == 0.0) {
            out = 0.0;
        } else if (r <= 6) {
            const double* __restrict__ nrm = nullptr;
            if (r == 0) {
                nrm = m.face_normal + 3 * (int64_t)f;
            } else if (r <= 3) {
                const int32_t v = m.triangles[3 * (int64_t)f + (r - 1)];
                if (v >= 0 && v < m.n_vertices && (m.vertex_flags[v] & K37_NO_SIGN_FLAGS) == 0) nrm = m.vertex_normal + 3 * (int64_t)v;
            } else {
                const int32_t e = m.edge_of_halfedge[3 * (int64_t)f + (r - 4)];
                if (e >= 0 && e < m.n_edges && m.edge_class[e] == 2) nrm = m.edge_normal + 3 * (int64_t)e;
            }
            if (nrm) {
                const double ux = queries[3 * i] - point[3 * i], uy = queries[3 * i + 1] - point[3 * i + 1], uz = queries[3 * i + 2] - point[3 * i + 2];
                const double dot = (ux * nrm[0] + uy * nrm[1]) + uz * nrm[2];
                const double d = sqrt(d2);
                if (dot > 0.0) out = d;
                if (dot < 0.0) out = -d;                // (dot == 0 or NaN: no sign)
            }
        }
    }
    signed_out[i] = out;
}

// ------------------------------------------------------------------------------------------------ entry points
#define K37_LIMIT ((int64_t)1 << 31)
#define K37_CHECK_MESH(who, n_faces, n_vertices)                                                                                     \
    GENS_CHECK_ARG((n_faces) >= 0 && (n_vertices) >= 0, GENS_EINVAL, "%s: %lld faces over %lld vertices", who, (long long)(n_faces), \
                   (long long)(n_vertices));                                                                                         \
    GENS_CHECK_ARG((n_vertices) < K37_LIMIT && 3 * (int64_t)(n_faces) < K37_LIMIT, GENS_ELIMIT,                                     \
                   "%s: %lld faces over %lld vertices (V and 3 T below 2^31)", who, (long long)(n_faces), (long long)(n_vertices))

extern "C" int gens_mesh_edge_keys(const int32_t* triangles, int64_t n_faces, int64_t n_vertices, int64_t* key, uint8_t* forward, void* stream) {
    const char* who = "gens_mesh_edge_keys";
    K37_CHECK_MESH(who, n_faces, n_vertices);
    if (n_faces == 0) return 0;
    GENS_CHECK_ARG(triangles && key && forward, GENS_EINVAL, "%s: null pointer", who);
    edge_keys_k<<<gens_blocks(3 * n_faces, 256), 256, 0, (hipStream_t)stream>>>(triangles, 3 * n_faces, n_vertices, key, forward);
    return gens_launch_status(who);
}

extern "C" int gens_mesh_edge_classify(const int64_t* edge_key, const int32_t* seg_start, const int32_t* order, const uint8_t* forward,
                                       int64_t n_edges, int64_t n_halfedges, int32_t* edges, int32_t* edge_count, int32_t* edge_forward,
                                       int32_t* edge_halfedges, uint8_t* edge_class, int32_t* edge_of_halfedge, void* stream) {
    const char* who = "gens_mesh_edge_classify";
    GENS_CHECK_ARG(n_edges >= 0 && n_halfedges >= 0, GENS_EINVAL, "%s: %lld edges over %lld half-edges", who, (long long)n_edges, (long long)n_halfedges);
    GENS_CHECK_ARG(n_halfedges < K37_LIMIT, GENS_ELIMIT, "%s: %lld half-edges (3 T below 2^31)", who, (long long)n_halfedges);
    GENS_CHECK_ARG(n_halfedges % 3 == 0, GENS_EINVAL, "%s: %lld half-edges (three per face)", who, (long long)n_halfedges);
    GENS_CHECK_ARG(n_edges <= n_halfedges, GENS_EINVAL, "%s: %lld edges over %lld half-edges (an edge has a use)", who, (long long)n_edges,
                   (long long)n_halfedges);
    if (n_halfedges == 0) return 0;
    GENS_CHECK_ARG(edge_of_halfedge, GENS_EINVAL, "%s: null pointer (edge_of_halfedge)", who);
    if (n_edges > 0)
        GENS_CHECK_ARG(edge_key && seg_start && order && forward && edges && edge_count && edge_forward && edge_halfedges && edge_class, GENS_EINVAL,
                       "%s: null pointer", who);
    fill_i32_k<<<gens_blocks(n_halfedges, 256), 256, 0, (hipStream_t)stream>>>(edge_of_halfedge, n_halfedges, -1);
    if (n_edges > 0)
        edge_classify_k<<<gens_blocks(n_edges, 256), 256, 0, (hipStream_t)stream>>>(edge_key, seg_start, order, forward, n_edges, n_halfedges, edges,
                                                                                   edge_count, edge_forward, edge_halfedges, edge_class,
                                                                                   edge_of_halfedge);
    return gens_launch_status(who);
}

extern "C" int gens_mesh_fan_pairs(const int32_t* triangles, int64_t n_faces, const int32_t* edges, const int32_t* edge_halfedges,
                                   const uint8_t* edge_class, int64_t n_edges, int32_t* pairs, void* stream) {
    const char* who = "gens_mesh_fan_pairs";
    GENS_CHECK_ARG(n_faces >= 0 && n_edges >= 0, GENS_EINVAL, "%s: %lld edges over %lld faces", who, (long long)n_edges, (long long)n_faces);
    GENS_CHECK_ARG(3 * n_faces < K37_LIMIT, GENS_ELIMIT, "%s: %lld faces (3 T below 2^31)", who, (long long)n_faces);
    GENS_CHECK_ARG(n_edges <= 3 * n_faces, GENS_EINVAL, "%s: %lld edges over %lld faces (an edge has a use)", who, (long long)n_edges, (long long)n_faces);
    if (n_edges == 0) return 0;
    GENS_CHECK_ARG(triangles && edges && edge_halfedges && edge_class && pairs, GENS_EINVAL, "%s: null pointer", who);
    fan_pairs_k<<<gens_blocks(n_edges, 256), 256, 0, (hipStream_t)stream>>>(triangles, n_faces, edges, edge_halfedges, edge_class, n_edges, pairs);
    return gens_launch_status(who);
}

extern "C" int gens_mesh_vertex_classify(const int32_t* corner_order, const int32_t* corner_start, const int32_t* corner_label,
                                         const int32_t* edge_of_halfedge, const uint8_t* edge_class, int64_t n_vertices, int64_t n_halfedges,
                                         int64_t n_edges, int32_t* valence, int32_t* fans, uint8_t* flags, void* stream) {
    const char* who = "gens_mesh_vertex_classify";
    GENS_CHECK_ARG(n_vertices >= 0 && n_halfedges >= 0 && n_edges >= 0, GENS_EINVAL, "%s: %lld vertices, %lld half-edges, %lld edges", who,
                   (long long)n_vertices, (long long)n_halfedges, (long long)n_edges);
    GENS_CHECK_ARG(n_vertices < K37_LIMIT && n_halfedges < K37_LIMIT, GENS_ELIMIT, "%s: %lld vertices, %lld half-edges (V and 3 T below 2^31)", who,
                   (long long)n_vertices, (long long)n_halfedges);
    GENS_CHECK_ARG(n_halfedges % 3 == 0 && n_edges <= n_halfedges, GENS_EINVAL, "%s: %lld half-edges (three per face), %lld edges (an edge has a use)",
                   who, (long long)n_halfedges, (long long)n_edges);
    if (n_vertices == 0) return 0;
    GENS_CHECK_ARG(corner_start && valence && fans && flags, GENS_EINVAL, "%s: null pointer", who);
    if (n_halfedges > 0) GENS_CHECK_ARG(corner_order && corner_label && edge_of_halfedge, GENS_EINVAL, "%s: null pointer (corners)", who);
    if (n_edges > 0) GENS_CHECK_ARG(edge_class, GENS_EINVAL, "%s: null pointer (edge_class)", who);
    vertex_classify_k<<<gens_blocks(n_vertices, 256), 256, 0, (hipStream_t)stream>>>(corner_order, corner_start, corner_label, edge_of_halfedge,
                                                                                    edge_class, n_vertices, n_halfedges, n_edges, valence, fans,
                                                                                    flags);
    return gens_launch_status(who);
}

extern "C" int gens_mesh_pseudonormals(const double* vertices, const int32_t* triangles, int64_t n_vertices, int64_t n_faces, int64_t n_edges,
                                       const int32_t* seg_start, const int32_t* order, const int32_t* corner_start, const int32_t* corner_order,
                                       double* face_normal, double* edge_normal, double* vertex_normal, void* stream) {
    const char* who = "gens_mesh_pseudonormals";
    K37_CHECK_MESH(who, n_faces, n_vertices);
    GENS_CHECK_ARG(n_edges >= 0 && n_edges <= 3 * n_faces, GENS_EINVAL, "%s: %lld edges over %lld faces (an edge has a use)", who, (long long)n_edges,
                   (long long)n_faces);
    if (n_vertices == 0 && n_faces == 0) return 0;
    if (n_vertices > 0) GENS_CHECK_ARG(corner_start && vertex_normal, GENS_EINVAL, "%s: null pointer (vertices' outputs)", who);
    if (n_faces > 0) GENS_CHECK_ARG(vertices && triangles && corner_order && face_normal, GENS_EINVAL, "%s: null pointer (faces)", who);
    if (n_edges > 0) GENS_CHECK_ARG(seg_start && order && edge_normal, GENS_EINVAL, "%s: null pointer (edges)", who);
    const hipStream_t st = (hipStream_t)stream;
    if (n_faces > 0) face_normals_k<<<gens_blocks(n_faces, 256), 256, 0, st>>>(vertices, triangles, n_vertices, n_faces, face_normal);
    if (n_edges > 0) edge_normals_k<<<gens_blocks(n_edges, 256), 256, 0, st>>>(seg_start, order, n_edges, 3 * n_faces, face_normal, edge_normal);
    if (n_vertices > 0)
        vertex_normals_k<<<gens_blocks(n_vertices, 256), 256, 0, st>>>(vertices, triangles, n_vertices, 3 * n_faces, corner_start, corner_order,
                                                                      face_normal, vertex_normal);
    return gens_launch_status(who);
}

extern "C" int gens_mesh_distance_sign(const double* queries, int64_t n_queries, const double* dist2, const int32_t* face, const double* point,
                                       const uint8_t* region, const int32_t* triangles, int64_t n_faces, int64_t n_vertices, int64_t n_edges,
                                       const double* face_normal, const double* edge_normal, const double* vertex_normal,
                                       const int32_t* edge_of_halfedge, const uint8_t* edge_class, const uint8_t* vertex_flags, double* signed_out,
                                       void* stream) {
    const char* who = "gens_mesh_distance_sign";
    GENS_CHECK_ARG(n_queries >= 0, GENS_EINVAL, "%s: %lld queries", who, (long long)n_queries);
    GENS_CHECK_ARG(n_queries < K37_LIMIT, GENS_ELIMIT, "%s: %lld queries (below 2^31)", who, (long long)n_queries);
    K37_CHECK_MESH(who, n_faces, n_vertices);
    GENS_CHECK_ARG(n_edges >= 0 && n_edges <= 3 * n_faces, GENS_EINVAL, "%s: %lld edges over %lld faces (an edge has a use)", who, (long long)n_edges,
                   (long long)n_faces);
    if (n_queries == 0) return 0;
    GENS_CHECK_ARG(queries && dist2 && face && point && region && signed_out, GENS_EINVAL, "%s: null pointer (per query)", who);
    if (n_faces > 0)
        GENS_CHECK_ARG(triangles && face_normal && edge_of_halfedge, GENS_EINVAL, "%s: null pointer (faces)", who);
    if (n_faces > 0 && n_vertices > 0) GENS_CHECK_ARG(vertex_normal && vertex_flags, GENS_EINVAL, "%s: null pointer (vertices)", who);
    if (n_edges > 0) GENS_CHECK_ARG(edge_normal && edge_class, GENS_EINVAL, "%s: null pointer (edges)", who);
    SignMesh m;
    m.triangles = triangles, m.face_normal = face_normal, m.edge_normal = edge_normal, m.vertex_normal = vertex_normal;
    m.edge_of_halfedge = edge_of_halfedge, m.edge_class = edge_class, m.vertex_flags = vertex_flags;
    m.n_faces = n_faces, m.n_vertices = n_vertices, m.n_edges = n_edges;
    distance_sign_k<<<gens_blocks(n_queries, 256), 256, 0, (hipStream_t)stream>>>(m, queries, n_queries, dist2, face, point, region, signed_out);
    return gens_launch_status(who);
}
