// K38: mesh repair -- drop invalid and duplicate faces, split every vertex into its fans, drop small components, re-orient every orientable
// component by majority and close small boundary loops (ops.repair_mesh, io.repair_mesh, python -m gens_amd.repair_mesh,
// ImplicitSurface.extract_geometry(repair=)).  The rules are the comment of K38 in include/gens_hip.h; tests/mesh_repair_reference.py restates
// them in numpy with dicts and loops.
//
// The kernels turn K37's tables into a new mesh: one thread per item (face, vertex, edge, loop, boundary half-edge), 256 per workgroup.  The
// sorts, run lengths and prefix sums stay in torch, the unions go through K23's gens_face_cc_hook / gens_face_cc_compress, as in K37.  A
// segment (the corners of a vertex, the vertices of a loop) is walked by ONE thread in stored order, so every rank and every float64 sum has
// one order: no atomics at all, the same bits on every run.  Every index read from memory is checked against its range before it is used as
// an address; what fails the check is skipped.  float64, every operation rounded on its own (no contraction).
#include "common.h"

#pragma clang fp contract(off)

#define K38_SENTINEL INT64_MAX          // both keys of a face that is not valid: sorts after every real key

__global__ __launch_bounds__(256) void k38_fill_i32_k(int32_t* __restrict__ p, int64_t n, int32_t value) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = value;
}

// ------------------------------------------------------------------------------------------------ a. dedupe: the sorted-triple key
__global__ __launch_bounds__(256) void face_keys_k(const int32_t* __restrict__ tri, int64_t n_faces, int64_t n_vertices, int64_t* __restrict__ key_major,
                                                   int64_t* __restrict__ key_minor) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_faces) return;
    const int32_t a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
    int64_t major = K38_SENTINEL, minor = K38_SENTINEL;
    if (a >= 0 && b >= 0 && c >= 0 && a < n_vertices && b < n_vertices && c < n_vertices && a != b && b != c && c != a) {
        const int32_t lo = min(a, min(b, c)), hi = max(a, max(b, c));
        const int32_t mid = (int32_t)((int64_t)a + b + c - lo - hi);
        major = (int64_t)lo;
        minor = ((int64_t)mid << 32) | (int64_t)hi;
    }
    key_major[t] = major;
    key_minor[t] = minor;
}

// ------------------------------------------------------------------------------------------------ b. split: one new vertex per fan
// new_corner is read back by the thread that wrote it (a fan's label is its smallest corner, which the walk meets first): no __restrict__
__global__ __launch_bounds__(256) void split_corners_k(const int32_t* __restrict__ corner_order, const int32_t* __restrict__ corner_start,
                                                       const int32_t* __restrict__ corner_label, const int32_t* __restrict__ vertex_base,
                                                       int64_t n_vertices, int64_t n_half, int64_t n_new, int32_t* new_corner,
                                                       int32_t* __restrict__ vertex_source) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_vertices) return;
    int64_t s = corner_start[v], end = corner_start[v + 1];
    s = s < 0 ? 0 : s, end = end > n_half ? n_half : end;
    const int64_t base = vertex_base[v];
    int64_t rank = 0;
    for (int64_t j = s; j < end; ++j) {
        const int32_t c = corner_order[j];
        if (c < 0 || c >= n_half) continue;             // (a planted id: skipped, never read through)
        const int32_t label = corner_label[c];
        if (label == c) {
            const int64_t id = base + rank;
            ++rank;
            if (base < 0 || id >= n_new) continue;
            new_corner[c] = (int32_t)id;
            vertex_source[id] = (int32_t)v;
        } else if (label >= 0 && label < c) {
            new_corner[c] = new_corner[label];          // (-1 if that corner is not a root of this segment)
        }
    }
}

// ------------------------------------------------------------------------------------------------ d. orient: the doubled graph
__global__ __launch_bounds__(256) void orient_pairs_k(const int32_t* __restrict__ edge_halfedges, const uint8_t* __restrict__ edge_class,
                                                      int64_t n_edges, int64_t n_faces, int32_t* __restrict__ pairs) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges) return;
    int32_t p0 = -1, p1 = -1, p2 = -1, p3 = -1;
    const uint8_t cls = edge_class[e];
    const int32_t h0 = edge_halfedges[2 * e], h1 = edge_halfedges[2 * e + 1];
    if ((cls == 2 || cls == 3) && h0 >= 0 && h1 >= 0 && h0 < 3 * n_faces && h1 < 3 * n_faces) {
        const int32_t fa = h0 / 3, fb = h1 / 3;
        const int32_t cross = cls == 3 ? 1 : 0;         // a flipped edge joins each face's node to the other face's OTHER node
        p0 = 2 * fa, p1 = 2 * fb + cross;
        p2 = 2 * fa + 1, p3 = 2 * fb + 1 - cross;
    }
    pairs[4 * e] = p0, pairs[4 * e + 1] = p1;
    pairs[4 * e + 2] = p2, pairs[4 * e + 3] = p3;
}

__global__ __launch_bounds__(256) void apply_flips_k(const int32_t* __restrict__ tri, const uint8_t* __restrict__ flip, int64_t n_faces,
                                                     int32_t* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_faces) return;
    const int32_t a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
    const bool f = flip[t] != 0;
    out[3 * t] = a, out[3 * t + 1] = f ? c : b, out[3 * t + 2] = f ? b : c;
}

// ------------------------------------------------------------------------------------------------ e. fill
__global__ __launch_bounds__(256) void loop_centroids_k(const double* __restrict__ vert, int64_t n_vertices, const int32_t* __restrict__ loop_start,
                                                        const int32_t* __restrict__ loop_vertices, int64_t n_loops, int64_t n_rim,
                                                        const int32_t* __restrict__ loop_slot, int64_t n_centroids, double* __restrict__ centroids) {
    const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= n_loops) return;
    const int64_t slot = loop_slot[l];
    if (slot < 0 || slot >= n_centroids) return;
    int64_t s = loop_start[l], end = loop_start[l + 1];
    s = s < 0 ? 0 : s, end = end > n_rim ? n_rim : end;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int64_t count = 0;
    for (int64_t j = s; j < end; ++j) {
        const int32_t v = loop_vertices[j];
        if (v < 0 || v >= n_vertices) continue;
        const double* __restrict__ p = vert + 3 * (int64_t)v;
        sx = sx + p[0], sy = sy + p[1], sz = sz + p[2];
        ++count;
    }
    const double k = (double)count;                     // (an empty loop: 0 / 0, which nothing refers to)
    centroids[3 * slot] = sx / k, centroids[3 * slot + 1] = sy / k, centroids[3 * slot + 2] = sz / k;
}

__global__ __launch_bounds__(256) void fill_emit_k(const int32_t* __restrict__ tri, int64_t n_faces, int64_t n_vertices,
                                                   const int32_t* __restrict__ rim_halfedges, const int32_t* __restrict__ rim_slot, int64_t n_rim,
                                                   const int32_t* __restrict__ loop_of_vertex, const int32_t* __restrict__ loop_start,
                                                   const int32_t* __restrict__ loop_vertices, const int32_t* __restrict__ loop_apex, int64_t n_loops,
                                                   int64_t n_fill, int32_t* __restrict__ faces) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_rim) return;
    const int64_t slot = rim_slot[i];
    const int32_t h = rim_halfedges[i];
    if (slot < 0 || slot >= n_fill) return;
    int32_t a = -1, b = -1, c = -1;
    if (h >= 0 && h < 3 * n_faces) {
        const int32_t t3 = h - h % 3, k = h % 3;
        a = tri[h], b = tri[t3 + (k + 1) % 3];
    }
    if (a >= 0 && a < n_vertices && b >= 0 && b < n_vertices) {
        const int32_t l = loop_of_vertex[a];
        if (l >= 0 && l < n_loops) {
            c = loop_apex[l];
            if (c < 0) {                                // a loop of three: its third vertex
                int64_t s = loop_start[l], end = loop_start[l + 1];
                s = s < 0 ? 0 : s, end = end > n_rim ? n_rim : end;
                for (int64_t j = s; j < end; ++j) {
                    const int32_t v = loop_vertices[j];
                    if (v != a && v != b && v >= 0 && v < n_vertices) c = v;
                }
            }
        }
    }
    const bool ok = c >= 0;                             // (what cannot be formed: a row of -1, which K37 counts as not valid)
    faces[3 * slot] = ok ? b : -1, faces[3 * slot + 1] = ok ? a : -1, faces[3 * slot + 2] = ok ? c : -1;
}

// ------------------------------------------------------------------------------------------------ entry points
#define K38_LIMIT ((int64_t)1 << 31)
#define K38_CHECK_MESH(who, n_faces, n_vertices)                                                                                     \
    GENS_CHECK_ARG((n_faces) >= 0 && (n_vertices) >= 0, GENS_EINVAL, "%s: %lld faces over %lld vertices", who, (long long)(n_faces), \
                   (long long)(n_vertices));                                                                                         \
    GENS_CHECK_ARG((n_vertices) < K38_LIMIT && 3 * (int64_t)(n_faces) < K38_LIMIT, GENS_ELIMIT,                                     \
                   "%s: %lld faces over %lld vertices (V and 3 T below 2^31)", who, (long long)(n_faces), (long long)(n_vertices))

extern "C" int gens_mesh_face_keys(const int32_t* triangles, int64_t n_faces, int64_t n_vertices, int64_t* key_major, int64_t* key_minor,
                                   void* stream) {
    const char* who = "gens_mesh_face_keys";
    K38_CHECK_MESH(who, n_faces, n_vertices);
    if (n_faces == 0) return 0;
    GENS_CHECK_ARG(triangles && key_major && key_minor, GENS_EINVAL, "%s: null pointer", who);
    face_keys_k<<<gens_blocks(n_faces, 256), 256, 0, (hipStream_t)stream>>>(triangles, n_faces, n_vertices, key_major, key_minor);
    return gens_launch_status(who);
}

extern "C" int gens_mesh_split_corners(const int32_t* corner_order, const int32_t* corner_start, const int32_t* corner_label,
                                       const int32_t* vertex_base, int64_t n_vertices, int64_t n_halfedges, int64_t n_new, int32_t* new_corner,
                                       int32_t* vertex_source, void* stream) {
    const char* who = "gens_mesh_split_corners";
    GENS_CHECK_ARG(n_vertices >= 0 && n_halfedges >= 0 && n_new >= 0, GENS_EINVAL, "%s: %lld vertices, %lld half-edges, %lld new vertices", who,
                   (long long)n_vertices, (long long)n_halfedges, (long long)n_new);
    GENS_CHECK_ARG(n_vertices < K38_LIMIT && n_halfedges < K38_LIMIT, GENS_ELIMIT, "%s: %lld vertices, %lld half-edges (V and 3 T below 2^31)", who,
                   (long long)n_vertices, (long long)n_halfedges);
    GENS_CHECK_ARG(n_halfedges % 3 == 0, GENS_EINVAL, "%s: %lld half-edges (three per face)", who, (long long)n_halfedges);
    GENS_CHECK_ARG(n_new <= n_halfedges, GENS_EINVAL, "%s: %lld new vertices over %lld half-edges (a fan has a corner)", who, (long long)n_new,
                   (long long)n_halfedges);
    if (n_halfedges == 0) return 0;
    GENS_CHECK_ARG(new_corner, GENS_EINVAL, "%s: null pointer (new_corner)", who);
    if (n_vertices > 0)
        GENS_CHECK_ARG(corner_order && corner_start && corner_label && vertex_base, GENS_EINVAL, "%s: null pointer (corners)", who);
    if (n_vertices > 0 && n_new > 0) GENS_CHECK_ARG(vertex_source, GENS_EINVAL, "%s: null pointer (vertex_source)", who);
    k38_fill_i32_k<<<gens_blocks(n_halfedges, 256), 256, 0, (hipStream_t)stream>>>(new_corner, n_halfedges, -1);
    if (n_vertices > 0)
        split_corners_k<<<gens_blocks(n_vertices, 256), 256, 0, (hipStream_t)stream>>>(corner_order, corner_start, corner_label, vertex_base,
                                                                                      n_vertices, n_halfedges, n_new, new_corner, vertex_source);
    return gens_launch_status(who);
}

extern "C" int gens_mesh_orient_pairs(const int32_t* edge_halfedges, const uint8_t* edge_class, int64_t n_edges, int64_t n_faces, int32_t* pairs,
                                      void* stream) {
    const char* who = "gens_mesh_orient_pairs";
    GENS_CHECK_ARG(n_faces >= 0 && n_edges >= 0, GENS_EINVAL, "%s: %lld edges over %lld faces", who, (long long)n_edges, (long long)n_faces);
    GENS_CHECK_ARG(3 * n_faces < K38_LIMIT, GENS_ELIMIT, "%s: %lld faces (3 T below 2^31)", who, (long long)n_faces);
    GENS_CHECK_ARG(n_edges <= 3 * n_faces, GENS_EINVAL, "%s: %lld edges over %lld faces (an edge has a use)", who, (long long)n_edges, (long long)n_faces);
    if (n_edges == 0) return 0;
    GENS_CHECK_ARG(edge_halfedges && edge_class && pairs, GENS_EINVAL, "%s: null pointer", who);
    orient_pairs_k<<<gens_blocks(n_edges, 256), 256, 0, (hipStream_t)stream>>>(edge_halfedges, edge_class, n_edges, n_faces, pairs);
    return gens_launch_status(who);
}

extern "C" int gens_mesh_apply_flips(const int32_t* triangles, const uint8_t* flip, int64_t n_faces, int32_t* out, void* stream) {
    const char* who = "gens_mesh_apply_flips";
    GENS_CHECK_ARG(n_faces >= 0, GENS_EINVAL, "%s: %lld faces", who, (long long)n_faces);
    GENS_CHECK_ARG(3 * n_faces < K38_LIMIT, GENS_ELIMIT, "%s: %lld faces (3 T below 2^31)", who, (long long)n_faces);
    if (n_faces == 0) return 0;
    GENS_CHECK_ARG(triangles && flip && out, GENS_EINVAL, "%s: null pointer", who);
    apply_flips_k<<<gens_blocks(n_faces, 256), 256, 0, (hipStream_t)stream>>>(triangles, flip, n_faces, out);
    return gens_launch_status(who);
}

extern "C" int gens_mesh_loop_centroids(const double* vertices, int64_t n_vertices, const int32_t* loop_start, const int32_t* loop_vertices,
                                        int64_t n_loops, int64_t n_rim, const int32_t* loop_slot, int64_t n_centroids, double* centroids,
                                        void* stream) {
    const char* who = "gens_mesh_loop_centroids";
    GENS_CHECK_ARG(n_vertices >= 0 && n_loops >= 0 && n_rim >= 0 && n_centroids >= 0, GENS_EINVAL,
                   "%s: %lld vertices, %lld loops, %lld rim vertices, %lld centroids", who, (long long)n_vertices, (long long)n_loops, (long long)n_rim,
                   (long long)n_centroids);
    GENS_CHECK_ARG(n_vertices < K38_LIMIT, GENS_ELIMIT, "%s: %lld vertices (V below 2^31)", who, (long long)n_vertices);
    GENS_CHECK_ARG(n_rim <= n_vertices && n_loops <= n_rim && n_centroids <= n_loops, GENS_EINVAL,
                   "%s: %lld centroids of %lld loops over %lld rim vertices of %lld (a loop has a vertex)", who, (long long)n_centroids,
                   (long long)n_loops, (long long)n_rim, (long long)n_vertices);
    if (n_loops == 0 || n_centroids == 0) return 0;
    GENS_CHECK_ARG(vertices && loop_start && loop_vertices && loop_slot && centroids, GENS_EINVAL, "%s: null pointer", who);
    loop_centroids_k<<<gens_blocks(n_loops, 256), 256, 0, (hipStream_t)stream>>>(vertices, n_vertices, loop_start, loop_vertices, n_loops, n_rim,
                                                                                loop_slot, n_centroids, centroids);
    return gens_launch_status(who);
}

extern "C" int gens_mesh_fill_emit(const int32_t* triangles, int64_t n_faces, int64_t n_vertices, const int32_t* rim_halfedges,
                                   const int32_t* rim_slot, int64_t n_rim, const int32_t* loop_of_vertex, const int32_t* loop_start,
                                   const int32_t* loop_vertices, const int32_t* loop_apex, int64_t n_loops, int64_t n_fill, int32_t* faces,
                                   void* stream) {
    const char* who = "gens_mesh_fill_emit";
    K38_CHECK_MESH(who, n_faces, n_vertices);
    GENS_CHECK_ARG(n_rim >= 0 && n_loops >= 0 && n_fill >= 0, GENS_EINVAL, "%s: %lld rim half-edges, %lld loops, %lld fill faces", who,
                   (long long)n_rim, (long long)n_loops, (long long)n_fill);
    GENS_CHECK_ARG(n_rim <= 3 * n_faces && n_rim <= n_vertices && n_loops <= n_rim && n_fill <= n_rim, GENS_EINVAL,
                   "%s: %lld fill faces, %lld loops, %lld rim half-edges over %lld faces and %lld vertices (a rim vertex has a rim half-edge)", who,
                   (long long)n_fill, (long long)n_loops, (long long)n_rim, (long long)n_faces, (long long)n_vertices);
    if (n_rim == 0 || n_fill == 0) return 0;
    GENS_CHECK_ARG(triangles && rim_halfedges && rim_slot && loop_of_vertex && loop_start && loop_vertices && loop_apex && faces, GENS_EINVAL,
                   "%s: null pointer", who);
    fill_emit_k<<<gens_blocks(n_rim, 256), 256, 0, (hipStream_t)stream>>>(triangles, n_faces, n_vertices, rim_halfedges, rim_slot, n_rim,
                                                                         loop_of_vertex, loop_start, loop_vertices, loop_apex, n_loops, n_fill, faces);
    return gens_launch_status(who);
}
