// K40: generalised winding numbers of a triangle mesh (ops.build_winding_plan, ops.winding_number, ops.mesh_inside,
// ops.signed_distance_to_mesh(sign="winding"), ops.mesh_distance(sign="winding"), io.compare_meshes, python -m gens_amd.compare_meshes --sign
// winding).  The definition is the comment of K40 in include/gens_hip.h; tests/winding_reference.py restates it in numpy.
//
//   moments: one thread per leaf (64 faces of the plan order) gathers the faces' corners ONCE, writes them packed in plan order (72 bytes a
//            face, nine zeros for a face that is not valid: its solid angle is then +-0 at every query) and sums the leaf's area, area vector,
//            centre and radius in face order; one thread per node does the same over its 64 leaves.  No atomics.
//   query:   one query per lane, ONE wave per workgroup.  Every lane of a wave walks the same nodes, leaves and faces, so what it reads --
//            a cluster's moments, a face's nine doubles -- has a wave-uniform address: the loads are scalar loads through the constant cache
//            into SGPRs, no LDS and no vector registers for the mesh at all; the vector registers hold the query, three running sums and the
//            temporaries of one fp64 atan2.  The lanes of a wave differ only in WHETHER they take part (a far cluster is accepted per lane;
//            a leaf nobody in the wave opens is skipped by a scalar branch), never in the order: a lane's sums are those of the definition's
//            tree -- faces into the leaf's partial, leaves into the node's, nodes into the total -- whatever its neighbours do, so a query's
//            bits do not depend on the batch.  No scratch that grows with the queries.
// float64, every operation rounded on its own (no contraction), in the order the definition writes.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

#define K40_LEAF 64                     // faces per leaf, leaves per node
#define K40_LIMIT ((int64_t)1 << 31)
#define K40_FOUR_PI 12.566370614359172  // 4 * M_PI (exact doubling of the double nearest pi)
#define K40_TWO_PI 6.283185307179586

__device__ __forceinline__ bool k40_face_valid(int32_t a, int32_t b, int32_t c, int64_t n_vertices) {
    return a >= 0 && b >= 0 && c >= 0 && a < n_vertices && b < n_vertices && c < n_vertices && a != b && b != c && c != a;
}

// ------------------------------------------------------------------------------------------------ moments
__global__ __launch_bounds__(64) void winding_leaf_k(gens_winding_plan p) {
    const int64_t l = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (l >= p.n_leaves) return;
    double* __restrict__ out = p.corners + 9 * K40_LEAF * l;
    double area = 0.0, nx = 0.0, ny = 0.0, nz = 0.0, sx = 0.0, sy = 0.0, sz = 0.0, mx = 0.0, my = 0.0, mz = 0.0;
    uint64_t valid = 0;
    int count = 0;
    for (int j = 0; j < K40_LEAF; ++j) {
        const int64_t pos = K40_LEAF * l + j;
        bool ok = false;
        double a[3], b[3], c[3];
        if (pos < p.n_faces) {
            const int32_t f = p.face_order[pos];
            if (f >= 0 && f < p.n_faces) {                  // (a planted id: not valid, never read through)
                const int32_t ia = p.triangles[3 * (int64_t)f], ib = p.triangles[3 * (int64_t)f + 1], ic = p.triangles[3 * (int64_t)f + 2];
                if (k40_face_valid(ia, ib, ic, p.n_vertices)) {
                    ok = true;
                    for (int m = 0; m < 3; ++m)
                        a[m] = p.vertices[3 * (int64_t)ia + m], b[m] = p.vertices[3 * (int64_t)ib + m], c[m] = p.vertices[3 * (int64_t)ic + m];
                }
            }
        }
        if (!ok) {
            for (int m = 0; m < 9; ++m) out[9 * j + m] = 0.0;
            continue;
        }
        for (int m = 0; m < 3; ++m) out[9 * j + m] = a[m], out[9 * j + 3 + m] = b[m], out[9 * j + 6 + m] = c[m];
        const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
        const double vx = c[0] - a[0], vy = c[1] - a[1], vz = c[2] - a[2];
        const double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
        const double af = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
        const double gx = ((a[0] + b[0]) + c[0]) / 3.0, gy = ((a[1] + b[1]) + c[1]) / 3.0, gz = ((a[2] + b[2]) + c[2]) / 3.0;
        area = area + af;
        nx = nx + 0.5 * cx, ny = ny + 0.5 * cy, nz = nz + 0.5 * cz;
        sx = sx + af * gx, sy = sy + af * gy, sz = sz + af * gz;
        mx = mx + gx, my = my + gy, mz = mz + gz;
        valid |= 1ull << j;
        ++count;
    }
    double px = 0.0, py = 0.0, pz = 0.0, r2 = 0.0;
    if (count > 0) {
        if (area > 0.0) px = sx / area, py = sy / area, pz = sz / area;
        else px = mx / (double)count, py = my / (double)count, pz = mz / (double)count;
        for (int j = 0; j < K40_LEAF; ++j) {
            if (!((valid >> j) & 1ull)) continue;
            for (int m = 0; m < 3; ++m) {               // (its own writes above: the same thread reads them back)
                const double dx = out[9 * j + 3 * m] - px, dy = out[9 * j + 3 * m + 1] - py, dz = out[9 * j + 3 * m + 2] - pz;
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 > r2) r2 = d2;
            }
        }
    }
    p.leaf_count[l] = count;
    p.leaf_area[l] = area;
    p.leaf_normal[3 * l] = nx, p.leaf_normal[3 * l + 1] = ny, p.leaf_normal[3 * l + 2] = nz;
    p.leaf_centre[3 * l] = px, p.leaf_centre[3 * l + 1] = py, p.leaf_centre[3 * l + 2] = pz;
    p.leaf_radius2[l] = r2;
}

__global__ __launch_bounds__(64) void winding_node_k(gens_winding_plan p) {
    const int64_t k = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (k >= p.n_nodes) return;
    const int64_t l0 = K40_LEAF * k, l1 = l0 + K40_LEAF < p.n_leaves ? l0 + K40_LEAF : p.n_leaves;
    double area = 0.0, nx = 0.0, ny = 0.0, nz = 0.0, sx = 0.0, sy = 0.0, sz = 0.0, mx = 0.0, my = 0.0, mz = 0.0;
    int count = 0;
    for (int64_t l = l0; l < l1; ++l) {
        const int cl = p.leaf_count[l];
        if (cl <= 0) continue;
        const double al = p.leaf_area[l], qx = p.leaf_centre[3 * l], qy = p.leaf_centre[3 * l + 1], qz = p.leaf_centre[3 * l + 2];
        area = area + al;
        nx = nx + p.leaf_normal[3 * l], ny = ny + p.leaf_normal[3 * l + 1], nz = nz + p.leaf_normal[3 * l + 2];
        sx = sx + al * qx, sy = sy + al * qy, sz = sz + al * qz;
        mx = mx + (double)cl * qx, my = my + (double)cl * qy, mz = mz + (double)cl * qz;
        count += cl;
    }
    double px = 0.0, py = 0.0, pz = 0.0, r = 0.0;
    if (count > 0) {
        if (area > 0.0) px = sx / area, py = sy / area, pz = sz / area;
        else px = mx / (double)count, py = my / (double)count, pz = mz / (double)count;
        for (int64_t l = l0; l < l1; ++l) {
            if (p.leaf_count[l] <= 0) continue;
            const double dx = p.leaf_centre[3 * l] - px, dy = p.leaf_centre[3 * l + 1] - py, dz = p.leaf_centre[3 * l + 2] - pz;
            const double reach = sqrt((dx * dx + dy * dy) + dz * dz) + sqrt(p.leaf_radius2[l]);
            if (reach > r) r = reach;
        }
    }
    p.node_count[k] = count;
    p.node_area[k] = area;
    p.node_normal[3 * k] = nx, p.node_normal[3 * k + 1] = ny, p.node_normal[3 * k + 2] = nz;
    p.node_centre[3 * k] = px, p.node_centre[3 * k + 1] = py, p.node_centre[3 * k + 2] = pz;
    p.node_radius2[k] = r * r;
}

// ------------------------------------------------------------------------------------------------ the query
// Van Oosterom and Strackee: the solid angle of the face (a, b, c) at q
__device__ __forceinline__ double k40_solid_angle(double qx, double qy, double qz, const double* __restrict__ f) {
    const double ax = f[0] - qx, ay = f[1] - qy, az = f[2] - qz;
    const double bx = f[3] - qx, by = f[4] - qy, bz = f[5] - qz;
    const double cx = f[6] - qx, cy = f[7] - qy, cz = f[8] - qz;
    const double la = sqrt((ax * ax + ay * ay) + az * az), lb = sqrt((bx * bx + by * by) + bz * bz), lc = sqrt((cx * cx + cy * cy) + cz * cz);
    const double ux = by * cz - bz * cy, uy = bz * cx - bx * cz, uz = bx * cy - by * cx;
    const double num = (ax * ux + ay * uy) + az * uz;
    const double ab = (ax * bx + ay * by) + az * bz, bc = (bx * cx + by * cy) + bz * cz, ca = (cx * ax + cy * ay) + cz * az;
    const double den = (((la * lb) * lc + ab * lc) + bc * la) + ca * lb;
    return 2.0 * atan2(num, den);
}

// The far-field test of one cluster for one lane: true, with the dipole's solid angle and the error bound, if d2 > beta2 r2.
__device__ __forceinline__ bool k40_far(double qx, double qy, double qz, double beta2, double area, const double* __restrict__ normal,
                                        const double* __restrict__ centre, double r2, double* omega, double* err) {
    const double dx = centre[0] - qx, dy = centre[1] - qy, dz = centre[2] - qz;
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    if (!(d2 > beta2 * r2)) return false;
    const double d = sqrt(d2), r = sqrt(r2), g = d - r;
    *omega = ((normal[0] * dx + normal[1] * dy) + normal[2] * dz) / (d2 * d);
    *err = (area * r) / (K40_TWO_PI * ((g * g) * g));
    return true;
}

template <bool FAST>
__global__ __launch_bounds__(64) void winding_query_k(gens_winding_plan p, const double* __restrict__ queries, int64_t n, double beta2,
                                                      double* __restrict__ w, double* __restrict__ bound) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const bool live = i < n;
    const double qx = live ? queries[3 * i] : 0.0, qy = live ? queries[3 * i + 1] : 0.0, qz = live ? queries[3 * i + 2] : 0.0;
    const bool act = live && isfinite(qx) && isfinite(qy) && isfinite(qz);
    const double* __restrict__ corners = p.corners;
    const int32_t* __restrict__ leaf_count = p.leaf_count;
    const int32_t* __restrict__ node_count = p.node_count;
    const double* __restrict__ leaf_area = p.leaf_area;
    const double* __restrict__ leaf_normal = p.leaf_normal;
    const double* __restrict__ leaf_centre = p.leaf_centre;
    const double* __restrict__ leaf_radius2 = p.leaf_radius2;
    const double* __restrict__ node_area = p.node_area;
    const double* __restrict__ node_normal = p.node_normal;
    const double* __restrict__ node_centre = p.node_centre;
    const double* __restrict__ node_radius2 = p.node_radius2;
    const int64_t n_faces = p.n_faces, n_leaves = p.n_leaves, n_nodes = p.n_nodes;
    double total = 0.0, bsum = 0.0;
    for (int64_t k = 0; k < n_nodes; ++k) {
        if (node_count[k] <= 0) continue;
        bool open = act;
        double part = 0.0;
        if (FAST) {
            double omega, err;
            if (act && k40_far(qx, qy, qz, beta2, node_area[k], node_normal + 3 * k, node_centre + 3 * k, node_radius2[k], &omega, &err))
                part = omega, bsum = bsum + err, open = false;
        }
        if (__any(open)) {
            const int64_t l1 = K40_LEAF * (k + 1) < n_leaves ? K40_LEAF * (k + 1) : n_leaves;
            for (int64_t l = K40_LEAF * k; l < l1; ++l) {
                if (leaf_count[l] <= 0) continue;
                bool near = open;
                double leaf = 0.0;
                if (FAST) {
                    double omega, err;
                    if (open && k40_far(qx, qy, qz, beta2, leaf_area[l], leaf_normal + 3 * l, leaf_centre + 3 * l, leaf_radius2[l], &omega, &err))
                        leaf = omega, bsum = bsum + err, near = false;
                }
                if (__any(near)) {
                    const int nj = (int)(n_faces - K40_LEAF * l < K40_LEAF ? n_faces - K40_LEAF * l : K40_LEAF);
                    const double* __restrict__ f = corners + 9 * K40_LEAF * l;
                    for (int j = 0; j < nj; ++j) {
                        const double omega = k40_solid_angle(qx, qy, qz, f + 9 * j);
                        if (near) leaf = leaf + omega;
                    }
                }
                if (open) part = part + leaf;
            }
        }
        if (act) total = total + part;
    }
    if (live) {
        w[i] = act ? total / K40_FOUR_PI : NAN;
        if (bound) bound[i] = act ? bsum : NAN;
    }
}

// ------------------------------------------------------------------------------------------------ entry points
static int k40_check_plan(const char* who, const gens_winding_plan* p) {
    GENS_CHECK_ARG(p, GENS_EINVAL, "%s: null plan", who);
    GENS_CHECK_ARG(p->n_vertices >= 0 && p->n_faces >= 0 && p->n_leaves >= 0 && p->n_nodes >= 0, GENS_EINVAL,
                   "%s: %lld vertices, %lld faces, %lld leaves, %lld nodes", who, (long long)p->n_vertices, (long long)p->n_faces,
                   (long long)p->n_leaves, (long long)p->n_nodes);
    GENS_CHECK_ARG(p->n_vertices < K40_LIMIT && p->n_faces < K40_LIMIT / 3 + 1 && 3 * p->n_faces < K40_LIMIT, GENS_ELIMIT,
                   "%s: %lld faces over %lld vertices (V and 3 T below 2^31)", who, (long long)p->n_faces, (long long)p->n_vertices);
    GENS_CHECK_ARG(p->n_leaves == (p->n_faces + K40_LEAF - 1) / K40_LEAF && p->n_nodes == (p->n_leaves + K40_LEAF - 1) / K40_LEAF, GENS_EINVAL,
                   "%s: %lld leaves and %lld nodes over %lld faces (64 faces a leaf, 64 leaves a node)", who, (long long)p->n_leaves,
                   (long long)p->n_nodes, (long long)p->n_faces);
    if (p->n_faces == 0) return 0;
    GENS_CHECK_ARG(p->corners && p->leaf_count && p->leaf_area && p->leaf_normal && p->leaf_centre && p->leaf_radius2 && p->node_count &&
                       p->node_area && p->node_normal && p->node_centre && p->node_radius2,
                   GENS_EINVAL, "%s: null pointer (in the plan)", who);
    return 0;
}

extern "C" int gens_mesh_winding_moments(const gens_winding_plan* plan, void* stream) {
    const char* who = "gens_mesh_winding_moments";
    const int rc = k40_check_plan(who, plan);
    if (rc != 0) return rc;
    if (plan->n_faces == 0) return 0;
    GENS_CHECK_ARG(plan->triangles && plan->face_order && (plan->vertices || plan->n_vertices == 0), GENS_EINVAL,
                   "%s: null pointer (vertices, triangles or face_order)", who);
    winding_leaf_k<<<gens_blocks(plan->n_leaves, 64), 64, 0, (hipStream_t)stream>>>(*plan);
    const int launched = gens_launch_status(who);
    if (launched != 0) return launched;
    winding_node_k<<<gens_blocks(plan->n_nodes, 64), 64, 0, (hipStream_t)stream>>>(*plan);
    return gens_launch_status(who);
}

extern "C" int gens_mesh_winding_number(const gens_winding_plan* plan, const double* queries, int64_t n_queries, double beta, double* w,
                                        double* bound, void* stream) {
    const char* who = "gens_mesh_winding_number";
    const int rc = k40_check_plan(who, plan);
    if (rc != 0) return rc;
    GENS_CHECK_ARG(n_queries >= 0, GENS_EINVAL, "%s: %lld queries", who, (long long)n_queries);
    GENS_CHECK_ARG(n_queries < K40_LIMIT, GENS_ELIMIT, "%s: %lld queries (below 2^31)", who, (long long)n_queries);
    GENS_CHECK_ARG(beta == 0.0 || (beta > 1.0 && isfinite(beta)), GENS_EINVAL, "%s: beta %g (0: exact; else a finite number > 1)", who, beta);   // (NaN fails)
    if (n_queries == 0) return 0;
    GENS_CHECK_ARG(queries && w, GENS_EINVAL, "%s: null pointer (queries or w)", who);
    GENS_CHECK_ARG(w != queries && bound != queries && bound != w, GENS_EINVAL, "%s: two of queries, w and bound share a buffer", who);
    if (beta == 0.0)
        winding_query_k<false><<<gens_blocks(n_queries, 64), 64, 0, (hipStream_t)stream>>>(*plan, queries, n_queries, 0.0, w, bound);
    else
        winding_query_k<true><<<gens_blocks(n_queries, 64), 64, 0, (hipStream_t)stream>>>(*plan, queries, n_queries, beta * beta, w, bound);
    return gens_launch_status(who);
}
