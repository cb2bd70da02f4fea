// K41: which pairs of faces of a triangle mesh intersect, decided exactly or not at all (include/gens_hip.h, K41).
//
//   faces:  one thread per face: VALID (K37's rule), its float64 AABB, and its class from the certified signs of the three components of
//           (b - a) x (c - a): ordinary (some component certainly not 0), degenerate (all certainly 0), uncertain (neither);
//   pairs:  one lane per ENTRY of K23's cell lists (cell c, position x); the lane walks the positions y > x of the same cell, a slice of
//           K41_CHUNK of them per blockIdx.y, so a long list is spread over lanes (n entries) and workgroups (n / K41_CHUNK slices each).
//           The pair (x, y) is a CANDIDATE of this cell iff the closed float64 AABBs overlap and the cell is the one that holds the lower
//           corner of their intersection -- per axis max(i0_x, i0_y), i0 computed with gens_mesh_grid_count's own expression, which is
//           monotone in the coordinate, so that cell lies in both faces' ranges and no other cell claims the pair: every candidate is met
//           exactly once, with no atomics and no sort.  The narrow phase follows in the same launch: the lane parks the six corners in its
//           own column of an LDS array (so the predicates index corners at run time without scratch) and evaluates the predicate form of
//           the header on signs in {-, 0, +, ?}.
//   The count launch adds the pairs to emit per cell and class, the totals and the faces' flag bits with integer atomics; the emit launch
//   repeats the walk and writes each pair at (the exclusive scan of the cell's count) + (a ticket from the cell's cursor).  The order
//   inside a cell is whatever the tickets give: the op sorts the pairs by (s << 32) | t.
//
// Certified signs.  A predicate is a polynomial in coordinate differences evaluated in float64 as an expression tree of height h (6 for
// orient3d and the k = 2 dot product, 3 for orient2d); with every operation rounded once, |computed - exact| <= ((1 + e)^h - 1) P with e = 2^-53
// and P the same tree over absolute values (the permanent), and the computed permanent is at least (1 - e)^h P, so
// |computed - exact| <= (h + 1) e P~: c = 8 and 4 (the file is built with -ffp-contract=off; a contracted product only drops a rounding).
// The bound assumes that nothing underflows or overflows: a sign is taken from it only if |value| > 2^-600 as well, and a face with a
// coordinate beyond 2^100 (or not finite) is UNCERTAIN, which keeps every product below 2^404 and every underflow's error below 2^-868.
// Otherwise the predicate is evaluated again with error-free transformations (two_sum for every difference and sum, fma for every
// product's tail, a product below 2^-900 counting as inexact): if every operation was exact the value IS the exact value and its sign is
// returned, else `?`.
#include <math.h>

#include "common.h"

#define K41_GRID_MAX_AXIS 512     // K23's limits and widening (k23_mesh_cull.hip: GRID_MAX_AXIS, GRID_EPS)
#define K41_GRID_EPS 1e-5
#define K41_CHUNK 128             // positions y one lane walks per slice
#define K41_THREADS 256
#define K41_EPS53 1.1102230246251565e-16      // 2^-53
#define K41_C2 4.0
#define K41_C3 8.0
#define K41_FLOOR 0x1p-600
#define K41_SMALL_PRODUCT 0x1p-900
#define K41_MAX_COORD 0x1p100
#define K41_LIMIT ((int64_t)1 << 31)

enum { SG_NEG = -1, SG_ZERO = 0, SG_POS = 1, SG_UNK = 2 };
enum { R_NO = 0, R_YES = 1, R_MAYBE = 2, K41_SEP = 4 };

__device__ __forceinline__ int sgn_of(double v) { return v > 0.0 ? SG_POS : (v < 0.0 ? SG_NEG : SG_ZERO); }
__device__ __forceinline__ bool strict(int s) { return s == SG_POS || s == SG_NEG; }

// error-free transformations: each returns the rounded result and clears `ok` unless it is the exact one
struct Exact {
    bool ok;
    __device__ __forceinline__ double sub(double x, double y) {
        const double d = x - y, bb = d - x;
        const double err = (x - (d - bb)) + (-y - bb);
        ok = ok && err == 0.0;      // (NaN after an overflow: not exact)
        return d;
    }
    __device__ __forceinline__ double add(double x, double y) {
        const double s = x + y, bb = s - x;
        const double err = (x - (s - bb)) + (y - bb);
        ok = ok && err == 0.0;
        return s;
    }
    __device__ __forceinline__ double mul(double x, double y) {
        const double p = x * y;
        const double tail = __builtin_fma(x, y, -p);
        ok = ok && (p == 0.0 ? (x == 0.0 || y == 0.0) : (fabs(p) >= K41_SMALL_PRODUCT && tail == 0.0));
        return p;
    }
};

__device__ __forceinline__ int filtered(double det, double perm, double c) {
    return (fabs(det) > c * K41_EPS53 * perm && fabs(det) > K41_FLOOR && perm < INFINITY) ? sgn_of(det) : SG_UNK;      // (NaN: ?)
}

// (p - r) x (q - r) in two dimensions
__device__ __forceinline__ int orient2d_sign(double px, double py, double qx, double qy, double rx, double ry) {
    {
        const double ax = px - rx, ay = py - ry, bx = qx - rx, by = qy - ry;
        const double l = ax * by, r = ay * bx;
        const int s = filtered(l - r, fabs(l) + fabs(r), K41_C2);
        if (s != SG_UNK) return s;
    }
    Exact e{true};
    const double ax = e.sub(px, rx), ay = e.sub(py, ry), bx = e.sub(qx, rx), by = e.sub(qy, ry);
    const double det = e.sub(e.mul(ax, by), e.mul(ay, bx));
    return e.ok ? sgn_of(det) : SG_UNK;
}

// A lane's corners: slot m (0 .. 5), axis a at P[(3 m + a) * K41_THREADS] (its own column of the workgroup's LDS array).
#define K41_AT(m, a) P[((m) * 3 + (a)) * K41_THREADS]

// orient3d of the corners in slots a, b, c, d (Shewchuk's form, pivot d)
__device__ __forceinline__ int orient3d_sign(const double* P, int a, int b, int c, int d) {
    const double dx = K41_AT(d, 0), dy = K41_AT(d, 1), dz = K41_AT(d, 2);
    const double ax = K41_AT(a, 0), ay = K41_AT(a, 1), az = K41_AT(a, 2);
    const double bx = K41_AT(b, 0), by = K41_AT(b, 1), bz = K41_AT(b, 2);
    const double cx = K41_AT(c, 0), cy = K41_AT(c, 1), cz = K41_AT(c, 2);
    {
        const double adx = ax - dx, ady = ay - dy, adz = az - dz, bdx = bx - dx, bdy = by - dy, bdz = bz - dz, cdx = cx - dx, cdy = cy - dy,
                     cdz = cz - dz;
        const double bc1 = bdx * cdy, bc2 = cdx * bdy, ca1 = cdx * ady, ca2 = adx * cdy, ab1 = adx * bdy, ab2 = bdx * ady;
        const double det = (adz * (bc1 - bc2) + bdz * (ca1 - ca2)) + cdz * (ab1 - ab2);
        const double perm = ((fabs(bc1) + fabs(bc2)) * fabs(adz) + (fabs(ca1) + fabs(ca2)) * fabs(bdz)) + (fabs(ab1) + fabs(ab2)) * fabs(cdz);
        const int s = filtered(det, perm, K41_C3);
        if (s != SG_UNK) return s;
    }
    Exact e{true};
    const double adx = e.sub(ax, dx), ady = e.sub(ay, dy), adz = e.sub(az, dz), bdx = e.sub(bx, dx), bdy = e.sub(by, dy), bdz = e.sub(bz, dz),
                 cdx = e.sub(cx, dx), cdy = e.sub(cy, dy), cdz = e.sub(cz, dz);
    const double t0 = e.mul(adz, e.sub(e.mul(bdx, cdy), e.mul(cdx, bdy)));
    const double t1 = e.mul(bdz, e.sub(e.mul(cdx, ady), e.mul(adx, cdy)));
    const double t2 = e.mul(cdz, e.sub(e.mul(adx, bdy), e.mul(bdx, ady)));
    const double det = e.add(e.add(t0, t1), t2);
    return e.ok ? sgn_of(det) : SG_UNK;
}

// ((b - a) x (c - a)) . ((b - a) x (d - a))
__device__ __forceinline__ int fold_dot_sign(const double* P, int a, int b, int c, int d) {
    double u[3], w[3], x[3];
    for (int k = 0; k < 3; ++k) {
        const double o = K41_AT(a, k);
        u[k] = K41_AT(b, k) - o, w[k] = K41_AT(c, k) - o, x[k] = K41_AT(d, k) - o;
    }
    {
        double det = 0.0, perm = 0.0;
        for (int k = 0; k < 3; ++k) {
            const int i = (k + 1) % 3, j = (k + 2) % 3;
            const double p1 = u[i] * w[j], p2 = u[j] * w[i], q1 = u[i] * x[j], q2 = u[j] * x[i];
            const double term = (p1 - p2) * (q1 - q2), pterm = (fabs(p1) + fabs(p2)) * (fabs(q1) + fabs(q2));
            det = k == 0 ? term : det + term;
            perm = k == 0 ? pterm : perm + pterm;
        }
        const int s = filtered(det, perm, K41_C3);
        if (s != SG_UNK) return s;
    }
    Exact e{true};
    for (int k = 0; k < 3; ++k) {
        const double o = K41_AT(a, k);
        u[k] = e.sub(K41_AT(b, k), o), w[k] = e.sub(K41_AT(c, k), o), x[k] = e.sub(K41_AT(d, k), o);
    }
    double det = 0.0;
    for (int k = 0; k < 3; ++k) {
        const int i = (k + 1) % 3, j = (k + 2) % 3;
        const double n1 = e.sub(e.mul(u[i], w[j]), e.mul(u[j], w[i])), n2 = e.sub(e.mul(u[i], x[j]), e.mul(u[j], x[i]));
        const double term = e.mul(n1, n2);
        det = k == 0 ? term : e.add(det, term);
    }
    return e.ok ? sgn_of(det) : SG_UNK;
}

// ---------------------------------------------------------------------------------------- the coplanar case, in two dimensions
__device__ __forceinline__ int o2(const double* P, int p, int q, int r, int u, int v) {
    return orient2d_sign(K41_AT(p, u), K41_AT(p, v), K41_AT(q, u), K41_AT(q, v), K41_AT(r, u), K41_AT(r, v));
}

// closed segments pq and ab
__device__ __forceinline__ int seg_seg_2d(const double* P, int p, int q, int a, int b, int u, int v) {
    const int o1 = o2(P, p, q, a, u, v), o2_ = o2(P, p, q, b, u, v);
    if (strict(o1) && o1 == o2_) return R_NO;
    const int o3 = o2(P, a, b, p, u, v), o4 = o2(P, a, b, q, u, v);
    if (strict(o3) && o3 == o4) return R_NO;
    if (o1 == SG_UNK || o2_ == SG_UNK || o3 == SG_UNK || o4 == SG_UNK) return R_MAYBE;
    if (o1 == 0 && o2_ == 0 && o3 == 0 && o4 == 0) {      // on one line: they meet iff their boxes do (exact comparisons)
        bool meet = true;
#pragma nounroll
        for (int k = 0; k < 2; ++k) {
            const int ax = k == 0 ? u : v;
            const double p0 = K41_AT(p, ax), q0 = K41_AT(q, ax), a0 = K41_AT(a, ax), b0 = K41_AT(b, ax);
            meet = meet && fmax(fmin(p0, q0), fmin(a0, b0)) <= fmin(fmax(p0, q0), fmax(a0, b0));
        }
        return meet ? R_YES : R_NO;
    }
    return R_YES;
}

// closed segment pq against the closed face (a, b, c), all five points in one plane: an end point in the face, or pq meets one of its edges
__device__ __forceinline__ int seg_tri_coplanar(const double* P, int p, int q, int a, int b, int c) {
    int axis = -1, o = 0;
#pragma nounroll
    for (int k = 0; k < 3 && axis < 0; ++k) {
        const int s = o2(P, b, c, a, (k + 1) % 3, (k + 2) % 3);       // component k of (b - a) x (c - a)
        if (strict(s)) axis = k, o = s;
    }
    if (axis < 0) return R_MAYBE;
    const int u = (axis + 1) % 3, v = (axis + 2) % 3;
    int res = R_NO;
#pragma nounroll
    for (int k = 0; k < 2; ++k) {
        const int z = k == 0 ? p : q;
        const int s1 = o2(P, a, b, z, u, v), s2 = o2(P, b, c, z, u, v), s3 = o2(P, c, a, z, u, v);
        if (s1 == -o || s2 == -o || s3 == -o) continue;
        if (s1 == SG_UNK || s2 == SG_UNK || s3 == SG_UNK)
            res = R_MAYBE;
        else
            return R_YES;
    }
#pragma nounroll
    for (int k = 0; k < 3; ++k) {
        const int e0 = k == 0 ? a : (k == 1 ? b : c), e1 = k == 0 ? b : (k == 1 ? c : a);
        const int r = seg_seg_2d(P, p, q, e0, e1, u, v);
        if (r == R_YES) return R_YES;
        if (r == R_MAYBE) res = R_MAYBE;
    }
    return res;
}

// ---------------------------------------------------------------------------------------- closed segment against closed face
// what the plane signs of the segment's ends say: 0 no; 1 coplanar; 2 the three edge signs decide; 3 the edge signs can only say no; 4 maybe
__device__ __forceinline__ int seg_plane_mode(int sp, int sq) {
    if (sp != SG_UNK && sq != SG_UNK) return sp * sq > 0 ? 0 : ((sp == 0 && sq == 0) ? 1 : 2);
    return (strict(sp) || strict(sq)) ? 3 : 4;
}
__device__ __forceinline__ int seg_edge_verdict(int mode, int e0, int e1, int e2) {
    const bool pos = e0 == SG_POS || e1 == SG_POS || e2 == SG_POS, neg = e0 == SG_NEG || e1 == SG_NEG || e2 == SG_NEG;
    if (pos && neg) return R_NO;          // the line pq, which is not in the plane, misses the face
    if (mode == 3 || e0 == SG_UNK || e1 == SG_UNK || e2 == SG_UNK) return R_MAYBE;
    return R_YES;
}

__device__ __forceinline__ unsigned enc(int s) { return (unsigned)(s + 1); }
__device__ __forceinline__ int dec(unsigned w, int i) { return (int)((w >> (2 * i)) & 3u) - 1; }
__device__ __forceinline__ bool one_strict_side3(unsigned w) { return w == 0u || w == 42u; }       // three signs, all - or all +

// k = 0: faces in slots sb .. sb + 2 and tb .. tb + 2
// (the pair functions return the verdict, + K41_SEP if one strict plane separation alone decided it)
__device__ __forceinline__ int pair_k0(const double* P, int sb, int tb) {
    unsigned ps = 0, pt = 0, E = 0;
#pragma nounroll
    for (int i = 0; i < 3; ++i) ps |= enc(orient3d_sign(P, tb, tb + 1, tb + 2, sb + i)) << (2 * i);
    if (one_strict_side3(ps)) return R_NO + K41_SEP;
#pragma nounroll
    for (int j = 0; j < 3; ++j) pt |= enc(orient3d_sign(P, sb, sb + 1, sb + 2, tb + j)) << (2 * j);
    if (one_strict_side3(pt)) return R_NO + K41_SEP;
#pragma nounroll
    for (int ij = 0; ij < 9; ++ij) {
        const int i = ij / 3, j = ij % 3;
        E |= enc(orient3d_sign(P, sb + i, sb + (i + 1) % 3, tb + j, tb + (j + 1) % 3)) << (2 * ij);
    }
    int res = R_NO;
#pragma nounroll
    for (int h = 0; h < 6; ++h) {
        const bool s_edge = h < 3;
        const int i = s_edge ? h : h - 3, i1 = (i + 1) % 3;
        const int mode = seg_plane_mode(dec(s_edge ? ps : pt, i), dec(s_edge ? ps : pt, i1));
        int r = R_NO;
        if (mode == 1)
            r = s_edge ? seg_tri_coplanar(P, sb + i, sb + i1, tb, tb + 1, tb + 2) : seg_tri_coplanar(P, tb + i, tb + i1, sb, sb + 1, sb + 2);
        else if (mode == 4)
            r = R_MAYBE;
        else if (mode != 0)       // (orient3d(t_j, t_j+1, s_i, s_i+1) has the sign of orient3d(s_i, s_i+1, t_j, t_j+1): an even permutation)
            r = s_edge ? seg_edge_verdict(mode, dec(E, 3 * i), dec(E, 3 * i + 1), dec(E, 3 * i + 2))
                       : seg_edge_verdict(mode, dec(E, i), dec(E, 3 + i), dec(E, 6 + i));
        if (r == R_YES) return R_YES;
        if (r == R_MAYBE) res = R_MAYBE;
    }
    return res;
}

// segment ab against the face (v, c, d) whose plane sees a and b at sa, sb; e_mid: the sign of orient3d(a, b, c, d) if known, else 3.
// -> verdict + 4 * (that sign + 1, or 4 if it was not needed)
__device__ __forceinline__ int seg_tri_lazy(const double* P, int sa, int sb, int a, int b, int v, int c, int d, int e_mid) {
    const int mode = seg_plane_mode(sa, sb);
    if (mode == 0) return R_NO + 16;
    if (mode == 1) return seg_tri_coplanar(P, a, b, v, c, d) + 16;
    if (mode == 4) return R_MAYBE + 16;
    const int e0 = orient3d_sign(P, a, b, v, c), e1 = e_mid != 3 ? e_mid : orient3d_sign(P, a, b, c, d), e2 = orient3d_sign(P, a, b, d, v);
    return seg_edge_verdict(mode, e0, e1, e2) + 4 * (e1 + 1);
}

// k = 1: the shared corner is slot v of the first face and slot vv of the second
__device__ __forceinline__ int pair_k1(const double* P, int sb, int vs, int tb, int vt) {
    const int v = sb + vs, a = sb + (vs + 1) % 3, b = sb + (vs + 2) % 3, vv = tb + vt, c = tb + (vt + 1) % 3, d = tb + (vt + 2) % 3;
    const int sa = orient3d_sign(P, vv, c, d, a), sbb = orient3d_sign(P, vv, c, d, b);
    if (strict(sa) && sa == sbb) return R_NO + K41_SEP;      // the first face touches the second's plane at v alone
    const int sc = orient3d_sign(P, v, a, b, c), sd = orient3d_sign(P, v, a, b, d);
    if (strict(sc) && sc == sd) return R_NO + K41_SEP;
    const int first = seg_tri_lazy(P, sa, sbb, a, b, vv, c, d, 3);
    const int r1 = first & 3, mid = (first >> 2) == 4 ? 3 : (first >> 2) - 1;
    if (r1 == R_YES) return R_YES;
    const int r2 = seg_tri_lazy(P, sc, sd, c, d, v, a, b, mid) & 3;       // (orient3d(c, d, a, b) has the sign of orient3d(a, b, c, d))
    if (r2 == R_YES) return R_YES;
    return (r1 == R_MAYBE || r2 == R_MAYBE) ? R_MAYBE : R_NO;
}

// k = 2: shared edge ab, opposite corners c and d: a flat fold iff coplanar and on the same side of ab
__device__ __forceinline__ int pair_k2(const double* P, int a, int b, int c, int d) {
    const int sd = fold_dot_sign(P, a, b, c, d);
    if (sd == SG_NEG || sd == SG_ZERO) return R_NO;
    const int so = orient3d_sign(P, a, b, c, d);
    if (strict(so)) return R_NO + K41_SEP;
    return (sd == SG_POS && so == SG_ZERO) ? R_YES : R_MAYBE;
}

// The verdict (+ K41_SEP) for two ordinary faces x (corners in slots 0 .. 2, index row x0, x1, x2) and y (slots 3 .. 5) sharing k < 3 indices.
__device__ __forceinline__ int decide_pair(const double* P, int x0, int x1, int x2, int y0, int y1, int y2) {
    // which corner of y each corner of x is (3: none)
    const int m0 = x0 == y0 ? 0 : (x0 == y1 ? 1 : (x0 == y2 ? 2 : 3));
    const int m1 = x1 == y0 ? 0 : (x1 == y1 ? 1 : (x1 == y2 ? 2 : 3));
    const int m2 = x2 == y0 ? 0 : (x2 == y1 ? 1 : (x2 == y2 ? 2 : 3));
    const int shared = (m0 != 3) + (m1 != 3) + (m2 != 3);
    // the roles do not depend on the faces' numbers: the first face is the one whose index row is the smaller
    const bool x_first = x0 != y0 ? x0 < y0 : (x1 != y1 ? x1 < y1 : x2 < y2);
    const int sb = x_first ? 0 : 3, tb = x_first ? 3 : 0;
    if (shared == 0) return pair_k0(P, sb, tb);
    if (shared == 1) {
        const int vx = m0 != 3 ? 0 : (m1 != 3 ? 1 : 2), vy = m0 != 3 ? m0 : (m1 != 3 ? m1 : m2);
        return x_first ? pair_k1(P, 0, vx, 3, vy) : pair_k1(P, 3, vy, 0, vx);
    }
    const int ox = m0 == 3 ? 0 : (m1 == 3 ? 1 : 2);          // x's corner off the edge
    const int oy = 3 - (m0 == 3 ? 0 : m0) - (m1 == 3 ? 0 : m1) - (m2 == 3 ? 0 : m2);       // y's: 0 + 1 + 2 less the two matched
    const int os = x_first ? ox : oy, ot = x_first ? oy : ox;  // the edge as the first face runs it
    return pair_k2(P, sb + (os + 1) % 3, sb + (os + 2) % 3, sb + os, tb + ot);
}

// ---------------------------------------------------------------------------------------- kernels
__global__ __launch_bounds__(K41_THREADS) void isect_faces_k(const double* __restrict__ V, int64_t nv, const int32_t* __restrict__ T, int64_t nt,
                                                             uint8_t* __restrict__ cls, double* __restrict__ box) {
    const int64_t f = (int64_t)blockIdx.x * K41_THREADS + threadIdx.x;
    if (f >= nt) return;
    const int64_t i0 = T[3 * f], i1 = T[3 * f + 1], i2 = T[3 * f + 2];
    double* o = box + 6 * f;
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= nv || i1 >= nv || i2 >= nv || i0 == i1 || i1 == i2 || i2 == i0) {
        cls[f] = 0;
        for (int k = 0; k < 6; ++k) o[k] = 0.0;
        return;
    }
    double a[3], b[3], c[3];
    bool bounded = true;
    for (int k = 0; k < 3; ++k) {
        a[k] = V[3 * i0 + k], b[k] = V[3 * i1 + k], c[k] = V[3 * i2 + k];
        o[k] = fmin(fmin(a[k], b[k]), c[k]);
        o[3 + k] = fmax(fmax(a[k], b[k]), c[k]);
        bounded = bounded && fabs(a[k]) <= K41_MAX_COORD && fabs(b[k]) <= K41_MAX_COORD && fabs(c[k]) <= K41_MAX_COORD;      // (NaN fails)
    }
    bool nonzero = false, unknown = !bounded;
    for (int k = 0; k < 3 && bounded; ++k) {
        const int u = (k + 1) % 3, v = (k + 2) % 3;
        const int s = orient2d_sign(b[u], b[v], c[u], c[v], a[u], a[v]);
        nonzero = nonzero || strict(s);
        unknown = unknown || s == SG_UNK;
    }
    cls[f] = nonzero ? 1 : (unknown ? 3 : 2);
}

struct K41Out {
    int32_t* cell_counts;              // count: (cells, 2)
    unsigned long long* totals;        // count: candidates, duplicate pairs, decided by one strict plane separation
    unsigned* flag_words;              // count: the faces' flag bytes, four to a word
    const int32_t* out_start;          // emit: (cells + 1)
    int32_t* cursor;                   // emit: (cells)
    int32_t* pairs;                    // emit: (n_out, 2)
    uint8_t* kinds;                    // emit: (n_out)
    int64_t n_out;
};

__device__ __forceinline__ int cell_coord(double x, double lo, double inv, double eps, int n) {      // face_cells' expression (k23_mesh_cull.hip)
    return (int)fmin(fmax(floor((x - lo) * inv + eps), 0.0), (double)(n - 1));
}

template <bool EMIT>
__global__ __launch_bounds__(K41_THREADS) void isect_pairs_k(gens_mesh_grid g, int64_t nv, int64_t n_entries, const uint8_t* __restrict__ cls,
                                                             const double* __restrict__ box, K41Out out) {
    __shared__ double corners[18 * K41_THREADS];
    const double* P = corners + threadIdx.x;
    double* Pw = corners + threadIdx.x;
    const int64_t e = (int64_t)blockIdx.x * K41_THREADS + threadIdx.x;
    unsigned n_cand = 0, n_dup = 0, n_sep = 0;
    int64_t cells = (int64_t)g.nx * g.ny * g.nz;
    bool live = e < n_entries;
    int64_t cell = 0, ce = 0;
    int fx = 0;
    if (live) {
        int64_t lo = 0, hi = cells;              // the last cell whose start is <= e
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)g.cell_start[mid] <= e)
                lo = mid;
            else
                hi = mid;
        }
        cell = lo;
        ce = g.cell_start[cell + 1];
        ce = ce < n_entries ? ce : n_entries;
        fx = g.cell_faces[e];
        live = (int64_t)g.cell_start[cell] <= e && e < ce && fx >= 0 && fx < g.n_faces;
    }
    const int cx = live ? cls[fx] : 0;
    live = live && (cx == 1 || cx == 3);
    if (live) {
        const double lo3[3] = {(double)g.lo_x, (double)g.lo_y, (double)g.lo_z};
        const double inv = 1.0 / (double)g.cell;
        const int n3[3] = {g.nx, g.ny, g.nz};
        const int c3[3] = {(int)(cell / ((int64_t)g.ny * g.nz)), (int)((cell / g.nz) % g.ny), (int)(cell % g.nz)};
        double bx[6];
        for (int k = 0; k < 6; ++k) bx[k] = box[6 * (int64_t)fx + k];
        int ix[3];
        for (int k = 0; k < 3; ++k) ix[k] = cell_coord(bx[k], lo3[k], inv, -K41_GRID_EPS, n3[k]);
        const int32_t x0 = g.triangles[3 * (int64_t)fx], x1 = g.triangles[3 * (int64_t)fx + 1], x2 = g.triangles[3 * (int64_t)fx + 2];
        const bool x_ok = x0 >= 0 && x1 >= 0 && x2 >= 0 && x0 < nv && x1 < nv && x2 < nv;
        if (x_ok && cx == 1) {
            for (int k = 0; k < 3; ++k) {
                Pw[(0 + k) * K41_THREADS] = g.vertices[3 * (int64_t)x0 + k];
                Pw[(3 + k) * K41_THREADS] = g.vertices[3 * (int64_t)x1 + k];
                Pw[(6 + k) * K41_THREADS] = g.vertices[3 * (int64_t)x2 + k];
            }
        }
        const int64_t stride = (int64_t)gridDim.y * K41_CHUNK;
        for (int64_t ys = e + 1 + (int64_t)blockIdx.y * K41_CHUNK; x_ok && ys < ce; ys += stride) {
            const int64_t ye = ys + K41_CHUNK < ce ? ys + K41_CHUNK : ce;
            for (int64_t y = ys; y < ye; ++y) {
                const int fy = g.cell_faces[y];
                if (fy < 0 || fy >= g.n_faces || fy == fx) continue;
                const int cy = cls[fy];
                if (cy != 1 && cy != 3) continue;
                double by[6];
                for (int k = 0; k < 6; ++k) by[k] = box[6 * (int64_t)fy + k];
                bool cand = true;
                for (int k = 0; k < 3; ++k) {
                    const int iy = cell_coord(by[k], lo3[k], inv, -K41_GRID_EPS, n3[k]);
                    cand = cand && bx[k] <= by[3 + k] && by[k] <= bx[3 + k] && (ix[k] > iy ? ix[k] : iy) == c3[k];
                }
                if (!cand) continue;
                const int32_t y0 = g.triangles[3 * (int64_t)fy], y1 = g.triangles[3 * (int64_t)fy + 1], y2 = g.triangles[3 * (int64_t)fy + 2];
                if (!(y0 >= 0 && y1 >= 0 && y2 >= 0 && y0 < nv && y1 < nv && y2 < nv)) continue;
                const int shared = (x0 == y0 || x0 == y1 || x0 == y2) + (x1 == y0 || x1 == y1 || x1 == y2) + (x2 == y0 || x2 == y1 || x2 == y2);
                if (shared == 3) {
                    ++n_dup;
                    continue;
                }
                ++n_cand;
                int res = R_MAYBE;
                if (cx == 1 && cy == 1) {
                    for (int k = 0; k < 3; ++k) {
                        Pw[(9 + k) * K41_THREADS] = g.vertices[3 * (int64_t)y0 + k];
                        Pw[(12 + k) * K41_THREADS] = g.vertices[3 * (int64_t)y1 + k];
                        Pw[(15 + k) * K41_THREADS] = g.vertices[3 * (int64_t)y2 + k];
                    }
                    res = decide_pair(P, x0, x1, x2, y0, y1, y2);
                }
                if (res & K41_SEP) ++n_sep;
                res &= 3;
                if (res == R_NO) continue;
                const int kind = res == R_YES ? 1 : 2;
                if (EMIT) {
                    const int64_t at = (int64_t)out.out_start[cell] + atomicAdd(out.cursor + cell, 1);
                    if (at < out.out_start[cell + 1] && at < out.n_out) {       // (always: the count launch saw the same pairs)
                        out.pairs[2 * at] = fx < fy ? fx : fy;
                        out.pairs[2 * at + 1] = fx < fy ? fy : fx;
                        out.kinds[at] = (uint8_t)kind;
                    }
                } else {
                    atomicAdd(out.cell_counts + 2 * cell + (kind - 1), 1);
                    atomicOr(out.flag_words + (fx >> 2), (unsigned)kind << (8 * (fx & 3)));
                    atomicOr(out.flag_words + (fy >> 2), (unsigned)kind << (8 * (fy & 3)));
                }
            }
        }
    }
    if (!EMIT) {
        for (int d = 32; d > 0; d >>= 1) {
            n_cand += __shfl_down(n_cand, d, 64);
            n_dup += __shfl_down(n_dup, d, 64);
            n_sep += __shfl_down(n_sep, d, 64);
        }
        if ((threadIdx.x & 63) == 0) {
            if (n_cand) atomicAdd(out.totals, (unsigned long long)n_cand);
            if (n_dup) atomicAdd(out.totals + 1, (unsigned long long)n_dup);
            if (n_sep) atomicAdd(out.totals + 2, (unsigned long long)n_sep);
        }
    }
}

// ---------------------------------------------------------------------------------------- entry points
static int k41_check_grid(const char* who, const gens_mesh_grid* g, int64_t nv, int64_t n_entries, int64_t longest) {
    GENS_CHECK_ARG(g, GENS_EINVAL, "%s: null grid", who);
    GENS_CHECK_ARG(g->n_faces >= 0 && nv >= 0 && n_entries >= 0 && longest >= 0, GENS_EINVAL, "%s: %lld faces, %lld vertices, %lld entries, longest list %lld",
                   who, (long long)g->n_faces, (long long)nv, (long long)n_entries, (long long)longest);
    GENS_CHECK_ARG(g->n_faces < K41_LIMIT / 3 + 1 && 3 * g->n_faces < K41_LIMIT && nv < K41_LIMIT && n_entries < K41_LIMIT, GENS_ELIMIT,
                   "%s: %lld faces over %lld vertices, %lld entries (V, 3 T and the entries below 2^31)", who, (long long)g->n_faces, (long long)nv,
                   (long long)n_entries);
    GENS_CHECK_ARG(g->nx >= 1 && g->nx <= K41_GRID_MAX_AXIS && g->ny >= 1 && g->ny <= K41_GRID_MAX_AXIS && g->nz >= 1 && g->nz <= K41_GRID_MAX_AXIS,
                   GENS_ELIMIT, "%s: grid %dx%dx%d (1 .. %d cells per axis)", who, g->nx, g->ny, g->nz, K41_GRID_MAX_AXIS);
    GENS_CHECK_ARG(g->cell > 0.0f && isfinite(g->cell) && isfinite(g->lo_x) && isfinite(g->lo_y) && isfinite(g->lo_z), GENS_ELIMIT, "%s: bad grid box", who);
    return 0;
}

static dim3 k41_pairs_grid(int64_t n_entries, int64_t longest) {
    int64_t slices = (longest + K41_CHUNK - 1) / K41_CHUNK;
    slices = slices < 1 ? 1 : (slices > 65535 ? 65535 : slices);       // (the kernel strides over what is left)
    return dim3(gens_blocks(n_entries, K41_THREADS), (unsigned)slices);
}

extern "C" int gens_mesh_isect_faces(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_faces, uint8_t* face_class,
                                     double* face_box, void* stream) {
    const char* who = "gens_mesh_isect_faces";
    GENS_CHECK_ARG(n_vertices >= 0 && n_faces >= 0, GENS_EINVAL, "%s: %lld vertices, %lld faces", who, (long long)n_vertices, (long long)n_faces);
    GENS_CHECK_ARG(n_vertices < K41_LIMIT && n_faces < K41_LIMIT / 3 + 1 && 3 * n_faces < K41_LIMIT, GENS_ELIMIT,
                   "%s: %lld faces over %lld vertices (V and 3 T below 2^31)", who, (long long)n_faces, (long long)n_vertices);
    if (n_faces == 0) return 0;
    GENS_CHECK_ARG(triangles && face_class && face_box && (vertices || n_vertices == 0), GENS_EINVAL, "%s: null pointer", who);
    isect_faces_k<<<gens_blocks(n_faces, K41_THREADS), K41_THREADS, 0, (hipStream_t)stream>>>(vertices, n_vertices, triangles, n_faces, face_class,
                                                                                              face_box);
    return gens_launch_status(who);
}

extern "C" int gens_mesh_isect_count(const gens_mesh_grid* grid, int64_t n_vertices, int64_t n_entries, int64_t longest_list,
                                     const uint8_t* face_class, const double* face_box, int32_t* cell_counts, int64_t* totals,
                                     uint8_t* face_flags, void* stream) {
    const char* who = "gens_mesh_isect_count";
    if (int rc = k41_check_grid(who, grid, n_vertices, n_entries, longest_list)) return rc;
    if (grid->n_faces == 0 || n_entries == 0) return 0;
    GENS_CHECK_ARG(grid->vertices && grid->triangles && grid->cell_start && grid->cell_faces && face_class && face_box && cell_counts && totals &&
                       face_flags,
                   GENS_EINVAL, "%s: null pointer", who);
    GENS_CHECK_ARG(((uintptr_t)face_flags & 3) == 0 && ((uintptr_t)totals & 7) == 0, GENS_EINVAL, "%s: face_flags is not 4-byte aligned, or totals not 8-byte",
                   who);
    K41Out out = {};
    out.cell_counts = cell_counts;
    out.totals = (unsigned long long*)totals;
    out.flag_words = (unsigned*)face_flags;
    isect_pairs_k<false><<<k41_pairs_grid(n_entries, longest_list), K41_THREADS, 0, (hipStream_t)stream>>>(*grid, n_vertices, n_entries, face_class,
                                                                                                          face_box, out);
    return gens_launch_status(who);
}

extern "C" int gens_mesh_isect_emit(const gens_mesh_grid* grid, int64_t n_vertices, int64_t n_entries, int64_t longest_list,
                                    const uint8_t* face_class, const double* face_box, const int32_t* out_start, int32_t* cursor, int64_t n_out,
                                    int32_t* pairs, uint8_t* kinds, void* stream) {
    const char* who = "gens_mesh_isect_emit";
    if (int rc = k41_check_grid(who, grid, n_vertices, n_entries, longest_list)) return rc;
    GENS_CHECK_ARG(n_out >= 0, GENS_EINVAL, "%s: %lld pairs", who, (long long)n_out);
    GENS_CHECK_ARG(n_out < K41_LIMIT, GENS_ELIMIT, "%s: %lld pairs (below 2^31)", who, (long long)n_out);
    if (grid->n_faces == 0 || n_entries == 0 || n_out == 0) return 0;
    GENS_CHECK_ARG(grid->vertices && grid->triangles && grid->cell_start && grid->cell_faces && face_class && face_box && out_start && cursor &&
                       pairs && kinds,
                   GENS_EINVAL, "%s: null pointer", who);
    K41Out out = {};
    out.out_start = out_start;
    out.cursor = cursor;
    out.pairs = pairs;
    out.kinds = kinds;
    out.n_out = n_out;
    isect_pairs_k<true><<<k41_pairs_grid(n_entries, longest_list), K41_THREADS, 0, (hipStream_t)stream>>>(*grid, n_vertices, n_entries, face_class,
                                                                                                         face_box, out);
    return gens_launch_status(who);
}
