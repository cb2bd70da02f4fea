// K23: the ray-cast half of the reference's validation-mesh cleaning on the device.
//
// Replaces clean_mesh_outside_frustum (/root/reference/utils/clean_mesh.py:38-106): pyembree's intersects_first for every masked,
// upsampled pixel of every view, then trimesh's face-adjacency components.  Four pieces:
//   grid count / fill: a uniform grid of cubic cells over the mesh, built by counting sort -- every face is listed in every cell its
//            closed AABB (widened by GRID_EPS cells) overlaps; the caller scans the counts in between;
//   first hit: one thread per ray, a 3-D DDA through the grid; each listed face gets the watertight ray / triangle test of Woop, Benthin
//            and Wald (JCGT 2013); both sides count (Embree's default), t > 0; the winner is the lexicographic minimum of (t, face), so
//            the order inside a cell's list does not matter; the walk stops once the best t is <= the current cell's exit t;
//   view rays: the same walk for the rays clean_mesh.py:50-66 builds, generated per pixel in the kernel (float32, in the order of ATen's CPU
//            kernels), marking the faces hit and whether a masked ray missed -- one kernel template for this cleaner (float masks,
//            upsampled, one row of flags for all views) and for K25's evaluation/clean_meshes.py:212-246 (uint8 masks, 1:1, rays that
//            start dep_min down the ray, one row per view);
//   components: union-find over the pairs of faces that share an edge used by exactly two faces (ECL-CC style: a hook launch with
//            agent-scope atomics on every parent access, then a compress launch), roots = smallest face index of each component.
//
// The intersection test runs in double precision throughout (vertices float64, rays widened from float32): the paper's float32 test
// with its double fallback for an edge function that is exactly 0 reduces to this one branch-free path, and the hits then agree with a
// float64 reference to ~1e-13 instead of float32's ~1e-4 relative to a lattice-sized triangle.  Watertightness does not depend on the
// precision: an edge's function is the same products in both of its faces (-ffp-contract=off keeps them unfused), exactly negated.
#include <math.h>

#include "common.h"

#define GRID_MAX_AXIS 512
#define GRID_EPS 1e-5   // (cells) widening of every face's AABB: covers the rounding of the cell coordinates and of the walk's exit t

// face f's cell range [i0, i1] per axis, clamped into the grid (NaN coordinates land in cell 0)
__device__ __forceinline__ void face_cells(const gens_mesh_grid& g, int64_t f, int i0[3], int i1[3]) {
    const int32_t* tri = g.triangles + 3 * f;
    const double lo[3] = {(double)g.lo_x, (double)g.lo_y, (double)g.lo_z};
    const double inv = 1.0 / (double)g.cell;
    const int n[3] = {g.nx, g.ny, g.nz};
    double mn[3], mx[3];
    for (int a = 0; a < 3; ++a) mn[a] = mx[a] = g.vertices[3 * (int64_t)tri[0] + a];
    for (int k = 1; k < 3; ++k)
        for (int a = 0; a < 3; ++a) {
            const double c = g.vertices[3 * (int64_t)tri[k] + a];
            mn[a] = fmin(mn[a], c);
            mx[a] = fmax(mx[a], c);
        }
    for (int a = 0; a < 3; ++a) {
        const double top = (double)(n[a] - 1);
        i0[a] = (int)fmin(fmax(floor((mn[a] - lo[a]) * inv - GRID_EPS), 0.0), top);
        i1[a] = (int)fmin(fmax(floor((mx[a] - lo[a]) * inv + GRID_EPS), 0.0), top);
    }
}

__global__ __launch_bounds__(256) void grid_count_k(gens_mesh_grid g, int32_t* __restrict__ counts) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= g.n_faces) return;
    int i0[3], i1[3];
    face_cells(g, f, i0, i1);
    for (int i = i0[0]; i <= i1[0]; ++i)
        for (int j = i0[1]; j <= i1[1]; ++j)
            for (int k = i0[2]; k <= i1[2]; ++k) atomicAdd(counts + ((int64_t)i * g.ny + j) * g.nz + k, 1);
}

__global__ __launch_bounds__(256) void grid_fill_k(gens_mesh_grid g, int32_t* __restrict__ cursor) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= g.n_faces) return;
    int i0[3], i1[3];
    face_cells(g, f, i0, i1);
    for (int i = i0[0]; i <= i1[0]; ++i)
        for (int j = i0[1]; j <= i1[1]; ++j)
            for (int k = i0[2]; k <= i1[2]; ++k) {
                const int64_t c = ((int64_t)i * g.ny + j) * g.nz + k;
                const int64_t at = (int64_t)g.cell_start[c] + atomicAdd(cursor + c, 1);
                if (at < g.cell_start[c + 1]) g.cell_faces[at] = (int32_t)f;     // (always: the count pass saw the same ranges)
            }
}

// A ray in the form the watertight test wants: kz = the axis of the largest |d|, (kx, ky) the other two in winding-preserving order,
// and the shear that maps d to (0, 0, 1).
struct WRay {
    double o[3], d[3];
    double sx, sy, sz;
    int kx, ky, kz;
};

__device__ __forceinline__ bool wray_setup(float ox, float oy, float oz, float dx, float dy, float dz, WRay& r) {
    r.o[0] = ox, r.o[1] = oy, r.o[2] = oz;
    r.d[0] = dx, r.d[1] = dy, r.d[2] = dz;
    const double ax = fabs(r.d[0]), ay = fabs(r.d[1]), az = fabs(r.d[2]);
    r.kz = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
    const double dk = r.d[r.kz];
    if (!(fabs(dk) > 0.0) || !isfinite(r.o[0] + r.o[1] + r.o[2]) || !isfinite(r.d[0] + r.d[1] + r.d[2])) return false;
    r.kx = r.kz == 2 ? 0 : r.kz + 1;
    r.ky = r.kx == 2 ? 0 : r.kx + 1;
    if (dk < 0.0) {
        const int s = r.kx;
        r.kx = r.ky, r.ky = s;
    }
    r.sx = r.d[r.kx] / dk;
    r.sy = r.d[r.ky] / dk;
    r.sz = 1.0 / dk;
    return true;
}

// Woop, Benthin, Wald 2013: edge functions of the sheared, translated triangle; inside iff they do not disagree in sign (0 counts as
// inside, so a ray through a shared edge or vertex hits at least one of its faces); both orientations; t > 0.
__device__ __forceinline__ bool wray_hit(const WRay& r, const double* __restrict__ V, const int32_t* __restrict__ tri, double& t) {
    double A[3], B[3], C[3];
    for (int a = 0; a < 3; ++a) {
        A[a] = V[3 * (int64_t)tri[0] + a] - r.o[a];
        B[a] = V[3 * (int64_t)tri[1] + a] - r.o[a];
        C[a] = V[3 * (int64_t)tri[2] + a] - r.o[a];
    }
    const double Ax = A[r.kx] - r.sx * A[r.kz], Ay = A[r.ky] - r.sy * A[r.kz];
    const double Bx = B[r.kx] - r.sx * B[r.kz], By = B[r.ky] - r.sy * B[r.kz];
    const double Cx = C[r.kx] - r.sx * C[r.kz], Cy = C[r.ky] - r.sy * C[r.kz];
    const double U = Cx * By - Cy * Bx;
    const double Vv = Ax * Cy - Ay * Cx;
    const double W = Bx * Ay - By * Ax;
    if ((U < 0.0 || Vv < 0.0 || W < 0.0) && (U > 0.0 || Vv > 0.0 || W > 0.0)) return false;
    const double det = U + Vv + W;
    if (det == 0.0) return false;
    const double T = U * (r.sz * A[r.kz]) + Vv * (r.sz * B[r.kz]) + W * (r.sz * C[r.kz]);
    t = T / det;
    return t > 0.0;     // (NaN fails)
}

// First hit of one ray: (face, t) with the smallest (t, face), face = -1 and t = +inf on a miss.
__device__ int first_hit(const gens_mesh_grid& g, const WRay& r, double& best_t) {
    best_t = INFINITY;
    int best_f = -1;
    const double inv = 1.0 / (double)g.cell;
    const double lo[3] = {(double)g.lo_x, (double)g.lo_y, (double)g.lo_z};
    const int n[3] = {g.nx, g.ny, g.nz};
    double p[3], q[3], iq[3];       // the ray in cell units: p + t q
    double t0 = 0.0, t1 = INFINITY;
    for (int a = 0; a < 3; ++a) {
        p[a] = (r.o[a] - lo[a]) * inv;
        q[a] = r.d[a] * inv;
        iq[a] = 1.0 / q[a];
        if (q[a] != 0.0) {
            double ta = (0.0 - p[a]) * iq[a], tb = ((double)n[a] - p[a]) * iq[a];
            if (ta > tb) {
                const double s = ta;
                ta = tb, tb = s;
            }
            t0 = fmax(t0, ta);
            t1 = fmin(t1, tb);
        } else if (!(p[a] >= 0.0 && p[a] <= (double)n[a])) {
            return -1;
        }
    }
    if (!(t0 <= t1)) return -1;
    int c[3], step[3];
    for (int a = 0; a < 3; ++a) {
        c[a] = (int)fmin(fmax(floor(p[a] + t0 * q[a]), 0.0), (double)(n[a] - 1));
        step[a] = q[a] > 0.0 ? 1 : (q[a] < 0.0 ? -1 : 0);
    }
    for (int it = n[0] + n[1] + n[2] + 3; it > 0; --it) {       // (a walk crosses each plane at most once: the bound is never reached)
        double tn[3];
        for (int a = 0; a < 3; ++a)
            tn[a] = step[a] > 0 ? ((double)(c[a] + 1) - p[a]) * iq[a] : (step[a] < 0 ? ((double)c[a] - p[a]) * iq[a] : INFINITY);
        const int ax = (tn[0] <= tn[1] && tn[0] <= tn[2]) ? 0 : (tn[1] <= tn[2] ? 1 : 2);
        const int64_t cell = ((int64_t)c[0] * n[1] + c[1]) * n[2] + c[2];
        const int32_t e = g.cell_start[cell + 1];
        for (int32_t k = g.cell_start[cell]; k < e; ++k) {
            const int f = g.cell_faces[k];
            double t;
            if (wray_hit(r, g.vertices, g.triangles + 3 * (int64_t)f, t) && (t < best_t || (t == best_t && f < best_f))) {
                best_t = t;
                best_f = f;
            }
        }
        if (best_t <= tn[ax]) break;
        c[ax] += step[ax];
        if (c[ax] < 0 || c[ax] >= n[ax]) break;
    }
    return best_f;
}

__global__ __launch_bounds__(256) void ray_first_hit_k(gens_mesh_grid g, const float* __restrict__ ro, const float* __restrict__ rd, int64_t n,
                                                       int32_t* __restrict__ face, float* __restrict__ t_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    WRay r;
    double t = INFINITY;
    int f = -1;
    if (wray_setup(ro[3 * i], ro[3 * i + 1], ro[3 * i + 2], rd[3 * i], rd[3 * i + 1], rd[3 * i + 2], r)) f = first_hit(g, r, t);
    face[i] = f;
    t_out[i] = f >= 0 ? (float)t : INFINITY;
}

// torch.linspace(start, end, steps)[i] as ATen's CPU kernel computes it in float32: the two halves counted from either end, each a fused
// multiply-add (the vectorised kernel's, and its scalar tail's).
__device__ __forceinline__ float linspace_cpu(float start, float end, int steps, int i) {
    if (steps == 1) return start;
    const float step = (end - start) / (float)(steps - 1);
    return i < steps / 2 ? fmaf(step, (float)i, start) : fmaf(-step, (float)(steps - 1 - i), end);
}

// The direction of the ray through pixel (x, y) of a view (cam: 21 floats, K^-1[:3,:3] row-major then c2w[:3,:4]), operation for operation
// as torch evaluates clean_mesh.py:50-66 on the CPU: p = K^-1 (x, y, 1) (bmm: plain products, summed left to right from 0); p / ||p|| (the
// norm's sum of squares by fused multiply-adds, then a correctly rounded square root and quotient); R p the same way as K^-1 p.
__device__ __forceinline__ void view_ray_dir(const float* __restrict__ cam, float x, float y, float rdir[3]) {
    const float* K = cam;
    const float* M = cam + 9;
    float q[3], d[3];
    for (int a = 0; a < 3; ++a) q[a] = ((0.0f + K[3 * a] * x) + K[3 * a + 1] * y) + K[3 * a + 2] * 1.0f;
    const float nrm = (float)sqrt((double)fmaf(q[2], q[2], fmaf(q[1], q[1], q[0] * q[0])));
    for (int a = 0; a < 3; ++a) d[a] = (float)((double)q[a] / (double)nrm);
    for (int a = 0; a < 3; ++a) rdir[a] = ((0.0f + M[4 * a] * d[0]) + M[4 * a + 1] * d[1]) + M[4 * a + 2] * d[2];
}

// The view rays of both mesh cleaners: one thread per pixel of the (hu, wu) image of view blockIdx.y, (x, y) from linspace over the
// (h, w) source image.  The pixel casts iff its nearest source pixel's mask is > threshold (F.interpolate's rule: source =
// min(floor(dst * (float)(1 / upscale)), size - 1); the pixel itself for hu = h, wu = w, inv_scale = 1, as long as h and w are below 2^24,
// where float32 still holds every index -- beyond any image: the entry points bound only h * w).  The ray is view_ray_dir's from
// c2w[:3, 3] advanced down the ray, o + d * dep_min, as a float32 product and a float32 sum (the file is compiled unfused); for
// dep_min = 0 a finite d adds +-0, which no later comparison sees, and a non-finite d is rejected by wray_setup either way.  View v marks
// the faces its rays hit first in flags + v * flag_stride and a cast ray that missed in any_miss[v * miss_stride].
//   K23 (utils/clean_mesh.py:45-78): float masks > 0, upsampled, dep_min = 0, one row for all views (strides 0, 0);
//   K25 (evaluation/clean_meshes.py:212-246): uint8 (dilated) masks > 128 (:235), 1:1, dep_min (:239), one row per view (strides
//   n_faces, 1): the script's Counter sees a face, and the -1 of the misses, once per view.
template <typename MaskT>
__global__ __launch_bounds__(256) void view_rays_k(gens_mesh_grid g, const MaskT* __restrict__ masks, MaskT threshold, const float* __restrict__ cams,
                                                   int h, int w, int hu, int wu, float inv_scale, float dep_min, int64_t flag_stride,
                                                   int miss_stride, uint8_t* __restrict__ flags, int32_t* __restrict__ any_miss) {
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= (int64_t)hu * wu) return;
    const int v = blockIdx.y;
    const int i = (int)(pix / wu), j = (int)(pix % wu);
    const int si = (int)fminf(floorf((float)i * inv_scale), (float)(h - 1));
    const int sj = (int)fminf(floorf((float)j * inv_scale), (float)(w - 1));
    if (!(masks[((int64_t)v * h + si) * w + sj] > threshold)) return;
    const float* M = cams + 21 * v + 9;
    float rdir[3], o[3];
    view_ray_dir(cams + 21 * v, linspace_cpu(0.0f, (float)(w - 1), wu, j), linspace_cpu(0.0f, (float)(h - 1), hu, i), rdir);
    for (int a = 0; a < 3; ++a) {
        const float adv = rdir[a] * dep_min;
        o[a] = M[4 * a + 3] + adv;
    }
    WRay r;
    double t = INFINITY;
    int f = -1;
    if (wray_setup(o[0], o[1], o[2], rdir[0], rdir[1], rdir[2], r)) f = first_hit(g, r, t);
    if (f >= 0)
        flags[(int64_t)v * flag_stride + f] = 1;       // (every writer stores the same value)
    else
        any_miss[v * miss_stride] = 1;
}

// ------------------------------------------------------------------------------------------------ components
__global__ __launch_bounds__(256) void cc_hook_k(const int32_t* __restrict__ pairs, int64_t n_pairs, int32_t* parent, int64_t n_faces) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pairs) return;
    int32_t a = pairs[2 * i], b = pairs[2 * i + 1];
    if (a < 0 || b < 0 || a >= n_faces || b >= n_faces) return;       // (the caller's pairs are face ids; nothing else is touched)
    gens_union_min(parent, a, b);
}

__global__ __launch_bounds__(256) void cc_compress_k(const int32_t* __restrict__ parent, int64_t n, int32_t* __restrict__ label) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= n) return;
    int32_t x = (int32_t)f, p = parent[x];
    while (p != x) {
        x = p;
        p = parent[x];
    }
    label[f] = x;
}

// ------------------------------------------------------------------------------------------------ entry points
static int check_grid(const gens_mesh_grid* g, bool lists, const char* who) {
    GENS_CHECK_ARG(g, GENS_EINVAL, "%s: null grid", who);
    GENS_CHECK_ARG(g->vertices && g->triangles && (!lists || (g->cell_start && g->cell_faces)), GENS_EINVAL, "%s: null pointer", who);
    GENS_CHECK_ARG(g->n_faces >= 0 && g->n_faces < ((int64_t)1 << 31), GENS_ELIMIT, "%s: %lld faces", who, (long long)g->n_faces);
    GENS_CHECK_ARG(g->nx >= 1 && g->nx <= GRID_MAX_AXIS && g->ny >= 1 && g->ny <= GRID_MAX_AXIS && g->nz >= 1 && g->nz <= GRID_MAX_AXIS, GENS_ELIMIT,
                   "%s: grid %dx%dx%d (1 .. %d cells per axis)", who, g->nx, g->ny, g->nz, GRID_MAX_AXIS);
    GENS_CHECK_ARG(g->cell > 0.0f && isfinite(g->cell) && isfinite(g->lo_x) && isfinite(g->lo_y) && isfinite(g->lo_z), GENS_ELIMIT,
                   "%s: bad grid box", who);
    return 0;
}

extern "C" int gens_mesh_grid_count(const gens_mesh_grid* g, int32_t* counts, void* stream) {
    if (int rc = check_grid(g, false, "gens_mesh_grid_count")) return rc;
    GENS_CHECK_ARG(counts, GENS_EINVAL, "gens_mesh_grid_count: null counts");
    if (g->n_faces == 0) return 0;
    grid_count_k<<<gens_blocks(g->n_faces, 256), 256, 0, (hipStream_t)stream>>>(*g, counts);
    return gens_launch_status("gens_mesh_grid_count");
}

extern "C" int gens_mesh_grid_fill(const gens_mesh_grid* g, int32_t* cursor, void* stream) {
    if (int rc = check_grid(g, true, "gens_mesh_grid_fill")) return rc;
    GENS_CHECK_ARG(cursor, GENS_EINVAL, "gens_mesh_grid_fill: null cursor");
    if (g->n_faces == 0) return 0;
    grid_fill_k<<<gens_blocks(g->n_faces, 256), 256, 0, (hipStream_t)stream>>>(*g, cursor);
    return gens_launch_status("gens_mesh_grid_fill");
}

extern "C" int gens_ray_first_hit(const gens_mesh_grid* g, const float* rays_o, const float* rays_d, int64_t n_rays, int32_t* face, float* t,
                                  void* stream) {
    if (int rc = check_grid(g, true, "gens_ray_first_hit")) return rc;
    GENS_CHECK_ARG(rays_o && rays_d && face && t, GENS_EINVAL, "gens_ray_first_hit: null pointer");
    GENS_CHECK_ARG(n_rays >= 0 && n_rays < ((int64_t)1 << 31), GENS_ELIMIT, "gens_ray_first_hit: %lld rays", (long long)n_rays);
    if (n_rays == 0) return 0;
    ray_first_hit_k<<<gens_blocks(n_rays, 256), 256, 0, (hipStream_t)stream>>>(*g, rays_o, rays_d, n_rays, face, t);
    return gens_launch_status("gens_ray_first_hit");
}

// what the two view-ray entry points check alike: the grid with its lists, and the pointers
static int check_view_rays(const gens_mesh_grid* g, const void* masks, const float* cams, const uint8_t* flags, const int32_t* any_miss,
                           const char* who) {
    if (int rc = check_grid(g, true, who)) return rc;
    GENS_CHECK_ARG(masks && cams && flags && any_miss, GENS_EINVAL, "%s: null pointer", who);
    return 0;
}

extern "C" int gens_view_rays_hit_faces(const gens_mesh_grid* g, const float* masks, const float* cams, int nv, int h, int w, int hu, int wu,
                                        float inv_scale, uint8_t* flags, int32_t* any_miss, void* stream) {
    if (int rc = check_view_rays(g, masks, cams, flags, any_miss, "gens_view_rays_hit_faces")) return rc;
    GENS_CHECK_ARG(nv >= 1 && nv <= 65535 && h >= 1 && w >= 1 && hu >= 1 && wu >= 1 && (int64_t)hu * wu < ((int64_t)1 << 31) &&
                       (int64_t)h * w < ((int64_t)1 << 31),
                   GENS_ELIMIT, "gens_view_rays_hit_faces: %d views of %dx%d, upsampled %dx%d", nv, h, w, hu, wu);
    GENS_CHECK_ARG(inv_scale > 0.0f && isfinite(inv_scale), GENS_ELIMIT, "gens_view_rays_hit_faces: 1 / upscale = %g", (double)inv_scale);
    const dim3 grid(gens_blocks((int64_t)hu * wu, 256), (unsigned)nv);
    view_rays_k<float><<<grid, 256, 0, (hipStream_t)stream>>>(*g, masks, 0.0f, cams, h, w, hu, wu, inv_scale, 0.0f, 0, 0, flags, any_miss);
    return gens_launch_status("gens_view_rays_hit_faces");
}

extern "C" int gens_view_rays_hit_counts(const gens_mesh_grid* g, const uint8_t* masks, const float* cams, int nv, int h, int w, float dep_min,
                                         uint8_t* flags, int32_t* any_miss, void* stream) {
    if (int rc = check_view_rays(g, masks, cams, flags, any_miss, "gens_view_rays_hit_counts")) return rc;
    GENS_CHECK_ARG(nv >= 1 && nv <= 65535 && h >= 1 && w >= 1 && (int64_t)h * w < ((int64_t)1 << 31), GENS_ELIMIT,
                   "gens_view_rays_hit_counts: %d views of %dx%d", nv, h, w);
    GENS_CHECK_ARG(isfinite(dep_min), GENS_ELIMIT, "gens_view_rays_hit_counts: dep_min = %g", (double)dep_min);
    const dim3 grid(gens_blocks((int64_t)h * w, 256), (unsigned)nv);
    view_rays_k<uint8_t><<<grid, 256, 0, (hipStream_t)stream>>>(*g, masks, (uint8_t)128, cams, h, w, h, w, 1.0f, dep_min, g->n_faces, 1, flags,
                                                                 any_miss);
    return gens_launch_status("gens_view_rays_hit_counts");
}

extern "C" int gens_face_cc_hook(const int32_t* pairs, int64_t n_pairs, int32_t* parent, int64_t n_faces, void* stream) {
    GENS_CHECK_ARG(pairs && parent, GENS_EINVAL, "gens_face_cc_hook: null pointer");
    GENS_CHECK_ARG(n_pairs >= 0 && n_pairs < ((int64_t)1 << 31) && n_faces >= 0 && n_faces < ((int64_t)1 << 31), GENS_ELIMIT,
                   "gens_face_cc_hook: %lld pairs over %lld faces", (long long)n_pairs, (long long)n_faces);
    if (n_pairs == 0) return 0;
    cc_hook_k<<<gens_blocks(n_pairs, 256), 256, 0, (hipStream_t)stream>>>(pairs, n_pairs, parent, n_faces);
    return gens_launch_status("gens_face_cc_hook");
}

extern "C" int gens_face_cc_compress(const int32_t* parent, int64_t n_faces, int32_t* label, void* stream) {
    GENS_CHECK_ARG(parent && label, GENS_EINVAL, "gens_face_cc_compress: null pointer");
    GENS_CHECK_ARG(n_faces >= 0 && n_faces < ((int64_t)1 << 31), GENS_ELIMIT, "gens_face_cc_compress: %lld faces", (long long)n_faces);
    if (n_faces == 0) return 0;
    cc_compress_k<<<gens_blocks(n_faces, 256), 256, 0, (hipStream_t)stream>>>(parent, n_faces, label);
    return gens_launch_status("gens_face_cc_compress");
}
