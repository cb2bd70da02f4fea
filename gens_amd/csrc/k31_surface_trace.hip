// K31: sphere tracing of the surface sdf + threshold = 0 along camera rays (ops.sphere_trace, ImplicitSurface.render_surface): the streaming
// launches between the network evaluations.  The definition is the comment of K31 in include/gens_hip.h; tests/surface_trace_reference.py
// restates it in numpy and the kernels equal that restatement bit for bit.
//
//   begin:   the slab test of every ray against the box and [near, far] -> the state of a LIVE ray at t0, or MISS / BAD; first points.
//   march:   one round: g = sdf + threshold at the point of every ray of a (compacted) list -> the next state, the next point, a live flag.
//   refine:  one bisection round of the BRACKET rays of a list; in its final mode the linear interpolation and HIT.
//   gather:  rows of the per-ray point array picked by a list -> the dense batch the evaluator takes.
//   pack:    t, the ray and gradient / colour / flags at the hit points -> depth, normal, normal image, 8-bit colour, seen, hit.
//
// One thread per ray (or list entry), 32-bit indices (n < 2^31 is an argument check).  The per-ray records are 4 and 12 bytes wide: a wave
// reads contiguous spans of its 64 rows when the list is the identity and scattered rows otherwise -- these launches move a few bytes per ray
// and are not what a trace waits for; the point is that every float32 operation is rounded on its own (no contraction) in the stated order.
// Divergent branches are short (a handful of stores each), so both sides of every `if` run predicated in a few cycles.
#include <math.h>

#include "common.h"
#include "pack_rules.h"

#pragma clang fp contract(off)

enum : uint8_t { T_LIVE = GENS_TRACE_LIVE, T_HIT = GENS_TRACE_HIT, T_MISS = GENS_TRACE_MISS, T_INSIDE = GENS_TRACE_INSIDE,
                 T_EXHAUSTED = GENS_TRACE_EXHAUSTED, T_BAD = GENS_TRACE_BAD, T_BRACKET = GENS_TRACE_BRACKET };

struct Box3 {
    float lo[3], hi[3];
};

__device__ __forceinline__ void write_point(const gens_trace_state& s, int r, float t) {
    for (int a = 0; a < 3; ++a) s.points[3 * r + a] = s.rays_o[3 * r + a] + t * s.rays_d[3 * r + a];
}

__global__ __launch_bounds__(256) void trace_begin_k(gens_trace_state s, const float* __restrict__ near, const float* __restrict__ far, int per_ray, Box3 box) {
    const int r = (int)(blockIdx.x * 256u + threadIdx.x);
    if (r >= (int)s.n) return;
    float o[3], d[3];
    bool finite = true;
    for (int a = 0; a < 3; ++a) {
        o[a] = s.rays_o[3 * r + a];
        d[a] = s.rays_d[3 * r + a];
        finite = finite && isfinite(o[a]) && isfinite(d[a]);
    }
    const double dx = d[0], dy = d[1], dz = d[2];
    const float len = (float)sqrt((dx * dx + dy * dy) + dz * dz);       // float64 from the float32 components, rounded once
    float t0 = near[per_ray ? r : 0], t1 = far[per_ray ? r : 0];
    bool miss = false;
    for (int a = 0; a < 3; ++a) {
        if (d[a] == 0.f) {
            if (!(box.lo[a] <= o[a] && o[a] <= box.hi[a])) miss = true;   // (else this axis bounds nothing: (-inf, +inf))
        } else {
            const float ta = (box.lo[a] - o[a]) / d[a], tb = (box.hi[a] - o[a]) / d[a];
            const float enter = ta < tb ? ta : tb, leave = ta < tb ? tb : ta;
            if (enter > t0) t0 = enter;
            if (leave < t1) t1 = leave;
        }
    }
    uint8_t st = T_LIVE;
    if (!finite) st = T_BAD;
    else if (miss || !(len > 0.f) || !(t0 < t1)) st = T_MISS;
    const bool live = st == T_LIVE;
    const float t = live ? t0 : 0.f;
    s.t[r] = t;
    s.t_lo[r] = t;
    s.t_hi[r] = t;
    s.g_lo[r] = 0.f;
    s.g_hi[r] = 0.f;
    s.t_end[r] = live ? t1 : 0.f;
    s.dlen[r] = len;
    s.status[r] = st;
    s.steps[r] = 0;
    s.live[r] = live ? 1 : 0;
    if (live) {
        write_point(s, r, t);
    } else {
        for (int a = 0; a < 3; ++a) s.points[3 * r + a] = 0.f;
    }
}

__global__ __launch_bounds__(256) void trace_march_k(gens_trace_state s, const float* __restrict__ sdf, const int64_t* __restrict__ idx, int m, float threshold,
                                                     float lipschitz, float min_step, int max_steps) {
    const int j = (int)(blockIdx.x * 256u + threadIdx.x);
    if (j >= m) return;
    const int64_t r64 = idx ? idx[j] : j;
    if (r64 < 0 || r64 >= s.n) return;                    // (a list entry outside the rays: nothing of this launch's to touch)
    const int r = (int)r64;
    if (s.status[r] != T_LIVE) return;
    const float g = sdf[j] + threshold;
    const float t = s.t[r];
    const int k = s.steps[r] + 1;
    s.steps[r] = k;
    uint8_t st = T_LIVE;
    if (!isfinite(g)) {
        st = T_BAD;
    } else if (g <= 0.f) {
        if (k == 1) {
            st = T_INSIDE;
        } else {
            st = T_BRACKET;
            s.t_hi[r] = t;
            s.g_hi[r] = g;
            const float tm = 0.5f * (s.t_lo[r] + t);      // the first refine round's point
            s.t[r] = tm;
            write_point(s, r, tm);
        }
    } else if (t == s.t_end[r]) {
        st = T_MISS;
    } else if (k == max_steps) {
        st = T_EXHAUSTED;
    } else {
        s.t_lo[r] = t;
        s.g_lo[r] = g;
        const float q = g / lipschitz;
        const float step = (q > min_step ? q : min_step) / s.dlen[r];
        const float tn = t + step, te = s.t_end[r];
        const float t_next = tn < te ? tn : te;
        s.t[r] = t_next;
        write_point(s, r, t_next);
    }
    s.status[r] = st;
    s.live[r] = st == T_LIVE ? 1 : 0;
}

__global__ __launch_bounds__(256) void trace_refine_k(gens_trace_state s, const float* __restrict__ sdf, const int64_t* __restrict__ idx, int m, float threshold,
                                                      int final) {
    const int j = (int)(blockIdx.x * 256u + threadIdx.x);
    if (j >= m) return;
    const int64_t r64 = idx ? idx[j] : j;
    if (r64 < 0 || r64 >= s.n) return;
    const int r = (int)r64;
    if (s.status[r] != T_BRACKET) return;
    float t_lo = s.t_lo[r], t_hi = s.t_hi[r], g_lo = s.g_lo[r], g_hi = s.g_hi[r];
    if (sdf) {
        const float g = sdf[j] + threshold, tm = s.t[r];
        if (g <= 0.f) {
            t_hi = tm;
            g_hi = g;
        } else {
            t_lo = tm;
            g_lo = g;
        }
        s.t_lo[r] = t_lo;
        s.t_hi[r] = t_hi;
        s.g_lo[r] = g_lo;
        s.g_hi[r] = g_hi;
    }
    float t;
    if (final) {
        t = t_lo + (t_hi - t_lo) * (g_lo / (g_lo - g_hi));
        s.status[r] = T_HIT;
    } else {
        t = 0.5f * (t_lo + t_hi);
    }
    s.t[r] = t;
    write_point(s, r, t);
}

__global__ __launch_bounds__(256) void trace_gather_k(const float* __restrict__ points, const int64_t* __restrict__ idx, int m3, int64_t n, float* __restrict__ out) {
    const int e = (int)(blockIdx.x * 256u + threadIdx.x);
    if (e >= m3) return;
    const int64_t r = idx[e / 3];
    out[e] = (r >= 0 && r < n) ? points[3 * r + e % 3] : 0.f;
}

__global__ __launch_bounds__(256) void surface_pack_k(gens_surface_pack_args a) {
    const int j = (int)(blockIdx.x * 256u + threadIdx.x);
    if (j >= (int)a.m) return;
    const int64_t r64 = a.idx ? a.idx[j] : j;
    if (r64 < 0 || r64 >= a.n) return;
    const int r = (int)r64;
    const bool hit = a.status[r] == T_HIT;
    if (a.hit) a.hit[r] = hit ? 1 : 0;
    if (a.depth) a.depth[r] = hit ? gens_pack_depth(a.rot, a.t[r], a.rays_d[3 * r], a.rays_d[3 * r + 1], a.rays_d[3 * r + 2]) : 0.f;
    if (a.grad) {
        float nx = 0.f, ny = 0.f, nz = 0.f;
        if (hit) gens_unit_normal(a.grad[3 * j], a.grad[3 * j + 1], a.grad[3 * j + 2], nx, ny, nz);
        if (a.normal) {
            a.normal[3 * r] = nx;
            a.normal[3 * r + 1] = ny;
            a.normal[3 * r + 2] = nz;
        }
        if (a.normal_img) {
            for (int k = 0; k < 3; ++k)
                a.normal_img[3 * r + k] = hit ? gens_normal_img(a.rot, k, nx, ny, nz) : 0.f;
        }
    }
    if (a.color) {
        for (int k = 0; k < 3; ++k) a.img[3 * r + k] = hit ? gens_color8(a.color[3 * j + k]) : 0;
        a.seen[r] = hit ? gens_any_flag(a.vis + (int64_t)j * a.n_src, a.n_src) : 0;
    }
}

// ------------------------------------------------------------------------------------------------ entry points
static int check_state(const char* who, const gens_trace_state* s) {
    GENS_CHECK_ARG(s, GENS_EINVAL, "%s: null pointer (the state)", who);
    GENS_CHECK_ARG(s->n >= 0, GENS_EINVAL, "%s: %lld rays", who, (long long)s->n);
    GENS_CHECK_ARG(s->n < ((int64_t)1 << 31), GENS_ELIMIT, "%s: %lld rays (below 2^31)", who, (long long)s->n);
    if (s->n == 0) return 0;
    GENS_CHECK_ARG(s->rays_o && s->rays_d && s->t && s->t_lo && s->t_hi && s->g_lo && s->g_hi && s->t_end && s->dlen && s->status && s->steps &&
                       s->points && s->live,
                   GENS_EINVAL, "%s: null pointer in the state", who);
    return 0;
}

extern "C" int gens_trace_begin(const gens_trace_state* s, const float* near, const float* far, int per_ray, const float* lo, const float* hi,
                                void* stream) {
    if (int rc = check_state("gens_trace_begin", s)) return rc;
    GENS_CHECK_ARG(lo && hi, GENS_EINVAL, "gens_trace_begin: null pointer (the box)");
    if (s->n == 0) return 0;
    GENS_CHECK_ARG(near && far, GENS_EINVAL, "gens_trace_begin: null pointer (near / far)");
    Box3 box;
    for (int a = 0; a < 3; ++a) {
        box.lo[a] = lo[a];
        box.hi[a] = hi[a];
    }
    trace_begin_k<<<gens_blocks(s->n, 256), 256, 0, (hipStream_t)stream>>>(*s, near, far, per_ray ? 1 : 0, box);
    return gens_launch_status("gens_trace_begin");
}

static int check_list(const char* who, const gens_trace_state* s, int64_t m) {
    if (int rc = check_state(who, s)) return rc;
    GENS_CHECK_ARG(m >= 0, GENS_EINVAL, "%s: a list of %lld rays", who, (long long)m);
    GENS_CHECK_ARG(m < ((int64_t)1 << 31), GENS_ELIMIT, "%s: a list of %lld rays (below 2^31)", who, (long long)m);
    return 0;
}

extern "C" int gens_trace_march(const gens_trace_state* s, const float* sdf, const int64_t* idx, int64_t m, float threshold, float lipschitz,
                                float min_step, int max_steps, void* stream) {
    if (int rc = check_list("gens_trace_march", s, m)) return rc;
    GENS_CHECK_ARG(lipschitz > 0.f && isfinite(lipschitz), GENS_EINVAL, "gens_trace_march: lipschitz = %g (a positive finite bound)", (double)lipschitz);
    GENS_CHECK_ARG(min_step > 0.f && isfinite(min_step), GENS_EINVAL, "gens_trace_march: min_step = %g (positive and finite)", (double)min_step);
    GENS_CHECK_ARG(max_steps >= 1, GENS_EINVAL, "gens_trace_march: max_steps = %d (at least 1)", max_steps);
    GENS_CHECK_ARG(isfinite(threshold), GENS_EINVAL, "gens_trace_march: threshold = %g (finite)", (double)threshold);
    GENS_CHECK_ARG(idx || m <= s->n, GENS_EINVAL, "gens_trace_march: %lld values for %lld rays without a list", (long long)m, (long long)s->n);
    if (m == 0) return 0;
    GENS_CHECK_ARG(sdf, GENS_EINVAL, "gens_trace_march: null pointer (the values)");
    trace_march_k<<<gens_blocks(m, 256), 256, 0, (hipStream_t)stream>>>(*s, sdf, idx, (int)m, threshold, lipschitz, min_step, max_steps);
    return gens_launch_status("gens_trace_march");
}

extern "C" int gens_trace_refine(const gens_trace_state* s, const float* sdf, const int64_t* idx, int64_t m, float threshold, int final,
                                 void* stream) {
    if (int rc = check_list("gens_trace_refine", s, m)) return rc;
    GENS_CHECK_ARG(isfinite(threshold), GENS_EINVAL, "gens_trace_refine: threshold = %g (finite)", (double)threshold);
    GENS_CHECK_ARG(idx || m <= s->n, GENS_EINVAL, "gens_trace_refine: %lld values for %lld rays without a list", (long long)m, (long long)s->n);
    GENS_CHECK_ARG(sdf || final, GENS_EINVAL, "gens_trace_refine: null pointer (no values and not the final round: nothing to do)");
    if (m == 0) return 0;
    trace_refine_k<<<gens_blocks(m, 256), 256, 0, (hipStream_t)stream>>>(*s, sdf, idx, (int)m, threshold, final ? 1 : 0);
    return gens_launch_status("gens_trace_refine");
}

extern "C" int gens_trace_gather(const float* points, const int64_t* idx, int64_t m, int64_t n, float* out, void* stream) {
    GENS_CHECK_ARG(m >= 0 && n >= 0, GENS_EINVAL, "gens_trace_gather: a list of %lld of %lld rays", (long long)m, (long long)n);
    GENS_CHECK_ARG(3 * m < ((int64_t)1 << 31) && n < ((int64_t)1 << 31), GENS_ELIMIT, "gens_trace_gather: a list of %lld of %lld rays (3 m and n below 2^31)",
                   (long long)m, (long long)n);
    if (m == 0) return 0;
    GENS_CHECK_ARG(points && idx && out, GENS_EINVAL, "gens_trace_gather: null pointer");
    trace_gather_k<<<gens_blocks(3 * m, 256), 256, 0, (hipStream_t)stream>>>(points, idx, (int)(3 * m), n, out);
    return gens_launch_status("gens_trace_gather");
}

extern "C" int gens_surface_pack(const gens_surface_pack_args* a, void* stream) {
    GENS_CHECK_ARG(a, GENS_EINVAL, "gens_surface_pack: null pointer (the arguments)");
    GENS_CHECK_ARG(a->n >= 0 && a->m >= 0, GENS_EINVAL, "gens_surface_pack: a list of %lld of %lld rays", (long long)a->m, (long long)a->n);
    GENS_CHECK_ARG(a->n < ((int64_t)1 << 31) && a->m < ((int64_t)1 << 31), GENS_ELIMIT, "gens_surface_pack: a list of %lld of %lld rays (below 2^31)",
                   (long long)a->m, (long long)a->n);
    GENS_CHECK_ARG(a->idx || a->m <= a->n, GENS_EINVAL, "gens_surface_pack: %lld rows for %lld rays without a list", (long long)a->m, (long long)a->n);
    if (a->m == 0) return 0;
    GENS_CHECK_ARG(a->status, GENS_EINVAL, "gens_surface_pack: null pointer (the status)");
    GENS_CHECK_ARG(!a->depth || (a->t && a->rays_d && a->rot), GENS_EINVAL, "gens_surface_pack: null pointer (the depth needs t, the rays and the rotation)");
    GENS_CHECK_ARG(!a->grad || ((a->normal || a->normal_img) && (!a->normal_img || a->rot)), GENS_EINVAL,
                   "gens_surface_pack: null pointer (a gradient needs normals to write, the normal image the rotation)");
    GENS_CHECK_ARG(a->grad || (!a->normal && !a->normal_img), GENS_EINVAL, "gens_surface_pack: null pointer (normals without a gradient)");
    GENS_CHECK_ARG(!a->color || (a->vis && a->img && a->seen), GENS_EINVAL, "gens_surface_pack: null pointer (a colour needs the flags, img and seen)");
    GENS_CHECK_ARG(!a->color || (a->n_src >= 1 && a->n_src <= 255), GENS_EINVAL, "gens_surface_pack: %d source views (1 to 255)", a->n_src);
    GENS_CHECK_ARG(a->depth || a->grad || a->color || a->hit, GENS_EINVAL, "gens_surface_pack: null pointer (nothing to write)");
    surface_pack_k<<<gens_blocks(a->m, 256), 256, 0, (hipStream_t)stream>>>(*a);
    return gens_launch_status("gens_surface_pack");
}
