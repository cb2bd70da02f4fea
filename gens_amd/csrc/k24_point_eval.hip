// K24: the three hot steps of the reference's DTU scoring (evaluation/dtu_eval.py) on the device.
//
//   mesh sampling (dtu_eval.py:11-20, 61-78): a thread per triangle; a count launch, the caller's exclusive scan, an emit launch.  Every
//            operation is the script's own float64 operation in the script's order (numpy sums a row of three left to right; np.cross is two
//            products and a difference; the quotients are IEEE divisions): the lattice test `k0 + k1 < 1` lands on exact equality all the time
//            (n1 = n2 = 2: 0.75 + 0.25), so one rounding anywhere else changes the number of points.  The file is compiled with
//            -ffp-contract=off like the rest of the library.
//   point grid: a uniform grid of cubic cells over a point cloud by counting sort (count, the caller's scan, fill).  The fill also writes the
//            coordinates in cell order, so a cell's points -- and the points of a run of cells along z -- are contiguous.
//   radius down-sampling (:94-102): the mask of the script's sequential loop for a given visiting order, decided in rounds.  A point is kept
//            iff no earlier-visited KEPT point lies within the radius.  One round, one thread per point of the cell-ordered cloud: an undecided
//            point becomes removed if an earlier neighbour is kept, kept if every earlier neighbour is removed.  A round reads the previous
//            round's states and writes new ones (two buffers), so the result AND the number of rounds are the same on every run; the earliest
//            undecided point is decided in every round.  The atomics count the undecided points only (an integer sum).
//   nearest neighbour with a cap (:127-130, 140-142): a thread per query, shells of cells around the query's (clamped) cell; a cell is skipped
//            when its box is farther than the best distance so far, the walk ends when the shell is.  The winner is the lexicographic minimum of
//            (squared distance, index): neither the order inside a cell nor the order of the cells matters.
#include <math.h>

#include "common.h"

#define PG_SLACK 1e-6            // (cells) the rounding of a cell coordinate, generously: boxes are widened by it before they prune anything
#define SAMPLE_MAX_STEPS 1048576.0   // lattice steps along one edge of one triangle; beyond it the count is SAMPLE_REFUSED (the caller's total trips)
#define SAMPLE_REFUSED ((int64_t)1 << 40)

// ------------------------------------------------------------------------------------------------ mesh sampling
struct TriLattice {
    double p0[3], v1[3], v2[3];
    double n1, n2;
};

// dtu_eval.py:61-72 for one triangle; false: no lattice points (zero area, an index out of range, n1 or n2 = 0 -- the script divides by 1e-7
// there, and (j + 0.5) / 1e-7 alone is >= 1)
__device__ __forceinline__ bool tri_lattice(const double* __restrict__ V, int64_t n_vertices, const int32_t* __restrict__ tri, double density,
                                            TriLattice& s) {
    const int64_t a = tri[0], b = tri[1], c = tri[2];
    if (a < 0 || b < 0 || c < 0 || a >= n_vertices || b >= n_vertices || c >= n_vertices) return false;
    for (int k = 0; k < 3; ++k) {
        s.p0[k] = V[3 * a + k];
        s.v1[k] = V[3 * b + k] - s.p0[k];
        s.v2[k] = V[3 * c + k] - s.p0[k];
    }
    const double l1 = sqrt((s.v1[0] * s.v1[0] + s.v1[1] * s.v1[1]) + s.v1[2] * s.v1[2]);
    const double l2 = sqrt((s.v2[0] * s.v2[0] + s.v2[1] * s.v2[1]) + s.v2[2] * s.v2[2]);
    const double cx = s.v1[1] * s.v2[2] - s.v1[2] * s.v2[1];
    const double cy = s.v1[2] * s.v2[0] - s.v1[0] * s.v2[2];
    const double cz = s.v1[0] * s.v2[1] - s.v1[1] * s.v2[0];
    const double area2 = sqrt((cx * cx + cy * cy) + cz * cz);
    if (!(area2 > 0.0)) return false;
    const double thr = density * sqrt(l1 * l2 / area2);
    s.n1 = floor(l1 / thr);
    s.n2 = floor(l2 / thr);
    return s.n1 >= 1.0 && s.n2 >= 1.0;      // (NaN fails)
}

__global__ __launch_bounds__(256) void sample_count_k(const double* __restrict__ V, int64_t n_vertices, const int32_t* __restrict__ T, int64_t n_tri,
                                                      double density, int64_t* __restrict__ counts) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= n_tri) return;
    TriLattice s;
    int64_t n = 0;
    if (tri_lattice(V, n_vertices, T + 3 * f, density, s)) {
        if (s.n1 > SAMPLE_MAX_STEPS || s.n2 > SAMPLE_MAX_STEPS) {
            n = SAMPLE_REFUSED;
        } else {
            const int m1 = (int)s.n1, m2 = (int)s.n2;
            for (int i = 0; i <= m1; ++i) {
                const double k0 = ((double)i + 0.5) / s.n1;
                if (!(k0 < 1.0)) break;                                      // (k1 > 0: nothing in this row or a later one)
                for (int j = 0; j <= m2 && k0 + ((double)j + 0.5) / s.n2 < 1.0; ++j) ++n;      // (the sum grows with j: the first failure ends the row)
            }
        }
    }
    counts[f] = n;
}

__global__ __launch_bounds__(256) void sample_emit_k(const double* __restrict__ V, int64_t n_vertices, const int32_t* __restrict__ T, int64_t n_tri,
                                                     double density, const int64_t* __restrict__ offsets, int64_t total, double* __restrict__ out) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= n_tri) return;
    TriLattice s;
    if (!tri_lattice(V, n_vertices, T + 3 * f, density, s) || s.n1 > SAMPLE_MAX_STEPS || s.n2 > SAMPLE_MAX_STEPS) return;
    int64_t at = offsets[f];
    if (at < 0) return;
    const int m1 = (int)s.n1, m2 = (int)s.n2;
    for (int i = 0; i <= m1; ++i) {
        const double k0 = ((double)i + 0.5) / s.n1;
        if (!(k0 < 1.0)) break;
        for (int j = 0; j <= m2; ++j) {
            const double k1 = ((double)j + 0.5) / s.n2;
            if (!(k0 + k1 < 1.0)) break;
            if (at >= total) return;                                          // (never: the count pass walked the same lattice)
            for (int k = 0; k < 3; ++k) out[3 * at + k] = (s.v1[k] * k0 + s.v2[k] * k1) + s.p0[k];
            ++at;
        }
    }
}

// ------------------------------------------------------------------------------------------------ point grid
__device__ __forceinline__ int pg_coord(double p, double lo, double inv_cell, int n) {      // (NaN lands in cell 0)
    return (int)fmin(fmax(floor((p - lo) * inv_cell), 0.0), (double)(n - 1));
}

__device__ __forceinline__ int64_t pg_cell_of(const gens_point_grid& g, const double* __restrict__ p) {
    const double inv = 1.0 / g.cell;
    return ((int64_t)pg_coord(p[0], g.lo_x, inv, g.nx) * g.ny + pg_coord(p[1], g.lo_y, inv, g.ny)) * g.nz + pg_coord(p[2], g.lo_z, inv, g.nz);
}

__global__ __launch_bounds__(256) void pg_count_k(gens_point_grid g, int32_t* __restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= g.n) return;
    atomicAdd(counts + pg_cell_of(g, g.points + 3 * i), 1);
}

__global__ __launch_bounds__(256) void pg_fill_k(gens_point_grid g, int32_t* __restrict__ cursor) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= g.n) return;
    const double* p = g.points + 3 * i;
    const int64_t c = pg_cell_of(g, p);
    const int64_t at = (int64_t)g.cell_start[c] + atomicAdd(cursor + c, 1);
    if (at < 0 || at >= g.cell_start[c + 1] || at >= g.n) return;              // (never: the count pass saw the same cells)
    g.cell_points[at] = (int32_t)i;
    for (int k = 0; k < 3; ++k) g.sorted[3 * at + k] = p[k];
}

// the slots [b, e) of the cells (ci, cj, k0 .. k1): one contiguous run
__device__ __forceinline__ void pg_run(const gens_point_grid& g, int ci, int cj, int k0, int k1, int64_t& b, int64_t& e) {
    const int64_t c = ((int64_t)ci * g.ny + cj) * g.nz;
    b = g.cell_start[c + k0];
    e = g.cell_start[c + k1 + 1];
    if (b < 0) b = 0;
    if (e > g.n) e = g.n;
}

// ------------------------------------------------------------------------------------------------ radius down-sampling
#define DS_UNDECIDED 0
#define DS_KEPT 1
#define DS_REMOVED 2

// One round over the cell-ordered cloud: slot s holds the point g.sorted[s], visited at position rank[s].  cell >= radius (checked by the
// entry), so every neighbour within the radius lies in the 3 x 3 x 3 cells around the point's own: nine runs along z.
__global__ __launch_bounds__(256) void ds_round_k(gens_point_grid g, const int32_t* __restrict__ rank, double r2, const uint8_t* __restrict__ in,
                                                  uint8_t* __restrict__ out, int32_t* __restrict__ undecided) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int mine = 0;
    if (s < g.n) {
        uint8_t st = in[s];
        if (st == DS_UNDECIDED) {
            const double p[3] = {g.sorted[3 * s], g.sorted[3 * s + 1], g.sorted[3 * s + 2]};
            const int32_t my_rank = rank[s];
            const double inv = 1.0 / g.cell;
            const int c0 = pg_coord(p[0], g.lo_x, inv, g.nx), c1 = pg_coord(p[1], g.lo_y, inv, g.ny), c2 = pg_coord(p[2], g.lo_z, inv, g.nz);
            const int k0 = max(c2 - 1, 0), k1 = min(c2 + 1, g.nz - 1);
            bool removed = false, waits = false;
            for (int i = max(c0 - 1, 0); i <= min(c0 + 1, g.nx - 1) && !removed; ++i)
                for (int j = max(c1 - 1, 0); j <= min(c1 + 1, g.ny - 1) && !removed; ++j) {
                    int64_t b, e;
                    pg_run(g, i, j, k0, k1, b, e);
                    for (int64_t t = b; t < e; ++t) {
                        if (!(rank[t] < my_rank)) continue;
                        const double dx = g.sorted[3 * t] - p[0], dy = g.sorted[3 * t + 1] - p[1], dz = g.sorted[3 * t + 2] - p[2];
                        if (!((dx * dx + dy * dy) + dz * dz <= r2)) continue;
                        const uint8_t other = in[t];
                        if (other == DS_KEPT) {
                            removed = true;
                            break;
                        }
                        waits = waits || other == DS_UNDECIDED;
                    }
                }
            st = removed ? DS_REMOVED : (waits ? DS_UNDECIDED : DS_KEPT);
            mine = st == DS_UNDECIDED;
        }
        out[s] = st;
    }
    const int n_wave = __popcll(__ballot(mine));
    if (n_wave && (threadIdx.x & (GENS_WAVE - 1)) == 0) atomicAdd(undecided, n_wave);
}

// ------------------------------------------------------------------------------------------------ nearest neighbour
// distance from q to the cell [lo + i cell, lo + (i + 1) cell] along one axis, the cell widened by PG_SLACK cells
__device__ __forceinline__ double pg_axis_gap(double q, double lo, double cell, int i) {
    const double a = lo + (double)i * cell, b = lo + (double)(i + 1) * cell;
    return fmax(fmax(a - q, q - b) - PG_SLACK * cell, 0.0);
}

__global__ __launch_bounds__(256) void nearest_k(gens_point_grid g, const double* __restrict__ Q, int64_t nq, double max_dist, double* __restrict__ dist,
                                                 int32_t* __restrict__ index) {
    const int64_t qi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (qi >= nq) return;
    const double q[3] = {Q[3 * qi], Q[3 * qi + 1], Q[3 * qi + 2]};
    const double inv = 1.0 / g.cell;
    const int c0 = pg_coord(q[0], g.lo_x, inv, g.nx), c1 = pg_coord(q[1], g.lo_y, inv, g.ny), c2 = pg_coord(q[2], g.lo_z, inv, g.nz);
    // pruning bound: nothing at or beyond the cap can win; a little above it, so that the exact test at the end decides
    double bound = max_dist < INFINITY ? max_dist * max_dist * (1.0 + 1e-9) : INFINITY;
    double best = INFINITY;
    int32_t best_i = -1;
    const int s_max = max(max(max(c0, g.nx - 1 - c0), max(c1, g.ny - 1 - c1)), max(c2, g.nz - 1 - c2));
    for (int s = 0; s <= s_max; ++s) {
        // every cell of shell s (Chebyshev distance s from the clamped cell of q) is at least (s - 1) cells away from q along some axis
        const double lb = ((double)(s - 1) - PG_SLACK) * g.cell;
        if (lb > 0.0 && lb * lb > bound) break;
        for (int i = max(c0 - s, 0); i <= min(c0 + s, g.nx - 1); ++i) {
            const double gx = pg_axis_gap(q[0], g.lo_x, g.cell, i);
            const int ai = abs(i - c0);
            for (int j = max(c1 - s, 0); j <= min(c1 + s, g.ny - 1); ++j) {
                const double gy = pg_axis_gap(q[1], g.lo_y, g.cell, j);
                const double gxy = gx * gx + gy * gy;
                if (gxy > bound) continue;
                const bool rim = ai == s || abs(j - c1) == s;       // the whole column of the shell, or only its two end cells
                const int step = rim ? 1 : max(2 * s, 1);
                for (int k = c2 - s; k <= c2 + s; k += step) {
                    if (k < 0 || k >= g.nz) continue;
                    const double gz = pg_axis_gap(q[2], g.lo_z, g.cell, k);
                    if (gxy + gz * gz > bound) continue;
                    int64_t b, e;
                    pg_run(g, i, j, k, k, b, e);
                    for (int64_t t = b; t < e; ++t) {
                        const double dx = g.sorted[3 * t] - q[0], dy = g.sorted[3 * t + 1] - q[1], dz = g.sorted[3 * t + 2] - q[2];
                        const double d2 = (dx * dx + dy * dy) + dz * dz;
                        const int32_t id = g.cell_points[t];
                        if (d2 < best || (d2 == best && id < best_i)) {
                            best = d2;
                            best_i = id;
                            bound = fmin(bound, d2);
                        }
                    }
                }
            }
        }
    }
    const double d = sqrt(best);
    const bool found = best_i >= 0 && d < max_dist;
    dist[qi] = found ? d : INFINITY;
    index[qi] = found ? best_i : -1;
}

// ------------------------------------------------------------------------------------------------ entry points
static int check_sample(const double* v, int64_t nv, const int32_t* t, int64_t nt, double density, const char* who) {
    GENS_CHECK_ARG(v && t, GENS_EINVAL, "%s: null pointer", who);
    GENS_CHECK_ARG(nv >= 0 && nt >= 0 && nv < ((int64_t)1 << 31) && nt < ((int64_t)1 << 31), GENS_EINVAL, "%s: %lld vertices, %lld triangles", who,
                   (long long)nv, (long long)nt);
    GENS_CHECK_ARG(density > 0.0 && isfinite(density), GENS_EINVAL, "%s: density %g (must be positive and finite)", who, density);
    return 0;
}

extern "C" int gens_mesh_sample_count(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, double density,
                                      int64_t* counts, void* stream) {
    if (int rc = check_sample(vertices, n_vertices, triangles, n_triangles, density, "gens_mesh_sample_count")) return rc;
    GENS_CHECK_ARG(counts, GENS_EINVAL, "gens_mesh_sample_count: null counts");
    if (n_triangles == 0) return 0;
    sample_count_k<<<gens_blocks(n_triangles, 256), 256, 0, (hipStream_t)stream>>>(vertices, n_vertices, triangles, n_triangles, density, counts);
    return gens_launch_status("gens_mesh_sample_count");
}

extern "C" int gens_mesh_sample_emit(const double* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles, double density,
                                     const int64_t* offsets, int64_t total, double* out, void* stream) {
    if (int rc = check_sample(vertices, n_vertices, triangles, n_triangles, density, "gens_mesh_sample_emit")) return rc;
    GENS_CHECK_ARG(offsets && out, GENS_EINVAL, "gens_mesh_sample_emit: null pointer");
    GENS_CHECK_ARG(total >= 0 && total < ((int64_t)1 << 31), GENS_EINVAL, "gens_mesh_sample_emit: %lld points", (long long)total);
    if (n_triangles == 0 || total == 0) return 0;
    sample_emit_k<<<gens_blocks(n_triangles, 256), 256, 0, (hipStream_t)stream>>>(vertices, n_vertices, triangles, n_triangles, density, offsets, total,
                                                                                  out);
    return gens_launch_status("gens_mesh_sample_emit");
}

static int check_point_grid(const gens_point_grid* g, bool filled, const char* who) {
    GENS_CHECK_ARG(g, GENS_EINVAL, "%s: null grid", who);
    GENS_CHECK_ARG(g->n >= 0 && g->n < ((int64_t)1 << 31), GENS_EINVAL, "%s: %lld points", who, (long long)g->n);
    GENS_CHECK_ARG(filled ? (g->sorted && g->cell_start && g->cell_points) : (g->points != nullptr), GENS_EINVAL, "%s: null pointer", who);
    GENS_CHECK_ARG(g->nx >= 1 && g->ny >= 1 && g->nz >= 1 && (int64_t)g->nx * g->ny < ((int64_t)1 << 31) &&
                       (int64_t)g->nx * g->ny * g->nz < ((int64_t)1 << 31),
                   GENS_ELIMIT, "%s: grid %dx%dx%d (1 .. 2^31 - 1 cells)", who, g->nx, g->ny, g->nz);
    GENS_CHECK_ARG(g->cell > 0.0 && isfinite(g->cell) && isfinite(g->lo_x) && isfinite(g->lo_y) && isfinite(g->lo_z), GENS_EINVAL, "%s: bad grid box",
                   who);
    return 0;
}

extern "C" int gens_point_grid_count(const gens_point_grid* g, int32_t* counts, void* stream) {
    if (int rc = check_point_grid(g, false, "gens_point_grid_count")) return rc;
    GENS_CHECK_ARG(counts, GENS_EINVAL, "gens_point_grid_count: null counts");
    if (g->n == 0) return 0;
    pg_count_k<<<gens_blocks(g->n, 256), 256, 0, (hipStream_t)stream>>>(*g, counts);
    return gens_launch_status("gens_point_grid_count");
}

extern "C" int gens_point_grid_fill(const gens_point_grid* g, int32_t* cursor, void* stream) {
    if (int rc = check_point_grid(g, false, "gens_point_grid_fill")) return rc;
    GENS_CHECK_ARG(cursor && g->sorted && g->cell_start && g->cell_points, GENS_EINVAL, "gens_point_grid_fill: null pointer");
    if (g->n == 0) return 0;
    pg_fill_k<<<gens_blocks(g->n, 256), 256, 0, (hipStream_t)stream>>>(*g, cursor);
    return gens_launch_status("gens_point_grid_fill");
}

extern "C" int gens_radius_downsample_round(const gens_point_grid* g, const int32_t* rank, double radius, const uint8_t* state_in, uint8_t* state_out,
                                            int32_t* undecided, void* stream) {
    GENS_CHECK_ARG(radius > 0.0 && isfinite(radius), GENS_EINVAL, "gens_radius_downsample_round: radius %g (must be positive and finite)", radius);
    if (int rc = check_point_grid(g, true, "gens_radius_downsample_round")) return rc;
    GENS_CHECK_ARG(rank && state_in && state_out && undecided && state_in != state_out, GENS_EINVAL,
                   "gens_radius_downsample_round: null pointer (or one state buffer for both sides)");
    GENS_CHECK_ARG(radius <= g->cell, GENS_ELIMIT, "gens_radius_downsample_round: radius %g exceeds the grid's cell %g", radius, g->cell);
    if (g->n == 0) return 0;
    ds_round_k<<<gens_blocks(g->n, 256), 256, 0, (hipStream_t)stream>>>(*g, rank, radius * radius, state_in, state_out, undecided);
    return gens_launch_status("gens_radius_downsample_round");
}

extern "C" int gens_nearest_point(const gens_point_grid* g, const double* queries, int64_t n_queries, double max_dist, double* dist, int32_t* index,
                                  void* stream) {
    GENS_CHECK_ARG(max_dist > 0.0, GENS_EINVAL, "gens_nearest_point: max_dist %g (must be positive; +inf for no cap)", max_dist);      // (NaN fails)
    if (int rc = check_point_grid(g, true, "gens_nearest_point")) return rc;
    GENS_CHECK_ARG(queries && dist && index, GENS_EINVAL, "gens_nearest_point: null pointer");
    GENS_CHECK_ARG(n_queries >= 0 && n_queries < ((int64_t)1 << 31), GENS_EINVAL, "gens_nearest_point: %lld queries", (long long)n_queries);
    if (n_queries == 0) return 0;
    nearest_k<<<gens_blocks(n_queries, 256), 256, 0, (hipStream_t)stream>>>(*g, queries, n_queries, max_dist, dist, index);
    return gens_launch_status("gens_nearest_point");
}
