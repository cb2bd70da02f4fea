// K25: the device pieces of the DTU mesh finalising step (evaluation/clean_meshes.py) that K23 does not already hold.
//
//   dilate:  grey-scale dilation of interleaved uint8 images by a structuring element given as per-row half-spans -- what
//            cv.dilate(img, cv.getStructuringElement(cv.MORPH_ELLIPSE, (k, k))) computes (:124-127, :213-216).  Pixels outside the image do
//            not take part (OpenCV's default border for dilation is a constant of the type's minimum, 0 for uint8); the anchor is the centre.
//            A workgroup stages its 16 x 64 pixel tile with the halo in LDS (out-of-image bytes as 0) and every thread takes the maximum over
//            the element's rows directly: there is no arithmetic, so the result is bit-equal to the definition.
//   votes:   clean_points_by_mask (:101-141), one thread per vertex: the float64 projection, rint, the shifted in-image test and the look-up in
//            the mask framed by one pixel of ones, the frame done by index logic.
//
// The third piece, the per-view ray cast (:212-246), extends K23's view-ray kernel and lives beside it in k23_mesh_cull.hip.
#include <math.h>

#include "common.h"

#define DILATE_MAX_K 63         // odd kernels up to 63 x 63
#define DILATE_TH 16
#define DILATE_TW 64

struct DilateSpans {
    signed char dx[DILATE_MAX_K];       // row i holds columns cx - dx[i] .. cx + dx[i], clipped to 0 .. kw - 1; negative: an empty row
};

// in (n, h, w, c) uint8 -> out (n, h, w, channels) uint8, channels <= c: the first `channels` channels of every pixel.
__global__ __launch_bounds__(256) void dilate_u8_k(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int h, int w, int c, int channels, int kw,
                                                   int kh, DilateSpans spans) {
    extern __shared__ uint8_t tile[];
    const int rx = kw / 2, ry = kh / 2;
    const int cols = DILATE_TW + 2 * rx, rows = DILATE_TH + 2 * ry;
    const int x0 = blockIdx.x * DILATE_TW, y0 = blockIdx.y * DILATE_TH;
    const int64_t img = (int64_t)blockIdx.z * h * w;
    const int row_bytes = cols * channels;
    for (int e = threadIdx.x; e < rows * row_bytes; e += 256) {
        const int r = e / row_bytes, rem = e - r * row_bytes;
        const int col = rem / channels, ch = rem - col * channels;
        const int gy = y0 + r - ry, gx = x0 + col - rx;
        uint8_t v = 0;
        if (gy >= 0 && gy < h && gx >= 0 && gx < w) v = in[(img + (int64_t)gy * w + gx) * c + ch];
        tile[e] = v;
    }
    __syncthreads();
    const int out_row = DILATE_TW * channels;
    for (int e = threadIdx.x; e < DILATE_TH * out_row; e += 256) {
        const int y = e / out_row, rem = e - y * out_row;
        const int x = rem / channels, ch = rem - x * channels;
        const int gy = y0 + y, gx = x0 + x;
        if (gy >= h || gx >= w) continue;
        unsigned m = 0;
        for (int i = 0; i < kh; ++i) {
            const int d = spans.dx[i];
            if (d < 0) continue;
            const int lo = max(rx - d, 0), hi = min(rx + d, kw - 1);        // element columns; tile column of (x, column k) is x + k
            const uint8_t* p = tile + ((y + i) * cols + x) * channels + ch;
            for (int k = lo; k <= hi; ++k) m = max(m, (unsigned)p[k * channels]);
        }
        out[(img + (int64_t)gy * w + gx) * channels + ch] = (uint8_t)m;
    }
}

// P (nv, 3, 4) float32, widened: q = P[:3,:3] x + P[:3,3] in float64 as numpy promotes float32 @ float64 (products summed left to right, the
// file is compiled unfused), q / q[2], rint (half to even, np.round), int32, + 1.  Inside iff 0 <= u <= w and 0 <= v <= h on the shifted
// coordinates and the mask framed by one pixel of ones holds a set pixel at (v, u): frame where u == 0 or v == 0, masks[v - 1][u - 1] > 128
// otherwise (u == w + 1 / v == h + 1 fail the in-image test first).  No test for points behind the camera.  A rounded coordinate that is not
// finite or whose magnitude is 2147483000 or more (q[2] == 0 among them; numpy's int32 cast is undefined there) is "not inside".
__global__ __launch_bounds__(256) void vertex_votes_k(const double* __restrict__ pts, int64_t n, const float* __restrict__ P, const uint8_t* __restrict__ masks,
                                                      int nv, int h, int w, int32_t* __restrict__ votes) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    int32_t count = 0;
    for (int v = 0; v < nv; ++v) {
        const float* p = P + 12 * v;
        double q[3];
        for (int a = 0; a < 3; ++a) q[a] = (((double)p[4 * a] * x + (double)p[4 * a + 1] * y) + (double)p[4 * a + 2] * z) + (double)p[4 * a + 3];
        const double ru = rint(q[0] / q[2]), rv = rint(q[1] / q[2]);
        if (!(fabs(ru) < 2147483000.0 && fabs(rv) < 2147483000.0)) continue;        // (NaN and inf fail)
        const int64_t u = (int64_t)ru + 1, vv = (int64_t)rv + 1;
        if (u < 0 || u > w || vv < 0 || vv > h) continue;
        if (u == 0 || vv == 0 || masks[((int64_t)v * h + (vv - 1)) * w + (u - 1)] > 128) ++count;
    }
    votes[i] = count;
}

// ------------------------------------------------------------------------------------------------ entry points
extern "C" int gens_dilate_u8(const uint8_t* in, uint8_t* out, int n, int h, int w, int c, int channels, int kw, int kh, const int* half_spans,
                              void* stream) {
    GENS_CHECK_ARG(in && out && half_spans && in != out, GENS_EINVAL, "gens_dilate_u8: null pointer (or one buffer for both sides)");
    GENS_CHECK_ARG(n >= 1 && n <= 65535 && h >= 1 && w >= 1 && (int64_t)h * w < ((int64_t)1 << 31), GENS_ELIMIT, "gens_dilate_u8: %d images of %dx%d", n,
                   h, w);
    GENS_CHECK_ARG((c == 1 || c == 3) && channels >= 1 && channels <= c, GENS_ELIMIT, "gens_dilate_u8: %d of %d channels (1 or 3 interleaved)", channels, c);
    GENS_CHECK_ARG(kw >= 1 && kh >= 1 && (kw & 1) && (kh & 1) && kw <= DILATE_MAX_K && kh <= DILATE_MAX_K, GENS_ELIMIT,
                   "gens_dilate_u8: kernel %dx%d (odd, at most %d)", kw, kh, DILATE_MAX_K);
    GENS_CHECK_ARG((h + DILATE_TH - 1) / DILATE_TH <= 65535, GENS_ELIMIT, "gens_dilate_u8: %d rows", h);
    DilateSpans spans;
    for (int i = 0; i < DILATE_MAX_K; ++i) spans.dx[i] = -1;
    for (int i = 0; i < kh; ++i) {
        GENS_CHECK_ARG(half_spans[i] <= kw / 2, GENS_ELIMIT, "gens_dilate_u8: half-span %d of row %d exceeds the kernel", half_spans[i], i);
        spans.dx[i] = (signed char)(half_spans[i] < 0 ? -1 : half_spans[i]);
    }
    const int lds = (DILATE_TH + 2 * (kh / 2)) * (DILATE_TW + 2 * (kw / 2)) * channels;      // at most 78 * 126 * 3 = 29484 bytes
    const dim3 grid(gens_blocks(w, DILATE_TW), gens_blocks(h, DILATE_TH), (unsigned)n);
    dilate_u8_k<<<grid, 256, lds, (hipStream_t)stream>>>(in, out, h, w, c, channels, kw, kh, spans);
    return gens_launch_status("gens_dilate_u8");
}

extern "C" int gens_vertex_mask_votes(const double* points, int64_t n_points, const float* proj, const uint8_t* masks, int nv, int h, int w,
                                      int32_t* votes, void* stream) {
    GENS_CHECK_ARG(points && proj && masks && votes, GENS_EINVAL, "gens_vertex_mask_votes: null pointer");
    GENS_CHECK_ARG(n_points >= 0 && n_points < ((int64_t)1 << 31), GENS_ELIMIT, "gens_vertex_mask_votes: %lld points", (long long)n_points);
    GENS_CHECK_ARG(nv >= 1 && nv <= 65535 && h >= 1 && w >= 1 && (int64_t)h * w < ((int64_t)1 << 31), GENS_ELIMIT,
                   "gens_vertex_mask_votes: %d views of %dx%d", nv, h, w);
    if (n_points == 0) return 0;
    vertex_votes_k<<<gens_blocks(n_points, 256), 256, 0, (hipStream_t)stream>>>(points, n_points, proj, masks, nv, h, w, votes);
    return gens_launch_status("gens_vertex_mask_votes");
}
