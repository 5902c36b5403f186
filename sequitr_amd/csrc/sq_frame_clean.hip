// Frame cleaning on the GPU: the two pipes the reference applies to raw microscope frames in front of ImageNorm,
//   ImageOutliers   (sequitr/pipeline.py:266-295): hot pixels against a small-window median,
//   ImageBGSubtract (sequitr/pipeline.py:360-405): a second-order polynomial surface fitted by least squares,
// per whole frame, before tiling (include/sequitr_hip.h "Frame cleaning").
//
// Hot pixels: a block stages a 256 x 32 pixel tile with its halo in LDS as float32 and every lane filters four
// neighbouring pixels of a row.  A lane reads each window row as the three 16-byte slots around its own four pixels
// (ds_read_b128); the lanes of a wave read one LDS row at consecutive slots, so a 16-lane group covers 64 distinct
// banks whatever the row pitch is (a multiple of four floats, so that the slots stay aligned).  The median is selected
// in registers (sq_rank_select.h).
//
// Background: six fp64 moments of every frame against the basis 1, s, t, s^2, st, t^2 in centred, scaled coordinates
// s = (u - (W-1)/2) / ((W-1)/2), t likewise for rows.  A block takes a strip of rows; its partial sums go to the
// workspace, and one thread per frame adds them in block order and solves the normal equations, whose matrix is known in
// closed form.  No atomics: the result is the same on every run, and a frame's strips depend on (H, W) only.
#include "sq_common.h"
#include "sq_rank_select.h"
#include "sq_bg_surface.h"   // the surface's coordinates (bg_axis), shared with the tile cutter (sq_frontend.hip)

namespace {

constexpr int OT_W = 256, OT_H = 32, OT_HALO = 4;               // outliers tile; halo columns = one 16-byte slot a side
constexpr int OT_PITCH = OT_W + 2 * OT_HALO;                    // 264 floats

// scipy's mode='reflect' (the edge pixel repeated), then kept inside the row: the positions a window never uses
// (beyond one reflection) are staged too, from any valid address
__device__ __forceinline__ int reflect_clamp(int i, int L) {
    i = i < 0 ? -i - 1 : (i >= L ? 2 * L - 1 - i : i);
    return i < 0 ? 0 : (i >= L ? L - 1 : i);
}

template <typename T, int K>
__global__ __launch_bounds__(256) void outliers_kernel(const T *__restrict__ frames, float *__restrict__ out, int H,
                                                       int W, float threshold, int vec_store) {
#pragma clang fp contract(off)
    constexpr int A = K / 2, NSLOT = K == 2 ? 2 : 3;            // window offsets -A .. K-1-A; size 2 never looks right
    constexpr int ROWS = OT_H + K - 1;
    __shared__ __attribute__((aligned(16))) float tile[ROWS * OT_PITCH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x0 = blockIdx.x * OT_W, y0 = blockIdx.y * OT_H;
    const size_t fbase = (size_t)blockIdx.z * H * W;
    const T *__restrict__ src = frames + fbase;
    for (int r = wave; r < ROWS; r += 4) {
        const size_t row = (size_t)reflect_clamp(y0 - A + r, H) * W;
        for (int c = lane; c < OT_PITCH; c += 64) tile[r * OT_PITCH + c] = (float)src[row + reflect_clamp(x0 - OT_HALO + c, W)];
    }
    __syncthreads();
    const int x = x0 + 4 * lane;
    if (x >= W) return;
#pragma unroll 1
    for (int rr = wave; rr < OT_H; rr += 4) {
        const int y = y0 + rr;
        if (y >= H) break;
        float win[K][4 * NSLOT];                                // win[j][4 + p] is pixel p's column in window row j
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const f32x4 *slot = reinterpret_cast<const f32x4 *>(&tile[(rr + j) * OT_PITCH + 4 * lane]);
#pragma unroll
            for (int q = 0; q < NSLOT; ++q) {
                const f32x4 v = slot[q];
                win[j][4 * q + 0] = v.x; win[j][4 * q + 1] = v.y; win[j][4 * q + 2] = v.z; win[j][4 * q + 3] = v.w;
            }
        }
        float res[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            float e[K * K];
#pragma unroll
            for (int j = 0; j < K; ++j)
#pragma unroll
                for (int i = 0; i < K; ++i) e[j * K + i] = win[j][4 + p - A + i];
            const float med = sq_rank_select<K * K, (K * K) / 2>(e);
            const float v = win[A][4 + p];
            res[p] = fabsf(v - med) > threshold ? med : v;
        }
        float *__restrict__ dst = out + fbase + (size_t)y * W + x;
        if (vec_store && x + 3 < W) {
            f32x4 o = {res[0], res[1], res[2], res[3]};
            *reinterpret_cast<f32x4 *>(dst) = o;
        } else {
#pragma unroll
            for (int p = 0; p < 4; ++p)
                if (x + p < W) dst[p] = res[p];
        }
    }
}

template <typename T>
int outliers_launch(const T *frames, float *out, int F, int H, int W, int size, float threshold, hipStream_t st) {
    const dim3 grid((W + OT_W - 1) / OT_W, (H + OT_H - 1) / OT_H, F), block(256);
    const int vec = (W % 4 == 0) && SQ_ALIGNED16(out);          // every row of every frame then starts on 16 bytes
    switch (size) {
    case 2: hipLaunchKernelGGL((outliers_kernel<T, 2>), grid, block, 0, st, frames, out, H, W, threshold, vec); break;
    case 3: hipLaunchKernelGGL((outliers_kernel<T, 3>), grid, block, 0, st, frames, out, H, W, threshold, vec); break;
    case 4: hipLaunchKernelGGL((outliers_kernel<T, 4>), grid, block, 0, st, frames, out, H, W, threshold, vec); break;
    case 5: hipLaunchKernelGGL((outliers_kernel<T, 5>), grid, block, 0, st, frames, out, H, W, threshold, vec); break;
    }
    return sq_check_launch("sq_frame_outliers_f32");
}

// ---- background ----------------------------------------------------------------------------------------------------
constexpr int BG_MAX_STRIPS = 256, BG_MIN_ROWS = 8, BG_SLOTS = 8;  // a strip's partials: 8 doubles (6 or 2 used)

inline int bg_strips(int H) {
    const int n = (H + BG_MIN_ROWS - 1) / BG_MIN_ROWS;
    return n < BG_MAX_STRIPS ? n : BG_MAX_STRIPS;
}

// sums of NV doubles over the block in a fixed order: xor butterfly inside a wave, then the four waves in order
template <int NV>
__device__ __forceinline__ void block_sums_to(double (&v)[NV], double *__restrict__ dst) {
    __shared__ double part[4][NV];
#pragma unroll
    for (int k = 0; k < NV; ++k)
        for (int m = 32; m > 0; m >>= 1) v[k] += __shfl_xor(v[k], m);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < NV; ++k) part[wave][k] = v[k];
    __syncthreads();
    if (threadIdx.x < NV) dst[threadIdx.x] = ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
}

// strip blockIdx.x of frame blockIdx.y: sum x * {1, s, t, s^2, st, t^2}
__global__ __launch_bounds__(256) void bg_moments_kernel(const float *__restrict__ frames, double *__restrict__ ws, int H,
                                                         int W, int nstrips) {
    const int f = blockIdx.y, strip = blockIdx.x;
    const int rows = (H + nstrips - 1) / nstrips;
    const int v0 = strip * rows, v1 = min(H, v0 + rows);
    const BgAxis ax = bg_axis(W), ay = bg_axis(H);
    const float *__restrict__ src = frames + (size_t)f * H * W;
    double m[6] = {0, 0, 0, 0, 0, 0};
    for (int v = v0; v < v1; ++v) {
        const float *__restrict__ row = src + (size_t)v * W;
        double r0 = 0, r1 = 0, r2 = 0;                          // this lane's share of the row: sum x, x s, x s^2
#pragma unroll 4
        for (int u = threadIdx.x; u < W; u += 256) {
            const double x = (double)row[u], s = ((double)u - ax.centre) * ax.inv, xs = x * s;
            r0 += x;
            r1 += xs;
            r2 += xs * s;
        }
        const double t = ((double)v - ay.centre) * ay.inv;
        m[0] += r0; m[1] += r1; m[2] += r0 * t; m[3] += r2; m[4] += r1 * t; m[5] += r0 * t * t;
    }
    block_sums_to<6>(m, ws + ((size_t)f * nstrips + strip) * BG_SLOTS);
}

// sum over one axis of s^2 and s^4, s = (i - (L-1)/2) / ((L-1)/2): closed forms of the sums of (i - c)^2 and (i - c)^4
__device__ __forceinline__ void axis_power_sums(int L, double &p2, double &p4) {
    const double n = (double)L, c = 0.5 * (n - 1.0), n2 = n * n;
    const double q2 = n * (n2 - 1.0) / 12.0, q4 = n * (n2 - 1.0) * (3.0 * n2 - 7.0) / 240.0;
    p2 = q2 / (c * c);
    p4 = q4 / (c * c * c * c);
}

// one frame per thread: partials added in strip order, then the 6 x 6 normal equations G k = m.  G is symmetric
// positive definite (H, W >= 3), so Gaussian elimination needs no pivoting.
__global__ void bg_solve_kernel(const double *__restrict__ ws, double *__restrict__ coef, int F, int H, int W, int nstrips) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    double m[6] = {0, 0, 0, 0, 0, 0};
    for (int b = 0; b < nstrips; ++b)
#pragma unroll
        for (int k = 0; k < 6; ++k) m[k] += ws[((size_t)f * nstrips + b) * BG_SLOTS + k];
    double a2, a4, b2, b4;
    axis_power_sums(W, a2, a4);
    axis_power_sums(H, b2, b4);
    const double w = (double)W, h = (double)H;
    double G[6][6] = {{w * h, 0, 0, h * a2, 0, w * b2},
                      {0, h * a2, 0, 0, 0, 0},
                      {0, 0, w * b2, 0, 0, 0},
                      {h * a2, 0, 0, h * a4, 0, a2 * b2},
                      {0, 0, 0, 0, a2 * b2, 0},
                      {w * b2, 0, 0, a2 * b2, 0, w * b4}};
#pragma unroll
    for (int p = 0; p < 6; ++p) {
#pragma unroll
        for (int r = p + 1; r < 6; ++r) {
            const double q = G[r][p] / G[p][p];
#pragma unroll
            for (int c = p; c < 6; ++c) G[r][c] -= q * G[p][c];
            m[r] -= q * m[p];
        }
    }
#pragma unroll
    for (int p = 5; p >= 0; --p) {
        double acc = m[p];
#pragma unroll
        for (int c = p + 1; c < 6; ++c) acc -= G[p][c] * m[c];
        m[p] = acc / G[p][p];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) coef[(size_t)f * 6 + k] = m[k];
}

// strip partials of the residual r = x - bg: sum r, sum r^2
__global__ __launch_bounds__(256) void bg_resid_sums_kernel(const float *__restrict__ frames, const double *__restrict__ coef,
                                                            double *__restrict__ ws, int H, int W, int nstrips) {
    const int f = blockIdx.y, strip = blockIdx.x;
    const int rows = (H + nstrips - 1) / nstrips;
    const int v0 = strip * rows, v1 = min(H, v0 + rows);
    const BgAxis ax = bg_axis(W), ay = bg_axis(H);
    const float *__restrict__ src = frames + (size_t)f * H * W;
    double m[2] = {0, 0};
    for (int v = v0; v < v1; ++v) {
        const float *__restrict__ row = src + (size_t)v * W;
        // sq_bg_surface.h's bg_row and bg_eval as plain expressions: the compiler's default contraction fuses the same five
        // multiply-adds (the ISA shows them), and this kernel's instruction stream stays the one its results were pinned on
        const double *__restrict__ k = coef + (size_t)f * 6;
        const double t = ((double)v - ay.centre) * ay.inv;
        const double ra = k[0] + t * (k[2] + k[5] * t), rb = k[1] + k[4] * t, rc = k[3];
#pragma unroll 4
        for (int u = threadIdx.x; u < W; u += 256) {
            const double s = ((double)u - ax.centre) * ax.inv;
            const double r = (double)row[u] - (ra + s * (rb + rc * s));
            m[0] += r;
            m[1] += r * r;
        }
    }
    block_sums_to<2>(m, ws + ((size_t)f * nstrips + strip) * BG_SLOTS);
}

// mean = sum r / n;  std = sqrt(sum r^2 / n - mean^2), np.std's population definition.  The residual of a fit that
// holds the constant has mean 0 up to rounding, so nothing cancels and the one-pass form is exact to fp64 rounding
// (errors of 1e-13 on the tall frames of tests/frame_side_cases.py).  With coefficients that fit nothing the two terms
// cancel: the variance is off by about 2^-53 mean^2 times the growth of the sums, the std by about 2^-54 (mean / std)^2
// of itself.  Measured on a 96 x 80 frame at level 60000 with noise 1 under zero coefficients: 2.0e-7 relative, seven
// float32 half-ulps; an fp64 emulation with pairwise sums gives 8e-7 at 2048 x 2048.  That is inside the surface's own
// bound of 2^-32 max|x| (1.4e-5 there), which tests/test_gpu_frame_side_sweep.py holds, but it is not below what float32
// tiles can show.
__global__ void bg_stats_finish_kernel(const double *__restrict__ ws, double *__restrict__ mean, double *__restrict__ stdv,
                                       int F, double n, int nstrips) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    double s1 = 0, s2 = 0;
    for (int b = 0; b < nstrips; ++b) {
        s1 += ws[((size_t)f * nstrips + b) * BG_SLOTS];
        s2 += ws[((size_t)f * nstrips + b) * BG_SLOTS + 1];
    }
    const double mu = s1 / n, var = s2 / n - mu * mu;
    mean[f] = mu;
    stdv[f] = sqrt(var > 0.0 ? var : 0.0);
}

inline bool bg_shape_ok(int F, int H, int W) {
    return F > 0 && F <= 65535 && H >= 3 && W >= 3 && (int64_t)H * W <= (1 << 24);
}

}  // namespace

extern "C" int sq_frame_outliers_f32(const void *frames, int dtype, float *out, int F, int H, int W, int size,
                                     float threshold, void *stream) {
    SQ_REQUIRE(frames && out, "sq_frame_outliers_f32: null pointer");
    SQ_REQUIRE(size >= 2 && size <= 5, "sq_frame_outliers_f32: window size %d is not 2, 3, 4 or 5", size);
    SQ_REQUIRE(F > 0 && F <= 65535 && H >= size && W >= size,
               "sq_frame_outliers_f32: %d frames of %d x %d pixels do not take a window of %d (1 .. 65535 frames, min(H, W) >= size)",
               F, H, W, size);
    SQ_REQUIRE((int64_t)H * W < ((int64_t)1 << 31) && (H + OT_H - 1) / OT_H <= 65535,
               "sq_frame_outliers_f32: frames of %d x %d pixels are too large", H, W);
    hipStream_t st = (hipStream_t)stream;
    switch (dtype) {
    case SQ_PIX_U8: return outliers_launch(reinterpret_cast<const uint8_t *>(frames), out, F, H, W, size, threshold, st);
    case SQ_PIX_U16: return outliers_launch(reinterpret_cast<const uint16_t *>(frames), out, F, H, W, size, threshold, st);
    case SQ_PIX_F32: return outliers_launch(reinterpret_cast<const float *>(frames), out, F, H, W, size, threshold, st);
    }
    sq_set_error("sq_frame_outliers_f32: unknown pixel type %d", dtype);
    return SQ_EINVAL;
}

extern "C" int64_t sq_frame_bgfit_workspace(int F, int H, int W) {
    if (!bg_shape_ok(F, H, W)) return -1;
    return (int64_t)F * bg_strips(H) * BG_SLOTS * 8;
}

extern "C" int sq_frame_bgfit_f64(const float *frames, double *coef, void *workspace, int F, int H, int W, void *stream) {
    SQ_REQUIRE(frames && coef && workspace, "sq_frame_bgfit_f64: null pointer");
    SQ_REQUIRE(bg_shape_ok(F, H, W), "sq_frame_bgfit_f64: need 1 .. 65535 frames, H, W >= 3 and H*W <= 2^24, got %d of %d x %d",
               F, H, W);
    hipStream_t st = (hipStream_t)stream;
    const int ns = bg_strips(H);
    double *ws = reinterpret_cast<double *>(workspace);
    hipLaunchKernelGGL(bg_moments_kernel, dim3(ns, F), dim3(256), 0, st, frames, ws, H, W, ns);
    hipLaunchKernelGGL(bg_solve_kernel, dim3((F + 63) / 64), dim3(64), 0, st, ws, coef, F, H, W, ns);
    return sq_check_launch("sq_frame_bgfit_f64");
}

extern "C" int sq_frame_bg_stats_f64(const float *frames, const double *coef, double *mean, double *stdv, void *workspace,
                                     int F, int H, int W, void *stream) {
    SQ_REQUIRE(frames && coef && mean && stdv && workspace, "sq_frame_bg_stats_f64: null pointer");
    SQ_REQUIRE(bg_shape_ok(F, H, W), "sq_frame_bg_stats_f64: need 1 .. 65535 frames, H, W >= 3 and H*W <= 2^24, got %d of %d x %d",
               F, H, W);
    hipStream_t st = (hipStream_t)stream;
    const int ns = bg_strips(H);
    double *ws = reinterpret_cast<double *>(workspace);
    hipLaunchKernelGGL(bg_resid_sums_kernel, dim3(ns, F), dim3(256), 0, st, frames, coef, ws, H, W, ns);
    hipLaunchKernelGGL(bg_stats_finish_kernel, dim3((F + 63) / 64), dim3(64), 0, st, ws, mean, stdv, F,
                       (double)H * (double)W, ns);
    return sq_check_launch("sq_frame_bg_stats_f64");
}
