// Multi-channel frames (include/sequitr_hip.h "Tile front end" and "Tile sampler", the _mc paragraphs): bright field and
// fluorescence stacks of one position (BF / GFP / RFP, sequitr/dataio/octopus.py:321-328) in front of a U-Net with
// num_inputs > 1.  On the device a batch is CHANNEL-MAJOR PLANES -- channel c of frame f is a contiguous (H, W) plane at
// element offset c * chan_stride + f * H * W -- which is how the streams arrive (one stack per channel) and what lets
// every per-frame kernel of the single-channel front end run unchanged on a channel's slice.  The networks read
// interleaved (N, T, T, C) tiles; the two kernels here are the only places where the planes are woven together.
//
//   sq_frames_to_tiles_mc    : sq_frames_to_tiles' geometry, every channel under its own mode (cast, ImageNorm, background
//                              residual, normalised residual), one launch.  A lane owns one tile pixel: it reads that pixel
//                              from each of the C planes -- a wave reads 64 consecutive pixels of a frame row per plane --
//                              and stores its C floats at once, so a wave writes 64 * C consecutive floats (b64 per lane at
//                              C = 2, b128 at 4, two b128 at 8).  A pixel's output offset is (flat pixel) * C floats, so the
//                              stores are aligned whatever the tile size is.  No LDS: nothing is read twice.
//   sq_tile_sample_affine_mc : sq_tile_sample_affine with CI image planes; coordinates, corners and bilinear weights once
//                              per pixel, the interpolation per channel.
//
// The expressions are those of the single-channel kernels, so that channel c of the result has the bits the single-channel
// entry gives on channel c's stack.  tiles_norm_kernel (sq_frontend.hip) and tile_sample_kernel (sq_tile_sampler.hip) are
// compiled with contraction off, tiles_bg_kernel (sq_frame_clean.hip) with the compiler's default, which fuses every
// multiply-add of the surface; here contraction is off for the whole file and the surface's fused operations are written
// out (bg_row, bg_eval), so the roundings are stated rather than left to the compiler.  The sampler's geometry and
// expressions are sq_tile_sample.h's, the one definition both samplers include.
#include "sq_tile_sample.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAXC = 8;

struct ChanModes {
    int m[MAXC];
};

// ---- tile cutter ---------------------------------------------------------------------------------------------------
constexpr int CUT_THREADS = 256, CUT_PER_THREAD = 4, CUT_CHUNK = CUT_THREADS * CUT_PER_THREAD;

struct BgAxis { double centre, inv; };                          // scaled coordinate = (index - centre) * inv
__device__ __forceinline__ BgAxis bg_axis(int L) {
    const double c = 0.5 * (double)(L - 1);
    return {c, 1.0 / c};
}
// the surface by rows, (c0 + c2 t + c5 t^2) + s ((c1 + c4 t) + c3 s), every multiply-add one fused operation
struct BgRow { double a, b, c; };
__device__ __forceinline__ BgRow bg_row(const double *__restrict__ k, double t) {
    return {__builtin_fma(t, __builtin_fma(k[5], t, k[2]), k[0]), __builtin_fma(k[4], t, k[1]), k[3]};
}
__device__ __forceinline__ double bg_eval(const BgRow &r, double s) {
    return __builtin_fma(s, __builtin_fma(r.c, s, r.b), r.a);
}

template <int C>
__device__ __forceinline__ void store_pixel(float *__restrict__ p, const float (&o)[C]) {
    if constexpr (C % 4 == 0) {
#pragma unroll
        for (int q = 0; q < C; q += 4) {
            const f32x4 v = {o[q], o[q + 1], o[q + 2], o[q + 3]};
            *reinterpret_cast<f32x4 *>(p + q) = v;
        }
    } else if constexpr (C % 2 == 0) {
#pragma unroll
        for (int q = 0; q < C; q += 2) *reinterpret_cast<float2 *>(p + q) = make_float2(o[q], o[q + 1]);
    } else {
#pragma unroll
        for (int q = 0; q < C; ++q) p[q] = o[q];
    }
}

// a block takes CUT_CHUNK consecutive pixels of the flat (tile, y, x) order; the one 64-bit division is the block's
template <typename T, int C>
__global__ __launch_bounds__(CUT_THREADS) void tiles_mc_kernel(
    const T *__restrict__ frames, int64_t chan_stride, ChanModes modes, const float *__restrict__ mean32,
    const float *__restrict__ std32, const double *__restrict__ coef, const double *__restrict__ mean64,
    const double *__restrict__ std64, const int *__restrict__ oy, const int *__restrict__ ox, float *__restrict__ tiles,
    int F, int H, int W, int TR, int TC, int TS, int64_t total) {
    const int64_t base = (int64_t)blockIdx.x * CUT_CHUNK;
    const int64_t base_row = base / TS;
    const unsigned base_x = (unsigned)(base - base_row * TS), uTS = (unsigned)TS;
    const BgAxis ax = bg_axis(W), ay = bg_axis(H);
#pragma unroll
    for (int it = 0; it < CUT_PER_THREAD; ++it) {
        const unsigned l = base_x + (unsigned)(it * CUT_THREADS) + threadIdx.x;
        const int64_t p = base + it * CUT_THREADS + threadIdx.x;
        if (p >= total) return;
        const unsigned row = (unsigned)base_row + l / uTS, x = l % uTS;     // row < F*TR*TC*TS < 2^31 (checked on the host)
        const unsigned y = row % uTS;
        unsigned t = row / uTS;
        const unsigned tx = t % (unsigned)TC;
        t /= (unsigned)TC;
        const unsigned ty = t % (unsigned)TR, f = t / (unsigned)TR;
        const int v = oy[ty] + (int)y, u = ox[tx] + (int)x;
        const size_t src = ((size_t)f * H + v) * W + u;
        const double tt = ((double)v - ay.centre) * ay.inv, ss = ((double)u - ax.centre) * ax.inv;
        float o[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int mode = modes.m[c];
            const size_t cf = (size_t)c * F + f;
            const T raw = frames[(size_t)c * chan_stride + src];
            if (mode == SQ_CH_CAST) {
                o[c] = (float)raw;
            } else if (mode == SQ_CH_NORM) {
                o[c] = ((float)raw - mean32[cf]) / std32[cf];                // tiles_norm_kernel's expression
            } else {                                                        // tiles_bg_kernel's expression
                const BgRow br = bg_row(coef + cf * 6, tt);
                const double r = (double)raw - bg_eval(br, ss);
                o[c] = (float)(mode == SQ_CH_BG_NORM ? (r - mean64[cf]) / (1e-99 + std64[cf]) : r);
            }
        }
        store_pixel<C>(tiles + (size_t)p * C, o);
    }
}

template <typename T, int C>
void tiles_mc_launch(const void *frames, int64_t chan_stride, const ChanModes &modes, const float *mean32,
                     const float *std32, const double *coef, const double *mean64, const double *std64, const int *oy,
                     const int *ox, float *tiles, int F, int H, int W, int TR, int TC, int TS, int64_t total, hipStream_t st) {
    hipLaunchKernelGGL((tiles_mc_kernel<T, C>), dim3((unsigned)((total + CUT_CHUNK - 1) / CUT_CHUNK)), dim3(CUT_THREADS), 0,
                       st, reinterpret_cast<const T *>(frames), chan_stride, modes, mean32, std32, coef, mean64, std64, oy,
                       ox, tiles, F, H, W, TR, TC, TS, total);
}

template <typename T>
int tiles_mc_dispatch(int C, const void *frames, int64_t chan_stride, const ChanModes &modes, const float *mean32,
                      const float *std32, const double *coef, const double *mean64, const double *std64, const int *oy,
                      const int *ox, float *tiles, int F, int H, int W, int TR, int TC, int TS, int64_t total, hipStream_t st) {
#define SQ_MC_CASE(N)                                                                                                   \
    case N:                                                                                                             \
        tiles_mc_launch<T, N>(frames, chan_stride, modes, mean32, std32, coef, mean64, std64, oy, ox, tiles, F, H, W,  \
                              TR, TC, TS, total, st);                                                                   \
        break;
    switch (C) {
        SQ_MC_CASE(1) SQ_MC_CASE(2) SQ_MC_CASE(3) SQ_MC_CASE(4) SQ_MC_CASE(5) SQ_MC_CASE(6) SQ_MC_CASE(7) SQ_MC_CASE(8)
    }
#undef SQ_MC_CASE
    return sq_check_launch("sq_frames_to_tiles_mc");
}

// ---- tile sampler (geometry and expressions: sq_tile_sample.h, shared with sq_tile_sampler.hip) ------------------------
constexpr int NU = PATCH / ROWS;

// grid (patches of a tile, count), block (PATCH, ROWS).  `vec`: out_image is 16-byte aligned, a pixel's CI floats go out
// in one piece.
template <typename T, int CI>
__global__ __launch_bounds__(PATCH * ROWS) void tile_sample_mc_kernel(
    const T *__restrict__ frames, int64_t chan_stride, const float *__restrict__ mean, const float *__restrict__ stdv,
    const uint8_t *__restrict__ labels, const float *__restrict__ wmap, const int *__restrict__ plan,
    const float *__restrict__ coef, float *__restrict__ out_image, uint8_t *__restrict__ out_onehot,
    float *__restrict__ out_weights, TileGeom g, int want_lds, int packed, int vec) {
    __shared__ float s_img[BOX * PITCH];
    __shared__ float s_wts[BOX * PITCH];
    __shared__ uint8_t s_lab[BOX * PITCH];
    const int k = blockIdx.y;
    const int i0 = (int)(blockIdx.x / g.px) * PATCH, j0 = (int)(blockIdx.x % g.px) * PATCH;
    const int *row = plan + (size_t)k * 4;
    const float *cf = coef + (size_t)k * 6;
    const int f = row[0];
    const long long oy = row[1], ox = row[2];
    const Affine t = {cf[0], cf[1], cf[2], cf[3], cf[4], cf[5]};
    const bool fok = (unsigned)f < (unsigned)g.F;
    const size_t fbase = fok ? (size_t)f * g.H * g.W : 0;
    const bool norm = mean != nullptr;
    float m[CI], s[CI];
#pragma unroll
    for (int c = 0; c < CI; ++c) {
        m[c] = (norm && fok) ? mean[(size_t)c * g.F + f] : 0.f;
        s[c] = (norm && fok) ? stdv[(size_t)c * g.F + f] : 1.f;
    }
    const int tx = threadIdx.x, ty = threadIdx.y;
    const unsigned H = (unsigned)g.H, W = (unsigned)g.W;

    // the patch's footprint, from its four corners (the same arithmetic in every thread: the decision is uniform)
    bool lds = want_lds != 0;
    int bx0 = 0, by0 = 0, bw = 0, bh = 0;
    if (lds) {
        const int i1 = min(i0 + PATCH, g.TH) - 1, j1 = min(j0 + PATCH, g.TW) - 1;
        float lox = INFINITY, hix = -INFINITY, loy = INFINITY, hiy = -INFINITY;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float sx, sy;
            source_xy(t, ox + ((c & 1) ? j1 : j0), oy + ((c & 2) ? i1 : i0), sx, sy);
            lds = lds && in_range(sx, sy);
            lox = fminf(lox, sx), hix = fmaxf(hix, sx), loy = fminf(loy, sy), hiy = fmaxf(hiy, sy);
        }
        if (lds) {
            bx0 = (int)floorf(lox), by0 = (int)floorf(loy);
            bw = (int)floorf(hix) + 2 - bx0, bh = (int)floorf(hiy) + 2 - by0;
            lds = bw <= BOX && bh <= BOX;
        }
    }
    const int j = j0 + tx;

    if (lds) {
        // One pass per image plane through the same staging buffer; labels and weights ride with the first.  Every thread of
        // the block reaches every barrier: a thread outside the tile stages and then skips the interpolation.
        const int tid = ty * PATCH + tx, sc = tid & 63, r0 = tid >> 6;
        const unsigned gc = (unsigned)(bx0 + sc);
        const bool col_ok = fok && sc < bw && gc < W;
        const int passes = out_image ? CI : 1;
        for (int c = 0; c < passes; ++c) {
            if (c) __syncthreads();                             // the previous plane has been read
            if (sc < bw) {                                      // lanes along the box's rows, 64 columns x 4 rows per pass
                const T *__restrict__ pl = frames + (size_t)c * chan_stride;
                for (int r = r0; r < bh; r += 4) {
                    const unsigned gr = (unsigned)(by0 + r);
                    const bool ok = col_ok && gr < H;
                    const size_t src = fbase + (size_t)(ok ? gr : 0u) * g.W + (ok ? gc : 0u);
                    if (out_image) s_img[r * PITCH + sc] = ok ? norm_pixel((float)pl[src], norm, m[c], s[c]) : 0.f;
                    if (c == 0 && out_weights) s_wts[r * PITCH + sc] = ok ? wmap[src] : 0.f;
                    if (c == 0 && out_onehot) s_lab[r * PITCH + sc] = ok ? labels[src] : (uint8_t)0;
                }
            }
            __syncthreads();
            if (j >= g.TW) continue;
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int i = i0 + ty + u * ROWS;
                if (i >= g.TH) break;
                float sx, sy;
                source_xy(t, ox + j, oy + i, sx, sy);
                const bool ok = in_range(sx, sy);
                const size_t pix = ((size_t)k * g.TH + i) * g.TW + j;
                float img = 0.f, wv = 0.f;
                unsigned label = 0;
                bool inside = false;
                if (ok) {
                    const float fx0 = floorf(sx), fy0 = floorf(sy);
                    const int x0 = (int)fx0, y0 = (int)fy0;
                    const int rr = (int)roundf(sy), cc = (int)roundf(sx);
                    inside = fok && (unsigned)rr < H && (unsigned)cc < W;
                    const int a = (y0 - by0) * PITCH + (x0 - bx0);
                    if (out_image) img = bilinear(sx, sy, fx0, fy0, s_img[a], s_img[a + 1], s_img[a + PITCH], s_img[a + PITCH + 1]);
                    if (c == 0 && out_weights)
                        wv = bilinear(sx, sy, fx0, fy0, s_wts[a], s_wts[a + 1], s_wts[a + PITCH], s_wts[a + PITCH + 1]);
                    if (c == 0 && out_onehot) label = s_lab[(rr - by0) * PITCH + (cc - bx0)];
                }
                if (out_image) out_image[pix * CI + c] = img;
                if (c == 0 && out_weights) out_weights[pix] = wv + (inside ? 0.f : 1.f);
                if (c == 0 && out_onehot) store_onehot(out_onehot + pix * g.C, label, g.C, packed != 0);
            }
        }
        return;
    }

    if (j >= g.TW) return;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int i = i0 + ty + u * ROWS;
        if (i >= g.TH) break;
        float sx, sy;
        source_xy(t, ox + j, oy + i, sx, sy);
        const bool ok = in_range(sx, sy);
        const size_t pix = ((size_t)k * g.TH + i) * g.TW + j;
        float img[CI], wv = 0.f;
#pragma unroll
        for (int c = 0; c < CI; ++c) img[c] = 0.f;
        unsigned label = 0;
        bool inside = false;
        if (ok) {
            const float fx0 = floorf(sx), fy0 = floorf(sy);
            const int x0 = (int)fx0, y0 = (int)fy0;
            const int rr = (int)roundf(sy), cc = (int)roundf(sx);
            inside = fok && (unsigned)rr < H && (unsigned)cc < W;
            const bool r0ok = fok && (unsigned)y0 < H, r1ok = fok && (unsigned)(y0 + 1) < H;
            const bool c0ok = (unsigned)x0 < W, c1ok = (unsigned)(x0 + 1) < W;
            const size_t a00 = fbase + (size_t)(r0ok ? y0 : 0) * g.W + (c0ok ? x0 : 0);
            const size_t a01 = fbase + (size_t)(r0ok ? y0 : 0) * g.W + (c1ok ? x0 + 1 : 0);
            const size_t a10 = fbase + (size_t)(r1ok ? y0 + 1 : 0) * g.W + (c0ok ? x0 : 0);
            const size_t a11 = fbase + (size_t)(r1ok ? y0 + 1 : 0) * g.W + (c1ok ? x0 + 1 : 0);
            const bool k00 = r0ok && c0ok, k01 = r0ok && c1ok, k10 = r1ok && c0ok, k11 = r1ok && c1ok;
            if (out_image) {
#pragma unroll
                for (int c = 0; c < CI; ++c) {
                    const T *__restrict__ pl = frames + (size_t)c * chan_stride;
                    const float v00 = k00 ? norm_pixel((float)pl[a00], norm, m[c], s[c]) : 0.f;
                    const float v01 = k01 ? norm_pixel((float)pl[a01], norm, m[c], s[c]) : 0.f;
                    const float v10 = k10 ? norm_pixel((float)pl[a10], norm, m[c], s[c]) : 0.f;
                    const float v11 = k11 ? norm_pixel((float)pl[a11], norm, m[c], s[c]) : 0.f;
                    img[c] = bilinear(sx, sy, fx0, fy0, v00, v01, v10, v11);
                }
            }
            if (out_weights) {
                const float v00 = k00 ? wmap[a00] : 0.f, v01 = k01 ? wmap[a01] : 0.f;
                const float v10 = k10 ? wmap[a10] : 0.f, v11 = k11 ? wmap[a11] : 0.f;
                wv = bilinear(sx, sy, fx0, fy0, v00, v01, v10, v11);
            }
            if (out_onehot && inside) label = labels[fbase + (size_t)rr * g.W + cc];
        }
        if (out_image) {
            if (vec) {
                store_pixel<CI>(out_image + pix * CI, img);
            } else {
#pragma unroll
                for (int c = 0; c < CI; ++c) out_image[pix * CI + c] = img[c];
            }
        }
        if (out_weights) out_weights[pix] = wv + (inside ? 0.f : 1.f);
        if (out_onehot) store_onehot(out_onehot + pix * g.C, label, g.C, packed != 0);
    }
}

template <typename T, int CI>
void sample_mc_launch(const void *frames, int64_t chan_stride, const float *mean, const float *stdv, const uint8_t *labels,
                      const float *weights, const int32_t *plan, const float *coef, float *out_image, uint8_t *out_onehot,
                      float *out_weights, const TileGeom &g, int py, int count, hipStream_t st) {
    const int C = g.C;
    const bool packed = (C & (C - 1)) == 0 && (uintptr_t)out_onehot % C == 0;
    hipLaunchKernelGGL((tile_sample_mc_kernel<T, CI>), dim3((unsigned)(g.px * py), (unsigned)count), dim3(PATCH, ROWS), 0, st,
                       reinterpret_cast<const T *>(frames), chan_stride, mean, stdv, labels, weights, plan, coef, out_image,
                       out_onehot, out_weights, g, (int)rotate_lds(), (int)packed, (int)SQ_ALIGNED16(out_image));
}

template <typename T>
int sample_mc_dispatch(int CI, const void *frames, int64_t chan_stride, const float *mean, const float *stdv,
                       const uint8_t *labels, const float *weights, const int32_t *plan, const float *coef, float *out_image,
                       uint8_t *out_onehot, float *out_weights, const TileGeom &g, int py, int count, hipStream_t st) {
#define SQ_MC_CASE(N)                                                                                                    \
    case N:                                                                                                              \
        sample_mc_launch<T, N>(frames, chan_stride, mean, stdv, labels, weights, plan, coef, out_image, out_onehot,     \
                               out_weights, g, py, count, st);                                                           \
        break;
    switch (CI) {
        SQ_MC_CASE(1) SQ_MC_CASE(2) SQ_MC_CASE(3) SQ_MC_CASE(4) SQ_MC_CASE(5) SQ_MC_CASE(6) SQ_MC_CASE(7) SQ_MC_CASE(8)
    }
#undef SQ_MC_CASE
    return sq_check_launch("sq_tile_sample_affine_mc");
}

inline int pix_bytes(int dtype) { return dtype == SQ_PIX_U8 ? 1 : dtype == SQ_PIX_U16 ? 2 : 4; }

}  // namespace

extern "C" int sq_frames_to_tiles_mc(const void *frames, int dtype, int64_t chan_stride, const int32_t *chan_mode,
                                     const float *mean32, const float *std32, const double *coef, const double *mean64,
                                     const double *std64, const int32_t *oy, const int32_t *ox, float *tiles, int F, int H,
                                     int W, int C, int TR, int TC, int TS, void *stream) {
    const char *what = "sq_frames_to_tiles_mc";
    SQ_REQUIRE(frames && chan_mode && oy && ox && tiles, "%s: null pointer", what);
    SQ_REQUIRE(C >= 1 && C <= MAXC, "%s: %d channels not in 1 .. %d", what, C, MAXC);
    SQ_REQUIRE(dtype == SQ_PIX_U8 || dtype == SQ_PIX_U16 || dtype == SQ_PIX_F32, "%s: unknown pixel type %d", what, dtype);
    SQ_REQUIRE(F > 0 && H > 0 && W > 0 && TR > 0 && TC > 0 && TS > 0 && TS <= H && TS <= W, "%s: tile %d does not fit %d x %d",
               what, TS, H, W);
    SQ_REQUIRE(chan_stride >= (int64_t)F * H * W, "%s: chan_stride %lld is less than F*H*W = %lld", what,
               (long long)chan_stride, (long long)F * H * W);
    ChanModes modes = {};
    bool need32 = false, need_coef = false, need64 = false;
    for (int c = 0; c < C; ++c) {
        const int m = chan_mode[c];
        SQ_REQUIRE(m == SQ_CH_CAST || m == SQ_CH_NORM || m == SQ_CH_BG || m == SQ_CH_BG_NORM, "%s: unknown mode %d of channel %d",
                   what, m, c);
        modes.m[c] = m;
        need32 = need32 || m == SQ_CH_NORM;
        need_coef = need_coef || m == SQ_CH_BG || m == SQ_CH_BG_NORM;
        need64 = need64 || m == SQ_CH_BG_NORM;
    }
    SQ_REQUIRE(!need32 || (mean32 && std32), "%s: null pointer: a channel in mode SQ_CH_NORM needs mean32 and std32", what);
    SQ_REQUIRE(!need_coef || coef, "%s: null pointer: a channel in mode SQ_CH_BG / SQ_CH_BG_NORM needs coef", what);
    SQ_REQUIRE(!need64 || (mean64 && std64), "%s: null pointer: a channel in mode SQ_CH_BG_NORM needs mean64 and std64", what);
    SQ_REQUIRE(!need_coef || (dtype == SQ_PIX_F32 && H >= 3 && W >= 3),
               "%s: the background modes read float32 frames of H, W >= 3, got pixel type %d of %d x %d", what, dtype, H, W);
    const int64_t rows = (int64_t)F * TR * TC * TS, total = rows * TS;
    SQ_REQUIRE(rows <= 0x7fffffff && (total + CUT_CHUNK - 1) / CUT_CHUNK <= 0x7fffffff, "%s: %lld tile rows are out of range",
               what, (long long)rows);
    SQ_REQUIRE_ALIGNED(tiles);
    SQ_REQUIRE((uintptr_t)frames % pix_bytes(dtype) == 0 && ((uintptr_t)mean32 | (uintptr_t)std32 | (uintptr_t)oy | (uintptr_t)ox) % 4 == 0 &&
                   ((uintptr_t)coef | (uintptr_t)mean64 | (uintptr_t)std64) % 8 == 0,
               "%s: arrays must be aligned to their elements", what);
    hipStream_t st = (hipStream_t)stream;
    switch (dtype) {
    case SQ_PIX_U8:
        return tiles_mc_dispatch<uint8_t>(C, frames, chan_stride, modes, mean32, std32, coef, mean64, std64, oy, ox, tiles, F,
                                          H, W, TR, TC, TS, total, st);
    case SQ_PIX_U16:
        return tiles_mc_dispatch<uint16_t>(C, frames, chan_stride, modes, mean32, std32, coef, mean64, std64, oy, ox, tiles, F,
                                           H, W, TR, TC, TS, total, st);
    }
    return tiles_mc_dispatch<float>(C, frames, chan_stride, modes, mean32, std32, coef, mean64, std64, oy, ox, tiles, F, H, W,
                                    TR, TC, TS, total, st);
}

extern "C" int sq_tile_sample_affine_mc(const void *frames, int dtype, int64_t chan_stride, const float *mean,
                                        const float *stdv, const uint8_t *labels, const float *weights, const int32_t *plan,
                                        const float *coef, float *out_image, uint8_t *out_onehot, float *out_weights, int F,
                                        int H, int W, int CI, int TH, int TW, int C, int count, void *stream) {
    const char *what = "sq_tile_sample_affine_mc";
    SQ_REQUIRE(plan && coef, "%s: null pointer (plan, coef)", what);
    SQ_REQUIRE((frames == nullptr) == (out_image == nullptr), "%s: null pointer: frames and out_image go together", what);
    SQ_REQUIRE((labels == nullptr) == (out_onehot == nullptr), "%s: null pointer: labels and out_onehot go together", what);
    SQ_REQUIRE((weights == nullptr) == (out_weights == nullptr), "%s: null pointer: weights and out_weights go together", what);
    SQ_REQUIRE(out_image || out_onehot || out_weights, "%s: null pointer: no output was asked for", what);
    SQ_REQUIRE((mean == nullptr) == (stdv == nullptr), "%s: give both mean and std, or neither", what);
    SQ_REQUIRE(F > 0 && H > 0 && W > 0 && TH > 0 && TW > 0, "%s: sizes must be positive", what);
    SQ_REQUIRE((int64_t)H * W <= (1 << 24), "%s: frames of %d x %d exceed 2^24 pixels", what, H, W);
    SQ_REQUIRE(CI >= 1 && CI <= MAXC, "%s: %d image channels not in 1 .. %d", what, CI, MAXC);
    SQ_REQUIRE(C >= 1 && C <= 16, "%s: %d classes not in 1 .. 16", what, C);
    SQ_REQUIRE(count > 0 && count <= 65535, "%s: count %d not in 1 .. 65535", what, count);
    const int px = (TW + PATCH - 1) / PATCH, py = (TH + PATCH - 1) / PATCH;
    SQ_REQUIRE((int64_t)px * py <= 0x7fffffff, "%s: tile %d x %d out of range", what, TH, TW);
    if (frames) {
        SQ_REQUIRE(dtype == SQ_PIX_U8 || dtype == SQ_PIX_U16 || dtype == SQ_PIX_F32, "%s: unknown pixel type %d", what, dtype);
        SQ_REQUIRE(chan_stride >= (int64_t)F * H * W, "%s: chan_stride %lld is less than F*H*W = %lld", what,
                   (long long)chan_stride, (long long)F * H * W);
        SQ_REQUIRE((uintptr_t)frames % pix_bytes(dtype) == 0 && (uintptr_t)out_image % 4 == 0,
                   "%s: frames and out_image must be aligned to their elements", what);
    }
    SQ_REQUIRE(((uintptr_t)weights | (uintptr_t)out_weights | (uintptr_t)coef | (uintptr_t)plan | (uintptr_t)mean |
                (uintptr_t)stdv) % 4 == 0, "%s: float and int32 arrays must be aligned to their elements", what);
    const TileGeom g = {F, H, W, TH, TW, C, px};
    hipStream_t st = (hipStream_t)stream;
    if (!frames) mean = stdv = nullptr;
    if (frames && dtype == SQ_PIX_U16)
        return sample_mc_dispatch<uint16_t>(CI, frames, chan_stride, mean, stdv, labels, weights, plan, coef, out_image,
                                            out_onehot, out_weights, g, py, count, st);
    if (frames && dtype == SQ_PIX_F32)
        return sample_mc_dispatch<float>(CI, frames, chan_stride, mean, stdv, labels, weights, plan, coef, out_image,
                                         out_onehot, out_weights, g, py, count, st);
    return sample_mc_dispatch<uint8_t>(CI, frames, chan_stride, mean, stdv, labels, weights, plan, coef, out_image,
                                       out_onehot, out_weights, g, py, count, st);
}
