// Tile front end on the GPU (the caller side of the inference hot path).
// Raw camera frames (uint8 / uint16 / float32, single channel; OctopusData .dat, dataio/octopus.py:231-245)
// -> ImageNorm (sequitr/pipeline.py:350-356: (x - mean) / (1e-99 + std) per frame, float32)
// -> fixed-size network tiles (N,T,T,1) f32 in HBM;  and back: tile masks -> full-frame masks.
//
// ImageNorm parity is BIT-EXACT with numpy, which means reproducing numpy's float32 summation order (sq_pairwise.h:
// 8192-element chunks, pairwise blocks of 128 with 8 accumulators, one wave per chunk).  HBM-bound: the frame is read 3
// times (mean, variance, normalise) at 1-4 B/pixel and the tiles written once at 4 B/pixel.
//
// One kernel cuts the tiles for every entry (sq_frames_to_tiles, sq_frames_to_tiles_bg, sq_frames_to_tiles_mc): frames are
// C channel-major planes (include/sequitr_hip.h "Tile front end"; the single-channel entries are C = 1), every channel
// under its own mode.  A lane owns one tile pixel: it reads that pixel from each of the C planes -- a wave reads 64
// consecutive pixels of a frame row per plane -- and stores its C floats at once, so a wave writes 64 * C consecutive
// floats (a scalar per lane at C = 1, b64 at 2, b128 at 4, two b128 at 8).  A pixel's output offset is (flat pixel) * C
// floats, so the stores are aligned whatever the tile size is.  No LDS: nothing is read twice.  Contraction is off and the
// background surface's fused operations are written out (sq_bg_surface.h), so the roundings are stated.
#include "sq_pairwise.h"   // numpy's summation order: frame_chunk_sums_kernel; contraction off from here on
#include "sq_bg_surface.h"

namespace {

// res = 0; res += chunk (in order); then mean = res / n   or   std = sqrt(res / n)
__global__ void frame_stats_finish_kernel(const float *__restrict__ chunk_sums, float *__restrict__ out, int F,
                                          int nchunks, float n, int take_sqrt) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    float res = 0.f;
    for (int c = 0; c < nchunks; ++c) res = res + chunk_sums[(size_t)f * nchunks + c];
    res = res / n;
    out[f] = take_sqrt ? sqrtf(res) : res;
}

constexpr int MAXC = 8;

struct ChanModes {
    int m[MAXC];
};

constexpr int CUT_THREADS = 256, CUT_PER_THREAD = 4, CUT_CHUNK = CUT_THREADS * CUT_PER_THREAD;

// tile t = (f, ty, tx), pixel (y, x), channel c: out[t][y][x][c] = mode c of plane c's frame[f][oy[ty]+y][ox[tx]+x].
// A block takes CUT_CHUNK consecutive pixels of the flat (tile, y, x) order; the one 64-bit division is the block's.
template <typename T, int C>
__global__ __launch_bounds__(CUT_THREADS) void tiles_kernel(
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
                o[c] = ((float)raw - mean32[cf]) / std32[cf];
            } else {                                                        // the one rounding to float32 of the chain
                const BgRow br = bg_row(coef + cf * 6, tt);
                const double r = (double)raw - bg_eval(br, ss);
                o[c] = (float)(mode == SQ_CH_BG_NORM ? (r - mean64[cf]) / (1e-99 + std64[cf]) : r);
            }
        }
        sq_store_pixel<C>(tiles + (size_t)p * C, o);
    }
}

// full-frame mask: pixel (y, x) takes the tile that owns it (ymap / xmap: tile index << 16 | local coordinate)
__global__ __launch_bounds__(256) void stitch_masks_kernel(const uint8_t *__restrict__ tile_masks,
                                                           const int *__restrict__ ymap, const int *__restrict__ xmap,
                                                           uint8_t *__restrict__ out, int F, int H, int W, int TR, int TC,
                                                           int TS) {
    const int64_t total = (int64_t)F * H * W;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % W), y = (int)((i / W) % H), f = (int)(i / ((int64_t)H * W));
        const int ym = ymap[y], xm = xmap[x];
        const size_t t = ((size_t)f * TR + (ym >> 16)) * TC + (xm >> 16);
        out[i] = tile_masks[(t * TS + (ym & 0xffff)) * TS + (xm & 0xffff)];
    }
}

inline unsigned fe_grid(int64_t items) {
    int64_t b = (items + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 16384 ? 16384 : b));
}

template <typename T>
int stats_launch(const T *frames, float *mean, float *stdv, float *ws, int F, int64_t npix, hipStream_t st) {
    const int nchunks = (int)((npix + CHUNK - 1) / CHUNK);
    dim3 grid((nchunks + 3) / 4, F);
    hipLaunchKernelGGL((frame_chunk_sums_kernel<T, false>), grid, dim3(256), 0, st, frames, (const float *)nullptr, ws,
                       npix, nchunks);
    hipLaunchKernelGGL(frame_stats_finish_kernel, dim3((F + 63) / 64), dim3(64), 0, st, ws, mean, F, nchunks, (float)npix, 0);
    hipLaunchKernelGGL((frame_chunk_sums_kernel<T, true>), grid, dim3(256), 0, st, frames, mean, ws, npix, nchunks);
    hipLaunchKernelGGL(frame_stats_finish_kernel, dim3((F + 63) / 64), dim3(64), 0, st, ws, stdv, F, nchunks, (float)npix, 1);
    return sq_check_launch("sq_frame_stats");
}

// what an entry hands the cutter once its own checks have passed
struct CutJob {
    const void *frames;
    int dtype;
    int64_t chan_stride;
    ChanModes modes;
    const float *mean32, *std32;
    const double *coef, *mean64, *std64;
    const int *oy, *ox;
    float *tiles;
    int F, H, W, C, TR, TC, TS;
};

template <typename T, int C>
void cut_launch(const CutJob &j, int64_t total, hipStream_t st) {
    hipLaunchKernelGGL((tiles_kernel<T, C>), dim3((unsigned)((total + CUT_CHUNK - 1) / CUT_CHUNK)), dim3(CUT_THREADS), 0, st,
                       reinterpret_cast<const T *>(j.frames), j.chan_stride, j.modes, j.mean32, j.std32, j.coef, j.mean64,
                       j.std64, j.oy, j.ox, j.tiles, j.F, j.H, j.W, j.TR, j.TC, j.TS, total);
}

template <typename T>
void cut_channels(const CutJob &j, int64_t total, hipStream_t st) {
    switch (j.C) {
    case 1: return cut_launch<T, 1>(j, total, st);
    case 2: return cut_launch<T, 2>(j, total, st);
    case 3: return cut_launch<T, 3>(j, total, st);
    case 4: return cut_launch<T, 4>(j, total, st);
    case 5: return cut_launch<T, 5>(j, total, st);
    case 6: return cut_launch<T, 6>(j, total, st);
    case 7: return cut_launch<T, 7>(j, total, st);
    case 8: return cut_launch<T, 8>(j, total, st);
    }
}

// the kernel indexes tile rows in 32 bits: every entry refuses more, among its own checks
int cut_range(const char *what, int F, int TR, int TC, int TS) {
    const int64_t rows = (int64_t)F * TR * TC * TS;
    SQ_REQUIRE(rows <= 0x7fffffff && (rows * TS + CUT_CHUNK - 1) / CUT_CHUNK <= 0x7fffffff, "%s: %lld tile rows are out of range",
               what, (long long)rows);
    return SQ_OK;
}

int cut_tiles(const char *what, const CutJob &j, void *stream) {
    const int64_t total = (int64_t)j.F * j.TR * j.TC * j.TS * j.TS;
    hipStream_t st = (hipStream_t)stream;
    switch (j.dtype) {
    case SQ_PIX_U8: cut_channels<uint8_t>(j, total, st); break;
    case SQ_PIX_U16: cut_channels<uint16_t>(j, total, st); break;
    default: cut_channels<float>(j, total, st); break;
    }
    return sq_check_launch(what);
}

inline int pix_bytes(int dtype) { return dtype == SQ_PIX_U8 ? 1 : dtype == SQ_PIX_U16 ? 2 : 4; }

}  // namespace

extern "C" int64_t sq_frame_stats_workspace(int F, int H, int W) {
    if (F <= 0 || H <= 0 || W <= 0) return -1;
    const int64_t npix = (int64_t)H * W;
    if (npix > (1 << 24)) return -1;                            // n must be exact in float32 (numpy divides by it)
    return (int64_t)F * ((npix + CHUNK - 1) / CHUNK) * 4;
}

extern "C" int sq_frame_stats(const void *frames, int dtype, float *mean, float *stdv, void *workspace, int F, int H,
                              int W, void *stream) {
    SQ_REQUIRE(frames && mean && stdv && workspace, "sq_frame_stats: null pointer");
    SQ_REQUIRE(sq_frame_stats_workspace(F, H, W) > 0, "sq_frame_stats: need F, H, W > 0 and H*W <= 2^24");
    // aligned to the pixel type: a channel's slice of multi-channel planes starts wherever c * chan_stride falls, as frame
    // f > 0 of an odd-sized stack always did (the kernel reads element by element)
    SQ_REQUIRE((uintptr_t)frames % (dtype == SQ_PIX_U16 ? 2 : dtype == SQ_PIX_F32 ? 4 : 1) == 0,
               "sq_frame_stats: frames not aligned to their pixel type");
    hipStream_t st = (hipStream_t)stream;
    const int64_t npix = (int64_t)H * W;
    float *ws = reinterpret_cast<float *>(workspace);
    switch (dtype) {
    case SQ_PIX_U8: return stats_launch(reinterpret_cast<const uint8_t *>(frames), mean, stdv, ws, F, npix, st);
    case SQ_PIX_U16: return stats_launch(reinterpret_cast<const uint16_t *>(frames), mean, stdv, ws, F, npix, st);
    case SQ_PIX_F32: return stats_launch(reinterpret_cast<const float *>(frames), mean, stdv, ws, F, npix, st);
    }
    sq_set_error("sq_frame_stats: unknown pixel type %d", dtype);
    return SQ_EINVAL;
}

extern "C" int sq_frames_to_tiles(const void *frames, int dtype, const float *mean, const float *stdv, const int32_t *oy,
                                  const int32_t *ox, float *tiles, int F, int H, int W, int TR, int TC, int TS,
                                  void *stream) {
    SQ_REQUIRE(frames && oy && ox && tiles, "sq_frames_to_tiles: null pointer");
    SQ_REQUIRE((mean == nullptr) == (stdv == nullptr), "sq_frames_to_tiles: give both mean and std, or neither");
    SQ_REQUIRE(F > 0 && TR > 0 && TC > 0 && TS > 0 && TS <= H && TS <= W, "sq_frames_to_tiles: tile %d does not fit %dx%d",
               TS, H, W);
    SQ_REQUIRE(dtype == SQ_PIX_U8 || dtype == SQ_PIX_U16 || dtype == SQ_PIX_F32, "sq_frames_to_tiles: unknown pixel type %d",
               dtype);
    if (const int e = cut_range("sq_frames_to_tiles", F, TR, TC, TS)) return e;
    const CutJob j = {frames, dtype, (int64_t)F * H * W, {{mean ? SQ_CH_NORM : SQ_CH_CAST}}, mean, stdv, nullptr, nullptr,
                      nullptr, oy, ox, tiles, F, H, W, 1, TR, TC, TS};
    return cut_tiles("sq_frames_to_tiles", j, stream);
}

extern "C" int sq_frames_to_tiles_bg(const float *frames, const double *coef, const double *mean, const double *stdv,
                                     const int32_t *oy, const int32_t *ox, float *tiles, int F, int H, int W, int TR, int TC,
                                     int TS, void *stream) {
    SQ_REQUIRE(frames && coef && oy && ox && tiles, "sq_frames_to_tiles_bg: null pointer");
    SQ_REQUIRE((mean == nullptr) == (stdv == nullptr), "sq_frames_to_tiles_bg: give both mean and std, or neither");
    SQ_REQUIRE(F > 0 && H >= 3 && W >= 3 && TR > 0 && TC > 0 && TS > 0 && TS <= H && TS <= W,
               "sq_frames_to_tiles_bg: tile %d does not fit %d x %d (H, W >= 3)", TS, H, W);
    if (const int e = cut_range("sq_frames_to_tiles_bg", F, TR, TC, TS)) return e;
    const CutJob j = {frames, SQ_PIX_F32, (int64_t)F * H * W, {{mean ? SQ_CH_BG_NORM : SQ_CH_BG}}, nullptr, nullptr, coef,
                      mean, stdv, oy, ox, tiles, F, H, W, 1, TR, TC, TS};
    return cut_tiles("sq_frames_to_tiles_bg", j, stream);
}

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
    if (const int e = cut_range(what, F, TR, TC, TS)) return e;
    SQ_REQUIRE_ALIGNED(tiles);
    SQ_REQUIRE((uintptr_t)frames % pix_bytes(dtype) == 0 && ((uintptr_t)mean32 | (uintptr_t)std32 | (uintptr_t)oy | (uintptr_t)ox) % 4 == 0 &&
                   ((uintptr_t)coef | (uintptr_t)mean64 | (uintptr_t)std64) % 8 == 0,
               "%s: arrays must be aligned to their elements", what);
    const CutJob j = {frames, dtype, chan_stride, modes, mean32, std32, coef, mean64, std64, oy, ox, tiles, F, H, W, C, TR, TC, TS};
    return cut_tiles(what, j, stream);
}

extern "C" int sq_stitch_masks_u8(const uint8_t *tile_masks, const int32_t *ymap, const int32_t *xmap, uint8_t *out, int F,
                                  int H, int W, int TR, int TC, int TS, void *stream) {
    SQ_REQUIRE(tile_masks && ymap && xmap && out, "sq_stitch_masks_u8: null pointer");
    SQ_REQUIRE(F > 0 && H > 0 && W > 0 && TR > 0 && TC > 0 && TS > 0 && TS < 65536, "sq_stitch_masks_u8: bad geometry");
    hipLaunchKernelGGL(stitch_masks_kernel, dim3(fe_grid((int64_t)F * H * W)), dim3(256), 0, (hipStream_t)stream, tile_masks,
                       ymap, xmap, out, F, H, W, TR, TC, TS);
    return sq_check_launch("sq_stitch_masks_u8");
}
