// Tile sampler: rotated training tiles cut out of whole frames that stay in HBM (include/sequitr_hip.h "Tile sampler"; the
// reference's tr_augment, sequitr/networks/unet.py:348-401: one random angle per element, image and weight map rotated
// bilinearly, labels by nearest neighbour, 1 - rotate(ones) added to the weights, a random crop, one-hot labels).  A
// sample is two rows, plan[k] = [f, oy, ox, 0] and coef[k] = [a0, a1, a2, b0, b1, b2]; the definition (the header's and
// tests/tile_sampler_cases.py's, word for word), for pixel (i, j) of sample k, tiles (TH, TW), frames (F, H, W):
//
//     x = float32(ox + j);  y = float32(oy + i)
//     sx = (a0*x + a1*y) + a2;   sy = (b0*x + b1*y) + b2     # float32, every * and + rounded on its own, no FMA
//     read_T(r, c) = T[f, r, c] if 0 <= f < F and 0 <= r < H and 0 <= c < W else 0
//     bilinear(T):  x0 = floor(sx), y0 = floor(sy), x1 = x0 + 1, y1 = y0 + 1
//         top = (x1 - sx) * read_T(y0, x0) + (sx - x0) * read_T(y0, x1)
//         bot = (x1 - sx) * read_T(y1, x0) + (sx - x0) * read_T(y1, x1)
//         val = (y1 - sy) * top + (sy - y0) * bot
//     nearest:  r = roundf(sy), c = roundf(sx)  (half away from zero);  inside = (r, c) in the frame and 0 <= f < F
//     image  [k,i,j,c] = bilinear(normalised plane c)                        # CI channel-major planes, "Tile front end"
//     onehot [k,i,j,q] = (read_labels(r, c) == q)                            # label 0 outside; label >= C: all zero
//     weights[k,i,j,0] = bilinear(weight map) + (inside ? 0.0f : 1.0f)
//
// A pixel whose sx or sy is NaN, or at or beyond +-2^23, reads fill everywhere (image 0, label 0, weight 1).  ox + j and
// oy + i are exact integer sums (64-bit) rounded once to float32.
//
// One kernel for both entries (sq_tile_sample_affine is CI = 1 with chan_stride = F*H*W), one launch for the three
// outputs; coordinates, corners and bilinear weights once per pixel, the interpolation per channel.  A block of 32 x 8 threads
// owns a 32 x 32 patch of one output tile (four rows per thread), so that its source footprint is compact at any angle.
//   direct form : every corner is a guarded global load -- the definition.
//   LDS form    : sx and sy are monotone in j for a fixed i and in i for a fixed j (each product and each sum is a monotone
//                 function of one argument, and rounding keeps the order), so over the patch their extremes lie at its four
//                 corners.  The block takes the bounding box of those four, widens it by the one-pixel bilinear apron
//                 (which also holds every nearest-neighbour pixel), stages the normalised image, the weights and the labels
//                 of the box into LDS -- lanes along the source rows, fill applied while staging -- and interpolates from
//                 there; one pass per image plane through the same buffer, labels and weights with the first.  A block
//                 whose box exceeds BOX x BOX pixels (a zooming or shearing row), or one of whose corners is out of range,
//                 takes the direct form; the decision is uniform per block.
// Both forms evaluate the same expressions on the same values, so they give the same bits.  SQ_ROTATE_LDS (read per
// launch): 0 selects the direct form everywhere, 1 the LDS form wherever the box fits; unset is the direct form, the faster
// one as measured.
#include <stdlib.h>
#include "sq_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int PATCH = 32;                                       // output pixels per block along each axis
constexpr int ROWS = 8;                                         // blockDim.y: a thread takes PATCH / ROWS rows
constexpr int BOX = 48;                                         // largest staged box: 31 * sqrt(2) + 1 + the apron, rounded up
constexpr int PITCH = BOX + 1;                                  // odd pitch: a column walk touches every bank
constexpr float LIMIT = 8388608.f;                              // 2^23
constexpr int MAXC = 8;                                         // image channels

struct TileGeom {
    int F, H, W, TH, TW, C, px;                                 // px: patches along a tile row
};

struct Affine {
    float a0, a1, a2, b0, b1, b2;
};

__device__ __forceinline__ void source_xy(const Affine &t, long long X, long long Y, float &sx, float &sy) {
#pragma clang fp contract(off)
    const float x = (float)X, y = (float)Y;
    const float p = t.a0 * x, q = t.a1 * y;
    sx = (p + q) + t.a2;
    const float u = t.b0 * x, v = t.b1 * y;
    sy = (u + v) + t.b2;
}

__device__ __forceinline__ bool in_range(float sx, float sy) {  // false for NaN
    return fabsf(sx) < LIMIT && fabsf(sy) < LIMIT;
}

__device__ __forceinline__ float bilinear(float sx, float sy, float fx0, float fy0, float v00, float v01, float v10, float v11) {
#pragma clang fp contract(off)
    const float fx1 = fx0 + 1.f, fy1 = fy0 + 1.f;
    const float wl = fx1 - sx, wr = sx - fx0;
    const float tl = wl * v00, tr = wr * v01;
    const float top = tl + tr;
    const float bl = wl * v10, br = wr * v11;
    const float bot = bl + br;
    const float a = (fy1 - sy) * top, b = (sy - fy0) * bot;
    return a + b;
}

__device__ __forceinline__ float norm_pixel(float r, bool norm, float m, float s) {
#pragma clang fp contract(off)
    return norm ? (r - m) / s : r;                              // ImageNorm: the tile cutter's expression
}

// C bytes (label == q), q = 0 .. C-1, at p; `packed`: p is aligned to C, a power of two
__device__ __forceinline__ void store_onehot(uint8_t *p, unsigned label, int C, bool packed) {
    if (packed) {
        const uint64_t lo = label < 8u ? (uint64_t)1 << (8 * label) : 0;
        switch (C) {
        case 1: *p = (uint8_t)lo; return;
        case 2: *reinterpret_cast<uint16_t *>(p) = (uint16_t)lo; return;
        case 4: *reinterpret_cast<uint32_t *>(p) = (uint32_t)lo; return;
        case 8: *reinterpret_cast<uint64_t *>(p) = lo; return;
        default: {                                              // 16
            const uint64_t hi = (label >= 8u && label < 16u) ? (uint64_t)1 << (8 * (label - 8u)) : 0;
            uint64_t *d = reinterpret_cast<uint64_t *>(p);
            d[0] = lo;
            d[1] = hi;
            return;
        }
        }
    }
    for (int q = 0; q < C; ++q) p[q] = (uint8_t)(label == (unsigned)q);
}

// SQ_ROTATE_LDS, read per launch: 0 = the direct gather everywhere, 1 = the LDS form wherever the box fits.  Unset is the
// direct gather, the faster of the two as measured (tools/tile_sampler_bench.py: 0.77x the LDS form's time at theta = 0,
// 0.96-0.97x at pi/4 and at random angles -- a 32 x 32 patch's footprint is compact enough for L2 to serve the four
// corners, and staging costs a barrier and a second pass).
inline bool rotate_lds() {
    const char *e = getenv("SQ_ROTATE_LDS");
    return e && e[0] == '1';
}

constexpr int NU = PATCH / ROWS;

// grid (patches of a tile, count), block (PATCH, ROWS).  `vec`: out_image is 16-byte aligned, a pixel's CI > 1 floats go
// out in one piece.
template <typename T, int CI>
__global__ __launch_bounds__(PATCH * ROWS) void tile_sample_kernel(
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
    // stage: lanes along the box's rows (the source's contiguous axis), 64 columns x 4 rows per pass
    const int tid = ty * PATCH + tx, sc = tid & 63, r0 = tid >> 6;
    const unsigned gc = (unsigned)(bx0 + sc);
    const bool col_ok = fok && sc < bw && gc < W;
    if (lds) {                                                  // the first image plane, the weights and the labels
        if (sc < bw) {
            for (int r = r0; r < bh; r += 4) {
                const unsigned gr = (unsigned)(by0 + r);
                const bool ok = col_ok && gr < H;
                const size_t src = fbase + (size_t)(ok ? gr : 0u) * g.W + (ok ? gc : 0u);
                if (out_image) s_img[r * PITCH + sc] = ok ? norm_pixel((float)frames[src], norm, m[0], s[0]) : 0.f;
                if (out_weights) s_wts[r * PITCH + sc] = ok ? wmap[src] : 0.f;
                if (out_onehot) s_lab[r * PITCH + sc] = ok ? labels[src] : (uint8_t)0;
            }
        }
        __syncthreads();
    }

    // Every thread of the block reaches every barrier below: a thread outside the tile only stages.
    const int j = j0 + tx;
    if (j < g.TW) {
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
                if (lds) {                                      // image planes 1 .. CI-1 follow, one pass each
                    const int a = (y0 - by0) * PITCH + (x0 - bx0);
                    if (out_image) img[0] = bilinear(sx, sy, fx0, fy0, s_img[a], s_img[a + 1], s_img[a + PITCH], s_img[a + PITCH + 1]);
                    if (out_weights) wv = bilinear(sx, sy, fx0, fy0, s_wts[a], s_wts[a + 1], s_wts[a + PITCH], s_wts[a + PITCH + 1]);
                    if (out_onehot) label = s_lab[(rr - by0) * PITCH + (cc - bx0)];
                } else {
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
            }
            if (out_image) {
                if (lds) {
                    out_image[pix * CI] = img[0];
                } else if (vec) {
                    sq_store_pixel<CI>(out_image + pix * CI, img);
                } else {
#pragma unroll
                    for (int c = 0; c < CI; ++c) out_image[pix * CI + c] = img[c];
                }
            }
            if (out_weights) out_weights[pix] = wv + (inside ? 0.f : 1.f);
            if (out_onehot) store_onehot(out_onehot + pix * g.C, label, g.C, packed != 0);
        }
    }

    if constexpr (CI > 1) {                                     // the LDS form's other image planes, through the same buffer
        if (!lds || !out_image) return;
        for (int c = 1; c < CI; ++c) {
            __syncthreads();                                    // the previous plane has been read
            if (sc < bw) {
                const T *__restrict__ pl = frames + (size_t)c * chan_stride;
                for (int r = r0; r < bh; r += 4) {
                    const unsigned gr = (unsigned)(by0 + r);
                    const bool ok = col_ok && gr < H;
                    const size_t src = fbase + (size_t)(ok ? gr : 0u) * g.W + (ok ? gc : 0u);
                    s_img[r * PITCH + sc] = ok ? norm_pixel((float)pl[src], norm, m[c], s[c]) : 0.f;
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
                float img = 0.f;
                if (in_range(sx, sy)) {
                    const float fx0 = floorf(sx), fy0 = floorf(sy);
                    const int a = ((int)fy0 - by0) * PITCH + ((int)fx0 - bx0);
                    img = bilinear(sx, sy, fx0, fy0, s_img[a], s_img[a + 1], s_img[a + PITCH], s_img[a + PITCH + 1]);
                }
                out_image[(((size_t)k * g.TH + i) * g.TW + j) * CI + c] = img;
            }
        }
    }
}

template <typename T, int CI>
void sample_launch(const void *frames, int64_t chan_stride, const float *mean, const float *stdv, const uint8_t *labels,
                   const float *weights, const int32_t *plan, const float *coef, float *out_image, uint8_t *out_onehot,
                   float *out_weights, const TileGeom &g, int py, int count, hipStream_t st) {
    const int C = g.C;
    const bool packed = (C & (C - 1)) == 0 && (uintptr_t)out_onehot % C == 0;
    hipLaunchKernelGGL((tile_sample_kernel<T, CI>), dim3((unsigned)(g.px * py), (unsigned)count), dim3(PATCH, ROWS), 0, st,
                       reinterpret_cast<const T *>(frames), chan_stride, mean, stdv, labels, weights, plan, coef, out_image,
                       out_onehot, out_weights, g, (int)rotate_lds(), (int)packed, (int)(CI > 1 && SQ_ALIGNED16(out_image)));
}

template <typename T>
void sample_channels(int CI, const void *frames, int64_t chan_stride, const float *mean, const float *stdv,
                     const uint8_t *labels, const float *weights, const int32_t *plan, const float *coef, float *out_image,
                     uint8_t *out_onehot, float *out_weights, const TileGeom &g, int py, int count, hipStream_t st) {
#define SQ_CI_CASE(N)                                                                                                    \
    case N:                                                                                                              \
        return sample_launch<T, N>(frames, chan_stride, mean, stdv, labels, weights, plan, coef, out_image, out_onehot, \
                                   out_weights, g, py, count, st);
    switch (CI) {
        SQ_CI_CASE(1) SQ_CI_CASE(2) SQ_CI_CASE(3) SQ_CI_CASE(4) SQ_CI_CASE(5) SQ_CI_CASE(6) SQ_CI_CASE(7) SQ_CI_CASE(8)
    }
#undef SQ_CI_CASE
}

// both entries' checks, in one order, and the launch; `what` names the entry in every message
int sample_affine(const char *what, const void *frames, int dtype, int64_t chan_stride, const float *mean, const float *stdv,
                  const uint8_t *labels, const float *weights, const int32_t *plan, const float *coef, float *out_image,
                  uint8_t *out_onehot, float *out_weights, int F, int H, int W, int CI, int TH, int TW, int C, int count,
                  void *stream) {
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
        SQ_REQUIRE((uintptr_t)frames % (dtype == SQ_PIX_U8 ? 1 : dtype == SQ_PIX_U16 ? 2 : 4) == 0 && (uintptr_t)out_image % 4 == 0,
                   "%s: frames and out_image must be aligned to their elements", what);
    }
    SQ_REQUIRE(((uintptr_t)weights | (uintptr_t)out_weights | (uintptr_t)coef | (uintptr_t)plan | (uintptr_t)mean |
                (uintptr_t)stdv) % 4 == 0, "%s: float and int32 arrays must be aligned to their elements", what);
    const TileGeom g = {F, H, W, TH, TW, C, px};
    hipStream_t st = (hipStream_t)stream;
    if (!frames) mean = stdv = nullptr;
    if (frames && dtype == SQ_PIX_U16)
        sample_channels<uint16_t>(CI, frames, chan_stride, mean, stdv, labels, weights, plan, coef, out_image, out_onehot,
                                  out_weights, g, py, count, st);
    else if (frames && dtype == SQ_PIX_F32)
        sample_channels<float>(CI, frames, chan_stride, mean, stdv, labels, weights, plan, coef, out_image, out_onehot,
                               out_weights, g, py, count, st);
    else
        sample_channels<uint8_t>(CI, frames, chan_stride, mean, stdv, labels, weights, plan, coef, out_image, out_onehot,
                                 out_weights, g, py, count, st);
    return sq_check_launch(what);
}

}  // namespace

extern "C" int sq_tile_sample_affine(const void *frames, int dtype, const float *mean, const float *stdv,
                                     const uint8_t *labels, const float *weights, const int32_t *plan, const float *coef,
                                     float *out_image, uint8_t *out_onehot, float *out_weights, int F, int H, int W, int TH,
                                     int TW, int C, int count, void *stream) {
    return sample_affine("sq_tile_sample_affine", frames, dtype, (int64_t)F * H * W, mean, stdv, labels, weights, plan, coef,
                         out_image, out_onehot, out_weights, F, H, W, 1, TH, TW, C, count, stream);
}

extern "C" int sq_tile_sample_affine_mc(const void *frames, int dtype, int64_t chan_stride, const float *mean,
                                        const float *stdv, const uint8_t *labels, const float *weights, const int32_t *plan,
                                        const float *coef, float *out_image, uint8_t *out_onehot, float *out_weights, int F,
                                        int H, int W, int CI, int TH, int TW, int C, int count, void *stream) {
    return sample_affine("sq_tile_sample_affine_mc", frames, dtype, chan_stride, mean, stdv, labels, weights, plan, coef,
                         out_image, out_onehot, out_weights, F, H, W, CI, TH, TW, C, count, stream);
}
