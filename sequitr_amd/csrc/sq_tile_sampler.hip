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
//     image  [k,i,j,0] = bilinear(normalised frame)
//     onehot [k,i,j,q] = (read_labels(r, c) == q)                            # label 0 outside; label >= C: all zero
//     weights[k,i,j,0] = bilinear(weight map) + (inside ? 0.0f : 1.0f)
//
// A pixel whose sx or sy is NaN, or at or beyond +-2^23, reads fill everywhere (image 0, label 0, weight 1).  ox + j and
// oy + i are exact integer sums (64-bit) rounded once to float32.
//
// One kernel, one launch for the three outputs, the coordinates computed once per pixel.  A block of 32 x 8 threads
// owns a 32 x 32 patch of one output tile (four rows per thread), so that its source footprint is compact at any angle.
//   direct form : every corner is a guarded global load -- the definition.
//   LDS form    : sx and sy are monotone in j for a fixed i and in i for a fixed j (each product and each sum is a monotone
//                 function of one argument, and rounding keeps the order), so over the patch their extremes lie at its four
//                 corners.  The block takes the bounding box of those four, widens it by the one-pixel bilinear apron
//                 (which also holds every nearest-neighbour pixel), stages the normalised image, the weights and the labels
//                 of the box into LDS -- lanes along the source rows, fill applied while staging -- and interpolates from
//                 there.  A block whose box exceeds BOX x BOX pixels (a zooming or shearing row), or one of whose corners
//                 is out of range, takes the direct form; the decision is uniform per block.
// Both forms evaluate the same expressions on the same values, so they give the same bits.  SQ_ROTATE_LDS (read per
// launch): 0 selects the direct form everywhere, 1 the LDS form wherever the box fits; unset is the direct form, the faster
// one as measured.
#include "sq_tile_sample.h"   // patch geometry, coordinates, bilinear, one-hot store, SQ_ROTATE_LDS: shared with the _mc entry

#pragma clang fp contract(off)

namespace {

// grid (patches of a tile, count), block (PATCH, ROWS)
template <typename T>
__global__ __launch_bounds__(PATCH * ROWS) void tile_sample_kernel(
    const T *__restrict__ frames, const float *__restrict__ mean, const float *__restrict__ stdv,
    const uint8_t *__restrict__ labels, const float *__restrict__ wmap, const int *__restrict__ plan,
    const float *__restrict__ coef, float *__restrict__ out_image, uint8_t *__restrict__ out_onehot,
    float *__restrict__ out_weights, TileGeom g, int want_lds, int packed) {
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
    const float m = (norm && fok) ? mean[f] : 0.f, s = (norm && fok) ? stdv[f] : 1.f;
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
    if (lds) {
        // stage: lanes along the box's rows (the source's contiguous axis), 64 columns x 4 rows per pass
        const int tid = ty * PATCH + tx, c = tid & 63, r0 = tid >> 6;
        const unsigned gc = (unsigned)(bx0 + c);
        const bool col_ok = fok && c < bw && gc < W;
        if (c < bw) {
            for (int r = r0; r < bh; r += 4) {
                const unsigned gr = (unsigned)(by0 + r);
                const bool ok = col_ok && gr < H;
                const size_t src = fbase + (size_t)(ok ? gr : 0u) * g.W + (ok ? gc : 0u);
                if (out_image) s_img[r * PITCH + c] = ok ? norm_pixel((float)frames[src], norm, m, s) : 0.f;
                if (out_weights) s_wts[r * PITCH + c] = ok ? wmap[src] : 0.f;
                if (out_onehot) s_lab[r * PITCH + c] = ok ? labels[src] : (uint8_t)0;
            }
        }
        __syncthreads();
    }

    const int j = j0 + tx;
    if (j >= g.TW) return;
#pragma unroll
    for (int u = 0; u < PATCH / ROWS; ++u) {
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
            if (lds) {
                const int a = (y0 - by0) * PITCH + (x0 - bx0);
                if (out_image) img = bilinear(sx, sy, fx0, fy0, s_img[a], s_img[a + 1], s_img[a + PITCH], s_img[a + PITCH + 1]);
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
                    const float v00 = k00 ? norm_pixel((float)frames[a00], norm, m, s) : 0.f;
                    const float v01 = k01 ? norm_pixel((float)frames[a01], norm, m, s) : 0.f;
                    const float v10 = k10 ? norm_pixel((float)frames[a10], norm, m, s) : 0.f;
                    const float v11 = k11 ? norm_pixel((float)frames[a11], norm, m, s) : 0.f;
                    img = bilinear(sx, sy, fx0, fy0, v00, v01, v10, v11);
                }
                if (out_weights) {
                    const float v00 = k00 ? wmap[a00] : 0.f, v01 = k01 ? wmap[a01] : 0.f;
                    const float v10 = k10 ? wmap[a10] : 0.f, v11 = k11 ? wmap[a11] : 0.f;
                    wv = bilinear(sx, sy, fx0, fy0, v00, v01, v10, v11);
                }
                if (out_onehot && inside) label = labels[fbase + (size_t)rr * g.W + cc];
            }
        }
        if (out_image) out_image[pix] = img;
        if (out_weights) out_weights[pix] = wv + (inside ? 0.f : 1.f);
        if (out_onehot) store_onehot(out_onehot + pix * g.C, label, g.C, packed != 0);
    }
}

template <typename T>
int sample_launch(const void *frames, const float *mean, const float *stdv, const uint8_t *labels, const float *weights,
                  const int32_t *plan, const float *coef, float *out_image, uint8_t *out_onehot, float *out_weights,
                  const TileGeom &g, int py, int count, hipStream_t st) {
    const int C = g.C;
    const bool packed = (C & (C - 1)) == 0 && (uintptr_t)out_onehot % C == 0;
    hipLaunchKernelGGL(tile_sample_kernel<T>, dim3((unsigned)(g.px * py), (unsigned)count), dim3(PATCH, ROWS), 0, st,
                       reinterpret_cast<const T *>(frames), mean, stdv, labels, weights, plan, coef, out_image, out_onehot,
                       out_weights, g, (int)rotate_lds(), (int)packed);
    return sq_check_launch("sq_tile_sample_affine");
}

}  // namespace

extern "C" int sq_tile_sample_affine(const void *frames, int dtype, const float *mean, const float *stdv,
                                     const uint8_t *labels, const float *weights, const int32_t *plan, const float *coef,
                                     float *out_image, uint8_t *out_onehot, float *out_weights, int F, int H, int W, int TH,
                                     int TW, int C, int count, void *stream) {
    const char *what = "sq_tile_sample_affine";
    SQ_REQUIRE(plan && coef, "%s: null pointer (plan, coef)", what);
    SQ_REQUIRE((frames == nullptr) == (out_image == nullptr), "%s: null pointer: frames and out_image go together", what);
    SQ_REQUIRE((labels == nullptr) == (out_onehot == nullptr), "%s: null pointer: labels and out_onehot go together", what);
    SQ_REQUIRE((weights == nullptr) == (out_weights == nullptr), "%s: null pointer: weights and out_weights go together", what);
    SQ_REQUIRE(out_image || out_onehot || out_weights, "%s: null pointer: no output was asked for", what);
    SQ_REQUIRE((mean == nullptr) == (stdv == nullptr), "%s: give both mean and std, or neither", what);
    SQ_REQUIRE(F > 0 && H > 0 && W > 0 && TH > 0 && TW > 0, "%s: sizes must be positive", what);
    SQ_REQUIRE((int64_t)H * W <= (1 << 24), "%s: frames of %d x %d exceed 2^24 pixels", what, H, W);
    SQ_REQUIRE(C >= 1 && C <= 16, "%s: %d classes not in 1 .. 16", what, C);
    SQ_REQUIRE(count > 0 && count <= 65535, "%s: count %d not in 1 .. 65535", what, count);
    const int px = (TW + PATCH - 1) / PATCH, py = (TH + PATCH - 1) / PATCH;
    SQ_REQUIRE((int64_t)px * py <= 0x7fffffff, "%s: tile %d x %d out of range", what, TH, TW);
    if (frames) {
        SQ_REQUIRE(dtype == SQ_PIX_U8 || dtype == SQ_PIX_U16 || dtype == SQ_PIX_F32, "%s: unknown pixel type %d", what, dtype);
        SQ_REQUIRE((uintptr_t)frames % (dtype == SQ_PIX_U8 ? 1 : dtype == SQ_PIX_U16 ? 2 : 4) == 0 && (uintptr_t)out_image % 4 == 0,
                   "%s: frames and out_image must be aligned to their elements", what);
    }
    SQ_REQUIRE(((uintptr_t)weights | (uintptr_t)out_weights | (uintptr_t)coef | (uintptr_t)plan | (uintptr_t)mean |
                (uintptr_t)stdv) % 4 == 0, "%s: float and int32 arrays must be aligned to their elements", what);
    const TileGeom g = {F, H, W, TH, TW, C, px};
    hipStream_t st = (hipStream_t)stream;
    if (!frames) mean = stdv = nullptr;
    if (frames && dtype == SQ_PIX_U16)
        return sample_launch<uint16_t>(frames, mean, stdv, labels, weights, plan, coef, out_image, out_onehot, out_weights, g,
                                       py, count, st);
    if (frames && dtype == SQ_PIX_F32)
        return sample_launch<float>(frames, mean, stdv, labels, weights, plan, coef, out_image, out_onehot, out_weights, g, py,
                                    count, st);
    return sample_launch<uint8_t>(frames, mean, stdv, labels, weights, plan, coef, out_image, out_onehot, out_weights, g, py,
                                  count, st);
}
