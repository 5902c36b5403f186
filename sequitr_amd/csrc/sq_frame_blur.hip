// ImageBlur on the GPU (sequitr/pipeline.py:244-263): scipy's gaussian_filter(image, sigma) of a whole raw frame, bit for
// bit, in one launch (include/sequitr_hip.h "Frame cleaning").
//
// A block owns a BT_H x TW pixel tile.  It stages the tile with a halo of R on all four sides in LDS as float32, the
// reflection applied while staging (any number of reflections: a frame may be far smaller than R), runs the pass along
// axis 0 into a second LDS array as float32 -- the definition's intermediate rounding; nothing goes through global
// memory -- and then the pass along axis 1, and writes four neighbouring pixels of a row with one 16-byte store where the
// rows of `out` are aligned.  Both passes add their taps in float64 in scipy's order k = R .. 1 with contraction off: the
// add, the multiply and the add are three roundings.
//
// In both passes a lane produces four neighbouring outputs along the filtered axis from one window of 2 R + 4 values, so a
// value is read from LDS and widened to float64 once for the four: four rows of one column in the first pass (the lanes
// of a wave at consecutive columns), four pixels of one row in the second (ds_read_b128, the lanes at consecutive 16-byte
// slots).
//
// The kernel is a template of the radius, one instance for each R = 0 .. 32: the tap loops are straight-line code, every
// register index is static and the weights sit in scalar registers.  The radius classes are the tile's three widths,
// chosen so that the halo stays in proportion and two blocks or more fit a CU's LDS:
//   R =  0 ..  8 : tile 32 x 128, LDS 32.0 .. 45.0 KB
//   R =  9 .. 16 : tile 32 x  96, LDS 37.2 .. 48.0 KB
//   R = 17 .. 32 : tile 32 x  64, LDS 38.3 .. 64.0 KB
#include <utility>

#include "sq_common.h"

namespace {

constexpr int BT_H = 32, BLUR_MAX_R = 32;

struct BlurWeights { double w[BLUR_MAX_R + 1]; };               // w[0] the centre; by value in the kernel arguments

// tile pixel (y, x) lies at row y + R, column x + R of the staged array and at row y, column x + R of the intermediate one
template <int R> struct BlurGeom {
    static constexpr int TW = R > 16 ? 64 : (R > 8 ? 96 : 128);
    static constexpr int NWIN = 2 * R + 4, NWIN4 = (NWIN + 3) & ~3;   // a window; in whole 16-byte slots (two floats more, R odd)
    static constexpr int PITCH = (TW + 2 * R + 3) & ~3;         // a window's slots stay inside the row for the last quad too
};

// scipy's mode='reflect' (the edge pixel repeated), repeated until the index is inside; L == 1 gives 0
__device__ __forceinline__ int reflect_full(int i, int L) {
    while (i < 0 || i >= L) i = i < 0 ? -i - 1 : 2 * L - 1 - i;
    return i;
}

// rows 0 .. ph - 1, columns 0 .. pw - 1 of the staged array: the frame at (y0 - R + r, x0 - R + c), reflected.  A lane
// has SB loads in flight, then writes the SB values.
template <typename T>
__device__ __forceinline__ void blur_stage(const T *__restrict__ src, float *__restrict__ stage, int pitch, int y0, int x0,
                                           int R, int ph, int pw, int H, int W) {
    constexpr int SB = 8;
    const int dq = 256 / pw, dr = 256 % pw;                     // a step of 256 elements in (row, column) of a pw-wide box
    int r = (int)threadIdx.x / pw, c = (int)threadIdx.x % pw;
    while (r < ph) {
        T v[SB];
        int at[SB];
#pragma unroll
        for (int u = 0; u < SB; ++u) {
            const int rr = min(r, ph - 1);                      // past the end: a valid address, read and dropped
            at[u] = r < ph ? r * pitch + c : -1;
            v[u] = src[(size_t)reflect_full(y0 - R + rr, H) * W + reflect_full(x0 - R + c, W)];
            r += dq;
            c += dr;
            if (c >= pw) { c -= pw; ++r; }
        }
#pragma unroll
        for (int u = 0; u < SB; ++u)
            if (at[u] >= 0) stage[at[u]] = (float)v[u];
    }
}

// four neighbouring outputs of one pass: output p sits at win[R + p], its taps at win[R + p -+ k]
template <int R, int N>
__device__ __forceinline__ void blur_taps4(const float (&win)[N], const BlurWeights &wt, float (&res)[4]) {
#pragma clang fp contract(off)
    double d[2 * R + 4];
#pragma unroll
    for (int i = 0; i < 2 * R + 4; ++i) d[i] = (double)win[i];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        double acc = d[R + p] * wt.w[0];
#pragma unroll
        for (int k = R; k >= 1; --k) acc = acc + (d[R + p - k] + d[R + p + k]) * wt.w[k];
        res[p] = (float)acc;
    }
}

template <int R>
__global__ __launch_bounds__(256, 2) void blur_kernel(const void *__restrict__ frames, int dtype, float *__restrict__ out,
                                                   BlurWeights wt, int H, int W, int tiles_x, int vec_store) {
    using G = BlurGeom<R>;
    constexpr int TW = G::TW, PITCH = G::PITCH, QROW = TW / 4;
    __shared__ __attribute__((aligned(16))) float stage[(BT_H + 2 * R) * PITCH];
    __shared__ __attribute__((aligned(16))) float mid[BT_H * PITCH];
    const int tid = threadIdx.x;
    const int x0 = (int)(blockIdx.x % (unsigned)tiles_x) * TW, y0 = (int)(blockIdx.x / (unsigned)tiles_x) * BT_H;
    const int th = min(BT_H, H - y0), tw = min(TW, W - x0);     // the part of the tile inside the frame
    const int pw = tw + 2 * R, ph = th + 2 * R;
    const size_t fbase = (size_t)blockIdx.y * H * W;
    if (dtype == SQ_PIX_U8) blur_stage(reinterpret_cast<const uint8_t *>(frames) + fbase, stage, PITCH, y0, x0, R, ph, pw, H, W);
    else if (dtype == SQ_PIX_U16) blur_stage(reinterpret_cast<const uint16_t *>(frames) + fbase, stage, PITCH, y0, x0, R, ph, pw, H, W);
    else blur_stage(reinterpret_cast<const float *>(frames) + fbase, stage, PITCH, y0, x0, R, ph, pw, H, W);
    __syncthreads();

    // axis 0: rows 4 yq .. 4 yq + 3 of staged column c; win[i] = stage[4 yq + i][c]
    {
        const int dq = 256 / pw, dr = 256 % pw;
        int yq = tid / pw, c = tid % pw;
        while (4 * yq < th) {
            const float *__restrict__ s = &stage[4 * yq * PITCH + c];
            float win[G::NWIN], res[4];
#pragma unroll
            for (int i = 0; i < G::NWIN; ++i) win[i] = s[i * PITCH];
            blur_taps4<R>(win, wt, res);
#pragma unroll
            for (int p = 0; p < 4; ++p) mid[(4 * yq + p) * PITCH + c] = res[p];
            yq += dq;
            c += dr;
            if (c >= pw) { c -= pw; ++yq; }
        }
    }
    __syncthreads();

    // axis 1: quad j of row y is the pixels 4j .. 4j+3; win[i] = mid[y][4j + i]
#pragma unroll 1
    for (int q = tid; q < th * QROW; q += 256) {
        const int y = q / QROW, xl = 4 * (q % QROW);
        if (xl >= tw) continue;
        float win[G::NWIN4], res[4];
#pragma unroll
        for (int v = 0; v < G::NWIN4 / 4; ++v) {
            const f32x4 t = *reinterpret_cast<const f32x4 *>(&mid[y * PITCH + xl + 4 * v]);
            win[4 * v + 0] = t.x; win[4 * v + 1] = t.y; win[4 * v + 2] = t.z; win[4 * v + 3] = t.w;
        }
        blur_taps4<R>(win, wt, res);
        const int x = x0 + xl;
        float *__restrict__ dst = out + fbase + (size_t)(y0 + y) * W + x;
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

using BlurLaunch = void (*)(const void *, int, float *, const BlurWeights &, int, int, int, hipStream_t);

template <int R>
void blur_launch(const void *frames, int dtype, float *out, const BlurWeights &wt, int F, int H, int W, hipStream_t st) {
    constexpr int TW = BlurGeom<R>::TW;
    const int tx = (W + TW - 1) / TW, ty = (H + BT_H - 1) / BT_H;   // tx * ty <= 2^24 / 32 + H + W: far inside a grid's x
    const int vec = (W % 4 == 0) && SQ_ALIGNED16(out);          // every row of every frame then starts on 16 bytes
    hipLaunchKernelGGL(blur_kernel<R>, dim3((unsigned)(tx * ty), F), dim3(256), 0, st, frames, dtype, out, wt, H, W, tx, vec);
}

template <int... Rs>
BlurLaunch blur_launcher(int radius, std::integer_sequence<int, Rs...>) {
    static const BlurLaunch table[] = {&blur_launch<Rs>...};
    return table[radius];
}

}  // namespace

extern "C" int sq_frame_blur_f32(const void *frames, int dtype, float *out, const double *weights, int radius, int F, int H,
                                 int W, void *stream) {
    SQ_REQUIRE(frames && out && weights, "sq_frame_blur_f32: null pointer");
    SQ_REQUIRE(radius >= 0 && radius <= BLUR_MAX_R, "sq_frame_blur_f32: radius %d is not 0 .. %d (sigma < 8.125)", radius,
               BLUR_MAX_R);
    SQ_REQUIRE(F > 0 && F <= 65535 && H >= 1 && W >= 1 && (int64_t)H * W <= (1 << 24),
               "sq_frame_blur_f32: need 1 .. 65535 frames, H, W >= 1 and H*W <= 2^24, got %d of %d x %d", F, H, W);
    SQ_REQUIRE(dtype == SQ_PIX_U8 || dtype == SQ_PIX_U16 || dtype == SQ_PIX_F32, "sq_frame_blur_f32: unknown pixel type %d",
               dtype);
    BlurWeights wt;
    for (int k = 0; k <= BLUR_MAX_R; ++k) {
        wt.w[k] = k <= radius ? weights[k] : 0.0;
        SQ_REQUIRE(wt.w[k] - wt.w[k] == 0.0, "sq_frame_blur_f32: weight %d is not finite", k);
    }
    blur_launcher(radius, std::make_integer_sequence<int, BLUR_MAX_R + 1>())(frames, dtype, out, wt, F, H, W,
                                                                             (hipStream_t)stream);
    return sq_check_launch("sq_frame_blur_f32");
}
