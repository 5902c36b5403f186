// GAN sampler: the progressive GAN's real images cut out of raw image stacks that stay in HBM (include/sequitr_hip.h
// "GAN sampler"; the reference's input pipeline, sequitr/networks/gan.py:347-407 and :682-684: every image normalised per
// channel by its own moments, a random crop, two random mirrors, a bilinear resize with align_corners=True to the current
// level's size).  Images are (N, H, W, C) with the channels interleaved.
//
// Statistics, once per stack: S1 = sum v and S2 = sum v^2 per (image, channel) as exact 64-bit integers -- integer adds in
// registers, across lanes, across waves and, one per block, as integer atomics, so that no order of arrival changes a bit --
// then a finishing kernel in float64, contraction off:
//
//     mean = S1 / n;   var = max(S2 / n - mean * mean, 0);   inv = 1 / sqrt(var + 1e-8);   stored as float32
//
// A sample is one row plan[k] = [n, oy, ox, bits]; the definition (the header's and tests/gan_sampler_cases.py's, word for
// word), for output pixel (i, j) and channel c of sample k, crop (CH, CW), output (SH, SW):
//
//     sy = SH > 1 ? float32(CH-1) / float32(SH-1) : 0.0f                              (sx likewise from CW, SW)
//     py = float32(i) * sy;  y0 = floor(py);  y1 = min(ceil(py), CH-1);  ly = py - y0  (x likewise)
//     crop(r, q) = src(oy + (bits&2 ? CH-1-r : r), ox + (bits&1 ? CW-1-q : q))
//     src(Y, X)  = (float32(v[n,Y,X,c]) - mean[n,c]) * inv[n,c]   if 0<=n<N, 0<=Y<H, 0<=X<W   else 0.0f
//     top = tl + (tr - tl) * lx;  bot = bl + (br - bl) * lx;  out = top + (bot - top) * ly
//
// every *, + and - rounded on its own in float32.  sy and sx are one IEEE division each, done on the host.
//
// One thread per output pixel over the flat (k, i, j) index, so that a level-0 batch (32 samples of 4 x 4) is two blocks and
// not 32 near-empty ones.  A thread reads the C channels of a corner in one load (C = 1, 2, 4; three element loads for
// C = 3) and writes its C floats in one store; consecutive lanes write consecutive pixels.  The four corners are guarded
// gathers: the plan is data, and no load leaves the stack.  Nothing here is matrix work; the kernel is launch- and
// gather-bound.
#include <algorithm>
#include "sq_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int STAT_PIXELS = 4096;                               // pixels a statistics block takes before a second one is worth it
constexpr int STAT_BLOCKS = 64;                                 // most blocks per image

// the C channels of one pixel: one load where C elements make a power-of-two vector
template <typename T, int C>
__device__ __forceinline__ void load_pixel(const T *__restrict__ p, T (&v)[C]) {
    if constexpr (C == 1) {
        v[0] = p[0];
    } else if constexpr (C == 3) {
        v[0] = p[0], v[1] = p[1], v[2] = p[2];
    } else {
        typedef T V __attribute__((ext_vector_type(C)));
        const V q = *reinterpret_cast<const V *>(p);
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = q[c];
    }
}

template <int C>
__device__ __forceinline__ void store_pixel(float *__restrict__ p, const float (&v)[C]) {
    if constexpr (C == 1) {
        p[0] = v[0];
    } else if constexpr (C == 3) {
        p[0] = v[0], p[1] = v[1], p[2] = v[2];
    } else {
        typedef float V __attribute__((ext_vector_type(C)));
        V q;
#pragma unroll
        for (int c = 0; c < C; ++c) q[c] = v[c];
        *reinterpret_cast<V *>(p) = q;
    }
}

// ---- statistics ---------------------------------------------------------------------------------------------------------

// grid (N * bpi), block THREADS: block b of image n strides over that image's pixels; sums[(n*C + c)*2 + {0, 1}] += S1, S2
template <typename T, int C>
__global__ __launch_bounds__(THREADS) void gan_sums_kernel(const T *__restrict__ images, unsigned long long *__restrict__ sums,
                                                           int npix, int bpi) {
    __shared__ unsigned long long part[THREADS / 64][2 * C];
    const unsigned n = blockIdx.x / (unsigned)bpi, b = blockIdx.x % (unsigned)bpi;
    const T *img = images + (size_t)n * npix * C;
    unsigned long long acc[2 * C];
#pragma unroll
    for (int c = 0; c < 2 * C; ++c) acc[c] = 0;
    for (int p = (int)b * THREADS + (int)threadIdx.x; p < npix; p += bpi * THREADS) {
        T v[C];
        load_pixel<T, C>(img + (size_t)p * C, v);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const unsigned u = (unsigned)v[c];                  // at most 65535: u * u fits 32 bits
            acc[2 * c] += u;
            acc[2 * c + 1] += u * u;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < 2 * C; ++c) {
        unsigned long long s = acc[c];
        for (int m = 32; m > 0; m >>= 1) s += __shfl_down(s, m);
        if (lane == 0) part[wave][c] = s;
    }
    __syncthreads();
    if (threadIdx.x < 2 * C) {
        unsigned long long s = 0;
#pragma unroll
        for (int w = 0; w < THREADS / 64; ++w) s += part[w][threadIdx.x];
        atomicAdd(&sums[(size_t)n * 2 * C + threadIdx.x], s);   // integer: the order of arrival changes nothing
    }
}

// one thread per (image, channel)
__global__ __launch_bounds__(THREADS) void gan_stats_finish_kernel(const unsigned long long *__restrict__ sums,
                                                                   float *__restrict__ mean, float *__restrict__ inv, int nc,
                                                                   double npix) {
#pragma clang fp contract(off)
    const int t = (int)(blockIdx.x * THREADS + threadIdx.x);
    if (t >= nc) return;
    const double s1 = (double)sums[2 * (size_t)t], s2 = (double)sums[2 * (size_t)t + 1];
    const double m = s1 / npix, q = s2 / npix;
    const double mm = m * m;
    double var = q - mm;
    var = var > 0.0 ? var : 0.0;                                // a nearly constant uint16 image can round the difference below 0
    const double r = 1.0 / sqrt(var + 1e-8);
    mean[t] = (float)m;
    inv[t] = (float)r;
}

template <typename T, int C>
int stats_launch(const void *images, unsigned long long *sums, int N, int npix, hipStream_t st) {
    const int bpi = std::min(std::max((npix + STAT_PIXELS - 1) / STAT_PIXELS, 1), STAT_BLOCKS);
    hipLaunchKernelGGL((gan_sums_kernel<T, C>), dim3((unsigned)((int64_t)N * bpi)), dim3(THREADS), 0, st,
                       reinterpret_cast<const T *>(images), sums, npix, bpi);
    return sq_check_launch("sq_gan_image_stats");
}

template <typename T>
int stats_channels(const void *images, unsigned long long *sums, int N, int npix, int C, hipStream_t st) {
    switch (C) {
    case 1: return stats_launch<T, 1>(images, sums, N, npix, st);
    case 2: return stats_launch<T, 2>(images, sums, N, npix, st);
    case 3: return stats_launch<T, 3>(images, sums, N, npix, st);
    default: return stats_launch<T, 4>(images, sums, N, npix, st);
    }
}

// ---- sampling -----------------------------------------------------------------------------------------------------------

struct GanGeom {
    int N, H, W, CH, CW, SH, SW;
    unsigned total;                                             // count * SH * SW output pixels, below 2^31
    float sy, sx;
};

// grid ceil(total / THREADS), block THREADS: thread t is output pixel (k, i, j) = unravel(t, (count, SH, SW))
template <typename T, int C>
__global__ __launch_bounds__(THREADS) void gan_sample_kernel(const T *__restrict__ images, const float *__restrict__ mean,
                                                             const float *__restrict__ inv, const int *__restrict__ plan,
                                                             float *__restrict__ out, GanGeom g) {
#pragma clang fp contract(off)
    const unsigned t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= g.total) return;
    const unsigned per = (unsigned)g.SH * (unsigned)g.SW;
    const unsigned k = t / per, rem = t % per;
    const int i = (int)(rem / (unsigned)g.SW), j = (int)(rem % (unsigned)g.SW);
    const int *row = plan + (size_t)k * 4;
    const int n = row[0], bits = row[3];
    const long long oy = row[1], ox = row[2];

    const float py = (float)i * g.sy, px = (float)j * g.sx;
    const float fy0 = floorf(py), fx0 = floorf(px);
    const float fy1 = fminf(ceilf(py), (float)(g.CH - 1)), fx1 = fminf(ceilf(px), (float)(g.CW - 1));
    const float ly = py - fy0, lx = px - fx0;
    const int r0 = (int)fy0, r1 = (int)fy1, q0 = (int)fx0, q1 = (int)fx1;
    const long long Y0 = oy + ((bits & 2) ? g.CH - 1 - r0 : r0), Y1 = oy + ((bits & 2) ? g.CH - 1 - r1 : r1);
    const long long X0 = ox + ((bits & 1) ? g.CW - 1 - q0 : q0), X1 = ox + ((bits & 1) ? g.CW - 1 - q1 : q1);

    const bool nok = (unsigned)n < (unsigned)g.N;
    const bool y0ok = nok && (unsigned long long)Y0 < (unsigned long long)g.H;
    const bool y1ok = nok && (unsigned long long)Y1 < (unsigned long long)g.H;
    const bool x0ok = (unsigned long long)X0 < (unsigned long long)g.W, x1ok = (unsigned long long)X1 < (unsigned long long)g.W;
    const bool norm = mean != nullptr;
    float m[C], s[C];
#pragma unroll
    for (int c = 0; c < C; ++c) m[c] = 0.f, s[c] = 1.f;
    if (norm && nok) {
        load_pixel<float, C>(mean + (size_t)n * C, m);
        load_pixel<float, C>(inv + (size_t)n * C, s);
    }
    const size_t base = nok ? (size_t)n * g.H * g.W : 0;        // every address below stays inside the stack
    const size_t ra = base + (size_t)(y0ok ? Y0 : 0) * g.W, rb = base + (size_t)(y1ok ? Y1 : 0) * g.W;
    const size_t ca = (size_t)(x0ok ? X0 : 0), cb = (size_t)(x1ok ? X1 : 0);
    T tl[C], tr[C], bl[C], br[C];
    load_pixel<T, C>(images + (ra + ca) * C, tl);
    load_pixel<T, C>(images + (ra + cb) * C, tr);
    load_pixel<T, C>(images + (rb + ca) * C, bl);
    load_pixel<T, C>(images + (rb + cb) * C, br);
    const bool k00 = y0ok && x0ok, k01 = y0ok && x1ok, k10 = y1ok && x0ok, k11 = y1ok && x1ok;
    float o[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float a = (float)tl[c], b = (float)tr[c], d = (float)bl[c], e = (float)br[c];
        const float v00 = k00 ? (norm ? (a - m[c]) * s[c] : a) : 0.f;
        const float v01 = k01 ? (norm ? (b - m[c]) * s[c] : b) : 0.f;
        const float v10 = k10 ? (norm ? (d - m[c]) * s[c] : d) : 0.f;
        const float v11 = k11 ? (norm ? (e - m[c]) * s[c] : e) : 0.f;
        const float dt = v01 - v00, db = v11 - v10;
        const float pt = dt * lx, pb = db * lx;
        const float top = v00 + pt, bot = v10 + pb;
        const float dv = bot - top;
        const float pv = dv * ly;
        o[c] = top + pv;
    }
    store_pixel<C>(out + (size_t)t * C, o);
}

template <typename T, int C>
int sample_launch(const void *images, const float *mean, const float *inv, const int32_t *plan, float *out, const GanGeom &g,
                  hipStream_t st) {
    const unsigned blocks = (g.total + THREADS - 1) / THREADS;
    hipLaunchKernelGGL((gan_sample_kernel<T, C>), dim3(blocks), dim3(THREADS), 0, st, reinterpret_cast<const T *>(images), mean,
                       inv, plan, out, g);
    return sq_check_launch("sq_gan_sample_f32");
}

template <typename T>
int sample_channels(const void *images, const float *mean, const float *inv, const int32_t *plan, float *out, int C,
                    const GanGeom &g, hipStream_t st) {
    switch (C) {
    case 1: return sample_launch<T, 1>(images, mean, inv, plan, out, g, st);
    case 2: return sample_launch<T, 2>(images, mean, inv, plan, out, g, st);
    case 3: return sample_launch<T, 3>(images, mean, inv, plan, out, g, st);
    default: return sample_launch<T, 4>(images, mean, inv, plan, out, g, st);
    }
}

// bytes a pixel's single load or store needs to be aligned to: the whole pixel where C elements make a vector
inline size_t pixel_align(size_t elem, int C) { return C == 3 ? elem : elem * (size_t)C; }

}  // namespace

extern "C" int64_t sq_gan_image_stats_workspace(int N, int C) {
    if (N <= 0 || C < 1 || C > 4) return 0;
    return (int64_t)N * C * 2 * (int64_t)sizeof(unsigned long long);
}

extern "C" int sq_gan_image_stats(const void *images, int dtype, float *mean, float *inv, void *workspace, int N, int H, int W,
                                  int C, void *stream) {
    const char *what = "sq_gan_image_stats";
    SQ_REQUIRE(images && mean && inv && workspace, "%s: null pointer", what);
    SQ_REQUIRE(dtype == SQ_PIX_U8 || dtype == SQ_PIX_U16, "%s: pixel type %d is not SQ_PIX_U8 or SQ_PIX_U16 (the sums are integers)",
               what, dtype);
    SQ_REQUIRE(C >= 1 && C <= 4, "%s: %d channels not in 1 .. 4", what, C);
    SQ_REQUIRE(N > 0 && H > 0 && W > 0, "%s: sizes must be positive", what);
    SQ_REQUIRE((int64_t)H * W <= (1 << 24), "%s: images of %d x %d exceed 2^24 pixels", what, H, W);
    SQ_REQUIRE((int64_t)N * STAT_BLOCKS <= 0x7fffffff, "%s: %d images are too many for one launch", what, N);
    const size_t elem = dtype == SQ_PIX_U8 ? 1 : 2;
    SQ_REQUIRE((uintptr_t)images % pixel_align(elem, C) == 0, "%s: images must be aligned to a pixel's load (%d bytes)", what,
               (int)pixel_align(elem, C));
    SQ_REQUIRE(((uintptr_t)mean | (uintptr_t)inv) % 4 == 0 && (uintptr_t)workspace % 8 == 0,
               "%s: mean and inv must be aligned to 4 bytes, the workspace to 8", what);
    hipStream_t st = (hipStream_t)stream;
    unsigned long long *sums = reinterpret_cast<unsigned long long *>(workspace);
    const hipError_t e = hipMemsetAsync(sums, 0, (size_t)sq_gan_image_stats_workspace(N, C), st);
    if (e != hipSuccess) {
        sq_set_error("%s: clearing the workspace failed: %s", what, hipGetErrorString(e));
        return SQ_ELAUNCH;
    }
    const int rc = dtype == SQ_PIX_U8 ? stats_channels<uint8_t>(images, sums, N, H * W, C, st)
                                      : stats_channels<uint16_t>(images, sums, N, H * W, C, st);
    if (rc != SQ_OK) return rc;
    const int nc = N * C;
    hipLaunchKernelGGL(gan_stats_finish_kernel, dim3((unsigned)((nc + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, sums, mean,
                       inv, nc, (double)((int64_t)H * W));
    return sq_check_launch(what);
}

extern "C" int sq_gan_sample_f32(const void *images, int dtype, const float *mean, const float *inv, const int32_t *plan,
                                 float *out, int N, int H, int W, int C, int CH, int CW, int SH, int SW, int count,
                                 void *stream) {
    const char *what = "sq_gan_sample_f32";
    SQ_REQUIRE(images && plan && out, "%s: null pointer (images, plan, out)", what);
    SQ_REQUIRE((mean == nullptr) == (inv == nullptr), "%s: null pointer: give both mean and inv, or neither", what);
    SQ_REQUIRE(dtype == SQ_PIX_U8 || dtype == SQ_PIX_U16 || dtype == SQ_PIX_F32, "%s: unknown pixel type %d", what, dtype);
    SQ_REQUIRE(C >= 1 && C <= 4, "%s: %d channels not in 1 .. 4", what, C);
    SQ_REQUIRE(count > 0 && count <= 65535, "%s: count %d not in 1 .. 65535", what, count);
    SQ_REQUIRE(N > 0 && H > 0 && W > 0 && CH > 0 && CW > 0 && SH > 0 && SW > 0, "%s: sizes must be positive", what);
    SQ_REQUIRE((int64_t)H * W <= (1 << 24), "%s: images of %d x %d exceed 2^24 pixels", what, H, W);
    SQ_REQUIRE(CH <= (1 << 24) && CW <= (1 << 24) && (int64_t)SH * SW <= (1 << 24),
               "%s: crop %d x %d or output %d x %d out of range (2^24 per crop axis, 2^24 output pixels)", what, CH, CW, SH, SW);
    SQ_REQUIRE((int64_t)N * H * W * C <= ((int64_t)1 << 46), "%s: a stack of %d images is out of range", what, N);
    const size_t elem = dtype == SQ_PIX_U8 ? 1 : dtype == SQ_PIX_U16 ? 2 : 4;
    SQ_REQUIRE((uintptr_t)images % pixel_align(elem, C) == 0 && (uintptr_t)out % pixel_align(4, C) == 0,
               "%s: images and out must be aligned to a pixel's load and store (%d and %d bytes)", what,
               (int)pixel_align(elem, C), (int)pixel_align(4, C));
    SQ_REQUIRE(((uintptr_t)mean | (uintptr_t)inv) % pixel_align(4, C) == 0 && (uintptr_t)plan % 4 == 0,
               "%s: mean and inv must be aligned to %d bytes, plan to 4", what, (int)pixel_align(4, C));
    SQ_REQUIRE((int64_t)count * SH * SW <= 0x7fffffff, "%s: %d samples of %d x %d are more than 2^31 - 1 output pixels", what, count,
               SH, SW);
    GanGeom g = {N, H, W, CH, CW, SH, SW, (unsigned)((int64_t)count * SH * SW), 0.f, 0.f};
    g.sy = SH > 1 ? (float)(CH - 1) / (float)(SH - 1) : 0.f;    // one IEEE division each, here on the host
    g.sx = SW > 1 ? (float)(CW - 1) / (float)(SW - 1) : 0.f;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == SQ_PIX_U16) return sample_channels<uint16_t>(images, mean, inv, plan, out, C, g, st);
    if (dtype == SQ_PIX_F32) return sample_channels<float>(images, mean, inv, plan, out, C, g, st);
    return sample_channels<uint8_t>(images, mean, inv, plan, out, C, g, st);
}
