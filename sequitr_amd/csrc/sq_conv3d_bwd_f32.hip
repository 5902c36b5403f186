// Backward of the volumetric (3-D) f32 operators of UNet3D for gfx950 (forward: sq_conv3d_f32.hip).  Tensors are NDHWC.
//
//   * the weight (and bias) gradient of the 3x3x3 SAME convolution, sq_conv3d_ndhwc_wgrad_f32, is the DT = 3 form of the
//     planar weight-gradient kernels and lives with them in sq_conv_wgrad_f32.hip.
//   * sq_conv3d_weight_transform_f32: the filter of the input gradient, which is the FORWARD conv3d of dY with it.
//   * sq_maxpool2x2x2_bwd_f32, sq_space_to_depth2x2x2_f32: streaming kernels, 16-B loads and stores.
#include "sq_common.h"

namespace {

constexpr int64_t LIM32 = (int64_t)1 << 31;

// ---- streaming kernels ---------------------------------------------------------------------------------------------------
// wt[kd][kh][kw][co][ci] = w[2-kd][2-kh][2-kw][ci][co]
__global__ __launch_bounds__(256) void conv3d_weight_transform_kernel(const float *__restrict__ w, float *__restrict__ wt,
                                                                       int Cin, int Cout) {
    const int total = 27 * Cin * Cout;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int ci = i % Cin, co = (i / Cin) % Cout, tap = i / (Cin * Cout);
    wt[i] = w[((26 - tap) * Cin + ci) * Cout + co];             // 26 - tap: all three axes reversed
}

// max-pool backward: the gradient goes to the FIRST maximum of the window in (depth, row, column) raster order.
// Thread per (output voxel, channel quad); every element of dx is written.
__global__ __launch_bounds__(256) void maxpool2x2x2_bwd_kernel(const float4 *__restrict__ x, const float4 *__restrict__ dy,
                                                                float4 *__restrict__ dx, int D, int H, int W, int C4,
                                                                int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int q = (int)(i % C4);
    int64_t p = i / C4;
    const int wo = (int)(p % (W / 2)); p /= (W / 2);
    const int ho = (int)(p % (H / 2)); p /= (H / 2);
    const int dout = (int)(p % (D / 2));
    const int64_t n = p / (D / 2);
    float4 v[8];
    int64_t at[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int dz = k >> 2, dr = (k >> 1) & 1, dc = k & 1;
        at[k] = (((n * D + 2 * dout + dz) * H + 2 * ho + dr) * (int64_t)W + 2 * wo + dc) * C4 + q;
        v[k] = x[at[k]];
    }
    const float4 g = dy[i];
    int kx = 0, ky = 0, kz = 0, kw = 0;
    float mx = v[0].x, my = v[0].y, mz = v[0].z, mw = v[0].w;
#pragma unroll
    for (int k = 1; k < 8; ++k) {
        if (v[k].x > mx) { mx = v[k].x; kx = k; }
        if (v[k].y > my) { my = v[k].y; ky = k; }
        if (v[k].z > mz) { mz = v[k].z; kz = k; }
        if (v[k].w > mw) { mw = v[k].w; kw = k; }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k)
        dx[at[k]] = make_float4(kx == k ? g.x : 0.f, ky == k ? g.y : 0.f, kz == k ? g.z : 0.f, kw == k ? g.w : 0.f);
}

// g[n,d,i,j, ((2a+b)*2+e)*C + c] = dy[n, 2d+a, 2i+b, 2j+e, c];  D, H, W = the SMALL side
__global__ __launch_bounds__(256) void space_to_depth2x2x2_kernel(const float4 *__restrict__ dy, float4 *__restrict__ g,
                                                                   int D, int H, int W, int C4, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C4);
    int64_t t = i / C4;
    const int abe = (int)(t & 7);
    t >>= 3;
    const int j = (int)(t % W); t /= W;
    const int ii = (int)(t % H); t /= H;
    const int d = (int)(t % D);
    const int64_t n = t / D;
    const int a = abe >> 2, b = (abe >> 1) & 1, e = abe & 1;
    g[i] = dy[(((n * 2 * D + 2 * d + a) * 2 * H + 2 * ii + b) * (int64_t)(2 * W) + 2 * j + e) * C4 + c];
}

unsigned grid1(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" int sq_conv3d_weight_transform_f32(const float *w, float *wt, int Cin, int Cout, void *stream) {
    SQ_REQUIRE(w && wt && Cin > 0 && Cout > 0, "sq_conv3d_weight_transform_f32: bad arguments");
    // the input gradient is the forward conv3d with the channels swapped: it must take Cin := Cout, Cout := Cin
    SQ_REQUIRE((Cout % 16 == 0 || Cout == 1 || Cout == 2) && Cin % 4 == 0,
               "sq_conv3d_weight_transform_f32: Cin=%d Cout=%d: the forward conv3d that evaluates the input gradient needs "
               "Cout in {1,2} or Cout %% 16 == 0, and Cin %% 4 == 0", Cin, Cout);
    SQ_REQUIRE((int64_t)27 * Cin * Cout < LIM32, "sq_conv3d_weight_transform_f32: filter too large");
    hipLaunchKernelGGL(conv3d_weight_transform_kernel, dim3(grid1((int64_t)27 * Cin * Cout)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), w, wt, Cin, Cout);
    return sq_check_launch("sq_conv3d_weight_transform_f32");
}

extern "C" int sq_maxpool2x2x2_bwd_f32(const float *x, const float *dy, float *dx, int N, int D, int H, int W, int C,
                                       void *stream) {
    SQ_REQUIRE(x && dy && dx, "sq_maxpool2x2x2_bwd_f32: null tensor pointer");
    SQ_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0 && C > 0 && D % 2 == 0 && H % 2 == 0 && W % 2 == 0 && C % 4 == 0,
               "sq_maxpool2x2x2_bwd_f32: need even D,H,W and C %% 4 == 0 (got %d,%d,%d,%d)", D, H, W, C);
    SQ_REQUIRE_ALIGNED(x); SQ_REQUIRE_ALIGNED(dy); SQ_REQUIRE_ALIGNED(dx);
    const int64_t total = (int64_t)N * (D / 2) * (H / 2) * (W / 2) * (C / 4);
    SQ_REQUIRE((total + 255) / 256 < LIM32, "sq_maxpool2x2x2_bwd_f32: volume too large");
    hipLaunchKernelGGL(maxpool2x2x2_bwd_kernel, dim3(grid1(total)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const float4 *>(x), reinterpret_cast<const float4 *>(dy),
                       reinterpret_cast<float4 *>(dx), D, H, W, C / 4, total);
    return sq_check_launch("sq_maxpool2x2x2_bwd_f32");
}

extern "C" int sq_space_to_depth2x2x2_f32(const float *dy, float *g, int N, int D, int H, int W, int C, void *stream) {
    SQ_REQUIRE(dy && g, "sq_space_to_depth2x2x2_f32: null tensor pointer");
    SQ_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "sq_space_to_depth2x2x2_f32: C %% 4 == 0");
    SQ_REQUIRE_ALIGNED(dy); SQ_REQUIRE_ALIGNED(g);
    const int64_t total = (int64_t)N * D * H * W * 8 * (C / 4);
    SQ_REQUIRE((total + 255) / 256 < LIM32, "sq_space_to_depth2x2x2_f32: volume too large");
    hipLaunchKernelGGL(space_to_depth2x2x2_kernel, dim3(grid1(total)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const float4 *>(dy), reinterpret_cast<float4 *>(g), D, H, W, C / 4, total);
    return sq_check_launch("sq_space_to_depth2x2x2_f32");
}
