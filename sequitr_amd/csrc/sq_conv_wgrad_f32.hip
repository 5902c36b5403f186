// Weight gradient of the KxK SAME convolution (conv_layer / weighted_conv2d backward) on
// v_mfma_f32_16x16x4_f32, gfx950.
//
//   dW[tap][ci][co] = sum over pixels p of  X[p + tap][ci] * dY[p][co]
//   db[co]          = sum over pixels p of  dY[p][co]
//
// GEMM view per (16-channel ci chunk, BN-channel co chunk) pair: D[i = ci][j = co], reduction
// over PIXELS (4 per MFMA: A[i][k] = X[pixel k][ci i], B[k][j] = dY[pixel k][co j]), one
// accumulator block per tap.  Blocks are persistent over 16x16 pixel tiles and keep their
// K*K*NR accumulator blocks in registers across all their tiles; the next tile's X halo and
// dY tile are prefetched into registers during the MFMA phase (as in sq_conv_f32_v2.hip).
// The reduction over the 4.2M pixels of a level-0 batch is split across blocks and finished
// by a second kernel that adds the block partials IN A FIXED ORDER: no float atomics, results
// are run-to-run reproducible (MI355X_MICROARCH.md "Global float atomics").
//
// One kernel family serves the planar (NHWC) and the volumetric (NDHWC, 3x3x3 SAME) convolution: every kernel takes the
// number of depth taps DT at compile time (1 = planar, 3 = volumetric).  The volumetric gradient
//   dW[kd][kh][kw][ci][co] = sum over voxels p of X[p + (kd-1, kh-1, kw-1)][ci] * dY[p][co],  db[co] = sum_p dY[p][co]
// is the planar one of the depth-stacked input xs[n,d,h,w, kd*Cin + c] = x[n, d+kd-1, h, w, c] over the N*D planar
// images; xs is never built.  At DT = 3
//   - the MFMA kernel's pair is (depth tap kd, ci chunk, co chunk): the X halo of the tile at output slice nd = n*D + d
//     is read from slice nd + kd - 1, or is all zeros when d + kd - 1 leaves [0, D) -- the tap never reaches into the
//     neighbouring volume of the batch; the dY tile comes from slice nd.  Accumulators and LDS per block are the planar
//     kernel's.  db is taken from the centre depth tap's partials only (every pair sums dY; the centre tap always reads
//     a real slice);
//   - the small-Cin kernel stages DT halo slices and keeps DT*CIN accumulators (Cin 1 and 2 only).
// Every element of dW and db is written: at D == 1 the taps kd = 0 and kd = 2 see only zero halos and come out as exact
// zeros.  Everything under DT is `if constexpr`: the DT = 1 instances compile to what they were without it.
#include "sq_common.h"
#include <stdlib.h>

namespace {

constexpr int TH = 16, TW = 16;
constexpr int64_t LIM32 = (int64_t)1 << 31;

template <int BN, int KS, int KC>
struct WCfg {
    static constexpr int HALO_W = TW + KS - 1;
    static constexpr int HP = HALO_W * (TH + KS - 1);
    static constexpr int PSX = KC;                               // kk*KC + ci: conflict-free for KC = 16
    static constexpr int PSY = (BN % 32 == 0) ? BN + 16 : BN;    // kk*PSY + co: conflict-free
    static constexpr int XS_FLOATS = HP * PSX;
    static constexpr int YS_FLOATS = TH * TW * PSY;
    static constexpr int NTAP = KS * KS;
    static constexpr int NR = BN / 16;
    static constexpr int ROWS = NTAP * 16 + 1;                   // +1: the bias-gradient row
    static constexpr int RED_FLOATS = ROWS * BN;                 // cross-wave reduction image
    static constexpr int LDS_FLOATS = (XS_FLOATS + YS_FLOATS) > RED_FLOATS ? (XS_FLOATS + YS_FLOATS) : RED_FLOATS;
    static constexpr int LDS_BYTES = LDS_FLOATS * 4;
    static constexpr int QPP = KC / 4;
    static constexpr int XITEMS = HP * QPP;
    static constexpr int XSLOTS = (XITEMS + 255) / 256;
    static constexpr int YITEMS = TH * TW * (BN / 4);
    static constexpr int YSLOTS = YITEMS / 256;
    static_assert(YITEMS % 256 == 0, "dY tile must divide evenly over the block");
    static_assert((XS_FLOATS * 4) % 16 == 0, "dY image must start 16-B aligned");
};

// partials layout: [gridDim.x][npairs][ROWS][BN]; pair = (kd * (Cin/KC) + ci chunk) * nco + co chunk = blockIdx.y.
// N counts planar images (N * D at DT = 3, D slices per volume); a tile is (tx, ty, n), walked n-major.
template <int BN, int KS, int KC, int DT>
__global__ __launch_bounds__(256, 2) void conv_wgrad_f32_kernel(
    const float *__restrict__ x, const float *__restrict__ dy, float *__restrict__ partials,
    int N, int H, int W, int Cin, int Cout, int tiles_x, int tiles_y, int ntiles, int tiles_per_block, int D) {
    using C = WCfg<BN, KS, KC>;
    constexpr int NR = C::NR, PAD = KS / 2;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *xs = smem;
    float *ys = smem + C::XS_FLOATS;

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int li = lane & 15, kk = lane >> 4;
    const int nco = (Cout + BN - 1) / BN;
    unsigned pair = blockIdx.y;
    int kd = 0;
    if constexpr (DT > 1) {
        const unsigned per_tap = (Cin / KC) * nco;
        kd = pair / per_tap, pair %= per_tap;
    }
    const int ci0 = (pair / nco) * KC, co0 = (pair % nco) * BN;
    const int t_begin = blockIdx.x * tiles_per_block;
    const int t_end = min(t_begin + tiles_per_block, ntiles);

    // whole tensors are < 2 GiB (the plans refuse anything else): one resource each, 32-bit byte offsets
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(x), 0, (int)((size_t)N * H * W * Cin * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t yrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(dy), 0, (int)((size_t)N * H * W * Cout * 4), 0x00020000);
    constexpr unsigned OOB = 0x80000000u;

    // the per-slot index decode is redone per tile (a few integer ops against 288+ MFMAs) instead of living in
    // ~40 registers next to the accumulators: the <32,3,16> instance spilled 59 VGPRs with the tables
    float4 xr[C::XSLOTS], yr[C::YSLOTS];
    auto issue = [&](int tile) {
        const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, n = tile / (tiles_x * tiles_y);
        const int x0 = tx * TW, y0 = ty * TH;
        // DT > 1: the depth tap reads slice n + kd - DT/2 of the SAME volume, else the depth border's zeros.  The slice
        // index is formed only for a slice that exists: slice N of a tensor just under 2 GiB would overflow the int
        bool depth_ok = true;
        int nx = n;
        if constexpr (DT > 1) {
            depth_ok = (unsigned)(n % D + kd - DT / 2) < (unsigned)D;
            nx = depth_ok ? n + kd - DT / 2 : 0;
        }
        const int xbase = (((nx * H + y0 - PAD) * W + x0 - PAD) * Cin) * 4;
        const int ybase = (((n * H + y0) * W + x0) * Cout) * 4;
#pragma unroll
        for (int sl = 0; sl < C::XSLOTS; ++sl) {
            const int idx = tid + sl * 256;
            const int pix = idx / C::QPP, q = idx % C::QPP;
            const int py = pix / C::HALO_W, px = pix % C::HALO_W;
            const bool inb = depth_ok && idx < C::XITEMS && (unsigned)(y0 - PAD + py) < (unsigned)H &&
                             (unsigned)(x0 - PAD + px) < (unsigned)W;
            const unsigned off = inb ? (unsigned)(xbase + ((py * W + px) * Cin + ci0 + q * 4) * 4) : OOB;
            const auto v = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, off, 0, 0);
            xr[sl] = *reinterpret_cast<const float4 *>(&v);
        }
#pragma unroll
        for (int sl = 0; sl < C::YSLOTS; ++sl) {
            const int idx = tid + sl * 256;
            const int pix = idx / (BN / 4), q = idx % (BN / 4);
            const int py = pix / TW, px = pix % TW;
            const bool inb = (y0 + py) < H && (x0 + px) < W && co0 + q * 4 < Cout;
            const unsigned off = inb ? (unsigned)(ybase + ((py * W + px) * Cout + co0 + q * 4) * 4) : OOB;
            const auto v = __builtin_amdgcn_raw_buffer_load_b128(yrsrc, off, 0, 0);
            yr[sl] = *reinterpret_cast<const float4 *>(&v);
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int sl = 0; sl < C::XSLOTS; ++sl) {
            const int idx = tid + sl * 256;
            if (idx < C::XITEMS)
                *reinterpret_cast<float4 *>(xs + (idx / C::QPP) * C::PSX + (idx % C::QPP) * 4) = xr[sl];
        }
#pragma unroll
        for (int sl = 0; sl < C::YSLOTS; ++sl) {
            const int idx = tid + sl * 256;
            *reinterpret_cast<float4 *>(ys + (idx / (BN / 4)) * C::PSY + (idx % (BN / 4)) * 4) = yr[sl];
        }
    };

    f32x4 acc[C::NTAP][NR];
    float bsum[NR];
#pragma unroll
    for (int t = 0; t < C::NTAP; ++t)
#pragma unroll
        for (int nb = 0; nb < NR; ++nb) acc[t][nb] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int nb = 0; nb < NR; ++nb) bsum[nb] = 0.f;

    // A: X[pixel kk of the group][ci li]; B: dY[pixel kk][co li]
    const float *xa_lds = xs + ((4 * wv) * C::HALO_W + kk) * C::PSX + li;
    const float *yb_lds = ys + ((4 * wv) * TW + kk) * C::PSY + li;

    auto load_frag = [&](int ks, float (&a)[C::NTAP], float (&b)[NR]) {
        const int r = ks >> 2, g = ks & 3;                     // tile row within the wave, 4-pixel group
#pragma unroll
        for (int t = 0; t < C::NTAP; ++t)
            a[t] = xa_lds[((r + t / KS) * C::HALO_W + 4 * g + t % KS) * C::PSX];
#pragma unroll
        for (int nb = 0; nb < NR; ++nb) b[nb] = yb_lds[(r * TW + 4 * g) * C::PSY + nb * 16];
    };

    if (t_begin < t_end) {
        issue(t_begin);
        commit();
    }
    __syncthreads();
    for (int tile = t_begin; tile < t_end; ++tile) {
        const bool has_next = tile + 1 < t_end;
        if (has_next) issue(tile + 1);
        {
            float a0[C::NTAP], b0[NR], a1[C::NTAP], b1[NR];
            load_frag(0, a0, b0);
#pragma unroll
            for (int ks = 0; ks < 16; ks += 2) {
                load_frag(ks + 1, a1, b1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int nb = 0; nb < NR; ++nb) {
                    bsum[nb] += b0[nb];
#pragma unroll
                    for (int t = 0; t < C::NTAP; ++t)
                        acc[t][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[t], b0[nb], acc[t][nb], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
                if (ks + 2 < 16) load_frag(ks + 2, a0, b0);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int nb = 0; nb < NR; ++nb) {
                    bsum[nb] += b1[nb];
#pragma unroll
                    for (int t = 0; t < C::NTAP; ++t)
                        acc[t][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[t], b1[nb], acc[t][nb], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __syncthreads();
        if (has_next) {
            commit();
            __syncthreads();
        }
    }

    // ---- cross-wave reduction in a fixed order (wave 0, 1, 2, 3), then one partial per block ----
    // D layout: lane holds rows (ci) 4*kk+{0..3}, column (co) li of every [tap][nb] block.
    float *red = smem;
#pragma unroll
    for (int nb = 0; nb < NR; ++nb) {       // fold the 4 pixel slots (kk) of the bias sums
        bsum[nb] += __shfl_xor(bsum[nb], 16);
        bsum[nb] += __shfl_xor(bsum[nb], 32);
    }
    for (int w = 0; w < 4; ++w) {
        if (wv == w) {
#pragma unroll
            for (int t = 0; t < C::NTAP; ++t)
#pragma unroll
                for (int nb = 0; nb < NR; ++nb)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float *d = red + (t * 16 + 4 * kk + j) * BN + nb * 16 + li;
                        *d = (w == 0) ? acc[t][nb][j] : *d + acc[t][nb][j];
                    }
            if (kk == 0) {
#pragma unroll
                for (int nb = 0; nb < NR; ++nb) {
                    float *d = red + (C::NTAP * 16) * BN + nb * 16 + li;
                    *d = (w == 0) ? bsum[nb] : *d + bsum[nb];
                }
            }
        }
        __syncthreads();
    }
    float *out = partials + ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * C::RED_FLOATS;
    for (int i = tid; i < C::RED_FLOATS; i += 256) out[i] = red[i];
}

// second stage: dW[kd][tap][ci][co] = sum_b partials[b][pair(kd, ci, co)][tap*16 + ci%KC][co%BN], b ascending, times
// dw_scale (dW only, not db); db[co] from the pairs (centre depth tap, ci chunk 0)
template <int BN, int KS, int KC, int DT>
__global__ __launch_bounds__(256) void conv_wgrad_finish_kernel(const float *__restrict__ partials,
                                                                 float *__restrict__ dw, float *__restrict__ db,
                                                                 int nblk, int Cin, int Cout, int G, float dw_scale) {
    using C = WCfg<BN, KS, KC>;
    const int nco = (Cout + BN - 1) / BN, nci = Cin / KC, npairs = DT * nci * nco;
    const int total = DT * C::NTAP * Cin * Cout;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int i = t / G, g = t % G;
    const size_t stride = (size_t)npairs * C::RED_FLOATS;
    if (i < total) {
        const int co = i % Cout, ci = (i / Cout) % Cin;
        int tap = i / (Cout * Cin), kd = 0;
        if constexpr (DT > 1) kd = tap / C::NTAP, tap %= C::NTAP;
        const int pair = (kd * nci + ci / KC) * nco + co / BN;
        const size_t off = (size_t)pair * C::RED_FLOATS + (tap * 16 + ci % KC) * BN + co % BN;
        const float s = sq_group_reduce(partials + off, stride, nblk, g, G);
        if (g == 0) dw[i] = dw_scale == 1.0f ? s : s * dw_scale;
    } else if (i < total + Cout) {
        const int co = i - total;
        const int pair = (DT / 2) * nci * nco + co / BN;
        const size_t off = (size_t)pair * C::RED_FLOATS + (C::NTAP * 16) * BN + co % BN;
        const float s = sq_group_reduce(partials + off, stride, nblk, g, G);
        if (g == 0 && db) db[co] = s;
    }
}

// N planar images (N * D at DT = 3); `who` names the entry point in a launch error
template <int BN, int KS, int KC, int DT>
int launch(const float *x, const float *dy, float *dw, float *db, float *ws, int N, int D, int H, int W, int Cin,
           int Cout, const int64_t *p, float dw_scale, hipStream_t st, const char *who) {
    using C = WCfg<BN, KS, KC>;
    static bool attr_set = false;
    auto kern = conv_wgrad_f32_kernel<BN, KS, KC, DT>;
    if (!attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                C::LDS_BYTES) != hipSuccess) {
            sq_set_error("%s: cannot reserve %d bytes of LDS", who, C::LDS_BYTES);
            return SQ_ELAUNCH;
        }
        attr_set = true;
    }
    const int gx = (int)p[SQ_WGP_GX], G = (int)p[SQ_WGP_G];
    const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
    hipLaunchKernelGGL(kern, dim3(gx, (unsigned)p[SQ_WGP_NPAIRS]), dim3(256), C::LDS_BYTES, st, x, dy, ws, N, H, W, Cin, Cout,
                       tiles_x, tiles_y, tiles_x * tiles_y * N, (int)p[SQ_WGP_TPB], D);
    int rc = sq_check_launch(who);
    if (rc) return rc;
    const int64_t total = ((int64_t)DT * KS * KS * Cin * Cout + Cout) * G;
    hipLaunchKernelGGL((conv_wgrad_finish_kernel<BN, KS, KC, DT>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                       ws, dw, db, gx, Cin, Cout, G, dw_scale);
    return sq_check_launch(who);
}

int launch_dispatch(const float *x, const float *dy, float *dw, float *db, float *ws, int N, int H, int W,
                    int Cin, int Cout, int K, const int64_t *p, float dw_scale, hipStream_t st) {
    const int KC = (int)p[SQ_WGP_NI], BN = (int)p[SQ_WGP_NO];
#define SQ_W32(BN_, KS_, KC_) if (BN == BN_ && K == KS_ && KC == KC_) return launch<BN_, KS_, KC_, 1>(x, dy, dw, db, ws, N, 1, H, W, Cin, Cout, p, dw_scale, st, "sq_conv2d_nhwc_wgrad_f32");
    SQ_W32(32, 3, 16) SQ_W32(16, 3, 16) SQ_W32(32, 1, 16) SQ_W32(16, 1, 16)
    SQ_W32(32, 3, 8) SQ_W32(16, 3, 8) SQ_W32(32, 1, 8) SQ_W32(16, 1, 8)
#undef SQ_W32
    sq_set_error("sq_conv2d_nhwc_wgrad_f32: no kernel for BN=%d K=%d KC=%d", BN, K, KC);
    return SQ_EINVAL;
}

// ---- first layer (Cin = 1..7, 3x3): the 9 in-plane taps ride the 16 MFMA rows, one accumulator per STACKED channel ----
//   A[i = tap][k = pixel] = X[slice n + kd - DT/2][pixel + tap][c] (rows 9..15 zero), B[k][j = co] = dY[slice n][pixel][co]
// partials: [gridDim.x][9*CS + 1][Cout], CS = DT*CIN stacked channels, row tap*CS + kd*CIN + c (at DT = 1: tap*CIN + c as
// in dW), then the bias row; blockIdx.y = 16-channel co group.  N counts planar images, D slices per volume.
template <typename TY, int CIN, int DT>
__global__ __launch_bounds__(256) void conv_wgrad_cin1_f32_kernel(
    const float *__restrict__ x, const TY *__restrict__ dy, float *__restrict__ partials, int N, int H, int W,
    int Cout, int tiles_x, int tiles_y, int ntiles, int tiles_per_block, int D) {
    constexpr int CS = DT * CIN, HW = TW + 2, HPC = HW * HW * CIN, ROWS = 9 * CS + 1;
    __shared__ float xs[DT * HPC + 8];                         // [kd][halo pixel][c]
    __shared__ __attribute__((aligned(16))) float ys[TH * TW * 16];
    __shared__ float red[4][ROWS * 16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int li = lane & 15, kk = lane >> 4;
    const int co0 = blockIdx.y * 16;
    const int t_begin = blockIdx.x * tiles_per_block, t_end = min(t_begin + tiles_per_block, ntiles);
    const int ky = li / 3, kx = li % 3;
    const bool live_row = li < 9;
    f32x4 acc[CS];
#pragma unroll
    for (int c = 0; c < CS; ++c) acc[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    // register double buffer: the next tile's loads are in flight while this one is multiplied (the kernel used to
    // load, wait, compute, and hid the HBM latency only through resident blocks)
    constexpr int XSL = (DT * HPC + 255) / 256;                 // halo items (one float) per thread
    constexpr int YV = sizeof(TY) == 4 ? 4 : 2;                 // 16-byte pieces of dY per thread: 256 px x 16 ch
    float xr[XSL];
    uint4 yr[YV];
    auto fetch = [&](int tile) {
        const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, n = tile / (tiles_x * tiles_y);
        const int x0 = tx * TW, y0 = ty * TH;
#pragma unroll
        for (int sl = 0; sl < XSL; ++sl) {
            const int idx = tid + sl * 256;
            const int kd = DT == 1 ? 0 : idx / HPC, r = idx - kd * HPC;
            const int pix = r / CIN, c = r % CIN;
            const int gy = y0 - 1 + pix / HW, gx = x0 - 1 + pix % HW;
            bool depth_ok = true;                               // slice n + kd - DT/2 of the same volume, else the
            if constexpr (DT > 1) depth_ok = (unsigned)(n % D + kd - DT / 2) < (unsigned)D;   // depth border's zeros
            xr[sl] = (idx < DT * HPC && depth_ok && gy >= 0 && gy < H && gx >= 0 && gx < W)
                         ? x[(((size_t)(n + kd - DT / 2) * H + gy) * W + gx) * CIN + c] : 0.f;
        }
#pragma unroll
        for (int v = 0; v < YV; ++v) {
            constexpr int PER = 16 / (16 / (int)sizeof(TY));   // 16-byte pieces per pixel: 4 (f32), 2 (bf16)
            constexpr int EL = 16 / (int)sizeof(TY);           // channels per piece
            const int idx = tid + v * 256, pix = idx / PER, q = idx % PER;
            const int gy = y0 + pix / TW, gx = x0 + pix % TW;
            yr[v] = make_uint4(0, 0, 0, 0);
            if (gy < H && gx < W && co0 + q * EL < Cout)        // Cout % 4 == 0; a partial last group (bf16: Cout % 8 == 4)
                yr[v] = (co0 + q * EL + EL <= Cout)             // is read 8 bytes wide
                            ? *reinterpret_cast<const uint4 *>(dy + (((size_t)n * H + gy) * W + gx) * Cout + co0 + q * EL)
                            : make_uint4(reinterpret_cast<const uint2 *>(dy + (((size_t)n * H + gy) * W + gx) * Cout + co0 + q * EL)->x,
                                         reinterpret_cast<const uint2 *>(dy + (((size_t)n * H + gy) * W + gx) * Cout + co0 + q * EL)->y, 0, 0);
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int sl = 0; sl < XSL; ++sl)
            if (tid + sl * 256 < DT * HPC) xs[tid + sl * 256] = xr[sl];
#pragma unroll
        for (int v = 0; v < YV; ++v) {
            const int idx = tid + v * 256;
            if constexpr (sizeof(TY) == 4) {
                *reinterpret_cast<uint4 *>(ys + (idx >> 2) * 16 + (idx & 3) * 4) = yr[v];
            } else {
                typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
                const bf16x8_t h = __builtin_bit_cast(bf16x8_t, yr[v]);
                float *dst = ys + (idx >> 1) * 16 + (idx & 1) * 8;
                *reinterpret_cast<float4 *>(dst) = make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
                *reinterpret_cast<float4 *>(dst + 4) = make_float4((float)h[4], (float)h[5], (float)h[6], (float)h[7]);
            }
        }
    };
    if (t_begin < t_end) fetch(t_begin);
    for (int tile = t_begin; tile < t_end; ++tile) {
        commit();
        __syncthreads();
        if (tile + 1 < t_end) fetch(tile + 1);
#pragma unroll 4
        for (int ks = 0; ks < 16; ++ks) {
            const int r = 4 * wv + (ks >> 2), g = ks & 3;
            const float b = ys[(r * TW + 4 * g + kk) * 16 + li];
            bsum += b;
            const float *xp = xs + ((r + ky) * HW + 4 * g + kk + kx) * CIN;
#pragma unroll
            for (int sc = 0; sc < CS; ++sc) {
                const float a = live_row ? xp[(sc / CIN) * HPC + sc % CIN] : 0.f;
                acc[sc] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[sc], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    bsum += __shfl_xor(bsum, 16);
    bsum += __shfl_xor(bsum, 32);
    // D: rows (taps) 4*kk + j, column (co) li
#pragma unroll
    for (int sc = 0; sc < CS; ++sc)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4 * kk + j < 9) red[wv][((4 * kk + j) * CS + sc) * 16 + li] = acc[sc][j];
    if (kk == 0) red[wv][9 * CS * 16 + li] = bsum;
    __syncthreads();
    for (int t = tid; t < ROWS * 16; t += 256) {
        const int row = t / 16, c = t % 16;
        if (co0 + c < Cout)
            partials[((size_t)blockIdx.x * ROWS + row) * Cout + co0 + c] =
                ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
    }
}

// rows = 9*DT*Cin + 1; row tap*(DT*Cin) + kd*Cin + c -> dW[kd][tap][c][co], which at DT = 1 is the row order itself
template <int DT>
__global__ __launch_bounds__(256) void conv_wgrad_cin1_finish_kernel(const float *__restrict__ partials,
                                                                      float *__restrict__ dw, float *__restrict__ db,
                                                                      int nblk, int Cin, int Cout, int G) {
    const int CS = DT * Cin, rows = 9 * CS + 1;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int i = t / G, g = t % G;
    if (i >= rows * Cout) return;
    const float s = sq_group_reduce(partials + i, (size_t)rows * Cout, nblk, g, G);
    if (g != 0) return;
    if (i >= (rows - 1) * Cout) {
        if (db) db[i - (rows - 1) * Cout] = s;
    } else if constexpr (DT == 1) {
        dw[i] = s;
    } else {
        const int row = i / Cout, co = i % Cout;
        const int tap = row / CS, kd = (row % CS) / Cin, c = row % Cin;
        dw[((kd * 9 + tap) * Cin + c) * Cout + co] = s;
    }
}

// The grid arithmetic of every plan: npairs block columns (blockIdx.y) of gx persistent blocks, each walking tpb of the
// ntiles 16x16 tiles and leaving one partial of `rows` rows: [rows][bn] per pair (MFMA kernels), [rows][Cout] per block
// (small-Cin kernel).
void fill_plan(int64_t *out, int K, int kc, int bn, int kind, int ntiles, int npairs, int rows, int Cout) {
    // the small-Cin kernel hides latency only through resident blocks, so its grid fills the block slots of every CU
    // (2048 blocks: -0.5 % on the bf16 step vs 1024, within noise of 4096)
    static const int cin1_blocks = [] { const char *e = getenv("SQ_CIN1_BLOCKS"); return e ? atoi(e) : 2048; }();
    int want = kind == SQ_WGP_F32_SMALL ? cin1_blocks : (512 + npairs - 1) / npairs;   // MFMA: ~2 resident blocks per CU overall
    if (want < 1) want = 1;
    const int tpb = (ntiles + want - 1) / want;
    const int gx = (ntiles + tpb - 1) / tpb;
    const int64_t wsf = (int64_t)gx * rows * (kind == SQ_WGP_F32_SMALL ? Cout : npairs * bn);
    const int64_t v[SQ_WGP_N] = {K, kc, bn, kind, 1, npairs, gx, tpb, sq_group_size(gx), wsf};
    for (int i = 0; i < SQ_WGP_N; ++i) out[i] = v[i];
}

bool shape_ok(int N, int H, int W, int Cin, int Cout, int K) {
    if (Cin >= 1 && Cin <= 7 && K == 3 && N > 0 && H > 0 && W > 0 && Cout > 0 && Cout % 4 == 0) return true;
    return N > 0 && H > 0 && W > 0 && (K == 1 || K == 3) && (Cin % 16 == 0 || Cin == 8) && Cin > 0 &&
           Cout > 0 && Cout % 4 == 0 && (size_t)N * H * W * (size_t)(Cin > Cout ? Cin : Cout) * 4 < ((size_t)1 << 31);
}

// p: a plan of kind SQ_WGP_F32_SMALL for N planar images (N * D at DT = 3: Cin 1 and 2 only)
template <typename TY, int DT>
int launch_cin_small(const float *x, const TY *dy, float *dw, float *db, float *workspace, int N, int D, int H, int W,
                     int Cin, int Cout, const int64_t *p, hipStream_t st, const char *who) {
    constexpr int MAXC = DT == 1 ? 7 : 2;
    void (*kern)(const float *, const TY *, float *, int, int, int, int, int, int, int, int, int) = nullptr;
#define SQ_CIN_SMALL(C) if constexpr (C <= MAXC) if (Cin == C) kern = conv_wgrad_cin1_f32_kernel<TY, C, DT>;
    SQ_CIN_SMALL(1) SQ_CIN_SMALL(2) SQ_CIN_SMALL(3) SQ_CIN_SMALL(4) SQ_CIN_SMALL(5) SQ_CIN_SMALL(6) SQ_CIN_SMALL(7)
#undef SQ_CIN_SMALL
    SQ_REQUIRE(kern && p[SQ_WGP_KIND] == SQ_WGP_F32_SMALL, "%s: Cin=%d unsupported (1..%d)", who, Cin, MAXC);
    const int gx = (int)p[SQ_WGP_GX], G = (int)p[SQ_WGP_G];
    const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
    hipLaunchKernelGGL(kern, dim3(gx, (Cout + 15) / 16), dim3(256), 0, st, x, dy, workspace, N, H, W, Cout, tiles_x, tiles_y,
                       tiles_x * tiles_y * N, (int)p[SQ_WGP_TPB], D);
    int rc = sq_check_launch(who);
    if (rc) return rc;
    const int rows = 9 * DT * Cin + 1;
    hipLaunchKernelGGL(conv_wgrad_cin1_finish_kernel<DT>, dim3((rows * Cout * G + 255) / 256), dim3(256), 0, st, workspace,
                       dw, db, gx, Cin, Cout, G);
    return sq_check_launch(who);
}

}  // namespace

// ---- launch plans (host only; the launchers and the workspace queries take their choices from here) -------------------
// the plan of a planar call (sq_wgrad_plan, family SQ_PLAN_F32): out[SQ_WGP_N]
int sq_wgrad_f32_plan(int N, int H, int W, int Cin, int Cout, int K, int64_t *out) {
    if (!shape_ok(N, H, W, Cin, Cout, K)) return SQ_EINVAL;
    const int ntiles = ((W + TW - 1) / TW) * ((H + TH - 1) / TH) * N;
    if (Cin <= 7) {                                             // the small-Cin kernel: 16-channel co groups, one input chunk
        fill_plan(out, K, Cin, 16, SQ_WGP_F32_SMALL, ntiles, (Cout + 15) / 16, 9 * Cin + 1, Cout);
    } else {
        const int kc = Cin % 16 == 0 ? 16 : 8, bn = Cout > 16 ? 32 : 16;
        fill_plan(out, K, kc, bn, SQ_WGP_F32, ntiles, (Cin / kc) * ((Cout + bn - 1) / bn), K * K * 16 + 1, Cout);   // WCfg<>::ROWS
    }
    return SQ_OK;
}

extern "C" int sq_conv3d_wgrad_plan(int N, int D, int H, int W, int Cin, int Cout, int64_t *out) {
    SQ_REQUIRE(out, "sq_conv3d_wgrad_plan: null out");
    SQ_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "sq_conv3d_wgrad_plan: bad shape");
    SQ_REQUIRE(Cin == 1 || Cin == 2 || Cin % 16 == 0,
               "sq_conv3d_wgrad_plan: Cin=%d unsupported (1, 2 or a multiple of 16, as the forward)", Cin);
    SQ_REQUIRE(Cout % 4 == 0, "sq_conv3d_wgrad_plan: Cout=%d must be a multiple of 4", Cout);
    const int64_t cmax = Cin > Cout ? Cin : Cout;
    const int64_t bytes = (int64_t)N * D * H * W * cmax * 4;
    SQ_REQUIRE(bytes < LIM32, "sq_conv3d_wgrad_plan: a tensor of %lld bytes; the gradient kernels address whole tensors "
               "with 32-bit offsets (< 2 GiB)", (long long)bytes);
    const int ntiles = ((W + TW - 1) / TW) * ((H + TH - 1) / TH) * N * D;
    if (Cin <= 2) {                                             // the small-Cin kernel: 16-channel co groups, one stacked chunk
        fill_plan(out, 3, 3 * Cin, 16, SQ_WGP_F32_SMALL, ntiles, (Cout + 15) / 16, 27 * Cin + 1, Cout);
    } else {                                                    // pair = (depth tap, ci chunk, co chunk)
        const int bn = Cout > 16 ? 32 : 16;
        fill_plan(out, 3, 16, bn, SQ_WGP_F32, ntiles, 3 * (Cin / 16) * ((Cout + bn - 1) / bn), 9 * 16 + 1, Cout);
    }
    return SQ_OK;
}

extern "C" int64_t sq_conv2d_nhwc_wgrad_workspace_f32(int N, int H, int W, int Cin, int Cout, int K) {
    int64_t p[SQ_WGP_N];
    return sq_wgrad_f32_plan(N, H, W, Cin, Cout, K, p) == SQ_OK ? p[SQ_WGP_WS] * 4 : -1;
}

extern "C" int64_t sq_conv3d_ndhwc_wgrad_workspace_f32(int N, int D, int H, int W, int Cin, int Cout) {
    int64_t p[SQ_WGP_N];
    return sq_conv3d_wgrad_plan(N, D, H, W, Cin, Cout, p) == SQ_OK ? p[SQ_WGP_WS] * 4 : -1;
}

// dW multiplied by dw_scale in the finish kernel (MFMA kernels: Cin 8 or a multiple of 16; the small-Cin kernel has no
// scaled form): see sq_conv2d_nhwc_wgrad_scaled_mixed_f32
extern "C" int sq_conv2d_nhwc_wgrad_scaled_f32(const float *x, const float *dy, float *dw, float *db, float *workspace,
                                               int N, int H, int W, int Cin, int Cout, int K, float dw_scale, void *stream) {
    SQ_REQUIRE(Cin > 7 || dw_scale == 1.0f, "sq_conv2d_nhwc_wgrad_scaled_f32: Cin=%d has no scaled form", Cin);
    SQ_REQUIRE(x && dy && dw && workspace, "sq_conv2d_nhwc_wgrad_f32: null pointer");
    SQ_REQUIRE(shape_ok(N, H, W, Cin, Cout, K),
               "sq_conv2d_nhwc_wgrad_f32: unsupported shape N=%d H=%d W=%d Cin=%d Cout=%d K=%d "
               "(Cin 1..7 with K 3, 8 or %%16; Cout %%4; K 1|3; tensors < 2 GiB)", N, H, W, Cin, Cout, K);
    SQ_REQUIRE_ALIGNED(x); SQ_REQUIRE_ALIGNED(dy); SQ_REQUIRE_ALIGNED(workspace);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int64_t p[SQ_WGP_N];
    sq_wgrad_f32_plan(N, H, W, Cin, Cout, K, p);
    if (Cin <= 7)
        return launch_cin_small<float, 1>(x, dy, dw, db, workspace, N, 1, H, W, Cin, Cout, p, st,
                                          "sq_conv2d_nhwc_wgrad_f32(small Cin)");
    return launch_dispatch(x, dy, dw, db, workspace, N, H, W, Cin, Cout, K, p, dw_scale, st);
}

extern "C" int sq_conv2d_nhwc_wgrad_f32(const float *x, const float *dy, float *dw, float *db,
                                        float *workspace, int N, int H, int W, int Cin, int Cout, int K,
                                        void *stream) {
    return sq_conv2d_nhwc_wgrad_scaled_f32(x, dy, dw, db, workspace, N, H, W, Cin, Cout, K, 1.0f, stream);
}

extern "C" int sq_conv3d_ndhwc_wgrad_f32(const float *x, const float *dy, float *dw, float *db, float *workspace, int N,
                                         int D, int H, int W, int Cin, int Cout, void *stream) {
    SQ_REQUIRE(x && dy && dw && workspace, "sq_conv3d_ndhwc_wgrad_f32: null pointer");
    int64_t p[SQ_WGP_N];
    const int rc = sq_conv3d_wgrad_plan(N, D, H, W, Cin, Cout, p);
    if (rc != SQ_OK) return rc;
    SQ_REQUIRE_ALIGNED(x); SQ_REQUIRE_ALIGNED(dy); SQ_REQUIRE_ALIGNED(workspace);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const char *who = "sq_conv3d_ndhwc_wgrad_f32";
    if (p[SQ_WGP_KIND] == SQ_WGP_F32_SMALL)
        return launch_cin_small<float, 3>(x, dy, dw, db, workspace, N * D, D, H, W, Cin, Cout, p, st, who);
    return p[SQ_WGP_NO] == 32 ? launch<32, 3, 16, 3>(x, dy, dw, db, workspace, N * D, D, H, W, Cin, Cout, p, 1.0f, st, who)
                              : launch<16, 3, 16, 3>(x, dy, dw, db, workspace, N * D, D, H, W, Cin, Cout, p, 1.0f, st, who);
}

// first-layer weight gradient with a bf16 dY (the bf16 training graph): same MFMA-over-taps kernel
extern "C" int64_t sq_conv3x3_first_wgrad_workspace_bf16(int N, int H, int W, int Cin, int Cout) {
    int64_t p[SQ_WGP_N];
    if (Cin < 1 || Cin > 7 || sq_wgrad_f32_plan(N, H, W, Cin, Cout, 3, p) != SQ_OK) return -1;
    return p[SQ_WGP_WS] * 4;
}

extern "C" int sq_conv3x3_first_wgrad_bf16(const float *x, const void *dy, float *dw, float *db, float *workspace,
                                           int N, int H, int W, int Cin, int Cout, void *stream) {
    int64_t p[SQ_WGP_N];
    SQ_REQUIRE(x && dy && dw && workspace && N > 0 && H > 0 && W > 0 && Cin >= 1 && Cin <= 7 && Cout > 0 && Cout % 4 == 0 &&
               sq_wgrad_f32_plan(N, H, W, Cin, Cout, 3, p) == SQ_OK,
               "sq_conv3x3_first_wgrad_bf16: bad arguments (Cin 1..7, Cout %% 4 == 0)");
    return launch_cin_small<__bf16, 1>(x, reinterpret_cast<const __bf16 *>(dy), dw, db, workspace, N, 1, H, W, Cin, Cout, p,
                                       reinterpret_cast<hipStream_t>(stream), "sq_conv3x3_first_wgrad_bf16");
}
