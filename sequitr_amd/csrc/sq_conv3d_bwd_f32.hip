// Backward of the volumetric (3-D) f32 operators of UNet3D for gfx950 (forward: sq_conv3d_f32.hip).  Tensors are NDHWC.
//
//   * sq_conv3d_ndhwc_wgrad_f32: weight (and bias) gradient of the 3x3x3 SAME convolution,
//       dW[kd][kh][kw][ci][co] = sum over voxels p of X[p + (kd-1, kh-1, kw-1)][ci] * dY[p][co],  db[co] = sum_p dY[p][co],
//     i.e. the planar weight gradient (sq_conv_wgrad_f32.hip) of the depth-stacked input xs[n,d,h,w, kd*Cin + c] =
//     x[n, d+kd-1, h, w, c] over the N*D planar images -- xs is never built.
//       - Cin % 16 == 0: conv_wgrad_f32_kernel's scheme (v_mfma_f32_16x16x4_f32, reduction over pixels, one accumulator
//         block per in-plane tap, persistent blocks over 16x16 pixel tiles, register prefetch of the next tile).  A pair
//         is (depth tap kd, 16-channel ci chunk, BN-channel co chunk): the X halo of the tile at output slice nd = n*D + d
//         is read from slice nd + kd - 1, or is all zeros when d + kd - 1 leaves [0, D) -- the tap never reaches into the
//         neighbouring volume of the batch; the dY tile comes from slice nd.  Accumulators and LDS per block are those of
//         the planar kernel (9 taps x NR blocks).
//       - Cin in {1,2}: conv_wgrad_cin1_f32_kernel's scheme (the 9 in-plane taps ride the 16 MFMA rows, one accumulator
//         per stacked channel) at 3*Cin = 3 or 6 stacked channels gathered from three slices.
//     Both are two-stage: block partials, then a finish kernel that adds them IN A FIXED ORDER (sq_group_reduce): no float
//     atomics, run-to-run bit-identical (MI355X_MICROARCH.md "Global float atomics").  db is taken from the centre depth
//     tap's partials only (every pair sums dY; kd = 1 always reads a real slice).  Every element of dW and db is written:
//     at D == 1 the taps kd = 0 and kd = 2 see only zero halos and come out as exact zeros.
//   * sq_conv3d_weight_transform_f32: the filter of the input gradient, which is the FORWARD conv3d of dY with it.
//   * sq_maxpool2x2x2_bwd_f32, sq_space_to_depth2x2x2_f32: streaming kernels, 16-B loads and stores.
#include "sq_common.h"

namespace {

constexpr int TH = 16, TW = 16;
constexpr int64_t LIM32 = (int64_t)1 << 31;

template <int BN>
struct W3Cfg {
    static constexpr int KS = 3, KC = 16;
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

// partials layout: [gridDim.x][npairs][ROWS][BN]; pair = (kd * (Cin/16) + ci chunk) * nco + co chunk = blockIdx.y.
// ND = N * D planar images; a tile is (tx, ty, nd), walked nd-major as in the forward kernel.
template <int BN>
__global__ __launch_bounds__(256, 2) void conv3d_wgrad_f32_kernel(
    const float *__restrict__ x, const float *__restrict__ dy, float *__restrict__ partials,
    int ND, int D, int H, int W, int Cin, int Cout, int tiles_x, int tiles_y, int ntiles, int tiles_per_block) {
    using C = W3Cfg<BN>;
    constexpr int NR = C::NR, PAD = 1, KS = 3, KC = 16;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *xs = smem;
    float *ys = smem + C::XS_FLOATS;

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int li = lane & 15, kk = lane >> 4;
    const int nco = (Cout + BN - 1) / BN, nci = Cin / KC;
    const int kd = blockIdx.y / (nci * nco), rem = blockIdx.y % (nci * nco);
    const int ci0 = (rem / nco) * KC, co0 = (rem % nco) * BN;
    const int t_begin = blockIdx.x * tiles_per_block;
    const int t_end = min(t_begin + tiles_per_block, ntiles);

    // whole tensors are < 2 GiB (the plan refuses anything else): one resource each, 32-bit byte offsets
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(x), 0, (int)((size_t)ND * H * W * Cin * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t yrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(dy), 0, (int)((size_t)ND * H * W * Cout * 4), 0x00020000);
    constexpr unsigned OOB = 0x80000000u;

    float4 xr[C::XSLOTS], yr[C::YSLOTS];
    auto issue = [&](int tile) {
        const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, nd = tile / (tiles_x * tiles_y);
        const int x0 = tx * TW, y0 = ty * TH;
        // the depth tap reads slice nd + kd - 1 of the SAME volume, else the depth border's zeros
        const bool depth_ok = (unsigned)(nd % D + kd - 1) < (unsigned)D;
        // formed only for a slice that exists: slice ND of a tensor just under 2 GiB would overflow the int
        const int xbase = depth_ok ? ((((nd + kd - 1) * H + y0 - PAD) * W + x0 - PAD) * Cin) * 4 : 0;
        const int ybase = (((nd * H + y0) * W + x0) * Cout) * 4;
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

// second stage: dW[kd][tap][ci][co] = sum_b partials[b][pair(kd, ci, co)][tap*16 + ci%16][co%BN], b ascending;
// db[co] from the pairs (kd = 1, ci chunk 0)
template <int BN>
__global__ __launch_bounds__(256) void conv3d_wgrad_finish_kernel(const float *__restrict__ partials,
                                                                   float *__restrict__ dw, float *__restrict__ db,
                                                                   int nblk, int Cin, int Cout, int G) {
    using C = W3Cfg<BN>;
    const int nco = (Cout + BN - 1) / BN, nci = Cin / 16, npairs = 3 * nci * nco;
    const int total = 27 * Cin * Cout;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int i = t / G, g = t % G;
    const size_t stride = (size_t)npairs * C::RED_FLOATS;
    if (i < total) {
        const int co = i % Cout, ci = (i / Cout) % Cin, tap27 = i / (Cout * Cin);
        const int kd = tap27 / 9, tap = tap27 % 9;
        const int pair = (kd * nci + ci / 16) * nco + co / BN;
        const size_t off = (size_t)pair * C::RED_FLOATS + (tap * 16 + ci % 16) * BN + co % BN;
        const float s = sq_group_reduce(partials + off, stride, nblk, g, G);
        if (g == 0) dw[i] = s;
    } else if (i < total + Cout) {
        const int co = i - total;
        const int pair = (1 * nci + 0) * nco + co / BN;
        const size_t off = (size_t)pair * C::RED_FLOATS + (C::NTAP * 16) * BN + co % BN;
        const float s = sq_group_reduce(partials + off, stride, nblk, g, G);
        if (g == 0 && db) db[co] = s;
    }
}

template <int BN>
int launch_mfma(const float *x, const float *dy, float *dw, float *db, float *ws, int N, int D, int H, int W, int Cin,
                int Cout, const int64_t *p, hipStream_t st) {
    using C = W3Cfg<BN>;
    static bool attr_set = false;
    auto kern = conv3d_wgrad_f32_kernel<BN>;
    if (!attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                C::LDS_BYTES) != hipSuccess) {
            sq_set_error("conv3d_wgrad_f32: cannot reserve %d bytes of LDS", C::LDS_BYTES);
            return SQ_ELAUNCH;
        }
        attr_set = true;
    }
    const int gx = (int)p[SQ_WGP_GX], G = (int)p[SQ_WGP_G];
    const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
    hipLaunchKernelGGL(kern, dim3(gx, (unsigned)p[SQ_WGP_NPAIRS]), dim3(256), C::LDS_BYTES, st, x, dy, ws, N * D, D, H, W,
                       Cin, Cout, tiles_x, tiles_y, tiles_x * tiles_y * N * D, (int)p[SQ_WGP_TPB]);
    int rc = sq_check_launch("sq_conv3d_ndhwc_wgrad_f32");
    if (rc) return rc;
    const int64_t total = ((int64_t)27 * Cin * Cout + Cout) * G;
    hipLaunchKernelGGL((conv3d_wgrad_finish_kernel<BN>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, ws, dw, db,
                       gx, Cin, Cout, G);
    return sq_check_launch("sq_conv3d_ndhwc_wgrad_f32(finish)");
}

// ---- first layer (Cin = 1, 2): the 9 in-plane taps ride the 16 MFMA rows, one accumulator per STACKED channel ---------
//   A[i = tap][k = pixel] = X[slice nd + kd - 1][pixel + tap][c] (rows 9..15 zero), B[k][j = co] = dY[slice nd][pixel][co]
// partials: [gridDim.x][9*CS + 1][Cout], row tap*CS + kd*CIN + c, then the bias row; blockIdx.y = 16-channel co group.
template <int CIN>
__global__ __launch_bounds__(256) void conv3d_wgrad_small_f32_kernel(
    const float *__restrict__ x, const float *__restrict__ dy, float *__restrict__ partials, int ND, int D, int H, int W,
    int Cout, int tiles_x, int tiles_y, int ntiles, int tiles_per_block) {
    constexpr int CS = 3 * CIN, HW = TW + 2, HPC = HW * HW * CIN, ROWS = 9 * CS + 1;
    __shared__ float xs[3 * HPC + 8];                          // [kd][halo pixel][c]
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
    // register double buffer: the next tile's loads are in flight while this one is multiplied
    constexpr int XSL = (3 * HPC + 255) / 256;                  // halo items (one float) per thread
    float xr[XSL];
    float4 yr[4];                                               // 256 px x 16 ch of dY: four 16-byte pieces per thread
    auto fetch = [&](int tile) {
        const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, nd = tile / (tiles_x * tiles_y);
        const int x0 = tx * TW, y0 = ty * TH, d = nd % D;
#pragma unroll
        for (int sl = 0; sl < XSL; ++sl) {
            const int idx = tid + sl * 256;
            const int kd = idx / HPC, r = idx - kd * HPC;
            const int pix = r / CIN, c = r % CIN;
            const int gy = y0 - 1 + pix / HW, gx = x0 - 1 + pix % HW;
            // slice nd + kd - 1 of the same volume, else the depth border's zeros
            xr[sl] = (idx < 3 * HPC && (unsigned)(d + kd - 1) < (unsigned)D && gy >= 0 && gy < H && gx >= 0 && gx < W)
                         ? x[(((size_t)(nd + kd - 1) * H + gy) * W + gx) * CIN + c] : 0.f;
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int idx = tid + v * 256, pix = idx >> 2, q = idx & 3;
            const int gy = y0 + pix / TW, gx = x0 + pix % TW;
            yr[v] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gy < H && gx < W && co0 + q * 4 < Cout)         // Cout % 4 == 0
                yr[v] = *reinterpret_cast<const float4 *>(dy + (((size_t)nd * H + gy) * W + gx) * Cout + co0 + q * 4);
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int sl = 0; sl < XSL; ++sl)
            if (tid + sl * 256 < 3 * HPC) xs[tid + sl * 256] = xr[sl];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int idx = tid + v * 256;
            *reinterpret_cast<float4 *>(ys + (idx >> 2) * 16 + (idx & 3) * 4) = yr[v];
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

// rows = 9*CS + 1; row tap*CS + kd*Cin + c -> dW[kd][tap][c][co]
__global__ __launch_bounds__(256) void conv3d_wgrad_small_finish_kernel(const float *__restrict__ partials,
                                                                         float *__restrict__ dw, float *__restrict__ db,
                                                                         int nblk, int Cin, int Cout, int G) {
    const int CS = 3 * Cin, rows = 9 * CS + 1;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int i = t / G, g = t % G;
    if (i >= rows * Cout) return;
    const float s = sq_group_reduce(partials + i, (size_t)rows * Cout, nblk, g, G);
    if (g != 0) return;
    const int row = i / Cout, co = i % Cout;
    if (row < rows - 1) {
        const int tap = row / CS, sc = row % CS, kd = sc / Cin, c = sc % Cin;
        dw[((kd * 9 + tap) * Cin + c) * Cout + co] = s;
    } else if (db) {
        db[co] = s;
    }
}

int launch_small(const float *x, const float *dy, float *dw, float *db, float *ws, int N, int D, int H, int W, int Cin,
                 int Cout, const int64_t *p, hipStream_t st) {
    const int gx = (int)p[SQ_WGP_GX], tpb = (int)p[SQ_WGP_TPB], G = (int)p[SQ_WGP_G];
    const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
    const dim3 grid(gx, (Cout + 15) / 16);
    if (Cin == 1)
        hipLaunchKernelGGL(conv3d_wgrad_small_f32_kernel<1>, grid, dim3(256), 0, st, x, dy, ws, N * D, D, H, W, Cout, tiles_x,
                           tiles_y, tiles_x * tiles_y * N * D, tpb);
    else
        hipLaunchKernelGGL(conv3d_wgrad_small_f32_kernel<2>, grid, dim3(256), 0, st, x, dy, ws, N * D, D, H, W, Cout, tiles_x,
                           tiles_y, tiles_x * tiles_y * N * D, tpb);
    int rc = sq_check_launch("sq_conv3d_ndhwc_wgrad_f32(small Cin)");
    if (rc) return rc;
    const int rows = 27 * Cin + 1;
    hipLaunchKernelGGL(conv3d_wgrad_small_finish_kernel, dim3((rows * Cout * G + 255) / 256), dim3(256), 0, st, ws, dw, db,
                       gx, Cin, Cout, G);
    return sq_check_launch("sq_conv3d_ndhwc_wgrad_f32(small Cin, finish)");
}

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

// ---- launch plan (host only; the launcher and the workspace query below take their choices from here) ------------------
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
    int gx, tpb, npairs, kc, bn;
    int64_t wsf;
    if (Cin <= 2) {                                             // the small-Cin kernel: 16-channel co groups, one stacked chunk
        tpb = (ntiles + 2047) / 2048;                           // fills the block slots of every CU, as the planar kernel's grid
        gx = (ntiles + tpb - 1) / tpb;
        kc = 3 * Cin, bn = 16, npairs = (Cout + 15) / 16;
        wsf = (int64_t)gx * (27 * Cin + 1) * Cout;
    } else {
        kc = 16;
        bn = Cout > 16 ? 32 : 16;
        npairs = 3 * (Cin / 16) * ((Cout + bn - 1) / bn);       // (depth tap, ci chunk, co chunk)
        int want = (512 + npairs - 1) / npairs;                 // ~2 resident blocks per CU overall
        if (want < 1) want = 1;
        tpb = (ntiles + want - 1) / want;
        if (tpb < 1) tpb = 1;
        gx = (ntiles + tpb - 1) / tpb;
        wsf = (int64_t)gx * npairs * (9 * 16 + 1) * bn;        // W3Cfg<>::RED_FLOATS per pair
    }
    const int64_t v[SQ_WGP_N] = {3, kc, bn, Cin <= 2 ? SQ_WGP_F32_SMALL : SQ_WGP_F32, 1, npairs, gx, tpb, sq_group_size(gx), wsf};
    for (int i = 0; i < SQ_WGP_N; ++i) out[i] = v[i];
    return SQ_OK;
}

extern "C" int64_t sq_conv3d_ndhwc_wgrad_workspace_f32(int N, int D, int H, int W, int Cin, int Cout) {
    int64_t p[SQ_WGP_N];
    return sq_conv3d_wgrad_plan(N, D, H, W, Cin, Cout, p) == SQ_OK ? p[SQ_WGP_WS] * 4 : -1;
}

extern "C" int sq_conv3d_ndhwc_wgrad_f32(const float *x, const float *dy, float *dw, float *db, float *workspace, int N,
                                         int D, int H, int W, int Cin, int Cout, void *stream) {
    SQ_REQUIRE(x && dy && dw && workspace, "sq_conv3d_ndhwc_wgrad_f32: null pointer");
    int64_t p[SQ_WGP_N];
    const int rc = sq_conv3d_wgrad_plan(N, D, H, W, Cin, Cout, p);
    if (rc != SQ_OK) return rc;
    SQ_REQUIRE_ALIGNED(x); SQ_REQUIRE_ALIGNED(dy); SQ_REQUIRE_ALIGNED(workspace);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (p[SQ_WGP_KIND] == SQ_WGP_F32_SMALL) return launch_small(x, dy, dw, db, workspace, N, D, H, W, Cin, Cout, p, st);
    return p[SQ_WGP_NO] == 32 ? launch_mfma<32>(x, dy, dw, db, workspace, N, D, H, W, Cin, Cout, p, st)
                              : launch_mfma<16>(x, dy, dw, db, workspace, N, D, H, W, Cin, Cout, p, st);
}

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
