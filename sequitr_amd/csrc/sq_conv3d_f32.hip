// Volumetric (3-D) f32 operators of UNet3D for gfx950: 3x3x3 SAME convolution, 2x2x2 max-pool and the 2x2x2 stride-2
// transpose convolution fused with the bridge.  Tensors are NDHWC (N,D,H,W,C).
//
// conv3d is DEFINED through the planar convolution (include/sequitr_hip.h, sq_conv3d_ndhwc_fwd_f32): it is the planar
// 3x3 conv of the depth-stacked input xs[n,d,h,w, kd*Cin + c] = x[n, d+kd-1, h, w, c] (zero slices past the depth ends)
// with the stacked filter ws[kh,kw, kd*Cin + c, o] = w[kd,kh,kw,c,o], evaluated as N*D planar images of 3*Cin channels.
// The kernels below never build xs: the virtual 3*Cin channel axis is gathered from three depth slices.
//   * Cin % 16 == 0: the pipelined implicit GEMM of sq_conv_f32_v2.hip (16x16-pixel tiles x BN channels, staged halo and
//     weight slab, T14 split staging, persistent blocks), reduced to its plain form.  A KC-channel chunk of the stacked
//     axis lies in ONE depth slice (KC divides Cin), so a chunk is (depth tap kd, channels c0 .. c0+KC-1): the halo is read
//     from slice d+kd-1 (or is all zeros), the weight slab from w[kd] -- the TF filter layout is addressed directly, no
//     host-side reordering.  Chain: depth tap, 16-channel chunk, in-plane tap (raster), channel.
//   * Cin in {1,2}: the direct VALU kernel of the planar path (Cin 3 or 6 there) with the stacked channel gathered per tap.
//     Chain: in-plane tap, depth tap, channel.
// Tiles are walked depth-major inside a volume (tile index = ((n*D + d)*tiles_y + ty)*tiles_x + tx): the blocks in flight
// cover a contiguous run of slices, so a slice is read by its three consumers (slices d-1, d, d+1) close together in time.
//
// Addressing: SQ_C3_FLAT -- every tensor is < 2 GiB: one buffer resource per tensor, 32-bit offsets.  SQ_C3_WINDOW -- a
// tensor reaches 2 GiB or more: each (tile, depth tap) builds its buffer resource from a 64-bit pointer to its depth slice
// and addresses inside that slice with 32-bit offsets (a slice must be < 2 GiB).  The plan (sq_conv3d_plan) picks the form
// and refuses what neither takes.
#include <stdlib.h>
#include <type_traits>
#include "sq_common.h"

namespace {

constexpr int TH = 16, TW = 16;
constexpr unsigned OOB = 0x80000000u;
constexpr int64_t LIM32 = (int64_t)1 << 31;

typedef unsigned u32x4 __attribute__((__vector_size__(4 * sizeof(unsigned))));

template <int BN, int KC>
struct Cfg3 {
    static constexpr int KS = 3;
    static constexpr int HALO_W = TW + KS - 1;
    static constexpr int HALO_H = TH + KS - 1;
    static constexpr int HP = HALO_W * HALO_H;
    static constexpr int PS = KC + 2;                       // pixel stride (floats): conflict-free B reads
    static constexpr int WSWZ = (KC == 32 && BN == 32) ? 16 : 0;   // as Cfg2 in sq_conv_f32_v2.hip
    static constexpr int BNS = WSWZ ? BN : ((BN % 32 == 0) ? BN + 16 : BN);
    static constexpr int WROWS = KS * KS * KC;
    static constexpr int XS_FLOATS = HP * PS;
    static constexpr int WS_FLOATS = WROWS * BNS;
    static constexpr int LDS_BYTES = (XS_FLOATS + WS_FLOATS) * 4;
    static constexpr int QPP = KC / 4;
    static constexpr int XITEMS = HP * QPP;
    static constexpr int XSLOTS = (XITEMS + 255) / 256;
    static constexpr int WITEMS = WROWS * (BN / 4);
    static constexpr int WSLOTS = (WITEMS + 255) / 256;
    static constexpr int NSTEP = KS * KS * (KC / 4);
    static constexpr int OCC = (BN >= 64 || KC == 32) ? 2 : (BN >= 32 ? 3 : 4);
    static_assert(KC == 16 || (KC == 32 && BN == 32), "the 32-channel stage exists for 32-channel blocks");
    static_assert((XS_FLOATS * 4) % 16 == 0, "weight slab must start 16-B aligned");
};

struct C3Args {
    const float *x, *w, *bias;
    float *y;
    int N, D, H, W, Cin, Cout, act;
    int tiles_x, tiles_y, ntiles;
};

template <bool WIN>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t slice_rsrc(const float *base, int slice, int slice_floats, int full_bytes,
                                                             bool valid) {
    // WIN: a resource over one depth slice from a 64-bit pointer; otherwise the whole tensor (offsets carry the slice)
    const float *p = WIN ? base + (size_t)slice * (size_t)slice_floats : base;
    const int nrec = valid ? (WIN ? slice_floats * 4 : full_bytes) : 0;    // 0: every lane reads zeros
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p), 0, nrec, 0x00020000);
}

template <int BN, int KC, bool WIN>
__global__ __launch_bounds__(256, (Cfg3<BN, KC>::OCC)) void conv3d_mfma_f32_kernel(const C3Args a) {
    using C = Cfg3<BN, KC>;
    constexpr int NR = BN / 16;
    constexpr int PAD = 1;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *xs = smem;
    float *ws = smem + C::XS_FLOATS;

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    __builtin_assume(tid < 256);
    const int li = lane & 15, kk = lane >> 4;
    const int H = a.H, W = a.W, D = a.D, Cin = a.Cin, Cout = a.Cout;
    const int n0 = blockIdx.y * BN;
    const int vb = (int)sq_xcd_remap(blockIdx.x, gridDim.x);
    const int tstride = (int)gridDim.x;                     // block b takes tiles b, b + G, b + 2G, ...
    const int t_begin = vb;
    if (t_begin >= a.ntiles) return;
    const int t_count = (a.ntiles - vb + tstride - 1) / tstride;
    const int nchunk = 3 * Cin / KC;
    const int nitems = t_count * nchunk;

    const int xsl = H * W * Cin, ysl = H * W * Cout;        // floats per depth slice (< 2^31 bytes, checked by the plan)
    const int x_bytes = WIN ? 0 : (int)((size_t)a.N * D * xsl * 4);
    const int y_bytes = WIN ? 0 : (int)((size_t)a.N * D * ysl * 4);
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(a.w), 0, 27 * Cin * Cout * 4, 0x00020000);

    int xrel[C::XSLOTS], xpy[C::XSLOTS], xpx[C::XSLOTS];
#pragma unroll
    for (int sl = 0; sl < C::XSLOTS; ++sl) {
        const int idx = tid + sl * 256;
        const int pix = idx / C::QPP, q = idx % C::QPP;
        xpy[sl] = pix / C::HALO_W;
        xpx[sl] = pix % C::HALO_W;
        xrel[sl] = idx < C::XITEMS ? ((xpy[sl] * W + xpx[sl]) * Cin + q * 4) * 4 : (int)OOB;
    }
    int wrel[C::WSLOTS];
#pragma unroll
    for (int sl = 0; sl < C::WSLOTS; ++sl) {
        const int idx = tid + sl * 256;
        const int r = idx / (BN / 4), q4 = idx % (BN / 4);
        const int tap = r / KC, c = r % KC;
        const int co = n0 + q4 * 4;
        wrel[sl] = (idx < C::WITEMS && co < Cout) ? ((tap * Cin + c) * Cout + co) * 4 : (int)OOB;
    }

    float4 xr[C::XSLOTS];
    float4 wr[C::WSLOTS];
    // ---- global loads of work item (tile, stacked chunk cc) into registers --------------------------------------------
    // nd = n * D + d is the tile's output slice; the chunk's depth tap kd reads slice nd + kd - 1 when d + kd - 1 is
    // inside the volume, otherwise the resource has no records and the whole halo reads as the depth border's zeros
    auto issue = [&](int tx, int ty, int nd, int cc) {
        const int kd = cc / Cin, c0 = cc - kd * Cin;
        const int d = nd % D;
        const bool depth_ok = (unsigned)(d + kd - 1) < (unsigned)D;
        const int s = nd + kd - 1;
        const __amdgpu_buffer_rsrc_t rs = slice_rsrc<WIN>(a.x, s, xsl, x_bytes, depth_ok);
        const int x0 = tx * TW - PAD, y0 = ty * TH - PAD;
        const int base = ((WIN ? 0 : s * xsl) + (y0 * W + x0) * Cin + c0) * 4;    // may be "negative": wraps back
        const bool inner = (BN >= 32 || KC == 32) && x0 >= 0 && y0 >= 0 && x0 + C::HALO_W <= W && y0 + C::HALO_H <= H;
        if (inner) {
#pragma unroll
            for (int sl = 0; sl < C::XSLOTS; ++sl) {
                const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, xrel[sl], base, 0);
                xr[sl] = *reinterpret_cast<const float4 *>(&v);
            }
        } else {
#pragma unroll
            for (int sl = 0; sl < C::XSLOTS; ++sl) {
                int hpy = xpy[sl], hpx = xpx[sl];
                if constexpr (KC == 32) {                       // halo coordinates recomputed (register pressure, as in v2)
                    int tv = tid;
                    asm volatile("" : "+v"(tv));
                    const int hp = (tv + sl * 256) / C::QPP;
                    hpy = hp / C::HALO_W;
                    hpx = hp - hpy * C::HALO_W;
                }
                const bool inb = (unsigned)(y0 + hpy) < (unsigned)H && (unsigned)(x0 + hpx) < (unsigned)W &&
                                 xrel[sl] != (int)OOB;
                const unsigned off = inb ? (unsigned)(base + xrel[sl]) : OOB;
                const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
                xr[sl] = *reinterpret_cast<const float4 *>(&v);
            }
        }
        // weight slab of (kd, c0 .. c0 + KC - 1): rows (tap, c) of w[kd] in the TF layout (kd, kh, kw, Cin, Cout)
        const int wbase = (kd * 9 * Cin + c0) * Cout * 4;
#pragma unroll
        for (int sl = 0; sl < C::WSLOTS; ++sl) {
            const auto v = KC == 32 ? __builtin_amdgcn_raw_buffer_load_b128(wrsrc, wrel[0], wbase + sl * Cin * Cout * 4, 0)
                                    : __builtin_amdgcn_raw_buffer_load_b128(
                                          wrsrc, wrel[sl] == (int)OOB ? OOB : (unsigned)(wbase + wrel[sl]), 0, 0);
            wr[sl] = *reinterpret_cast<const float4 *>(&v);
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int sl = 0; sl < C::XSLOTS; ++sl) {
            const int idx = tid + sl * 256;
            if (idx < C::XITEMS) {
                const int pix = idx / C::QPP, q = idx % C::QPP;
                float *dst = xs + pix * C::PS + q * 4;
                *reinterpret_cast<float2 *>(dst) = make_float2(xr[sl].x, xr[sl].y);
                *reinterpret_cast<float2 *>(dst + 2) = make_float2(xr[sl].z, xr[sl].w);
            }
        }
#pragma unroll
        for (int sl = 0; sl < C::WSLOTS; ++sl) {
            const int idx = tid + sl * 256;
            if (idx < C::WITEMS) {
                const int r = idx / (BN / 4), q4 = idx % (BN / 4);
                *reinterpret_cast<float4 *>(ws + r * C::BNS + ((q4 * 4) ^ ((r & 1) ? C::WSWZ : 0))) = wr[sl];
            }
        }
    };

    f32x4 acc[4][NR];
    const float *xb_lds = xs + ((4 * wv) * C::HALO_W + li) * C::PS + kk;
    const float *wa_lds = ws + kk * C::BNS + li;
    // step st of an item: taps in raster order, 4 channels per step (KC == 32: the item's two 16-channel halves in turn,
    // the chain is unchanged)
    auto load_frag = [&](int st, float (&av)[NR], float (&bv)[4]) {
        constexpr int SPC = 9 * 4;
        const int sub = KC > 16 ? st / SPC : 0, sr = KC > 16 ? st % SPC : st;
        constexpr int Q = 4;
        const int tap = sr / Q, s = sr % Q;
        const int ky = tap / 3, kx = tap % 3;
        const int ch = sub * 16 + s * 4;
#pragma unroll
        for (int nb = 0; nb < NR; ++nb)
            av[nb] = wa_lds[(tap * KC + ch) * C::BNS + ((nb * 16) ^ ((kk & 1) ? C::WSWZ : 0))];
#pragma unroll
        for (int r = 0; r < 4; ++r) bv[r] = xb_lds[((r + ky) * C::HALO_W + kx) * C::PS + ch];
    };

    const bool is_relu = a.act == SQ_ACT_RELU;
    const float slope = a.act == SQ_ACT_LEAKY ? 0.2f : 1.0f;
    float4 bvr[NR];
#pragma unroll
    for (int nb = 0; nb < NR; ++nb) {
        const int co = n0 + nb * 16 + 4 * kk;
        bvr[nb] = (a.bias && co < Cout) ? *reinterpret_cast<const float4 *>(a.bias + co) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    auto epilogue = [&](int tx, int ty, int nd) {
        const __amdgpu_buffer_rsrc_t yrsrc = slice_rsrc<WIN>(a.y, nd, ysl, y_bytes, true);
        const int ybase = WIN ? 0 : nd * ysl;
        const int gx = tx * TW + li;
#pragma unroll
        for (int nb = 0; nb < NR; ++nb) {
            const int co = n0 + nb * 16 + 4 * kk;
            const float4 bv = bvr[nb];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gy = ty * TH + 4 * wv + r;
                f32x4 o;
                o[0] = a.bias ? acc[r][nb][0] + bv.x : acc[r][nb][0];
                o[1] = a.bias ? acc[r][nb][1] + bv.y : acc[r][nb][1];
                o[2] = a.bias ? acc[r][nb][2] + bv.z : acc[r][nb][2];
                o[3] = a.bias ? acc[r][nb][3] + bv.w : acc[r][nb][3];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float neg = is_relu ? 0.0f : o[e] * slope;
                    o[e] = o[e] > 0.0f ? o[e] : neg;
                }
                const bool ok = gy < H && gx < W && co < Cout;
                const unsigned off = ok ? (unsigned)((ybase + (gy * W + gx) * Cout + co) * 4) : OOB;
                // soffset = 0: the b128-store hazard
                __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<const u32x4 *>(&o), yrsrc, off, 0, 0);
                acc[r][nb] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
        }
    };

    // tile coordinates advance by carries; cn is the output slice nd = n * D + d
    const int per_image = a.tiles_x * a.tiles_y;
    const int s_n = tstride / per_image, s_y = (tstride % per_image) / a.tiles_x, s_x = (tstride % per_image) % a.tiles_x;
    int ctx = t_begin % a.tiles_x, cty = (t_begin / a.tiles_x) % a.tiles_y, cn = t_begin / per_image;
    int ntx = ctx + s_x, nty = cty, nn = cn;
    if (ntx >= a.tiles_x) { ntx -= a.tiles_x; nty += 1; }
    nty += s_y;
    if (nty >= a.tiles_y) { nty -= a.tiles_y; nn += 1; }
    nn += s_n;
    issue(ctx, cty, cn, 0);
    __builtin_amdgcn_s_waitcnt(0x0F70);                         // vmcnt(0)
    commit();
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int nb = 0; nb < NR; ++nb) acc[r][nb] = (f32x4){0.f, 0.f, 0.f, 0.f};
    __syncthreads();

    int tile = t_begin, chunk = 0;
    for (int it = 0; it < nitems; ++it) {
        int ntile = tile, nchk = chunk + 1;
        if (nchk == nchunk) { nchk = 0; ntile = tile + tstride; }
        const bool has_next = it + 1 < nitems;
        const bool same = ntile == tile;
        const int itx = same ? ctx : ntx, ity = same ? cty : nty, itn = same ? cn : nn;
        if (has_next) issue(itx, ity, itn, nchk * KC);
        {
            float a0[NR], b0[4], a1[NR], b1[4];
            load_frag(0, a0, b0);
            __builtin_amdgcn_s_setprio(0);
#pragma unroll
            for (int st = 0; st < C::NSTEP; st += 2) {
                if (st + 1 < C::NSTEP) load_frag(st + 1, a1, b1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int nb = 0; nb < NR; ++nb)
                        acc[r][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[nb], b0[r], acc[r][nb], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (st + 1 < C::NSTEP) {
                    if (st + 2 < C::NSTEP) load_frag(st + 2, a0, b0);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int nb = 0; nb < NR; ++nb)
                            acc[r][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[nb], b1[r], acc[r][nb], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            __builtin_amdgcn_s_setprio(3);
        }
        __builtin_amdgcn_s_waitcnt(0x0F70);                     // the prefetch has landed (see sq_conv_f32_v2.hip)
        if (has_next) {
            __syncthreads();
            commit();
        }
        if (chunk == nchunk - 1) epilogue(ctx, cty, cn);
        if (has_next) __syncthreads();
        if (ntile != tile) {
            ctx = ntx; cty = nty; cn = nn;
            ntx += s_x;
            if (ntx >= a.tiles_x) { ntx -= a.tiles_x; nty += 1; }
            nty += s_y;
            if (nty >= a.tiles_y) { nty -= a.tiles_y; nn += 1; }
            nn += s_n;
        }
        tile = ntile;
        chunk = nchk;
    }
}

// Cin in {1,2}: thread per pixel, 16 output channels per block (blockIdx.y).  A block computes one 16x16 tile of DB
// consecutive output slices: the DB + 2 input slices they read are staged once (each input slice feeds three outputs),
// as are the 9 x 3*Cin x 16 filter slab and the 16 bias values.  64-bit addressing throughout.
constexpr int DB = 4;                                           // output slices per block
template <int CIN>
__global__ __launch_bounds__(256) void conv3d_direct_f32_kernel(const C3Args a) {
    constexpr int CS = 3 * CIN;                                 // stacked channels
    constexpr int HALO_W = TW + 2, HP = HALO_W * (TH + 2);
    constexpr int NS = DB + 2;                                  // staged input slices
    __shared__ float xs[NS * HP * CIN];                         // [slice][halo pixel][c]
    __shared__ float wsl[9 * CS * 16];
    const int tid = threadIdx.x;
    const int H = a.H, W = a.W, D = a.D, Cout = a.Cout;
    const int per_image = a.tiles_x * a.tiles_y;
    const int dgroups = (D + DB - 1) / DB;
    const int sp = blockIdx.x;
    const int tx = sp % a.tiles_x, ty = (sp / a.tiles_x) % a.tiles_y, ng = sp / per_image;
    const int n = ng / dgroups, d0 = (ng - n * dgroups) * DB;   // output slices d0 .. d0 + DB - 1 of volume n
    const int x0 = tx * TW, y0 = ty * TH, n0 = blockIdx.y * 16;
    // input slice d0 - 1 + s; consecutive threads read consecutive pixels (and channels) of one slice row
    for (int idx = tid; idx < NS * HP * CIN; idx += 256) {
        const int sl = idx / (HP * CIN), r = idx - sl * (HP * CIN), pix = r / CIN, c = r % CIN;
        const int gy = y0 - 1 + pix / HALO_W, gx = x0 - 1 + pix % HALO_W, dz = d0 - 1 + sl;
        float v = 0.f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W && (unsigned)dz < (unsigned)D)
            v = a.x[((((size_t)n * D + dz) * H + gy) * W + gx) * CIN + c];
        xs[idx] = v;
    }
    for (int idx = tid; idx < 9 * CS * 16; idx += 256) {
        const int r = idx / 16, o = idx % 16;                  // r = tap * CS + kd * CIN + c
        const int tap = r / CS, sc = r % CS, kd = sc / CIN, c = sc % CIN;
        wsl[idx] = (n0 + o < Cout) ? a.w[((size_t)(kd * 9 + tap) * CIN + c) * Cout + n0 + o] : 0.f;
    }
    // the block's 16 bias values, once: read inside the slice loop they were 64 dependent vector loads per wave behind
    // the stores of the previous slice (a.bias may alias a.y as far as the compiler knows) -- 3x the planar kernel's
    // vector-memory instructions, and most of its time
    float bq[16];
#pragma unroll
    for (int o = 0; o < 16; ++o) bq[o] = (a.bias && n0 + o < Cout) ? a.bias[n0 + o] : 0.f;
    __syncthreads();
    const int py = tid >> 4, px = tid & 15;
    const int gy = y0 + py, gx = x0 + px;
#pragma unroll 1
    for (int j = 0; j < DB; ++j) {
        const int d = d0 + j;
        if (d >= D) break;                                      // block-uniform
        float acc[16];
#pragma unroll
        for (int o = 0; o < 16; ++o) acc[o] = 0.f;
        // taps kept rolled: unrolled, hipcc hoists every (wave-uniform) weight read into registers and spills.
        // Chain: in-plane tap, then stacked channel kd * CIN + c (input slice j + kd of the staged ones)
#pragma unroll 1
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll 1
            for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                for (int sc = 0; sc < CS; ++sc) {
                    const int kd = sc / CIN, c = sc % CIN;
                    const float xv = xs[((j + kd) * HP + (py + ky) * HALO_W + px + kx) * CIN + c];
                    const float *wr = wsl + ((ky * 3 + kx) * CS + sc) * 16;
#pragma unroll
                    for (int o = 0; o < 16; ++o) acc[o] = __builtin_fmaf(wr[o], xv, acc[o]);
                }
        if (gy < H && gx < W) {
            float *yo = a.y + ((((size_t)n * D + d) * H + gy) * W + gx) * Cout + n0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (n0 + q * 4 >= Cout) break;
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int o = q * 4 + e;
                    v[e] = sq_act(a.bias ? acc[o] + bq[o] : acc[o], a.act);
                }
                *reinterpret_cast<float4 *>(yo + q * 4) = make_float4(v[0], v[1], v[2], v[3]);
            }
        }
    }
}

int64_t ntiles3(int N, int D, int H, int W) { return (int64_t)((W + TW - 1) / TW) * ((H + TH - 1) / TH) * N * D; }

template <int BN, int KC, bool WIN>
int launch3(const C3Args &a0, int gx, hipStream_t st) {
    using C = Cfg3<BN, KC>;
    static bool attr_set = false;
    auto kern = conv3d_mfma_f32_kernel<BN, KC, WIN>;
    if (!attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                C::LDS_BYTES) != hipSuccess) {
            sq_set_error("conv3d_mfma_f32: cannot reserve %d bytes of LDS", C::LDS_BYTES);
            return SQ_ELAUNCH;
        }
        attr_set = true;
    }
    const int gy = (a0.Cout + BN - 1) / BN;
    hipLaunchKernelGGL(kern, dim3(gx, gy), dim3(256), C::LDS_BYTES, st, a0);
    return sq_check_launch("sq_conv3d_ndhwc_fwd_f32");
}

template <bool WIN>
int dispatch3(int bn, int kc, const C3Args &a, int gx, hipStream_t st) {
    if (kc == 32) return launch3<32, 32, WIN>(a, gx, st);
    if (bn == 64) return launch3<64, 16, WIN>(a, gx, st);
    if (bn == 32) return launch3<32, 16, WIN>(a, gx, st);
    return launch3<16, 16, WIN>(a, gx, st);
}

}  // namespace

// ---- launch plan (host only; the launcher below takes its choices from here) ------------------------------------------
extern "C" int sq_conv3d_plan(int N, int D, int H, int W, int Cin, int Cout, int *out) {
    SQ_REQUIRE(out, "sq_conv3d_plan: null out");
    SQ_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "sq_conv3d_plan: bad shape");
    SQ_REQUIRE(Cin == 1 || Cin == 2 || Cin % 16 == 0,
               "sq_conv3d_plan: Cin=%d unsupported (1, 2 or a multiple of 16: the planar kernels' 3*Cin channels)", Cin);
    SQ_REQUIRE(Cout % 4 == 0, "sq_conv3d_plan: Cout=%d must be a multiple of 4", Cout);
    const int64_t cmax = Cin > Cout ? Cin : Cout;
    const int64_t slice_bytes = (int64_t)H * W * cmax * 4;
    SQ_REQUIRE(slice_bytes < LIM32, "sq_conv3d_plan: one depth slice of %d x %d x %lld channels is %lld bytes; the kernels "
               "address inside a slice with 32-bit offsets (< 2 GiB)", H, W, (long long)cmax, (long long)slice_bytes);
    const int64_t nt = ntiles3(N, D, H, W);
    SQ_REQUIRE(nt < LIM32, "sq_conv3d_plan: %lld pixel tiles exceed the 32-bit tile index", (long long)nt);
    const int64_t total_bytes = (int64_t)N * D * slice_bytes;
    for (int i = 0; i < SQ_C3P_N; ++i) out[i] = 0;
    out[SQ_C3P_ADDR] = total_bytes < LIM32 ? SQ_C3_FLAT : SQ_C3_WINDOW;
    if (Cin <= 2) {
        out[SQ_C3P_KIND] = SQ_C3_DIRECT;
        out[SQ_C3P_BN] = 16;
        out[SQ_C3P_KC] = 3 * Cin;
        out[SQ_C3P_GY] = (Cout + 15) / 16;
        out[SQ_C3P_GX] = (int)(nt / D * ((D + DB - 1) / DB));    // one block per tile and DB output slices
        return SQ_OK;
    }
    // the planar plan of the stacked layer (N*D images of 3*Cin channels): same block width and chunk rules
    const int bn = sq_plan_f32_bn(nt, Cout);
    const bool s32 = sq_plan_f32_stage32(bn, 3, 16, Cin, false);
    const int kc = s32 ? 32 : 16;
    const int gy = (Cout + bn - 1) / bn;
    const int occ = (bn >= 64 || kc == 32) ? 2 : (bn >= 32 ? 3 : 4);
    int want = (256 * occ + gy - 1) / gy;
    if (want < 1) want = 1;
    int64_t tpb = (nt + want - 1) / want;
    if (tpb < 1) tpb = 1;
    out[SQ_C3P_KIND] = SQ_C3_MFMA;
    out[SQ_C3P_BN] = bn;
    out[SQ_C3P_KC] = kc;
    out[SQ_C3P_GY] = gy;
    out[SQ_C3P_GX] = (int)((nt + tpb - 1) / tpb);
    return SQ_OK;
}

extern "C" int sq_conv3d_ndhwc_fwd_f32(const float *x, const float *w, const float *bias, float *y, int N, int D, int H,
                                       int W, int Cin, int Cout, int act, void *stream) {
    SQ_REQUIRE(x && w && y, "sq_conv3d_ndhwc_fwd_f32: null tensor pointer");
    SQ_REQUIRE(act >= SQ_ACT_NONE && act <= SQ_ACT_LEAKY, "sq_conv3d_ndhwc_fwd_f32: bad activation %d", act);
    int plan[SQ_C3P_N];
    const int rc = sq_conv3d_plan(N, D, H, W, Cin, Cout, plan);
    if (rc != SQ_OK) return rc;
    SQ_REQUIRE_ALIGNED(x); SQ_REQUIRE_ALIGNED(w); SQ_REQUIRE_ALIGNED(y);
    if (bias) SQ_REQUIRE_ALIGNED(bias);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    C3Args a = {};
    a.x = x; a.w = w; a.bias = bias; a.y = y;
    a.N = N; a.D = D; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.act = act;
    a.tiles_x = (W + TW - 1) / TW;
    a.tiles_y = (H + TH - 1) / TH;
    a.ntiles = (int)ntiles3(N, D, H, W);
    if (plan[SQ_C3P_KIND] == SQ_C3_DIRECT) {
        const dim3 grid(plan[SQ_C3P_GX], plan[SQ_C3P_GY]);
        if (Cin == 1) hipLaunchKernelGGL(conv3d_direct_f32_kernel<1>, grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL(conv3d_direct_f32_kernel<2>, grid, dim3(256), 0, st, a);
        return sq_check_launch("sq_conv3d_ndhwc_fwd_f32(direct)");
    }
    return plan[SQ_C3P_ADDR] == SQ_C3_WINDOW ? dispatch3<true>(plan[SQ_C3P_BN], plan[SQ_C3P_KC], a, plan[SQ_C3P_GX], st)
                                             : dispatch3<false>(plan[SQ_C3P_BN], plan[SQ_C3P_KC], a, plan[SQ_C3P_GX], st);
}

// ---- 2x2x2 / stride-2 VALID max pooling: thread per (output voxel, channel quad), 16-B loads and stores --------------
namespace {
__global__ __launch_bounds__(256) void maxpool2x2x2_f32_kernel(const float4 *__restrict__ x, float4 *__restrict__ y,
                                                               int D, int H, int W, int C4, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int q = (int)(i % C4);
    int64_t p = i / C4;
    const int wo = (int)(p % (W / 2)); p /= (W / 2);
    const int ho = (int)(p % (H / 2)); p /= (H / 2);
    const int dout = (int)(p % (D / 2));
    const int64_t n = p / (D / 2);
    float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int dz = k >> 2, dy = (k >> 1) & 1, dx = k & 1;
        const float4 v = x[(((n * D + 2 * dout + dz) * H + 2 * ho + dy) * (int64_t)W + 2 * wo + dx) * C4 + q];
        if (k == 0) m = v;
        else {
            m.x = v.x > m.x ? v.x : m.x;
            m.y = v.y > m.y ? v.y : m.y;
            m.z = v.z > m.z ? v.z : m.z;
            m.w = v.w > m.w ? v.w : m.w;
        }
    }
    y[i] = m;
}

// ---- 2x2x2 / stride-2 transpose convolution + bias + bridge: the 8 parity classes (a, b, c) of an output voxel are the
// 8 taps of the filter.  Thread per (input voxel, output-channel quad): one read of the input voxel's channels feeds all
// 8 x 4 chains (c ascending from +0, as the planar kernel and oracle_convT2x2s2_nhwc_f32), then + bias, then the bridge.
// The block's 256 threads share their channel quad (blockIdx.y), so the filter reads are wave-uniform.
template <int BRIDGE>
__global__ __launch_bounds__(256) void convT2x2x2_f32_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                             const float *__restrict__ bias, const float *__restrict__ skip,
                                                             float *__restrict__ y, int D, int H, int W, int Cin, int Cout,
                                                             int64_t P) {
    // the block's filter slice in LDS as wl[c][k][e] = w[k][o + e][c]: per input channel 8 broadcast float4 reads
    extern __shared__ __attribute__((aligned(16))) float wl[];
    // block -> (pixel block, channel quad) with the quad fastest, dealt so that each XCD takes a contiguous run
    // (sq_xcd_remap): the Cout / 4 blocks of one pixel block run together on one XCD, so their re-reads of the input
    // pixels hit its L2 and the 16-B pieces of an output pixel's channels reach L2 close together in time
    const int Q = Cout / 4;
    const unsigned vb = sq_xcd_remap(blockIdx.x, gridDim.x);
    const int o = (int)(vb % (unsigned)Q) * 4;
    const int64_t pblk = vb / (unsigned)Q;
    for (int idx = threadIdx.x; idx < 32 * Cin; idx += 256) {
        const int c = idx >> 5, k = (idx >> 2) & 7, e = idx & 3;
        wl[idx] = w[((size_t)k * Cout + o + e) * Cin + c];
    }
    __syncthreads();
    const int64_t p = pblk * 256 + threadIdx.x;
    if (p >= P) return;
    const float4 *xp = reinterpret_cast<const float4 *>(x + p * Cin);
    float acc[8][4];
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[k][e] = 0.f;
    for (int c4 = 0; c4 < Cin / 4; ++c4) {
        const float4 v = xp[c4];
        const float xv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float4 *wc = reinterpret_cast<const float4 *>(wl + (4 * c4 + j) * 32);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float4 wk = wc[k];
                acc[k][0] = __builtin_fmaf(wk.x, xv[j], acc[k][0]);
                acc[k][1] = __builtin_fmaf(wk.y, xv[j], acc[k][1]);
                acc[k][2] = __builtin_fmaf(wk.z, xv[j], acc[k][2]);
                acc[k][3] = __builtin_fmaf(wk.w, xv[j], acc[k][3]);
            }
        }
    }
    const int j = (int)(p % W);
    int64_t t = p / W;
    const int i = (int)(t % H); t /= H;
    const int d = (int)(t % D);
    const int64_t n = t / D;
    const float4 bq = bias ? *reinterpret_cast<const float4 *>(bias + o) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float bv[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int pa = k >> 2, pb = (k >> 1) & 1, pc = k & 1;
        const size_t ob = ((((size_t)n * 2 * D + 2 * d + pa) * 2 * H + 2 * i + pb) * (size_t)(2 * W) + 2 * j + pc) * Cout + o;
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (BRIDGE != SQ_BRIDGE_NONE) s = *reinterpret_cast<const float4 *>(skip + ob);
        const float sk[4] = {s.x, s.y, s.z, s.w};
        float r[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float v = bias ? acc[k][e] + bv[e] : acc[k][e];
            if constexpr (BRIDGE == SQ_BRIDGE_ADD) v = v + sk[e];
            if constexpr (BRIDGE == SQ_BRIDGE_MUL) v = v * sk[e];
            if constexpr (BRIDGE == SQ_BRIDGE_SUB) v = v - sk[e];
            r[e] = v;
        }
        *reinterpret_cast<float4 *>(y + ob) = make_float4(r[0], r[1], r[2], r[3]);
    }
}

unsigned grid1(int64_t n) { return (unsigned)((n + 255) / 256); }
}  // namespace

extern "C" int sq_maxpool2x2x2_fwd_f32(const float *x, float *y, int N, int D, int H, int W, int C, void *stream) {
    SQ_REQUIRE(x && y, "sq_maxpool2x2x2_fwd_f32: null tensor pointer");
    SQ_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0 && C > 0 && D % 2 == 0 && H % 2 == 0 && W % 2 == 0 && C % 4 == 0,
               "sq_maxpool2x2x2_fwd_f32: need even D,H,W and C %% 4 == 0 (got %d,%d,%d,%d)", D, H, W, C);
    SQ_REQUIRE_ALIGNED(x); SQ_REQUIRE_ALIGNED(y);
    const int64_t total = (int64_t)N * (D / 2) * (H / 2) * (W / 2) * (C / 4);
    SQ_REQUIRE(grid1(total) < (1u << 31), "sq_maxpool2x2x2_fwd_f32: volume too large");
    hipLaunchKernelGGL(maxpool2x2x2_f32_kernel, dim3(grid1(total)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const float4 *>(x), reinterpret_cast<float4 *>(y), D, H, W, C / 4, total);
    return sq_check_launch("sq_maxpool2x2x2_fwd_f32");
}

extern "C" int sq_convT2x2x2s2_ndhwc_fwd_f32(const float *x, const float *w, const float *bias, const float *skip, float *y,
                                             int N, int D, int H, int W, int Cin, int Cout, int bridge, void *stream) {
    SQ_REQUIRE(x && w && y, "sq_convT2x2x2s2_ndhwc_fwd_f32: null tensor pointer");
    SQ_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0, "sq_convT2x2x2s2_ndhwc_fwd_f32: bad shape");
    SQ_REQUIRE(Cin > 0 && Cin % 16 == 0 && Cout > 0 && Cout % 4 == 0,
               "sq_convT2x2x2s2_ndhwc_fwd_f32: Cin=%d (multiple of 16), Cout=%d (multiple of 4)", Cin, Cout);
    SQ_REQUIRE(bridge >= SQ_BRIDGE_NONE && bridge <= SQ_BRIDGE_SUB, "sq_convT2x2x2s2_ndhwc_fwd_f32: bad bridge %d", bridge);
    SQ_REQUIRE(bridge == SQ_BRIDGE_NONE || skip, "sq_convT2x2x2s2_ndhwc_fwd_f32: bridge %d needs a skip tensor", bridge);
    SQ_REQUIRE_ALIGNED(x); SQ_REQUIRE_ALIGNED(w); SQ_REQUIRE_ALIGNED(y);
    if (bias) SQ_REQUIRE_ALIGNED(bias);
    if (skip) SQ_REQUIRE_ALIGNED(skip);
    const int64_t P = (int64_t)N * D * H * W;
    SQ_REQUIRE(grid1(P) < (1u << 31), "sq_convT2x2x2s2_ndhwc_fwd_f32: volume too large");
    SQ_REQUIRE(Cin <= 1024, "sq_convT2x2x2s2_ndhwc_fwd_f32: Cin=%d above 1024 (the filter slice lives in LDS)", Cin);
    SQ_REQUIRE((int64_t)grid1(P) * (Cout / 4) < ((int64_t)1 << 31), "sq_convT2x2x2s2_ndhwc_fwd_f32: volume too large");
    const dim3 grid(grid1(P) * (unsigned)(Cout / 4));
    const size_t lds = (size_t)32 * Cin * 4;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    static bool attr_set[4] = {false, false, false, false};
    const void *kerns[4] = {reinterpret_cast<const void *>(convT2x2x2_f32_kernel<SQ_BRIDGE_NONE>),
                            reinterpret_cast<const void *>(convT2x2x2_f32_kernel<SQ_BRIDGE_ADD>),
                            reinterpret_cast<const void *>(convT2x2x2_f32_kernel<SQ_BRIDGE_MUL>),
                            reinterpret_cast<const void *>(convT2x2x2_f32_kernel<SQ_BRIDGE_SUB>)};
    if (!attr_set[bridge]) {
        if (hipFuncSetAttribute(kerns[bridge], hipFuncAttributeMaxDynamicSharedMemorySize, 32 * 1024 * 4) != hipSuccess) {
            sq_set_error("convT2x2x2_f32: cannot reserve %d bytes of LDS", 32 * 1024 * 4);
            return SQ_ELAUNCH;
        }
        attr_set[bridge] = true;
    }
    switch (bridge) {
        case SQ_BRIDGE_ADD: hipLaunchKernelGGL(convT2x2x2_f32_kernel<SQ_BRIDGE_ADD>, grid, dim3(256), lds, st, x, w, bias, skip, y, D, H, W, Cin, Cout, P); break;
        case SQ_BRIDGE_MUL: hipLaunchKernelGGL(convT2x2x2_f32_kernel<SQ_BRIDGE_MUL>, grid, dim3(256), lds, st, x, w, bias, skip, y, D, H, W, Cin, Cout, P); break;
        case SQ_BRIDGE_SUB: hipLaunchKernelGGL(convT2x2x2_f32_kernel<SQ_BRIDGE_SUB>, grid, dim3(256), lds, st, x, w, bias, skip, y, D, H, W, Cin, Cout, P); break;
        default: hipLaunchKernelGGL(convT2x2x2_f32_kernel<SQ_BRIDGE_NONE>, grid, dim3(256), lds, st, x, w, bias, nullptr, y, D, H, W, Cin, Cout, P); break;
    }
    return sq_check_launch("sq_convT2x2x2s2_ndhwc_fwd_f32");
}
