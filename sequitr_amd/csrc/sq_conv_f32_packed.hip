// The 64-channel-block form of the f32 3x3 implicit-GEMM convolution (conv_mfma_f32_v2_kernel<64,3,16,0> of sq_conv_f32_v2.hip)
// with the filter read from a per-model FRAGMENT PACK instead of being re-laid-out through registers and LDS by every block
// for every (tile, 16-channel chunk) item.  Same tile walk, same item order, the same 16 MFMAs per step on the same operand
// values in the same order: every output's fmaf chain is the one of the unpacked kernel, so the results are bit-identical.
//   * the pack (sq_conv_pack_filter_f32) is a permutation of the stored (3,3,Cin,Cout) weights: for each (64-channel block, chunk,
//     tap, 4-channel k-step) the 64 lanes' four A values as one float4 per lane -- one MFMA step's A operands are ONE
//     buffer_load_b128 per lane, 1 KiB contiguous per wave, the steps of a block's walk consecutive in memory;
//   * the A operands ride in a register ring RING steps ahead that runs on across item and tile boundaries (the stream of a
//     block is periodic in the tile: chunk 0 follows the last chunk);
//   * the LDS the weight slab occupied double-buffers the halo: the next item's halo is loaded at the top of an item and
//     written into the other buffer during the later MFMA steps, so an item costs ONE barrier and has no commit phase.
// vmcnt is one in-order counter for loads and stores: the halo loads of the next item are issued in front of the item's ring
// loads, and the ring's loads for the first steps of the next item are in flight before the epilogue's stores are issued.
#include <stdlib.h>
#include <type_traits>
#include "sq_common.h"
#include "sq_conv_epi.h"

#ifndef SQ_PK_RING
#define SQ_PK_RING 4             // A-operand steps in flight (divides the 36 steps of an item: the ring slot of a step is static)
#endif
#ifndef SQ_PK_OCC
#define SQ_PK_OCC 2              // resident blocks per CU = the unpacked 64-channel form's, so both walk the same grid (3: an experiment,
#endif                           // HISTORY.md; it is another walk and would need a form code of its own in sq_conv_walk_plan)
#ifndef SQ_PK_WRITE_AT
#define SQ_PK_WRITE_AT 22        // first MFMA step that writes a slot of the next halo into the other buffer (one slot per step)
#endif

namespace {

constexpr int TH = 16, TW = 16, BN = 64, KC = 16, NR = BN / 16;
constexpr int HALO_W = TW + 2, HALO_H = TH + 2, HP = HALO_W * HALO_H;
constexpr int PS = KC + 2;                                  // pixel stride (floats): conflict-free B reads, as Cfg2
constexpr int XS_FLOATS = HP * PS;
constexpr int QPP = KC / 4, XITEMS = HP * QPP, XSLOTS = (XITEMS + 255) / 256;
constexpr int NSTEP = 9 * (KC / 4);                         // 36 MFMA steps per item
constexpr int RING = SQ_PK_RING;
constexpr int STEP_BYTES = 64 * 16, ITEM_BYTES = NSTEP * STEP_BYTES;
constexpr int LDS_BYTES = (2 * XS_FLOATS + 64 * 4) * 4;       // two halo images + the dump row of put_slot
constexpr int OCC = SQ_PK_OCC;
static_assert(SQ_PK_OCC != 2 || sq_v2_occ(BN, KC, false) == 2, "the default walks the unpacked form's grid");
static_assert(NSTEP % RING == 0 && RING >= 2 && RING <= 6, "the ring slot of a step must not depend on the item");
static_assert(SQ_PK_WRITE_AT + XSLOTS <= NSTEP, "the halo writes must fit the item's steps");
static_assert((XS_FLOATS * 4) % 16 == 0, "second halo buffer must start 16-B aligned");

// one thread per float4 of the pack: e = (((cb * nchunk + c) * 9 + tap) * 4 + s) * 64 + lane, lane = 16 kk + li
__global__ __launch_bounds__(256) void pack_filter_f32_kernel(const float *__restrict__ w, float4 *__restrict__ wp,
                                                              int Cin, int Cout, int total) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int lane = e & 63, li = lane & 15, kk = lane >> 4;
    int t = e >> 6;
    const int s = t & 3;
    t >>= 2;
    const int tap = t % 9;
    t /= 9;
    const int nchunk = Cin / KC, c = t % nchunk, cb = t / nchunk;
    const float *src = w + (size_t)(tap * Cin + c * KC + 4 * s + kk) * Cout + cb * BN + li;
    wp[e] = make_float4(src[0], src[16], src[32], src[48]);
}

__global__ __launch_bounds__(256, OCC) void conv_mfma_f32_packed_kernel(
    const float *__restrict__ x, const float *__restrict__ wp, const float *__restrict__ bias, float *__restrict__ y,
    int N, int H, int W, int Cin, int Cout, int act, int tiles_x, int tiles_y, int ntiles, float *__restrict__ pooled) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    __builtin_assume(tid < 256);
    const int li = lane & 15, kk = lane >> 4;
    const int n0 = blockIdx.y * BN;
    const int vb = (int)sq_xcd_remap(blockIdx.x, gridDim.x);
    // block b takes tiles b, b + G, b + 2G, ... (the walk of conv_mfma_f32_v2_kernel)
    const int tstride = (int)gridDim.x;
    const int t_begin = vb;
    if (t_begin >= ntiles) return;
    const int t_count = (ntiles - vb + tstride - 1) / tstride;
    const int nchunk = Cin / KC;
    const int nitems = t_count * nchunk;

    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(x), 0, (int)((size_t)N * H * W * Cin * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(wp), 0, 9 * Cin * Cout * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t yrsrc = __builtin_amdgcn_make_buffer_rsrc(y, 0, (int)((size_t)N * H * W * Cout * 4), 0x00020000);
    constexpr unsigned OOB = 0x80000000u;   // tensors are < 2 GiB (checked on the host)

    // per-thread, tile-independent part of the halo addresses; a slot past the halo's 1296 quads sits at a row no image has
    int xrel[XSLOTS], xpy[XSLOTS], xpx[XSLOTS];
#pragma unroll
    for (int sl = 0; sl < XSLOTS; ++sl) {
        const int idx = tid + sl * 256;
        const int pix = idx / QPP, q = idx % QPP;
        xpy[sl] = idx < XITEMS ? pix / HALO_W : (1 << 24);
        xpx[sl] = pix % HALO_W;
        xrel[sl] = idx < XITEMS ? ((pix / HALO_W * W + xpx[sl]) * Cin + q * 4) * 4 : (int)OOB;
    }
    float4 xr[XSLOTS];
    // global loads of one item's halo into registers.  ONE straight-line path: behind an if / else of two address forms (the
    // unpacked kernel's SGPR-offset form for interior halos) the compiler merges the two paths' pending loads conservatively
    // and waits for the halo at the item's first MFMA step -- vmcnt(4) where this form gets vmcnt(9).
    // live == false: every offset out of range, nothing is fetched
    auto issue = [&](int tx, int ty, int n, int cc, bool live) {
        const int x0 = tx * TW - 1, y0 = ty * TH - 1;
        const int base = (((n * H + y0) * W + x0) * Cin + cc) * 4;          // may be "negative": wraps back
        const unsigned Hl = live ? (unsigned)H : 0u;                        // no row is inside a dead item
#pragma unroll
        for (int sl = 0; sl < XSLOTS; ++sl) {
            const bool inb = (unsigned)(y0 + xpy[sl]) < Hl && (unsigned)(x0 + xpx[sl]) < (unsigned)W;
            const unsigned off = inb ? (unsigned)(base + xrel[sl]) : OOB;
            const auto v = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, off, 0, 0);
            xr[sl] = *reinterpret_cast<const float4 *>(&v);
        }
    };
    // one slot of the halo registers -> the LDS image `xs` (same index map as the unpacked kernel's commit()).  The last slot's
    // lanes past the halo's 1296 quads write their (zero) quad into a dump row behind the two images instead of skipping the
    // write: a conditional write lets the compiler sink that slot's LOAD down to it, where it then waits vmcnt(0)
    float *const dump = smem + 2 * XS_FLOATS + lane * 4;
    auto put_slot = [&](float *xs, int sl) {
        const int idx = tid + sl * 256;
        const int pix = idx / QPP, q = idx % QPP;
        float *d = idx < XITEMS ? xs + pix * PS + q * 4 : dump;
        *reinterpret_cast<float2 *>(d) = make_float2(xr[sl].x, xr[sl].y);
        *reinterpret_cast<float2 *>(d + 2) = make_float2(xr[sl].z, xr[sl].w);
    };

    // A operands: step `st` of the item whose 36 KiB start at byte `item_off` of the pack
    const int a_lane = lane * 16;
    auto load_a = [&](int item_off, int st) {
        const auto v = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, a_lane, item_off + st * STEP_BYTES, 0);
        return *reinterpret_cast<const float4 *>(&v);
    };
    const int xb_off = ((4 * wv) * HALO_W + li) * PS + kk;
    auto load_b = [&](const float *xs, int st, float (&b)[4]) {
        const int tap = st / 4, s = st % 4;
        const int ky = tap / 3, kx = tap % 3;
#pragma unroll
        for (int r = 0; r < 4; ++r) b[r] = xs[xb_off + ((r + ky) * HALO_W + kx) * PS + s * 4];
    };

    const float slope = act == SQ_ACT_LEAKY ? 0.2f : 1.0f;
    const bool is_relu = act == SQ_ACT_RELU;
    auto actk = [&](float v, auto fastc) {
        if constexpr (decltype(fastc)::value) return __builtin_fmaxf(v, 0.0f);       // NaN -> 0, -0 -> +0, as v > 0 ? v : 0
        else {
            const float neg = is_relu ? 0.0f : v * slope;
            return v > 0.0f ? v : neg;
        }
    };
    float4 bvr[NR];
#pragma unroll
    for (int nb = 0; nb < NR; ++nb)
        bvr[nb] = bias ? *reinterpret_cast<const float4 *>(bias + n0 + nb * 16 + 4 * kk) : make_float4(0.f, 0.f, 0.f, 0.f);
    const int fast_lane = (((4 * wv) * W + li) * Cout + 4 * kk) * 4;    // the lane's part of a full tile's output offsets

    f32x4 acc[4][NR];
    // the epilogue of conv_mfma_f32_v2_kernel<64,3,16,0> (store, + 2x2 max-pool), value for value
    auto epilogue = [&](int tx, int ty, int n, auto fastc) {
        constexpr bool FAST = decltype(fastc)::value;
        auto actf = [&](float v) { return actk(v, fastc); };
        const int gx = tx * TW + li;
#pragma unroll
        for (int nb = 0; nb < NR; ++nb) {
            const int co = n0 + nb * 16 + 4 * kk;
            const float4 bv = bvr[nb];
            f32x4 o[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gy = ty * TH + 4 * wv + r;
                o[r][0] = actf(bias ? acc[r][nb][0] + bv.x : acc[r][nb][0]);
                o[r][1] = actf(bias ? acc[r][nb][1] + bv.y : acc[r][nb][1]);
                o[r][2] = actf(bias ? acc[r][nb][2] + bv.z : acc[r][nb][2]);
                o[r][3] = actf(bias ? acc[r][nb][3] + bv.w : acc[r][nb][3]);
                unsigned off;
                if constexpr (FAST) {
                    off = (unsigned)(fast_lane + nb * 64) + (unsigned)((((n * H + ty * TH + r) * W + tx * TW) * Cout + n0) * 4);
                } else {
                    const bool ok = gy < H && gx < W;
                    off = ok ? (unsigned)((((n * H + gy) * W + gx) * Cout + co) * 4) : OOB;
                }
                __builtin_amdgcn_raw_buffer_store_b128(
                    *reinterpret_cast<__attribute__((__vector_size__(4 * sizeof(unsigned)))) unsigned *>(&o[r]), yrsrc, off, 0, 0);
                acc[r][nb] = (f32x4){0.f, 0.f, 0.f, 0.f};      // ready for the next tile
            }
            if (pooled) {                                       // rows (0,1) and (2,3) in registers, x-neighbour = lane ^ 1
#pragma unroll
                for (int pr = 0; pr < 2; ++pr) {
                    float mp[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float a = o[2 * pr][j], b = o[2 * pr + 1][j];
                        const float v = b > a ? b : a;
                        const float u = __shfl_xor(v, 1);
                        mp[j] = u > v ? u : v;
                    }
                    const int py = (ty * TH + 4 * wv) / 2 + pr, px = gx >> 1;
                    if ((li & 1) == 0 && py < (H >> 1) && px < (W >> 1))
                        *reinterpret_cast<float4 *>(pooled + ((size_t)(n * (H >> 1) + py) * (W >> 1) + px) * Cout + co) =
                            make_float4(mp[0], mp[1], mp[2], mp[3]);
                }
            }
        }
    };

    // tile coordinates advance by carries, as in the unpacked kernel
    const int per_image = tiles_x * tiles_y;
    const int s_n = tstride / per_image, s_y = (tstride % per_image) / tiles_x, s_x = (tstride % per_image) % tiles_x;
    int ctx = t_begin % tiles_x, cty = (t_begin / tiles_x) % tiles_y, cn = t_begin / per_image;   // the tile being multiplied
    int ntx = ctx + s_x, nty = cty, nn = cn;                                                      // the next one of the walk
    if (ntx >= tiles_x) { ntx -= tiles_x; nty += 1; }
    nty += s_y;
    if (nty >= tiles_y) { nty -= tiles_y; nn += 1; }
    nn += s_n;

    // prologue: the first item's halo into buffer 0, the ring's first RING steps in flight
    const int cb_off = blockIdx.y * nchunk * ITEM_BYTES;       // this channel block's part of the pack
    issue(ctx, cty, cn, 0, true);
    float4 ar[RING];
#pragma unroll
    for (int j = 0; j < RING; ++j) ar[j] = load_a(cb_off, j);
#pragma unroll
    for (int sl = 0; sl < XSLOTS; ++sl) put_slot(smem, sl);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int nb = 0; nb < NR; ++nb) acc[r][nb] = (f32x4){0.f, 0.f, 0.f, 0.f};
    __syncthreads();

    int chunk = 0;
    for (int it = 0; it < nitems; ++it) {
        const float *xs = smem + (it & 1) * XS_FLOATS;          // this item's halo
        float *xo = smem + ((it & 1) ^ 1) * XS_FLOATS;          // the next item's
        int nchk = chunk + 1;
        const bool same = nchk != nchunk;                       // the next item stays on this tile
        if (!same) nchk = 0;
        const bool has_next = it + 1 < nitems;
        // the next item's halo first: vmcnt retires in order, so everything the ring loads below it is waited for after it
        issue(same ? ctx : ntx, same ? cty : nty, same ? cn : nn, nchk * KC, has_next);
        const int item_off = cb_off + chunk * ITEM_BYTES, next_off = cb_off + nchk * ITEM_BYTES;   // the stream wraps: always in range
        {
            float b0[4], b1[4];
            load_b(xs, 0, b0);
            __builtin_amdgcn_s_setprio(0);
#pragma unroll
            for (int st = 0; st < NSTEP; ++st) {
                float (&bc)[4] = (st & 1) ? b1 : b0;
                float (&bn)[4] = (st & 1) ? b0 : b1;
                const float4 a = ar[st % RING];
                if (st + 1 < NSTEP) load_b(xs, st + 1, bn);
                if (st >= SQ_PK_WRITE_AT && st < SQ_PK_WRITE_AT + XSLOTS) put_slot(xo, st - SQ_PK_WRITE_AT);
                __builtin_amdgcn_sched_barrier(0);
                const float av[NR] = {a.x, a.y, a.z, a.w};
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int nb = 0; nb < NR; ++nb)
                        acc[r][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[nb], bc[r], acc[r][nb], 0, 0, 0);
                // refill the slot just consumed: step st + RING of the stream (past the item: the next item's first steps)
                ar[st % RING] = st + RING < NSTEP ? load_a(item_off, st + RING) : load_a(next_off, st + RING - NSTEP);
                __builtin_amdgcn_sched_barrier(0);
            }
            __builtin_amdgcn_s_setprio(3);
        }
        // the ONE barrier of the item: every wave has read this item's halo and written its part of the next one
        __syncthreads();
        if (!same) {
            const bool fast = is_relu && cty * TH + TH <= H && ctx * TW + TW <= W;
            if (fast) epilogue(ctx, cty, cn, std::integral_constant<bool, true>{});
            else epilogue(ctx, cty, cn, std::integral_constant<bool, false>{});
            ctx = ntx; cty = nty; cn = nn;                      // the walk moves on by one tile stride
            ntx += s_x;
            if (ntx >= tiles_x) { ntx -= tiles_x; nty += 1; }
            nty += s_y;
            if (nty >= tiles_y) { nty -= tiles_y; nn += 1; }
            nn += s_n;
        }
        chunk = nchk;
    }
}

bool packed_switch_on() {
    const char *e = getenv("SQ_CONV_PACKED");                   // SQ_CONV_PACKED=0: A/B switch back to the unpacked kernel; read per
    return !(e && e[0] == '0');                                 // call: the parity tests flip it in-process
}

bool pack_eligible(int K, int Cin, int Cout) { return K == 3 && Cin > 0 && Cin % KC == 0 && Cout > 0 && Cout % BN == 0; }

}  // namespace

extern "C" int64_t sq_conv_packed_filter_elems_f32(int K, int Cin, int Cout) {
    return pack_eligible(K, Cin, Cout) ? (int64_t)9 * Cin * Cout : -1;
}

extern "C" int sq_conv_pack_filter_f32(const float *w, float *wp, int K, int Cin, int Cout, void *stream) {
    SQ_REQUIRE(w && wp, "sq_conv_pack_filter_f32: null pointer");
    SQ_REQUIRE(pack_eligible(K, Cin, Cout), "sq_conv_pack_filter_f32: unsupported K=%d Cin=%d Cout=%d (3x3, Cin %% 16 == 0, Cout %% 64 == 0)",
               K, Cin, Cout);
    SQ_REQUIRE((int64_t)9 * Cin * Cout * 4 < ((int64_t)1 << 31), "sq_conv_pack_filter_f32: the pack must be < 2 GiB");
    SQ_REQUIRE_ALIGNED(w); SQ_REQUIRE_ALIGNED(wp);
    const int total = 9 * Cin * Cout / 4;
    hipLaunchKernelGGL(pack_filter_f32_kernel, dim3((total + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       w, reinterpret_cast<float4 *>(wp), Cin, Cout, total);
    return sq_check_launch("sq_conv_pack_filter_f32");
}

// does a call that brings a pack run the packed kernel?  (host only: the eligibility of the pack, the plan's 64-channel blocks,
// tensors below 2 GiB, the SQ_CONV_PACKED switch)  No shape on that plan is held back: each of the workload's ten is 2.8-5.7 % faster than the
// unpacked kernel, beyond its own spread (profiles/conv_packed_ab.json); a shape that measures otherwise gets its test here.
extern "C" int sq_conv_packed_takes_f32(int N, int H, int W, int Cin, int Cout, int K) {
    if (N <= 0 || H <= 0 || W <= 0 || !pack_eligible(K, Cin, Cout) || !packed_switch_on()) return 0;
    // 32-bit buffer offsets, as the unpacked persistent kernel: a tensor of 2 GiB or more runs what it runs today (the plain
    // entry's 64-bit-addressed kernel; the pooled entry refuses it)
    if ((size_t)N * H * W * (size_t)(Cin > Cout ? Cin : Cout) * 4 >= ((size_t)1 << 31)) return 0;
    const int64_t ntiles = (int64_t)((W + TW - 1) / TW) * ((H + TH - 1) / TH) * N;
    return sq_plan_f32_bn(ntiles, Cout) == 64 ? 1 : 0;
}

// the packed launch behind sq_conv2d_packed_nhwc_fwd_f32 / sq_conv3x3_pool_packed_fwd_f32 (arguments validated there)
static int sq_conv_packed_launch(const float *x, const float *wp, const float *bias, float *y, float *pooled, int N, int H, int W,
                          int Cin, int Cout, int act, hipStream_t st) {
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(conv_mfma_f32_packed_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES) != hipSuccess) {
            sq_set_error("conv_mfma_f32_packed: cannot reserve %d bytes of LDS", LDS_BYTES);
            return SQ_ELAUNCH;
        }
        attr_set = true;
    }
    const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
    const int ntiles = tiles_x * tiles_y * N;
    const int gy = Cout / BN;
    int tpb;
    const int gx = sq_plan_v2_grid(ntiles, gy, OCC, &tpb);      // the grid of the unpacked 64-channel form
    hipLaunchKernelGGL(conv_mfma_f32_packed_kernel, dim3(gx, gy), dim3(256), LDS_BYTES, st, x, wp, bias, y, N, H, W, Cin, Cout,
                       act, tiles_x, tiles_y, ntiles, pooled);
    return sq_check_launch("sq_conv2d_packed_nhwc_fwd_f32");
}

namespace {
// a packed call's own argument checks (the unpacked entry points check theirs; sq_conv_packed_takes_f32 has seen the sizes)
int packed_args_ok(const char *who, const float *x, const float *wp, const float *bias, const float *y, const float *pooled,
                   int N, int H, int W, int Cin, int Cout, int act) {
    SQ_REQUIRE(x && y, "%s: null tensor pointer", who);
    SQ_REQUIRE(act >= SQ_ACT_NONE && act <= SQ_ACT_LEAKY, "%s: bad activation %d", who, act);
    SQ_REQUIRE_ALIGNED(x); SQ_REQUIRE_ALIGNED(wp); SQ_REQUIRE_ALIGNED(y);
    if (bias) SQ_REQUIRE_ALIGNED(bias);
    if (pooled) SQ_REQUIRE_ALIGNED(pooled);
    return SQ_OK;
}
}  // namespace

// sq_conv2d_nhwc_fwd_f32 with the filter's fragment pack beside it: wp = sq_conv_pack_filter_f32(w) or NULL.  Where the pack is
// not used (NULL, wscale != 1, SQ_CONV_IMPL=1, a call sq_conv_packed_takes_f32 declines) this IS sq_conv2d_nhwc_fwd_f32 on w.  Same bits.
extern "C" int sq_conv2d_packed_nhwc_fwd_f32(const float *x, const float *w, const float *wp, const float *bias, float *y,
                                             int N, int H, int W, int Cin, int Cout, int K, float wscale, int act, void *stream) {
    // SQ_CONV_IMPL=1 (sq_conv_f32.hip: the plain entry's switch back to the first MFMA kernel, read once) holds for this entry too
    static const bool impl1 = [] { const char *e = getenv("SQ_CONV_IMPL"); return e && e[0] == '1'; }();
    if (!wp || wscale != 1.0f || impl1 || !sq_conv_packed_takes_f32(N, H, W, Cin, Cout, K))
        return sq_conv2d_nhwc_fwd_f32(x, w, bias, y, N, H, W, Cin, Cout, K, wscale, act, stream);
    const int rc = packed_args_ok("sq_conv2d_packed_nhwc_fwd_f32", x, wp, bias, y, nullptr, N, H, W, Cin, Cout, act);
    if (rc != SQ_OK) return rc;
    return sq_conv_packed_launch(x, wp, bias, y, nullptr, N, H, W, Cin, Cout, act, reinterpret_cast<hipStream_t>(stream));
}

// sq_conv3x3_pool_fwd_f32 with the filter's fragment pack beside it (same rule)
extern "C" int sq_conv3x3_pool_packed_fwd_f32(const float *x, const float *w, const float *wp, const float *bias, float *y,
                                              float *pooled, int N, int H, int W, int Cin, int Cout, int act, void *stream) {
    if (!wp || !pooled || H % 2 || W % 2 || !sq_conv_packed_takes_f32(N, H, W, Cin, Cout, 3))
        return sq_conv3x3_pool_fwd_f32(x, w, bias, y, pooled, N, H, W, Cin, Cout, act, stream);
    const int rc = packed_args_ok("sq_conv3x3_pool_packed_fwd_f32", x, wp, bias, y, pooled, N, H, W, Cin, Cout, act);
    if (rc != SQ_OK) return rc;
    return sq_conv_packed_launch(x, wp, bias, y, pooled, N, H, W, Cin, Cout, act, reinterpret_cast<hipStream_t>(stream));
}
