// The 32 -> 32 channel 3x3 convolutions of the f32 U-Net at level 1 (down1/conv2 + pool, up1/conv1, up1/conv2: 256^2 tiles
// at the benchmark shape) -- the same arithmetic and the same fmaf chains as conv_mfma_f32_v2_kernel<32, 3, 32, 0>
// (bit-identical results), built like the level-0 kernel (sq_conv_f32_l0.hip) round the filter in REGISTERS:
//   * a 32 -> 32 layer has one 32-channel chunk and one channel block, so the filter never changes across a block's tiles.
//     A wave owns ONE 16-channel output tile and 8 pixel rows (waves 0/1: channels 0-15 / 16-31 of rows 0-7, waves 2/3: rows
//     8-15) and holds its 72 A fragments (9 taps x 8 four-channel steps) for the whole launch, loaded once from the stored
//     HWIO tensor: no weight slab in LDS, no A reads;
//   * the halo image is channel-TRANSPOSED, [pixel][16-channel half][kk][s] = channel 16 half + 4 s + kk, 40 floats per pixel
//     (the stride of the level-0 UP form's low-resolution patch): one ds_read_b128 hands a lane its B operands of the four
//     channel steps of a tap and half, conflict-free.  The chain of an output is chunk (half) -> tap -> channel, so the wave
//     walks its 10 halo rows once per half: 60 ds_read_b128 per tile where the generic form issues 432 ds_read_b32;
//   * a thread stages (pixel, half) items: four 16-byte loads of 16 consecutive channels, transposed by register naming
//     alone, four 16-byte LDS writes.  ONE straight-line load path with the bounds folded into the offset, and the items past
//     the halo write into a dump row instead of skipping the write (the two compiler lessons of sq_conv_f32_packed.hip);
//   * with the slab gone the halo (51 840 B) fits two blocks per CU single-buffered; the next tile's halo is prefetched into
//     registers under the MFMA phase, as in the level-0 plain form;
//   * the stores of a tile ride in the MFMA phase of the NEXT tile: output row r is first overwritten at step r of the next
//     phase, so row r + 1 is biased, ReLU'd (v_max) and stored behind the MFMAs of step r (row 0 from a copy of its four
//     accumulators), and the next halo's loads are issued behind step 8.  What is left between two MFMA phases of a block is
//     wait, barrier, 12 LDS writes, barrier: with two blocks per CU the waves of a SIMD take turns at the matrix pipe, and
//     every cycle both spend outside their MFMA phases is a cycle the pipe stands still (tools/conv_ablation.py timeline r32:
//     the epilogue between the phases cost 12 % of the launch).  Only a block's last tile has an epilogue of its own;
//   * the epilogue is compiled per kind (store / store + 2x2 max-pool), 16-byte stores with the tile offset in the VGPR
//     (the store hazard noted in sq_conv_f32_l0.hip), offsets out of range while there is no previous tile.
// It walks the grid of the generic form (sq_plan_v2_grid at two blocks per CU, block b takes tiles b, b + G, ...), so
// sq_conv_walk_plan describes it too.  Which calls it takes: sq_plan_r32_takes (sq_conv_plan.hip); SQ_CONV_R32=0 is the A/B
// switch back to the generic kernel.
#include "sq_common.h"
#include "sq_conv_epi.h"

#ifndef SQ_R32_SETPRIO
#define SQ_R32_SETPRIO 1             // wave priority low while feeding the matrix pipe, high while staging / storing (A/B switch)
#endif

namespace {

constexpr int TH = 16, TW = 16, HWD = 18, HP = HWD * HWD;
constexpr int C = 32;
constexpr int PS = 40;                          // floats per halo pixel: [half][kk][s] + 8 of padding (conflict-free b128)
constexpr int XS_FLOATS = HP * PS;              // 12960 floats = 51840 B
constexpr int XITEMS = HP * 2, XSLOTS = 3;      // 648 (pixel, half) items over 256 threads
constexpr int DUMP_FLOATS = 64 * 16;            // where the items past the halo write: 16 floats per lane
constexpr int LDS_BYTES = (XS_FLOATS + DUMP_FLOATS) * 4;
constexpr int ROWS = 8, HROWS = ROWS + 2;       // output rows and halo rows of a wave
constexpr int OCC = 2;
constexpr unsigned OOB = 0x80000000u;
static_assert(sq_v2_occ(32, 32, false) == OCC, "the kernel walks the grid of the generic <32,3,32,0> form");

enum { EPI_STORE = 0, EPI_POOL = 1 };

struct R32Args {
    const float *x, *w, *bias;
    float *y, *pooled;
    int N, H, W;
    int tiles_x, tiles_y, ntiles;
    int gx, gy, gn;                             // the grid stride G = gn * tiles_x * tiles_y + gy * tiles_x + gx
};

struct Pos { int tx, ty, n; };

typedef unsigned u32x4 __attribute__((__vector_size__(4 * sizeof(unsigned))));

__device__ __forceinline__ float relu(float v) { return __builtin_fmaxf(v, 0.0f); }   // NaN -> 0, -0 -> +0 like (v > 0 ? v : 0)

template <int EPI>
__global__ __launch_bounds__(256, OCC) void conv_r32_kernel(const R32Args a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *xs = smem;

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    __builtin_assume(tid < 256);
    const int li = lane & 15, kk = lane >> 4;
    const int nb = wv & 1, rh = wv >> 1;        // the wave's 16-channel output tile and its half of the pixel rows
    const int H = a.H, W = a.W;
    const int G = (int)gridDim.x;
    const int vb = (int)sq_xcd_remap(blockIdx.x, gridDim.x);
    if (vb >= a.ntiles) return;
    const int t_count = (a.ntiles - vb + G - 1) / G;

    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(a.x), 0, (int)((size_t)a.N * H * W * C * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t yrsrc = __builtin_amdgcn_make_buffer_rsrc(
        a.y, 0, (int)((size_t)a.N * H * W * C * 4), 0x00020000);

    // ---- the filter, once per launch: A[m = output channel 16 nb + li][k = channel 4 k8 + kk] of tap t (k8 = 4 chunk + s)
    float af[9][8];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int k8 = 0; k8 < 8; ++k8) af[t][k8] = a.w[(t * C + 4 * k8 + kk) * C + nb * 16 + li];
    const float4 bv = a.bias ? *reinterpret_cast<const float4 *>(a.bias + nb * 16 + 4 * kk) : make_float4(0.f, 0.f, 0.f, 0.f);

    auto decode = [&](int tile) {
        Pos p;
        p.tx = tile % a.tiles_x;
        p.ty = (tile / a.tiles_x) % a.tiles_y;
        p.n = tile / (a.tiles_x * a.tiles_y);
        return p;
    };
    auto advance = [&](Pos p) {                 // tile + G, by carries
        p.tx += a.gx;
        if (p.tx >= a.tiles_x) { p.tx -= a.tiles_x; p.ty += 1; }
        p.ty += a.gy;
        if (p.ty >= a.tiles_y) { p.ty -= a.tiles_y; p.n += 1; }
        p.n += a.gn;
        return p;
    };

    // ---- halo loads: thread -> (pixel, 16-channel half) items, 4 x 16 B each; an item past the halo sits at a row no image has
    float4 xr[XSLOTS][4];
    int xrel[XSLOTS], xpy[XSLOTS], xpx[XSLOTS];
#pragma unroll
    for (int sl = 0; sl < XSLOTS; ++sl) {
        const int idx = tid + sl * 256, pix = idx >> 1, hf = idx & 1;
        xpy[sl] = idx < XITEMS ? pix / HWD : (1 << 24);
        xpx[sl] = pix % HWD;
        xrel[sl] = idx < XITEMS ? ((pix / HWD * W + xpx[sl]) * C + hf * 16) * 4 : (int)OOB;
    }
    // live == false: every offset out of range, nothing is fetched
    auto issue_halo = [&](const Pos &p, bool live) {
        const int x0 = p.tx * TW - 1, y0 = p.ty * TH - 1;
        const int base = (((p.n * H + y0) * W + x0) * C) * 4;       // may be "negative" on the top / left border: wraps back
        const unsigned Hl = live ? (unsigned)H : 0u;
#pragma unroll
        for (int sl = 0; sl < XSLOTS; ++sl) {
            const bool inb = (unsigned)(y0 + xpy[sl]) < Hl && (unsigned)(x0 + xpx[sl]) < (unsigned)W;
            const unsigned off = inb ? (unsigned)(base + xrel[sl]) : OOB;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const auto v = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, off + q * 16, 0, 0);   // OOB + 48 is still past every tensor
                xr[sl][q] = *reinterpret_cast<const float4 *>(&v);
            }
        }
    };
    // channel 4 s + j of the half (register j of load s) -> [kk = j][s]: the transpose is the registers' naming
    float *cw[XSLOTS];
#pragma unroll
    for (int sl = 0; sl < XSLOTS; ++sl) {
        const int idx = tid + sl * 256;
        cw[sl] = idx < XITEMS ? xs + (idx >> 1) * PS + (idx & 1) * 16 : smem + XS_FLOATS + lane * 16;
    }
    auto commit_halo = [&]() {
#pragma unroll
        for (int sl = 0; sl < XSLOTS; ++sl) {
            float *d = cw[sl];
            *reinterpret_cast<float4 *>(d) = make_float4(xr[sl][0].x, xr[sl][1].x, xr[sl][2].x, xr[sl][3].x);
            *reinterpret_cast<float4 *>(d + 4) = make_float4(xr[sl][0].y, xr[sl][1].y, xr[sl][2].y, xr[sl][3].y);
            *reinterpret_cast<float4 *>(d + 8) = make_float4(xr[sl][0].z, xr[sl][1].z, xr[sl][2].z, xr[sl][3].z);
            *reinterpret_cast<float4 *>(d + 12) = make_float4(xr[sl][0].w, xr[sl][1].w, xr[sl][2].w, xr[sl][3].w);
        }
    };

    // ---- the 3x3 convolution of one tile: per 16-channel half c the wave walks halo rows h = 0 .. 9 of its 8 output rows;
    // row h feeds tap row ky of output row r = h - ky.  Per output the order is c, ky, kx, channel: the chain of the oracle
    f32x4 acc[ROWS];
    const float *xb = xs + ((ROWS * rh) * HWD + li) * PS + 4 * kk;
    // after_step(st): what rides behind the MFMAs of step st (the previous tile's stores, the next halo's loads)
    auto mfma_phase = [&](auto &&after_step) {
        float4 bq[2][3];
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) bq[0][kx] = *reinterpret_cast<const float4 *>(xb + kx * PS);
#if SQ_R32_SETPRIO
        __builtin_amdgcn_s_setprio(0);
#endif
#pragma unroll
        for (int st = 0; st < 2 * HROWS; ++st) {
            const int c = st / HROWS, h = st % HROWS;
            if (st + 1 < 2 * HROWS) {
                const int c1 = (st + 1) / HROWS, h1 = (st + 1) % HROWS;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
                    bq[(st + 1) & 1][kx] = *reinterpret_cast<const float4 *>(xb + (h1 * HWD + kx) * PS + c1 * 16);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const float4 q = bq[st & 1][kx];
                const float b[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int s = 0; s < 4; ++s) {
#pragma unroll
                    for (int ky = 2; ky >= 0; --ky) {                // oldest output row first
                        const int r = h - ky;
                        if (r < 0 || r >= ROWS) continue;
                        const bool first = c == 0 && ky == 0 && kx == 0 && s == 0;
                        acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[ky * 3 + kx][4 * c + s], b[s],
                                                                      first ? (f32x4){0.f, 0.f, 0.f, 0.f} : acc[r], 0, 0, 0);
                    }
                }
            }
            after_step(st);
            __builtin_amdgcn_sched_barrier(0);
        }
#if SQ_R32_SETPRIO
        __builtin_amdgcn_s_setprio(3);
#endif
    };

    // ---- the epilogue of a block's LAST tile: lane (li, kk) holds channels 16 nb + 4 kk .. + 3 of pixel column li of its 8 rows
    const int Hl = H >> 1, Wl = W >> 1;
    const int yvoff = (((ROWS * rh) * W + li) * C + nb * 16 + 4 * kk) * 4;
    const __amdgpu_buffer_rsrc_t prsrc = __builtin_amdgcn_make_buffer_rsrc(
        a.pooled, 0, EPI == EPI_POOL ? (int)((size_t)a.N * Hl * Wl * C * 4) : 0, 0x00020000);
    const int pvoff = (((ROWS / 2 * rh) * Wl + (li >> 1)) * C + nb * 16 + 4 * kk) * 4;
    auto epilogue = [&](const Pos &p) {
        float o[ROWS][4];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            o[r][0] = relu(acc[r][0] + bv.x); o[r][1] = relu(acc[r][1] + bv.y);
            o[r][2] = relu(acc[r][2] + bv.z); o[r][3] = relu(acc[r][3] + bv.w);
        }
        const int tbase = (((p.n * H + p.ty * TH) * W + p.tx * TW) * C) * 4;
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const f32x4 t = (f32x4){o[r][0], o[r][1], o[r][2], o[r][3]};
            // the tile offset goes into the VGPR offset, not the SGPR one (sq_conv_f32_l0.hip: the 16-byte store hazard)
            __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<const u32x4 *>(&t), yrsrc, yvoff + tbase + r * W * C * 4, 0, 0);
        }
        if constexpr (EPI == EPI_POOL) {        // rows (2 pr, 2 pr + 1) in registers, the x neighbour is lane ^ 1
            const int pbase = (((p.n * Hl + p.ty * (TH / 2)) * Wl + p.tx * (TW / 2)) * C) * 4;
#pragma unroll
            for (int pr = 0; pr < ROWS / 2; ++pr) {
                f32x4 mp;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float v = __builtin_fmaxf(o[2 * pr][j], o[2 * pr + 1][j]);
                    const float u = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
                    mp[j] = __builtin_fmaxf(u, v);
                }
                __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<const u32x4 *>(&mp), prsrc,
                                                       (li & 1) ? (int)OOB : pvoff + pbase + pr * Wl * C * 4, 0, 0);
            }
        }
    };

    // one row of the PREVIOUS tile (its accumulators are still in place: output row r is first overwritten at step r); the
    // offsets are out of range while there is none
    float keep[4] = {0.f, 0.f, 0.f, 0.f};
    auto store_row = [&](int r, const f32x4 &v, int ybase, int pbase) {
        const float o[4] = {relu(v[0] + bv.x), relu(v[1] + bv.y), relu(v[2] + bv.z), relu(v[3] + bv.w)};
        const f32x4 t = (f32x4){o[0], o[1], o[2], o[3]};
        __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<const u32x4 *>(&t), yrsrc, ybase + r * W * C * 4, 0, 0);
        if constexpr (EPI == EPI_POOL) {
            if (r & 1) {
                f32x4 mp;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float m = __builtin_fmaxf(keep[j], o[j]);
                    const float u = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, m), 0xB1, 0xF, 0xF, true));
                    mp[j] = __builtin_fmaxf(u, m);
                }
                __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<const u32x4 *>(&mp), prsrc, pbase + (r >> 1) * Wl * C * 4, 0, 0);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) keep[j] = o[j];
            }
        }
    };

    // ---- the tile loop: the stores of a tile ride in the MFMA phase of the next one -------------------------------------
    Pos cur = decode(vb), nxt = cur, prev = cur;
    bool pend = false;
    f32x4 pa0 = (f32x4){0.f, 0.f, 0.f, 0.f};
    issue_halo(cur, true);
    __builtin_amdgcn_s_waitcnt(0x0F70);                             // vmcnt(0)
    commit_halo();
    __syncthreads();
    for (int it = 0; it < t_count; ++it) {
        const bool has_next = it + 1 < t_count;
        nxt = advance(cur);
        const int tbase = (((prev.n * H + prev.ty * TH) * W + prev.tx * TW) * C) * 4;
        const int ybase = pend ? yvoff + tbase : (int)OOB;
        const int pb = (((prev.n * Hl + prev.ty * (TH / 2)) * Wl + prev.tx * (TW / 2)) * C) * 4;
        const int pbase = (pend && !(li & 1)) ? pvoff + pb : (int)OOB;
        mfma_phase([&](int st) {
            if (st == 0) store_row(0, pa0, ybase, pbase);
            if (st + 1 < ROWS) store_row(st + 1, acc[st + 1], ybase, pbase);
            if (st == ROWS) issue_halo(nxt, has_next);
        });
        pa0 = acc[0];
        prev = cur;
        pend = true;
        __builtin_amdgcn_s_waitcnt(0x0F70);                         // the prefetch has landed; stated outside the branch (v2 kernel, main loop)
        if (has_next) {
            __syncthreads();                                        // every wave is done reading this tile's halo image
            commit_halo();
            __syncthreads();
        }
        cur = nxt;
    }
    epilogue(prev);                                                 // the last tile's own
}

template <int EPI>
int launch_r32(const R32Args &a0, hipStream_t st) {
    static bool attr_set = false;
    auto kern = conv_r32_kernel<EPI>;
    if (!attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES) != hipSuccess) {
            sq_set_error("conv_r32: cannot reserve %d bytes of LDS", LDS_BYTES);
            return SQ_ELAUNCH;
        }
        attr_set = true;
    }
    R32Args a = a0;
    a.tiles_x = a.W / TW;
    a.tiles_y = a.H / TH;
    a.ntiles = a.tiles_x * a.tiles_y * a.N;
    // the grid of the generic form and its stride in tile coordinates, shared with sq_conv_walk_plan
    int tpb;
    const int G = sq_plan_v2_grid(a.ntiles, 1, OCC, &tpb);
    sq_plan_tile_stride(G, a.tiles_x, a.tiles_y, &a.gx, &a.gy, &a.gn);
    hipLaunchKernelGGL(kern, dim3(G), dim3(256), LDS_BYTES, st, a);
    return sq_check_launch("conv_r32");
}

}  // namespace

int sq_conv_r32_launch(const float *x, const float *w, const float *bias, float *y, int N, int H, int W, int Cin, int Cout,
                       int K, float wscale, int act, const SqConvEpi &epi, hipStream_t st) {
    // which calls are its own: sq_plan_r32_takes, shared with sq_conv_r32_takes_f32
    if (!sq_plan_r32_takes(N, H, W, Cin, Cout, K, act, wscale == 1.0f, epi.x2 != nullptr, epi.head_w != nullptr,
                           epi.pooled != nullptr))
        return SQ_L0_NOT_MINE;
    if (epi.first_w || epi.up_x || !epi.store_y || !y) return SQ_L0_NOT_MINE;
    R32Args a = {};
    a.x = x; a.w = w; a.bias = bias; a.y = y; a.pooled = epi.pooled; a.N = N; a.H = H; a.W = W;
    return epi.pooled ? launch_r32<EPI_POOL>(a, st) : launch_r32<EPI_STORE>(a, st);
}
