// Volume clean-up, splitting (include/sequitr_hip.h, "Volume clean-up: splitting"): cut a one-voxel sheet of background
// between the parts of an object that its eroded cores tell apart.  (N, D, H, W) uint8 masks.
//   seeds    : plane structures: sq_mask_morph_u8's erosion of the (N D, H, W) view, one launch; cross and cube: a chain of
//              sq_volume_morph_u8 erosions of at most SQ_MORPH3D_MAX_ITER steps each, ping-pong between the workspace's byte
//              plane and `out`, the last one into the workspace plane
//   labels   : sq_ccl.h's row scan / merge (planes = D) / compress on the seed plane; a seed voxel's label is its root + 1
//   regrowth : T synchronous steps.  SQ_SPLIT3D_LDS=1: a block owns a brick, stages the class bytes and the labels of the
//              brick and a halo of as many voxels as the launch runs steps (at most SQ_SPLIT3D_STEPS) in LDS, runs the
//              steps there and stores its brick's labels to the other global plane; SQ_SPLIT3D_LDS=0: one step per launch
//              on the global planes
//   cut      : one pointwise pass, labels + mask -> out
#include <stdlib.h>
#include "sq_ccl.h"

namespace {

constexpr int VS_D = SQ_SPLIT3D_TILE_D, VS_H = SQ_SPLIT3D_TILE_H, VS_W = SQ_SPLIT3D_TILE_W, VS_K = SQ_SPLIT3D_STEPS;
constexpr int SS_D = VS_D + 2 * VS_K, SS_H = VS_H + 2 * VS_K, SS_W = VS_W + 2 * VS_K;   // the staged region
constexpr int SS_HW = SS_H * SS_W, SS_CELLS = SS_D * SS_HW;
constexpr int VS_THREADS = 512;                                 // of the LDS kernel: up to 17 staged cells a thread
constexpr int SS_PER = (SS_CELLS + VS_THREADS - 1) / VS_THREADS;                  // staged cells a thread owns
constexpr int VS_CELLS = VS_D * VS_H * VS_W, VS_PER = VS_CELLS / VS_THREADS;   // brick cells a thread stores
constexpr int CONN_PER_WORD = 5, CONN_WORDS = (SS_PER + CONN_PER_WORD - 1) / CONN_PER_WORD;   // 6 bits per cell
constexpr bool SS_EXACT = SS_CELLS % VS_THREADS == 0;
static_assert(VS_CELLS % VS_THREADS == 0, "the brick's cells divide among the threads");
static_assert(SS_PER <= 64, "a thread's cells have one bit each in a 64-bit word");
static_assert(SS_CELLS * 5 <= 160 * 1024, "labels and class bytes fit the static LDS of a block");

// Which form runs when SQ_SPLIT3D_LDS is not set: the one tools/volume_split_bench.py measured faster (README.md).
constexpr bool VS_LDS_DEFAULT = SQ_SPLIT3D_LDS_DEFAULT != 0;

// The label of voxel g as a launch finds it.  The first launch (seed given) reads the labelling itself: root index + 1 on
// a seed voxel of a class, none elsewhere (the erosion copies bytes >= C through and the labelling numbers them: ignored).
__device__ __forceinline__ int vsplit_label(const int *__restrict__ lab, const uint8_t *__restrict__ seed, int64_t g, int C) {
    const int v = lab[g];
    if (!seed) return v;
    const int s = seed[g];
    return (s >= 1 && s < C) ? v + 1 : 0;
}

// smallest non-zero label: labels travel as label - 1 in unsigned, so that "none" is the largest value
__device__ __forceinline__ unsigned vs_umin(unsigned a, unsigned b) { return a < b ? a : b; }

// `steps` <= VS_K synchronous steps on one brick.  Outside the volume, and outside the halo of `steps` voxels, there is
// nothing (class 0): what is missing beyond the halo can change a result at most `steps` voxels inwards, not on the brick.
// The second copy of the labels that a synchronous step needs is held in registers: every thread owns SS_PER staged
// cells, computes their new labels from LDS, and writes them after a barrier.
__global__ __launch_bounds__(VS_THREADS) void vsplit_grow_lds_kernel(const uint8_t *__restrict__ mask,
                                                                        const uint8_t *__restrict__ seed,
                                                                        const int *__restrict__ src, int *__restrict__ dst, int D,
                                                                        int H, int W, int C, int steps, int tiles_x, int tiles_y,
                                                                        int tiles_z) {
    __shared__ int lab[SS_CELLS];
    __shared__ uint8_t cls[SS_CELLS];
    const int t = threadIdx.x;
    int bid = blockIdx.x;
    const int tx = bid % tiles_x;
    bid /= tiles_x;
    const int ty = bid % tiles_y;
    bid /= tiles_y;
    const int tz = bid % tiles_z, n = bid / tiles_z;
    const int x0 = tx * VS_W - VS_K, y0 = ty * VS_H - VS_K, z0 = tz * VS_D - VS_K;     // volume coordinates of staged (0,0,0)
    const int lo = VS_K - steps, hi_d = VS_K + VS_D + steps, hi_h = VS_K + VS_H + steps, hi_w = VS_K + VS_W + steps;
    const int64_t vb = (int64_t)n * D * H * W;

    // At most ten cells' loads in flight at a time: with a halo of 4 (30 cells a thread) the fully unrolled loop's
    // addresses and values cost 70 VGPRs more than the steps.
    u64 need = 0;                                               // bit k: my k-th cell carries a class and no label yet
#pragma unroll 10
    for (int k = 0; k < SS_PER; ++k) {
        const int idx = t + VS_THREADS * k;
        if (!SS_EXACT && idx >= SS_CELLS) break;
        const int p = idx / SS_HW, r = (idx % SS_HW) / SS_W, c = idx % SS_W, z = z0 + p, y = y0 + r, x = x0 + c;
        int m = 0, l = 0;
        if (p >= lo && p < hi_d && r >= lo && r < hi_h && c >= lo && c < hi_w && z >= 0 && z < D && y >= 0 && y < H &&
            x >= 0 && x < W) {
            const int64_t g = vb + ((int64_t)z * H + y) * W + x;
            m = mask[g];
            if (m >= 1 && m < C) l = vsplit_label(src, seed, g, C);
            else m = 0;                                         // bytes >= C belong to no class: they conduct nothing
        }
        lab[idx] = l;
        cls[idx] = (uint8_t)m;
        if (m && !l) need |= 1ULL << k;
    }
    __syncthreads();

    // per cell that can still take a label: which of the 6 neighbours conduct (same class); 6 bits, 5 cells per word
    unsigned conn[CONN_WORDS];
#pragma unroll
    for (int w = 0; w < CONN_WORDS; ++w) conn[w] = 0;
#pragma unroll
    for (int k = 0; k < SS_PER; ++k) {
        if (!((need >> k) & 1ULL)) continue;
        const int idx = t + VS_THREADS * k, p = idx / SS_HW, r = (idx % SS_HW) / SS_W, c = idx % SS_W;
        const uint8_t m = cls[idx];
        unsigned six = 0;
        if (p > 0 && cls[idx - SS_HW] == m) six |= 1u;
        if (p < SS_D - 1 && cls[idx + SS_HW] == m) six |= 2u;
        if (r > 0 && cls[idx - SS_W] == m) six |= 4u;
        if (r < SS_H - 1 && cls[idx + SS_W] == m) six |= 8u;
        if (c > 0 && cls[idx - 1] == m) six |= 16u;
        if (c < SS_W - 1 && cls[idx + 1] == m) six |= 32u;
        conn[k / CONN_PER_WORD] |= six << (6 * (k % CONN_PER_WORD));
    }

    for (int s = 0; s < steps; ++s) {
        int nl[SS_PER];
        int any = 0;
#pragma unroll
        for (int k = 0; k < SS_PER; ++k) {
            nl[k] = 0;
            const unsigned six = (conn[k / CONN_PER_WORD] >> (6 * (k % CONN_PER_WORD))) & 63u;
            if (!six) continue;
            const int idx = t + VS_THREADS * k;
            unsigned best = ~0u;
            if (six & 1u) best = vs_umin(best, (unsigned)lab[idx - SS_HW] - 1u);
            if (six & 2u) best = vs_umin(best, (unsigned)lab[idx + SS_HW] - 1u);
            if (six & 4u) best = vs_umin(best, (unsigned)lab[idx - SS_W] - 1u);
            if (six & 8u) best = vs_umin(best, (unsigned)lab[idx + SS_W] - 1u);
            if (six & 16u) best = vs_umin(best, (unsigned)lab[idx - 1] - 1u);
            if (six & 32u) best = vs_umin(best, (unsigned)lab[idx + 1] - 1u);
            nl[k] = (int)(best + 1u);
            any |= nl[k];
        }
        if (!__syncthreads_or(any)) break;                      // a step that changes nothing: so does every later one
#pragma unroll
        for (int k = 0; k < SS_PER; ++k)
            if (nl[k]) {
                lab[t + VS_THREADS * k] = nl[k];
                conn[k / CONN_PER_WORD] &= ~(63u << (6 * (k % CONN_PER_WORD)));
            }
        __syncthreads();
    }

#pragma unroll
    for (int k = 0; k < VS_PER; ++k) {
        const int item = t + VS_THREADS * k, p = item / (VS_H * VS_W), r = (item / VS_W) % VS_H, c = item % VS_W;
        const int z = tz * VS_D + p, y = ty * VS_H + r, x = tx * VS_W + c;
        if (z < D && y < H && x < W)
            dst[vb + ((int64_t)z * H + y) * W + x] = lab[(VS_K + p) * SS_HW + (VS_K + r) * SS_W + VS_K + c];
    }
}

// SQ_SPLIT3D_LDS=0: one synchronous step per launch on the global planes
__global__ __launch_bounds__(256) void vsplit_grow_step_kernel(const uint8_t *__restrict__ mask, const uint8_t *__restrict__ seed,
                                                               const int *__restrict__ src, int *__restrict__ dst, int64_t total,
                                                               int D, int H, int W, int C) {
    const int64_t HW = (int64_t)H * W;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int m = mask[g];
        int l = 0;
        if (m >= 1 && m < C) {
            l = vsplit_label(src, seed, g, C);
            if (!l) {
                const int col = (int)(g % W), row = (int)((g / W) % H), pl = (int)((g / HW) % D);
                unsigned best = ~0u;
                if (pl > 0 && mask[g - HW] == m) best = vs_umin(best, (unsigned)vsplit_label(src, seed, g - HW, C) - 1u);
                if (pl < D - 1 && mask[g + HW] == m) best = vs_umin(best, (unsigned)vsplit_label(src, seed, g + HW, C) - 1u);
                if (row > 0 && mask[g - W] == m) best = vs_umin(best, (unsigned)vsplit_label(src, seed, g - W, C) - 1u);
                if (row < H - 1 && mask[g + W] == m) best = vs_umin(best, (unsigned)vsplit_label(src, seed, g + W, C) - 1u);
                if (col > 0 && mask[g - 1] == m) best = vs_umin(best, (unsigned)vsplit_label(src, seed, g - 1, C) - 1u);
                if (col < W - 1 && mask[g + 1] == m) best = vs_umin(best, (unsigned)vsplit_label(src, seed, g + 1, C) - 1u);
                l = (int)(best + 1u);
            }
        }
        dst[g] = l;
    }
}

// out = 0 where a labelled voxel has a same-class neighbour with a smaller label, the mask elsewhere
__global__ __launch_bounds__(256) void vsplit_cut_kernel(const uint8_t *__restrict__ mask, const int *__restrict__ lab,
                                                         uint8_t *__restrict__ out, int64_t total, int D, int H, int W, int C) {
    const int64_t HW = (int64_t)H * W;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int m = mask[g];
        int o = m;
        if (m >= 1 && m < C) {
            const unsigned l = (unsigned)lab[g] - 1u;           // none: the largest value, nothing is below "none" but a label
            if (l != ~0u) {
                const int col = (int)(g % W), row = (int)((g / W) % H), pl = (int)((g / HW) % D);
                bool cut = false;
                if (pl > 0 && mask[g - HW] == m) cut |= (unsigned)lab[g - HW] - 1u < l;
                if (pl < D - 1 && mask[g + HW] == m) cut |= (unsigned)lab[g + HW] - 1u < l;
                if (row > 0 && mask[g - W] == m) cut |= (unsigned)lab[g - W] - 1u < l;
                if (row < H - 1 && mask[g + W] == m) cut |= (unsigned)lab[g + W] - 1u < l;
                if (col > 0 && mask[g - 1] == m) cut |= (unsigned)lab[g - 1] - 1u < l;
                if (col < W - 1 && mask[g + 1] == m) cut |= (unsigned)lab[g + 1] - 1u < l;
                if (cut) o = 0;
            }
        }
        out[g] = (uint8_t)o;
    }
}

inline bool vs_overlap(const void *a, int64_t abytes, const void *b, int64_t bbytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + (uintptr_t)bbytes && y < x + (uintptr_t)abytes;
}

}  // namespace

extern "C" int64_t sq_volume_split_workspace(int N, int D, int H, int W) {
    if (N <= 0 || D <= 0 || H <= 0 || W <= 0) return -1;
    const int64_t total = (int64_t)N * D * H * W;               // each factor < 2^31: no overflow before the last product
    if ((int64_t)N * D >= ((int64_t)1 << 31) || (int64_t)H * W >= ((int64_t)1 << 31) || total >= ((int64_t)1 << 31)) return -1;
    return (total * 9 + 15) / 16 * 16;                         // two label planes, the seed plane
}

extern "C" int sq_volume_split_u8(const uint8_t *mask, uint8_t *out, int N, int D, int H, int W, int C, int erosions,
                                  int structure, int reach, void *workspace, void *stream) {
    const char *who = "sq_volume_split_u8";
    SQ_REQUIRE(mask && out && workspace, "%s: null pointer", who);
    SQ_REQUIRE(C >= 2 && C <= 256, "%s: C must be 2 .. 256 classes, got %d", who, C);
    SQ_REQUIRE(structure >= 0 && structure <= SQ_SPLIT3D_PLANE_SQUARE,
               "%s: structure must be SQ_MORPH3D_CROSS, SQ_MORPH3D_CUBE, SQ_SPLIT3D_PLANE_CROSS or SQ_SPLIT3D_PLANE_SQUARE, got %d",
               who, structure);
    SQ_REQUIRE(erosions >= 1 && erosions <= SQ_SPLIT3D_MAX_EROSIONS, "%s: erosions must be 1 .. %d, got %d", who,
               SQ_SPLIT3D_MAX_EROSIONS, erosions);
    SQ_REQUIRE(reach >= 1 && reach <= SQ_SPLIT3D_MAX_REACH, "%s: reach must be 1 .. %d, got %d", who, SQ_SPLIT3D_MAX_REACH,
               reach);
    const int64_t ws_bytes = sq_volume_split_workspace(N, D, H, W);
    SQ_REQUIRE(ws_bytes > 0, "%s: the mask must have at least one and fewer than 2^31 elements, got (%d,%d,%d,%d)", who, N, D,
               H, W);
    SQ_REQUIRE((((uintptr_t)workspace) & 15u) == 0, "%s: workspace must be 16-byte aligned", who);
    const int64_t total = (int64_t)N * D * H * W;
    SQ_REQUIRE(!vs_overlap(mask, total, out, total), "%s: out must not overlap mask", who);
    SQ_REQUIRE(!vs_overlap(workspace, ws_bytes, mask, total) && !vs_overlap(workspace, ws_bytes, out, total),
               "%s: workspace must not overlap mask or out", who);
    hipStream_t st = (hipStream_t)stream;
    int *plane[2] = {reinterpret_cast<int *>(workspace), reinterpret_cast<int *>(workspace) + total};
    uint8_t *seed = reinterpret_cast<uint8_t *>(plane[1] + total);

    if (structure >= SQ_SPLIT3D_PLANE_CROSS) {                  // the planar erosion slice by slice
        static_assert(SQ_SPLIT3D_MAX_EROSIONS <= SQ_MORPH_MAX_ITER, "one planar launch erodes as often as a split may ask");
        const int rc = sq_mask_morph_u8(mask, seed, N * D, H, W, C, SQ_MORPH_ERODE,
                                        structure == SQ_SPLIT3D_PLANE_CROSS ? SQ_MORPH_CROSS : SQ_MORPH_SQUARE, erosions, stream);
        if (rc != SQ_OK) return rc;
    } else {                                                    // erosions compose exactly: a chain that ends in `seed`
        const int launches = (erosions + SQ_MORPH3D_MAX_ITER - 1) / SQ_MORPH3D_MAX_ITER;
        const uint8_t *from = mask;
        for (int i = 0, left = erosions; i < launches; ++i) {
            uint8_t *to = ((launches - 1 - i) & 1) ? out : seed;
            const int it = left < SQ_MORPH3D_MAX_ITER ? left : SQ_MORPH3D_MAX_ITER;
            const int rc = sq_volume_morph_u8(from, to, N, D, H, W, C, SQ_MORPH_ERODE, structure, it, stream);
            if (rc != SQ_OK) return rc;
            left -= it;
            from = to;
        }
    }
    const int rows = N * D * H;
    const dim3 rgrid((rows + 3) / 4), tgrid(cc_grid(total)), blk(256);
    hipLaunchKernelGGL(cc_rowscan_kernel<false>, rgrid, blk, 0, st, (const uint8_t *)seed, plane[0], (unsigned *)nullptr,
                       (u64 *)nullptr, rows, W);
    hipLaunchKernelGGL(cc_merge_kernel, tgrid, blk, 0, st, (const uint8_t *)seed, plane[0], total, D, H, W);
    hipLaunchKernelGGL(cc_compress_kernel, tgrid, blk, 0, st, plane[0], total);

    const char *e = getenv("SQ_SPLIT3D_LDS");                   // read per call: 0 is the one-step-per-launch form
    const bool lds = e && (e[0] == '0' || e[0] == '1') ? e[0] == '1' : VS_LDS_DEFAULT;
    const int per = lds ? VS_K : 1;
    const int tiles_x = (W + VS_W - 1) / VS_W, tiles_y = (H + VS_H - 1) / VS_H, tiles_z = (D + VS_D - 1) / VS_D;
    const int64_t blocks = (int64_t)N * tiles_x * tiles_y * tiles_z;     // fewer than there are voxels
    int cur = 0;
    for (int done = 0; done < reach; done += per, cur ^= 1) {
        const uint8_t *first = done == 0 ? seed : nullptr;      // the first launch turns roots into labels as it reads
        const int steps = reach - done < per ? reach - done : per;
        if (lds)
            hipLaunchKernelGGL(vsplit_grow_lds_kernel, dim3((unsigned)blocks), dim3(VS_THREADS), 0, st, mask, first, (const int *)plane[cur],
                               plane[cur ^ 1], D, H, W, C, steps, tiles_x, tiles_y, tiles_z);
        else
            hipLaunchKernelGGL(vsplit_grow_step_kernel, tgrid, blk, 0, st, mask, first, (const int *)plane[cur], plane[cur ^ 1],
                               total, D, H, W, C);
    }
    hipLaunchKernelGGL(vsplit_cut_kernel, tgrid, blk, 0, st, mask, (const int *)plane[cur], out, total, D, H, W, C);
    return sq_check_launch(who);
}
