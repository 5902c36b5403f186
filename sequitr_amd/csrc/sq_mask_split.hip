// Mask clean-up, splitting (include/sequitr_hip.h, "Mask clean-up: splitting"): cut a one-pixel line of background
// between the parts of an object that its eroded cores tell apart.  Planar (N, H, W) uint8 masks.
//   seeds    : sq_mask_morph_u8's erosion of all class planes, one launch, into a byte plane of the workspace
//   labels   : sq_ccl.h's row scan / merge / compress on the seed plane; a seed pixel's label is its root index + 1
//   regrowth : T synchronous steps.  A block owns a 64 x 64 tile, stages the class bytes and the labels of the tile and a
//              halo of as many pixels as the launch runs steps (at most SQ_SPLIT_STEPS) in LDS, runs the steps there and
//              stores its tile's labels to the other global plane; SQ_SPLIT_LDS=0 runs one step per launch on the planes
//   cut      : one pointwise pass, labels + mask -> out
#include <stdlib.h>
#include "sq_ccl.h"

namespace {

constexpr int ST_ROWS = SQ_SPLIT_TILE_ROWS, ST_COLS = SQ_SPLIT_TILE_COLS, ST_K = SQ_SPLIT_STEPS;
constexpr int SS_ROWS = ST_ROWS + 2 * ST_K, SS_COLS = ST_COLS + 2 * ST_K;     // the staged region
constexpr int SS_CELLS = SS_ROWS * SS_COLS, SS_PER = SS_CELLS / 256;          // staged cells, and how many a thread owns
constexpr int ST_PER = ST_ROWS * ST_COLS / 256;                                // tile cells a thread stores
static_assert(SS_CELLS % 256 == 0 && ST_ROWS * ST_COLS % 256 == 0, "the cells divide among 256 threads");
static_assert(SS_PER <= 32, "a thread's cells have one bit each in a 32-bit word");
static_assert(SS_CELLS * 5 <= 64 * 1024, "labels and class bytes fit the static LDS of a block");

// The label of pixel g as a launch finds it.  The first launch (seed given) reads the labelling itself: root index + 1 on
// a seed pixel of a class, none elsewhere (the erosion copies bytes >= C through and the labelling numbers them: ignored).
__device__ __forceinline__ int split_label(const int *__restrict__ lab, const uint8_t *__restrict__ seed, int64_t g, int C) {
    const int v = lab[g];
    if (!seed) return v;
    const int s = seed[g];
    return (s >= 1 && s < C) ? v + 1 : 0;
}

// smallest non-zero label: labels travel as label - 1 in unsigned, so that "none" is the largest value
__device__ __forceinline__ unsigned umin_(unsigned a, unsigned b) { return a < b ? a : b; }

// `steps` <= ST_K synchronous steps on one tile.  Outside the frame, and outside the halo of `steps` pixels, there is
// nothing (class 0): what is missing beyond the halo can change a result at most `steps` pixels inwards, not on the tile.
// The second copy of the labels that a synchronous step needs is held in registers: every thread owns SS_PER staged
// cells, computes their new labels from LDS, and writes them after a barrier.
__global__ __launch_bounds__(256) void split_grow_lds_kernel(const uint8_t *__restrict__ mask, const uint8_t *__restrict__ seed,
                                                             const int *__restrict__ src, int *__restrict__ dst, int H, int W,
                                                             int C, int steps, int tiles_x, int tiles_y) {
    __shared__ int lab[SS_CELLS];
    __shared__ uint8_t cls[SS_CELLS];
    const int t = threadIdx.x, bid = blockIdx.x;
    const int tx = bid % tiles_x, ty = (bid / tiles_x) % tiles_y, n = bid / (tiles_x * tiles_y);
    const int x0 = tx * ST_COLS - ST_K, y0 = ty * ST_ROWS - ST_K;              // frame coordinates of staged (0, 0)
    const int lo = ST_K - steps, hi_r = ST_K + ST_ROWS + steps, hi_c = ST_K + ST_COLS + steps;
    const int64_t fb = (int64_t)n * H * W;

    unsigned need = 0;                                          // bit k: my k-th cell carries a class and no label yet
#pragma unroll
    for (int k = 0; k < SS_PER; ++k) {
        const int idx = t + 256 * k, r = idx / SS_COLS, c = idx % SS_COLS, y = y0 + r, x = x0 + c;
        int m = 0, l = 0;
        if (r >= lo && r < hi_r && c >= lo && c < hi_c && y >= 0 && y < H && x >= 0 && x < W) {
            const int64_t g = fb + (int64_t)y * W + x;
            m = mask[g];
            if (m >= 1 && m < C) l = split_label(src, seed, g, C);
            else m = 0;                                         // bytes >= C belong to no class: they conduct nothing
        }
        lab[idx] = l;
        cls[idx] = (uint8_t)m;
        if (m && !l) need |= 1u << k;
    }
    __syncthreads();

    // per cell that can still take a label: which of the 4 neighbours conduct (same class); 4 bits, 8 cells per word
    unsigned conn[(SS_PER + 7) / 8];
#pragma unroll
    for (int w = 0; w < (SS_PER + 7) / 8; ++w) conn[w] = 0;
#pragma unroll
    for (int k = 0; k < SS_PER; ++k) {
        if (!((need >> k) & 1u)) continue;
        const int idx = t + 256 * k, r = idx / SS_COLS, c = idx % SS_COLS;
        const uint8_t m = cls[idx];
        unsigned nib = 0;
        if (r > 0 && cls[idx - SS_COLS] == m) nib |= 1u;
        if (r < SS_ROWS - 1 && cls[idx + SS_COLS] == m) nib |= 2u;
        if (c > 0 && cls[idx - 1] == m) nib |= 4u;
        if (c < SS_COLS - 1 && cls[idx + 1] == m) nib |= 8u;
        conn[k >> 3] |= nib << (4 * (k & 7));
    }

    for (int s = 0; s < steps; ++s) {
        int nl[SS_PER];
        int any = 0;
#pragma unroll
        for (int k = 0; k < SS_PER; ++k) {
            nl[k] = 0;
            const unsigned nib = (conn[k >> 3] >> (4 * (k & 7))) & 15u;
            if (!nib) continue;
            const int idx = t + 256 * k;
            unsigned best = ~0u;
            if (nib & 1u) best = umin_(best, (unsigned)lab[idx - SS_COLS] - 1u);
            if (nib & 2u) best = umin_(best, (unsigned)lab[idx + SS_COLS] - 1u);
            if (nib & 4u) best = umin_(best, (unsigned)lab[idx - 1] - 1u);
            if (nib & 8u) best = umin_(best, (unsigned)lab[idx + 1] - 1u);
            nl[k] = (int)(best + 1u);
            any |= nl[k];
        }
        if (!__syncthreads_or(any)) break;                      // a step that changes nothing: so does every later one
#pragma unroll
        for (int k = 0; k < SS_PER; ++k)
            if (nl[k]) {
                lab[t + 256 * k] = nl[k];
                conn[k >> 3] &= ~(15u << (4 * (k & 7)));
            }
        __syncthreads();
    }

#pragma unroll
    for (int k = 0; k < ST_PER; ++k) {
        const int item = t + 256 * k, r = item / ST_COLS, c = item % ST_COLS;
        const int y = ty * ST_ROWS + r, x = tx * ST_COLS + c;
        if (y < H && x < W) dst[fb + (int64_t)y * W + x] = lab[(ST_K + r) * SS_COLS + ST_K + c];
    }
}

// SQ_SPLIT_LDS=0: one synchronous step per launch on the global planes
__global__ __launch_bounds__(256) void split_grow_step_kernel(const uint8_t *__restrict__ mask, const uint8_t *__restrict__ seed,
                                                              const int *__restrict__ src, int *__restrict__ dst, int64_t total,
                                                              int H, int W, int C) {
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int m = mask[g];
        int l = 0;
        if (m >= 1 && m < C) {
            l = split_label(src, seed, g, C);
            if (!l) {
                const int col = (int)(g % W), row = (int)((g / W) % H);
                unsigned best = ~0u;
                if (row > 0 && mask[g - W] == m) best = umin_(best, (unsigned)split_label(src, seed, g - W, C) - 1u);
                if (row < H - 1 && mask[g + W] == m) best = umin_(best, (unsigned)split_label(src, seed, g + W, C) - 1u);
                if (col > 0 && mask[g - 1] == m) best = umin_(best, (unsigned)split_label(src, seed, g - 1, C) - 1u);
                if (col < W - 1 && mask[g + 1] == m) best = umin_(best, (unsigned)split_label(src, seed, g + 1, C) - 1u);
                l = (int)(best + 1u);
            }
        }
        dst[g] = l;
    }
}

// out = 0 where a labelled pixel has a same-class neighbour with a smaller label, the mask elsewhere
__global__ __launch_bounds__(256) void split_cut_kernel(const uint8_t *__restrict__ mask, const int *__restrict__ lab,
                                                        uint8_t *__restrict__ out, int64_t total, int H, int W, int C) {
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int m = mask[g];
        int o = m;
        if (m >= 1 && m < C) {
            const unsigned l = (unsigned)lab[g] - 1u;           // none: the largest value, nothing is below "none" but a label
            if (l != ~0u) {
                const int col = (int)(g % W), row = (int)((g / W) % H);
                bool cut = false;
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

inline bool ranges_overlap(const void *a, int64_t abytes, const void *b, int64_t bbytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + (uintptr_t)bbytes && y < x + (uintptr_t)abytes;
}

}  // namespace

extern "C" int64_t sq_mask_split_workspace(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return -1;
    const int64_t total = (int64_t)N * H * W;
    if (total >= ((int64_t)1 << 31)) return -1;
    return (total * 9 + 15) / 16 * 16;                         // two label planes, the seed plane
}

extern "C" int sq_mask_split_u8(const uint8_t *mask, uint8_t *out, int N, int H, int W, int C, int erosions, int structure,
                                int reach, void *workspace, void *stream) {
    const char *who = "sq_mask_split_u8";
    SQ_REQUIRE(mask && out && workspace, "%s: null pointer", who);
    SQ_REQUIRE(C >= 2 && C <= 256, "%s: C must be 2 .. 256 classes, got %d", who, C);
    SQ_REQUIRE(structure == SQ_MORPH_CROSS || structure == SQ_MORPH_SQUARE,
               "%s: structure must be SQ_MORPH_CROSS or SQ_MORPH_SQUARE, got %d", who, structure);
    SQ_REQUIRE(erosions >= 1 && erosions <= SQ_MORPH_MAX_ITER, "%s: erosions must be 1 .. %d, got %d", who, SQ_MORPH_MAX_ITER,
               erosions);
    SQ_REQUIRE(reach >= 1 && reach <= SQ_SPLIT_MAX_REACH, "%s: reach must be 1 .. %d, got %d", who, SQ_SPLIT_MAX_REACH, reach);
    SQ_REQUIRE(N > 0 && H > 0 && W > 0 && (int64_t)N * H * W < ((int64_t)1 << 31),
               "%s: the mask must have at least one and fewer than 2^31 elements, got (%d,%d,%d)", who, N, H, W);
    SQ_REQUIRE((((uintptr_t)workspace) & 15u) == 0, "%s: workspace must be 16-byte aligned", who);
    const int64_t total = (int64_t)N * H * W, ws_bytes = sq_mask_split_workspace(N, H, W);
    SQ_REQUIRE(!ranges_overlap(mask, total, out, total), "%s: out must not overlap mask", who);
    SQ_REQUIRE(!ranges_overlap(workspace, ws_bytes, mask, total) && !ranges_overlap(workspace, ws_bytes, out, total),
               "%s: workspace must not overlap mask or out", who);
    hipStream_t st = (hipStream_t)stream;
    int *plane[2] = {reinterpret_cast<int *>(workspace), reinterpret_cast<int *>(workspace) + total};
    uint8_t *seed = reinterpret_cast<uint8_t *>(plane[1] + total);

    const int rc = sq_mask_morph_u8(mask, seed, N, H, W, C, SQ_MORPH_ERODE, structure, erosions, stream);
    if (rc != SQ_OK) return rc;
    const int rows = N * H;
    const dim3 rgrid((rows + 3) / 4), tgrid(cc_grid(total)), blk(256);
    hipLaunchKernelGGL(cc_rowscan_kernel<false>, rgrid, blk, 0, st, (const uint8_t *)seed, plane[0], (unsigned *)nullptr,
                       (u64 *)nullptr, rows, W);
    hipLaunchKernelGGL(cc_merge_kernel, tgrid, blk, 0, st, (const uint8_t *)seed, plane[0], total, 1, H, W);
    hipLaunchKernelGGL(cc_compress_kernel, tgrid, blk, 0, st, plane[0], total);

    const char *e = getenv("SQ_SPLIT_LDS");                     // read per launch: 0 is the one-step-per-launch form
    const bool lds = !(e && e[0] == '0');
    const int per = lds ? ST_K : 1;
    const int tiles_x = (W + ST_COLS - 1) / ST_COLS, tiles_y = (H + ST_ROWS - 1) / ST_ROWS;
    const int64_t blocks = (int64_t)N * tiles_x * tiles_y;      // fewer than there are pixels
    int cur = 0;
    for (int done = 0; done < reach; done += per, cur ^= 1) {
        const uint8_t *first = done == 0 ? seed : nullptr;      // the first launch turns roots into labels as it reads
        const int steps = reach - done < per ? reach - done : per;
        if (lds)
            hipLaunchKernelGGL(split_grow_lds_kernel, dim3((unsigned)blocks), blk, 0, st, mask, first, (const int *)plane[cur],
                               plane[cur ^ 1], H, W, C, steps, tiles_x, tiles_y);
        else
            hipLaunchKernelGGL(split_grow_step_kernel, tgrid, blk, 0, st, mask, first, (const int *)plane[cur], plane[cur ^ 1],
                               total, H, W, C);
    }
    hipLaunchKernelGGL(split_cut_kernel, tgrid, blk, 0, st, mask, (const int *)plane[cur], out, total, H, W, C);
    return sq_check_launch(who);
}
