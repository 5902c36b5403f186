// Clean-up, splitting (include/sequitr_hip.h, "Mask clean-up: splitting" and "Volume clean-up: splitting"): cut a
// one-pixel line (one-voxel sheet) of background between the parts of an object that its eroded cores tell apart.
// (N, H, W) and (N, D, H, W) uint8 masks; a frame is a volume with D = 1, and everything after the seeds is one program.
//   seeds    : each entry's own.  Frames: sq_mask_morph_u8's erosion of all class planes, one launch, into the byte plane of
//              the workspace.  Volumes, plane structures: the same launch on the (N D, H, W) view; cross and cube: a chain
//              of sq_volume_morph_u8 erosions of at most SQ_MORPH3D_MAX_ITER steps each, ping-pong between the workspace's
//              byte plane and `out`, the last one into the workspace plane
//   labels   : sq_ccl.h's row scan / merge (planes = D) / compress on the seed plane; a seed cell's label is its root + 1
//   regrowth : T synchronous steps.  LDS form: a block owns a tile (64 x 64 pixels, or a brick of 8 x 16 x 32 voxels),
//              stages the class bytes and the labels of the tile and a halo of as many cells as the launch runs steps (at
//              most SQ_SPLIT_STEPS / SQ_SPLIT3D_STEPS) in LDS, runs the steps there and stores its tile's labels to the
//              other global plane.  Step form (SQ_SPLIT_LDS=0, SQ_SPLIT3D_LDS=0): one step per launch on the global planes
//   cut      : one pointwise pass, labels + mask -> out
#include <stdlib.h>
#include <type_traits>
#include "sq_cleanup.h"

namespace {

// The label of cell g as a launch finds it.  The first launch (seed given) reads the labelling itself: root index + 1 on
// a seed cell of a class, none elsewhere (the erosion copies bytes >= C through and the labelling numbers them: ignored).
__device__ __forceinline__ int split_label(const int *__restrict__ lab, const uint8_t *__restrict__ seed, int64_t g, int C) {
    const int v = lab[g];
    if (!seed) return v;
    const int s = seed[g];
    return (s >= 1 && s < C) ? v + 1 : 0;
}

// smallest non-zero label: labels travel as label - 1 in unsigned, so that "none" is the largest value
__device__ __forceinline__ unsigned umin_(unsigned a, unsigned b) { return a < b ? a : b; }

// `steps` <= K synchronous steps on one tile of TD x TH x TW cells; TD = 1 is a frame's tile, with no halo in depth and
// 4 neighbours.  Outside the mask, and outside the halo of `steps` cells, there is nothing (class 0): what is missing
// beyond the halo can change a result at most `steps` cells inwards, not on the tile.  The second copy of the labels that
// a synchronous step needs is held in registers: every thread owns PER staged cells, computes their new labels from LDS,
// and writes them after a barrier.  STAGE: how many cells' loads the staging loop keeps in flight.
template <int TD, int TH, int TW, int K, int THREADS, int STAGE>
__global__ __launch_bounds__(THREADS) void split_grow_lds_kernel(const uint8_t *__restrict__ mask, const uint8_t *__restrict__ seed,
                                                                 const int *__restrict__ src, int *__restrict__ dst, int D, int H,
                                                                 int W, int C, int steps, int tiles_x, int tiles_y, int tiles_z) {
    constexpr bool DEPTH = TD > 1;
    constexpr int KD = DEPTH ? K : 0;                           // the halo in depth
    constexpr int SD = TD + 2 * KD, SH = TH + 2 * K, SW = TW + 2 * K, SHW = SH * SW, CELLS = SD * SHW;   // the staged region
    constexpr int PER = (CELLS + THREADS - 1) / THREADS;        // staged cells a thread owns
    constexpr int TILE_PER = TD * TH * TW / THREADS;            // tile cells a thread stores
    constexpr bool EXACT = CELLS % THREADS == 0;
    // which neighbours conduct: DEPTH: 6 bits a cell, 5 cells a word, the two in depth lowest; else 4 bits, 8 cells a word
    constexpr int BITS = DEPTH ? 6 : 4, PER_WORD = 32 / BITS, WORDS = (PER + PER_WORD - 1) / PER_WORD;
    constexpr unsigned ALL = (1u << BITS) - 1u, UP = DEPTH ? 4u : 1u, DOWN = UP << 1, LEFT = UP << 2, RIGHT = UP << 3;
    static_assert(TD * TH * TW % THREADS == 0, "the tile's cells divide among the threads");
    static_assert(PER <= 64, "a thread's cells have one bit each in a 32- or 64-bit word");
    static_assert(CELLS * 5 <= (DEPTH ? 160 : 64) * 1024, "labels and class bytes fit the static LDS of a block");
    typedef typename std::conditional<(PER <= 32), unsigned, u64>::type need_t;

    __shared__ int lab[CELLS];
    __shared__ uint8_t cls[CELLS];
    const int t = threadIdx.x;
    int bid = blockIdx.x;
    const int tx = bid % tiles_x;
    bid /= tiles_x;
    const int ty = bid % tiles_y;
    bid /= tiles_y;
    const int tz = DEPTH ? bid % tiles_z : 0, n = DEPTH ? bid / tiles_z : bid;
    const int x0 = tx * TW - K, y0 = ty * TH - K, z0 = tz * TD - KD;           // mask coordinates of staged (0, 0, 0)
    const int lo = K - steps, hi_d = K + TD + steps, hi_h = K + TH + steps, hi_w = K + TW + steps;
    const int64_t vb = (int64_t)n * D * H * W;

    // The volume form keeps at most ten cells' loads in flight at a time: with a halo of 4 (30 cells a thread) the fully
    // unrolled loop's addresses and values cost 70 VGPRs more than the steps.  The planar form unrolls fully.
    need_t need = 0;                                            // bit k: my k-th cell carries a class and no label yet
#pragma unroll STAGE
    for (int k = 0; k < PER; ++k) {
        const int idx = t + THREADS * k;
        if (!EXACT && idx >= CELLS) break;
        const int p = DEPTH ? idx / SHW : 0, r = DEPTH ? (idx % SHW) / SW : idx / SW, c = idx % SW;
        const int z = z0 + p, y = y0 + r, x = x0 + c;
        int m = 0, l = 0;
        if ((!DEPTH || (p >= lo && p < hi_d && z >= 0 && z < D)) && r >= lo && r < hi_h && c >= lo && c < hi_w && y >= 0 &&
            y < H && x >= 0 && x < W) {
            const int64_t g = vb + ((int64_t)z * H + y) * W + x;
            m = mask[g];
            if (m >= 1 && m < C) l = split_label(src, seed, g, C);
            else m = 0;                                         // bytes >= C belong to no class: they conduct nothing
        }
        lab[idx] = l;
        cls[idx] = (uint8_t)m;
        if (m && !l) need |= (need_t)1 << k;
    }
    __syncthreads();

    // per cell that can still take a label: which of its neighbours conduct (same class)
    unsigned conn[WORDS];
#pragma unroll
    for (int w = 0; w < WORDS; ++w) conn[w] = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        if (!((need >> k) & 1)) continue;
        const int idx = t + THREADS * k;
        const int p = DEPTH ? idx / SHW : 0, r = DEPTH ? (idx % SHW) / SW : idx / SW, c = idx % SW;
        const uint8_t m = cls[idx];
        unsigned bits = 0;
        if (DEPTH && p > 0 && cls[idx - SHW] == m) bits |= 1u;
        if (DEPTH && p < SD - 1 && cls[idx + SHW] == m) bits |= 2u;
        if (r > 0 && cls[idx - SW] == m) bits |= UP;
        if (r < SH - 1 && cls[idx + SW] == m) bits |= DOWN;
        if (c > 0 && cls[idx - 1] == m) bits |= LEFT;
        if (c < SW - 1 && cls[idx + 1] == m) bits |= RIGHT;
        conn[k / PER_WORD] |= bits << (BITS * (k % PER_WORD));
    }

    for (int s = 0; s < steps; ++s) {
        int nl[PER];
        int any = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            nl[k] = 0;
            const unsigned bits = (conn[k / PER_WORD] >> (BITS * (k % PER_WORD))) & ALL;
            if (!bits) continue;
            const int idx = t + THREADS * k;
            unsigned best = ~0u;
            if (DEPTH && (bits & 1u)) best = umin_(best, (unsigned)lab[idx - SHW] - 1u);
            if (DEPTH && (bits & 2u)) best = umin_(best, (unsigned)lab[idx + SHW] - 1u);
            if (bits & UP) best = umin_(best, (unsigned)lab[idx - SW] - 1u);
            if (bits & DOWN) best = umin_(best, (unsigned)lab[idx + SW] - 1u);
            if (bits & LEFT) best = umin_(best, (unsigned)lab[idx - 1] - 1u);
            if (bits & RIGHT) best = umin_(best, (unsigned)lab[idx + 1] - 1u);
            nl[k] = (int)(best + 1u);
            any |= nl[k];
        }
        if (!__syncthreads_or(any)) break;                      // a step that changes nothing: so does every later one
#pragma unroll
        for (int k = 0; k < PER; ++k)
            if (nl[k]) {
                lab[t + THREADS * k] = nl[k];
                conn[k / PER_WORD] &= ~(ALL << (BITS * (k % PER_WORD)));
            }
        __syncthreads();
    }

#pragma unroll
    for (int k = 0; k < TILE_PER; ++k) {
        const int item = t + THREADS * k;
        const int p = DEPTH ? item / (TH * TW) : 0, r = DEPTH ? (item / TW) % TH : item / TW, c = item % TW;
        const int z = tz * TD + p, y = ty * TH + r, x = tx * TW + c;
        if ((!DEPTH || z < D) && y < H && x < W)
            dst[vb + ((int64_t)z * H + y) * W + x] = lab[(KD + p) * SHW + (K + r) * SW + K + c];
    }
}

// The step form: one synchronous step per launch on the global planes.  DEPTH: the neighbours at g -+ H W count too
// (at D = 1 they would not exist; a frame's launch does not test for them).
template <bool DEPTH>
__global__ __launch_bounds__(256) void split_grow_step_kernel(const uint8_t *__restrict__ mask, const uint8_t *__restrict__ seed,
                                                              const int *__restrict__ src, int *__restrict__ dst, int64_t total,
                                                              int D, int H, int W, int C) {
    const int64_t HW = (int64_t)H * W;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int m = mask[g];
        int l = 0;
        if (m >= 1 && m < C) {
            l = split_label(src, seed, g, C);
            if (!l) {
                const int col = (int)(g % W), row = (int)((g / W) % H), pl = DEPTH ? (int)((g / HW) % D) : 0;
                unsigned best = ~0u;
                if (DEPTH && pl > 0 && mask[g - HW] == m) best = umin_(best, (unsigned)split_label(src, seed, g - HW, C) - 1u);
                if (DEPTH && pl < D - 1 && mask[g + HW] == m) best = umin_(best, (unsigned)split_label(src, seed, g + HW, C) - 1u);
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

// out = 0 where a labelled cell has a same-class neighbour with a smaller label, the mask elsewhere
template <bool DEPTH>
__global__ __launch_bounds__(256) void split_cut_kernel(const uint8_t *__restrict__ mask, const int *__restrict__ lab,
                                                        uint8_t *__restrict__ out, int64_t total, int D, int H, int W, int C) {
    const int64_t HW = (int64_t)H * W;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int m = mask[g];
        int o = m;
        if (m >= 1 && m < C) {
            const unsigned l = (unsigned)lab[g] - 1u;           // none: the largest value, nothing is below "none" but a label
            if (l != ~0u) {
                const int col = (int)(g % W), row = (int)((g / W) % H), pl = DEPTH ? (int)((g / HW) % D) : 0;
                bool cut = false;
                if (DEPTH && pl > 0 && mask[g - HW] == m) cut |= (unsigned)lab[g - HW] - 1u < l;
                if (DEPTH && pl < D - 1 && mask[g + HW] == m) cut |= (unsigned)lab[g + HW] - 1u < l;
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

// The workspace of `total` cells: two int32 label planes, then the seed plane
inline int64_t split_bytes(int64_t total) { return total > 0 ? (total * 9 + 15) / 16 * 16 : -1; }
inline uint8_t *split_seed_plane(void *workspace, int64_t total) { return reinterpret_cast<uint8_t *>(workspace) + 8 * total; }

// What both entries check after their own structure, erosions and reach.  mask, out, workspace, N, H, W are the entry's
// arguments; D is its fourth extent, or 1 for a frame.  fmt and what follows print the extents as the entry takes them.
#define SQ_SPLIT_BUFFERS(who, D, fmt, ...)                                                                                \
    const int64_t total = volume_elements(N, D, H, W), ws_bytes = split_bytes(total);                                     \
    SQ_REQUIRE(total > 0, "%s: the mask must have at least one and fewer than 2^31 elements, got " fmt, who, __VA_ARGS__); \
    SQ_REQUIRE((((uintptr_t)workspace) & 15u) == 0, "%s: workspace must be 16-byte aligned", who);                        \
    SQ_REQUIRE(!ranges_overlap(mask, total, out, total), "%s: out must not overlap mask", who);                           \
    SQ_REQUIRE(!ranges_overlap(workspace, ws_bytes, mask, total) && !ranges_overlap(workspace, ws_bytes, out, total),     \
               "%s: workspace must not overlap mask or out", who)

// Everything after the seeds, which lie in the workspace's byte plane: labels, `reach` steps of regrowth, the cut.
// DEPTH: a volume's call; a frame's passes D = 1.  `lds`: the tiled form with the geometry of the template arguments.
template <int TD, int TH, int TW, int K, int THREADS, int STAGE>
int split_run(const char *who, const uint8_t *mask, uint8_t *out, int N, int D, int H, int W, int C, int reach, bool lds,
              void *workspace, hipStream_t st) {
    constexpr bool DEPTH = TD > 1;
    const int64_t total = (int64_t)N * D * H * W;
    int *plane[2] = {reinterpret_cast<int *>(workspace), reinterpret_cast<int *>(workspace) + total};
    const uint8_t *seed = split_seed_plane(workspace, total);
    const int rows = N * D * H;
    const dim3 rgrid((rows + 3) / 4), tgrid(cc_grid(total)), blk(256);
    hipLaunchKernelGGL(cc_rowscan_kernel<false>, rgrid, blk, 0, st, seed, plane[0], (unsigned *)nullptr, (u64 *)nullptr, rows,
                       W);
    hipLaunchKernelGGL(cc_merge_kernel, tgrid, blk, 0, st, seed, plane[0], total, D, H, W);
    hipLaunchKernelGGL(cc_compress_kernel, tgrid, blk, 0, st, plane[0], total);

    const int per = lds ? K : 1;
    const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH, tiles_z = (D + TD - 1) / TD;
    const int64_t blocks = (int64_t)N * tiles_x * tiles_y * tiles_z;     // fewer than there are cells
    int cur = 0;
    for (int done = 0; done < reach; done += per, cur ^= 1) {
        const uint8_t *first = done == 0 ? seed : nullptr;      // the first launch turns roots into labels as it reads
        const int steps = reach - done < per ? reach - done : per;
        if (lds)
            hipLaunchKernelGGL((split_grow_lds_kernel<TD, TH, TW, K, THREADS, STAGE>), dim3((unsigned)blocks), dim3(THREADS), 0,
                               st, mask, first, (const int *)plane[cur], plane[cur ^ 1], D, H, W, C, steps, tiles_x, tiles_y,
                               tiles_z);
        else
            hipLaunchKernelGGL(split_grow_step_kernel<DEPTH>, tgrid, blk, 0, st, mask, first, (const int *)plane[cur],
                               plane[cur ^ 1], total, D, H, W, C);
    }
    hipLaunchKernelGGL(split_cut_kernel<DEPTH>, tgrid, blk, 0, st, mask, (const int *)plane[cur], out, total, D, H, W, C);
    return sq_check_launch(who);
}

}  // namespace

extern "C" int64_t sq_mask_split_workspace(int N, int H, int W) { return split_bytes(volume_elements(N, 1, H, W)); }
extern "C" int64_t sq_volume_split_workspace(int N, int D, int H, int W) { return split_bytes(volume_elements(N, D, H, W)); }

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
    SQ_SPLIT_BUFFERS(who, 1, "(%d,%d,%d)", N, H, W);
    const int rc = sq_mask_morph_u8(mask, split_seed_plane(workspace, total), N, H, W, C, SQ_MORPH_ERODE, structure, erosions,
                                    stream);
    if (rc != SQ_OK) return rc;
    const char *e = getenv("SQ_SPLIT_LDS");                     // read per call: 0 is the one-step-per-launch form
    return split_run<1, SQ_SPLIT_TILE_ROWS, SQ_SPLIT_TILE_COLS, SQ_SPLIT_STEPS, 256, 25>(
        who, mask, out, N, 1, H, W, C, reach, !(e && e[0] == '0'), workspace, (hipStream_t)stream);
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
    SQ_SPLIT_BUFFERS(who, D, "(%d,%d,%d,%d)", N, D, H, W);
    uint8_t *seed = split_seed_plane(workspace, total);
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
    // read per call: 0 is the one-step-per-launch form, 1 the LDS bricks; otherwise the form that
    // tools/volume_split_bench.py measured faster (README.md)
    const char *e = getenv("SQ_SPLIT3D_LDS");
    const bool lds = e && (e[0] == '0' || e[0] == '1') ? e[0] == '1' : SQ_SPLIT3D_LDS_DEFAULT != 0;
    return split_run<SQ_SPLIT3D_TILE_D, SQ_SPLIT3D_TILE_H, SQ_SPLIT3D_TILE_W, SQ_SPLIT3D_STEPS, 512, 10>(
        who, mask, out, N, D, H, W, C, reach, lds, workspace, (hipStream_t)stream);
}
