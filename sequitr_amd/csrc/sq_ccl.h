// Connected-component labelling shared by the centroid path (sq_centroids.hip) and the object measurements
// (sq_objects.hip): all classes in one pass, two pixels connected iff they are neighbours (4 in a plane, plus the same
// pixel of the previous plane for volumes) AND carry the same class value > 0.  Union-find with the smaller linear index
// as the root, so a component's root is its first pixel in raster order -- scipy numbers its labels in exactly that order.
//   row scan : one wave per image row; parent = first pixel of the horizontal run (ballot + clz, no atomics)
//   merge    : one union per place where a run starts to overlap a run of the row (plane) above
//   compress : parent = root
// Every definition sits in an anonymous namespace: each translation unit that includes this header gets its own copy.
#pragma once
#include "sq_common.h"

namespace {

typedef unsigned long long u64;

__device__ __forceinline__ int cc_find(const int *parent, int a) {
    int p = parent[a];
    while (p != a) {
        a = p;
        p = parent[a];
    }
    return a;
}

__device__ __forceinline__ void cc_unite(int *parent, int a, int b) {
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }          // a = larger root, hangs under b
        const int old = atomicMin(&parent[a], b);
        if (old == a) return;
        a = old;                                               // someone re-rooted a meanwhile: retry from there
    }
}

// Row scan shared by the labelling and the accumulation kernels.  For the 64-pixel segment starting at column c0 of one
// row: v = class of this lane's pixel (0 outside the row), `same` = continues the run of the pixel to its left,
// j = lane index where this lane's run starts inside the segment, or -1 when it started in an earlier
// segment (then `carry` = that run's start column).
struct SegScan {
    int v;
    bool same;
    int j;
};

__device__ __forceinline__ SegScan seg_scan(const uint8_t *__restrict__ row, int W, int c0, int lane, int prev_last) {
    SegScan s;
    const int col = c0 + lane;
    s.v = col < W ? (int)row[col] : 0;
    int left = __shfl_up(s.v, 1);
    if (lane == 0) left = prev_last;
    s.same = s.v != 0 && s.v == left;
    const u64 B = __ballot(s.same);
    const u64 upto = lane == 63 ? ~0ULL : ((2ULL << lane) - 1ULL);
    const u64 m = ~B & upto;                                   // lanes <= mine that START something
    s.j = m ? 63 - __clzll((long long)m) : -1;
    return s;
}

// SUMS: also zero the per-pixel accumulators of the centroid path at run starts (a root is always one); without it
// cnt and sums are not touched and may be null
template <bool SUMS>
__global__ __launch_bounds__(256) void cc_rowscan_kernel(const uint8_t *__restrict__ mask, int *__restrict__ parent,
                                                         unsigned *__restrict__ cnt, u64 *__restrict__ sums,
                                                         int rows, int W) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const uint8_t *row = mask + (size_t)r * W;
    const int base = r * W;
    int prev_last = 0, carry = 0;
    for (int c0 = 0; c0 < W; c0 += 64) {
        const SegScan s = seg_scan(row, W, c0, lane, prev_last);
        const int start = s.j >= 0 ? c0 + s.j : carry;
        const int col = c0 + lane;
        if (col < W) {
            const int g = base + col;
            parent[g] = s.v ? base + start : -1;
            if (SUMS && s.v && start == col) {                  // a root is always the first pixel of a run
                cnt[g] = 0u;
                sums[3 * (size_t)g] = 0ULL;
                sums[3 * (size_t)g + 1] = 0ULL;
                sums[3 * (size_t)g + 2] = 0ULL;
            }
        }
        prev_last = __shfl(s.v, 63);
        carry = __shfl(start, 63);
    }
}

// planes: 1 for images; for volumes every frame is `planes` consecutive (H, W) planes and voxels are also
// linked to the same-class voxel of the previous plane (6-connectivity, scipy's default 3-D structure)
__global__ __launch_bounds__(256) void cc_merge_kernel(const uint8_t *__restrict__ mask, int *__restrict__ parent,
                                                       int64_t total, int planes, int H, int W) {
    const int64_t HW = (int64_t)H * W;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int col = (int)(g % W), rowi = (int)((g / W) % H), plane = (int)((g / HW) % planes);
        const int v = mask[g];
        if (v == 0) continue;
        const bool left_same = col > 0 && mask[g - 1] == v;
        // the pixel to the left makes the same link when it is in my run and also touches the same neighbour run
        if (rowi > 0 && mask[g - W] == v && !(left_same && mask[g - W - 1] == v)) cc_unite(parent, (int)g, (int)(g - W));
        if (plane > 0 && mask[g - HW] == v && !(left_same && mask[g - HW - 1] == v)) cc_unite(parent, (int)g, (int)(g - HW));
    }
}

__global__ __launch_bounds__(256) void cc_compress_kernel(int *__restrict__ parent, int64_t total) {
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int p = parent[g];
        if (p >= 0) parent[g] = cc_find(parent, p);
    }
}

inline unsigned cc_grid(int64_t items) {
    int64_t b = (items + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

}  // namespace
