// Mask -> connected components -> centroids on the GPU: the step after the segmentation hot path
// (CentroidWriter.write, sequitr/utils.py:531-578: per frame and per class c > 0,
// scipy.ndimage.label(out == c) with the default 4-connectivity, then center_of_mass of every label).
//
// All classes are labelled in one pass: two pixels are connected iff they are 4-neighbours AND carry the
// same class value > 0.  Union-find with the smaller linear index as the root, so a component's root is
// its first pixel in raster order -- scipy numbers its labels in exactly that order.
//   1. row scan   : one wave per image row; parent = first pixel of the horizontal run (ballot + clz, no
//                   atomics); accumulators zeroed at run starts (a root is always one)
//   2. merge      : one union per place where a run starts to overlap a run of the row above
//   3. compress   : parent = root
//   4. accumulate : row scan again; one atomic triple (count, sum row, sum col) per run segment, integer
//                   arithmetic => exact and order-independent
//   5. emit       : every root writes [frame, x = row centre, y = col centre, 0, class] and its sort key
// HBM-bound integer/byte work: ~1 B/pixel of mask read three times + 4 B/pixel of parent written and read
// a few times; the accumulators are touched only at roots.
// The labelling phase (steps 1 to 3) is sq_ccl.h, shared with the object measurements (sq_objects.hip).
#include "sq_ccl.h"

namespace {

__global__ __launch_bounds__(256) void cc_accumulate_kernel(const uint8_t *__restrict__ mask,
                                                            const int *__restrict__ parent, unsigned *__restrict__ cnt,
                                                            u64 *__restrict__ sums, int rows, int planes, int H,
                                                            int W) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const uint8_t *row = mask + (size_t)r * W;
    const int base = r * W, rowi = r % H, plane = (r / H) % planes;
    int prev_last = 0;
    for (int c0 = 0; c0 < W; c0 += 64) {
        const SegScan s = seg_scan(row, W, c0, lane, prev_last);
        const bool next_same = __shfl_down((int)s.same, 1) != 0 && lane != 63;
        if (s.v != 0 && !next_same) {                           // last lane of a run segment
            const int j = s.j >= 0 ? s.j : 0;                    // the part of the run inside this segment
            const unsigned len = (unsigned)(lane - j + 1);
            const int root = parent[base + c0 + lane];
            atomicAdd(&cnt[root], len);
            atomicAdd(&sums[3 * (size_t)root], (u64)len * (u64)rowi);
            atomicAdd(&sums[3 * (size_t)root + 1], (u64)len * (u64)(2 * c0 + lane + j) / 2ULL);
            if (planes > 1) atomicAdd(&sums[3 * (size_t)root + 2], (u64)len * (u64)plane);
        }
        prev_last = __shfl(s.v, 63);
    }
}

__global__ __launch_bounds__(256) void cc_emit_kernel(const uint8_t *__restrict__ mask, const int *__restrict__ parent,
                                                      const unsigned *__restrict__ cnt, const u64 *__restrict__ sums,
                                                      int64_t total, int planes, int H, int W,
                                                      int *__restrict__ count, float *__restrict__ out,
                                                      int *__restrict__ keys, int max_out) {
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        if (parent[g] != (int)g) continue;
        const int idx = atomicAdd(count, 1);
        if (idx >= max_out) continue;
        const double c = (double)mask[g];
        // scipy.ndimage.center_of_mass(out, labels, index): sum(out * grid) / sum(out) in float64, out == c
        const double norm = c * (double)cnt[g];
        const float crow = (float)(c * (double)sums[3 * (size_t)g] / norm);
        const float ccol = (float)(c * (double)sums[3 * (size_t)g + 1] / norm);
        out[5 * (size_t)idx + 0] = (float)(g / ((int64_t)planes * H * W));
        if (planes > 1) {                                       // (x, y, z) = the three axes of the volume in order
            out[5 * (size_t)idx + 1] = (float)(c * (double)sums[3 * (size_t)g + 2] / norm);
            out[5 * (size_t)idx + 2] = crow;
            out[5 * (size_t)idx + 3] = ccol;
        } else {
            out[5 * (size_t)idx + 1] = crow;
            out[5 * (size_t)idx + 2] = ccol;
            out[5 * (size_t)idx + 3] = 0.0f;
        }
        out[5 * (size_t)idx + 4] = (float)c;
        keys[idx] = (int)g;
    }
}

}  // namespace

static int centroids_launch(const uint8_t *mask, int N, int planes, int H, int W, void *workspace, int32_t *count, float *out,
                            int32_t *keys, int max_out, void *stream, const char *who) {
    SQ_REQUIRE(mask && workspace && count && out && keys && max_out > 0, "%s: null pointer", who);
    SQ_REQUIRE(N > 0 && planes > 0 && H > 0 && W > 0 && (int64_t)N * planes * H * W < ((int64_t)1 << 31),
               "%s: the mask must have fewer than 2^31 elements", who);
    SQ_REQUIRE((((uintptr_t)workspace) & 15u) == 0, "%s: workspace must be 16-byte aligned", who);
    hipStream_t st = (hipStream_t)stream;
    const int64_t total = (int64_t)N * planes * H * W;
    unsigned long long *sums = reinterpret_cast<unsigned long long *>(workspace);     // 8-byte items first
    int *parent = reinterpret_cast<int *>(sums + 3 * total);
    unsigned *cnt = reinterpret_cast<unsigned *>(parent + total);
    const int rows = N * planes * H;
    if (hipMemsetAsync(count, 0, sizeof(int32_t), st) != hipSuccess) {
        sq_set_error("%s: cannot clear the counter", who);
        return SQ_ELAUNCH;
    }
    hipLaunchKernelGGL(cc_rowscan_kernel<true>, dim3((rows + 3) / 4), dim3(256), 0, st, mask, parent, cnt, sums, rows, W);
    hipLaunchKernelGGL(cc_merge_kernel, dim3(cc_grid(total)), dim3(256), 0, st, mask, parent, total, planes, H, W);
    hipLaunchKernelGGL(cc_compress_kernel, dim3(cc_grid(total)), dim3(256), 0, st, parent, total);
    hipLaunchKernelGGL(cc_accumulate_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, mask, parent, cnt, sums, rows, planes, H,
                       W);
    hipLaunchKernelGGL(cc_emit_kernel, dim3(cc_grid(total)), dim3(256), 0, st, mask, parent, cnt, sums, total, planes, H, W,
                       count, out, keys, max_out);
    return sq_check_launch(who);
}

extern "C" int64_t sq_mask_centroids_workspace(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0 || (int64_t)N * H * W >= ((int64_t)1 << 31)) return -1;
    return (int64_t)N * H * W * (4 + 4 + 24);                  // parent, count, three coordinate sums
}

extern "C" int sq_mask_centroids_u8(const uint8_t *mask, int N, int H, int W, void *workspace, int32_t *count,
                                    float *out, int32_t *keys, int max_out, void *stream) {
    return centroids_launch(mask, N, 1, H, W, workspace, count, out, keys, max_out, stream, "sq_mask_centroids_u8");
}

// volumes: mask (N, D0, D1, D2) uint8, 6-connectivity; rows [frame, x, y, z, class] with (x, y, z) the centre along
// (D0, D1, D2); workspace = sq_mask_centroids_workspace(N * D0, D1, D2)
extern "C" int sq_volume_centroids_u8(const uint8_t *mask, int N, int D0, int D1, int D2, void *workspace, int32_t *count,
                                      float *out, int32_t *keys, int max_out, void *stream) {
    return centroids_launch(mask, N, D0, D1, D2, workspace, count, out, keys, max_out, stream, "sq_volume_centroids_u8");
}
