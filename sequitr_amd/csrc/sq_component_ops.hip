// The two component operations of the clean-up (include/sequitr_hip.h, "Mask clean-up" and "Volume clean-up"), on the
// labelling of sq_ccl.h.  One implementation for (N, D, H, W) uint8 masks; a frame is a volume with D = 1 whose border is
// its four lateral faces.
//   fill_holes   : per class, label the complement plane; a root that owns a border voxel is no hole
//   clear_border : label the mask itself; a root that owns a voxel of the chosen faces goes
// Whatever is cleared or copied is cleared or copied by a kernel: a captured call is a chain of kernel nodes and nothing else.
#include "sq_cleanup.h"

namespace {

// the complement plane of class c; the first class also copies the mask to `out`
__global__ __launch_bounds__(256) void complement_kernel(const uint8_t *__restrict__ mask, uint8_t *__restrict__ comp,
                                                         uint8_t *__restrict__ out, int64_t total, int c, int copy) {
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const uint8_t v = mask[g];
        comp[g] = (int)v != c ? (uint8_t)1 : (uint8_t)0;
        if (copy) out[g] = v;
    }
}

// the per-voxel counts or flags, cleared after the labelling and just before they are used: cleared in the complement
// pass, before the labelling's traffic, the counts cost the checkerboard's fill_holes 7-10 % (0.39 -> 0.43 ms, 8 x 2048^2)
__global__ __launch_bounds__(256) void clear_kernel(int *__restrict__ flag, int64_t total) {
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) flag[g] = 0;
}

// voxels of a volume's faces the enumerator visits: 2 D W + 2 D H on the four lateral faces, plus 2 H W on the first and
// last plane unless `lateral`; voxels on edges come twice or three times
__host__ __device__ __forceinline__ int64_t face_count(int D, int H, int W, bool lateral) {
    return 2 * (int64_t)D * W + 2 * (int64_t)D * H + (lateral ? 0 : 2 * (int64_t)H * W);
}

// the k-th of them as a linear index into the (D, H, W) volume.  With D = 1 and `lateral` these are a frame's outer rows
// and columns: row 0, row H - 1, column 0, column W - 1.
__device__ __forceinline__ int64_t face_voxel(int64_t k, int D, int H, int W, bool lateral) {
    const int64_t HW = (int64_t)H * W, DW = (int64_t)D * W, DH = (int64_t)D * H;
    if (!lateral) {
        if (k < HW) return k;                                   // z = 0
        if (k < 2 * HW) return (D - 1) * HW + (k - HW);         // z = D - 1
        k -= 2 * HW;
    }
    if (k < DW) return (k / W) * HW + k % W;                    // h = 0
    if (k < 2 * DW) return ((k - DW) / W) * HW + (int64_t)(H - 1) * W + (k - DW) % W;   // h = H - 1
    k -= 2 * DW;
    if (k < DH) return (k / H) * HW + (k % H) * W;              // w = 0
    k -= DH;
    return (k / H) * HW + (k % H) * W + (W - 1);                // w = W - 1
}

// plane != 0 on a face voxel: its root gets `value` (every writer stores the same value)
__global__ __launch_bounds__(256) void face_roots_kernel(const uint8_t *__restrict__ plane, const int *__restrict__ parent,
                                                         int *__restrict__ info, int N, int D, int H, int W, int lateral,
                                                         int value) {
    const int64_t per = face_count(D, H, W, lateral != 0), items = (int64_t)N * per, DHW = (int64_t)D * H * W;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t g = (i / per) * DHW + face_voxel(i % per, D, H, W, lateral != 0);
        if (plane[g]) info[parent[g]] = value;
    }
}

__global__ __launch_bounds__(256) void count_kernel(const int *__restrict__ parent, int *__restrict__ info, int64_t total) {
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int p = parent[g];
        if (p >= 0 && info[p] >= 0) atomicAdd(&info[p], 1);     // -1: reached from the border, stays -1
    }
}

__global__ __launch_bounds__(256) void fill_kernel(const uint8_t *__restrict__ mask, const int *__restrict__ parent,
                                                   const int *__restrict__ info, uint8_t *__restrict__ out, int64_t total, int c,
                                                   int limit) {
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        if (mask[g] != 0 || out[g] != 0) continue;              // only background that no smaller class has taken
        const int a = info[parent[g]];                          // background is in the complement of every class
        if (a >= 0 && (limit <= 0 || a <= limit)) out[g] = (uint8_t)c;
    }
}

__global__ __launch_bounds__(256) void apply_kernel(const uint8_t *__restrict__ mask, const int *__restrict__ parent,
                                                    const int *__restrict__ flag, uint8_t *__restrict__ out, int64_t total,
                                                    int C) {
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int v = mask[g];
        out[g] = (v != 0 && v < C && flag[parent[g]]) ? (uint8_t)0 : (uint8_t)v;
    }
}

int64_t fill_holes_bytes(int64_t total) { return total < 0 ? -1 : (total * 9 + 15) / 16 * 16; }     // parent, info, the complement plane
int64_t clear_border_bytes(int64_t total) { return total < 0 ? -1 : (total * 8 + 15) / 16 * 16; }   // parent, flag

// the grids of both chains: a wave per row, a thread per voxel, a thread per border item
struct Grids {
    int rows;
    dim3 rgrid, tgrid, fgrid;
    Grids(int64_t total, int N, int D, int H, int W, bool lateral)
        : rows(N * D * H), rgrid((rows + 3) / 4), tgrid(cc_grid(total)), fgrid(cc_grid(N * face_count(D, H, W, lateral))) {}
};

// the entry has made SQ_CLEANUP_COMMON's checks; limit64 <= 0 or >= the element count: no limit
int fill_holes_impl(const char *who, const uint8_t *mask, uint8_t *out, int N, int D, int H, int W, int C, int64_t limit64,
                    int lateral, void *workspace, void *stream) {
    SQ_REQUIRE(workspace, "%s: null pointer", who);
    SQ_REQUIRE((((uintptr_t)workspace) & 15u) == 0, "%s: workspace must be 16-byte aligned", who);
    hipStream_t st = (hipStream_t)stream;
    const int64_t total = volume_elements(N, D, H, W);
    int *parent = reinterpret_cast<int *>(workspace);
    int *info = parent + total;
    uint8_t *comp = reinterpret_cast<uint8_t *>(info + total);
    const int limit = limit64 <= 0 || limit64 >= total ? 0 : (int)limit64;   // no component is larger than the mask
    const Grids g(total, N, D, H, W, lateral != 0);
    const dim3 blk(256);
    for (int c = 1; c < C; ++c) {
        hipLaunchKernelGGL(complement_kernel, g.tgrid, blk, 0, st, mask, comp, out, total, c, c == 1);
        hipLaunchKernelGGL(cc_rowscan_kernel<false>, g.rgrid, blk, 0, st, (const uint8_t *)comp, parent, (unsigned *)nullptr,
                           (u64 *)nullptr, g.rows, W);
        hipLaunchKernelGGL(cc_merge_kernel, g.tgrid, blk, 0, st, (const uint8_t *)comp, parent, total, D, H, W);
        hipLaunchKernelGGL(cc_compress_kernel, g.tgrid, blk, 0, st, parent, total);
        hipLaunchKernelGGL(clear_kernel, g.tgrid, blk, 0, st, info, total);
        hipLaunchKernelGGL(face_roots_kernel, g.fgrid, blk, 0, st, (const uint8_t *)comp, (const int *)parent, info, N, D, H, W,
                           lateral, -1);
        if (limit > 0) hipLaunchKernelGGL(count_kernel, g.tgrid, blk, 0, st, (const int *)parent, info, total);
        hipLaunchKernelGGL(fill_kernel, g.tgrid, blk, 0, st, mask, (const int *)parent, (const int *)info, out, total, c, limit);
    }
    return sq_check_launch(who);
}

int clear_border_impl(const char *who, const uint8_t *mask, uint8_t *out, int N, int D, int H, int W, int C, int lateral,
                      void *workspace, void *stream) {
    SQ_REQUIRE(workspace, "%s: null pointer", who);
    SQ_REQUIRE((((uintptr_t)workspace) & 15u) == 0, "%s: workspace must be 16-byte aligned", who);
    hipStream_t st = (hipStream_t)stream;
    const int64_t total = volume_elements(N, D, H, W);
    int *parent = reinterpret_cast<int *>(workspace);
    int *flag = parent + total;
    const Grids g(total, N, D, H, W, lateral != 0);
    const dim3 blk(256);
    hipLaunchKernelGGL(cc_rowscan_kernel<false>, g.rgrid, blk, 0, st, mask, parent, (unsigned *)nullptr, (u64 *)nullptr, g.rows, W);
    hipLaunchKernelGGL(cc_merge_kernel, g.tgrid, blk, 0, st, mask, parent, total, D, H, W);
    hipLaunchKernelGGL(cc_compress_kernel, g.tgrid, blk, 0, st, parent, total);
    hipLaunchKernelGGL(clear_kernel, g.tgrid, blk, 0, st, flag, total);
    hipLaunchKernelGGL(face_roots_kernel, g.fgrid, blk, 0, st, mask, (const int *)parent, flag, N, D, H, W, lateral, 1);
    hipLaunchKernelGGL(apply_kernel, g.tgrid, blk, 0, st, mask, (const int *)parent, (const int *)flag, out, total, C);
    return sq_check_launch(who);
}

}  // namespace

extern "C" int64_t sq_mask_fill_holes_workspace(int N, int H, int W) { return fill_holes_bytes(volume_elements(N, 1, H, W)); }
extern "C" int64_t sq_mask_clear_border_workspace(int N, int H, int W) { return clear_border_bytes(volume_elements(N, 1, H, W)); }
extern "C" int64_t sq_volume_fill_holes_workspace(int N, int D, int H, int W) {
    return fill_holes_bytes(volume_elements(N, D, H, W));
}
extern "C" int64_t sq_volume_clear_border_workspace(int N, int D, int H, int W) {
    return clear_border_bytes(volume_elements(N, D, H, W));
}

extern "C" int sq_mask_fill_holes_u8(const uint8_t *mask, uint8_t *out, int N, int H, int W, int C, int64_t max_area,
                                     void *workspace, void *stream) {
    const char *who = "sq_mask_fill_holes_u8";
    SQ_CLEANUP_COMMON(who, 1, "(%d,%d,%d)", N, H, W);
    return fill_holes_impl(who, mask, out, N, 1, H, W, C, max_area, 1, workspace, stream);
}

extern "C" int sq_mask_clear_border_u8(const uint8_t *mask, uint8_t *out, int N, int H, int W, int C, void *workspace,
                                       void *stream) {
    const char *who = "sq_mask_clear_border_u8";
    SQ_CLEANUP_COMMON(who, 1, "(%d,%d,%d)", N, H, W);
    return clear_border_impl(who, mask, out, N, 1, H, W, C, 1, workspace, stream);
}

extern "C" int sq_volume_fill_holes_u8(const uint8_t *mask, uint8_t *out, int N, int D, int H, int W, int C, int64_t max_voxels,
                                       void *workspace, void *stream) {
    const char *who = "sq_volume_fill_holes_u8";
    SQ_CLEANUP_COMMON(who, D, "(%d,%d,%d,%d)", N, D, H, W);
    return fill_holes_impl(who, mask, out, N, D, H, W, C, max_voxels, 0, workspace, stream);
}

extern "C" int sq_volume_clear_border_u8(const uint8_t *mask, uint8_t *out, int N, int D, int H, int W, int C, int faces,
                                         void *workspace, void *stream) {
    const char *who = "sq_volume_clear_border_u8";
    SQ_CLEANUP_COMMON(who, D, "(%d,%d,%d,%d)", N, D, H, W);
    SQ_REQUIRE(faces == SQ_FACES_ALL || faces == SQ_FACES_LATERAL, "%s: faces must be SQ_FACES_ALL or SQ_FACES_LATERAL, got %d",
               who, faces);
    return clear_border_impl(who, mask, out, N, D, H, W, C, faces == SQ_FACES_LATERAL, workspace, stream);
}
