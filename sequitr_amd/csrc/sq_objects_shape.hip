// Shape columns of the measured objects, from the labelling sq_objects_measure left in its workspace (sq_objects.h):
// second-order coordinate sums, exposed faces per axis, boundary voxels, and for planar masks the three counts of the
// 4-neighbourhood perimeter estimator.  Everything is an integer defined on the mask and accumulated with 64-bit integer
// atomics: exact, and independent of the order in which they arrive.
//   runs      : one wave per image row over 64-column segments (seg_scan, as obj_accumulate_kernel).  Per run segment the
//               last lane adds the segment's share of every sum to its object's row: the coordinate products in closed
//               form from the segment's ends, the exposed faces and boundary voxels as population counts of ballots
//               over the segment's lane range.  faces_c counts true run ends only: a run that goes on across a
//               segment seam has `same` set at the next lane 0 and its last lane here sees its own byte to the right.
//   perimeter : planar masks; a PT_H x PT_W tile of the mask with a halo of 2 in LDS, boundary flags for tile + halo 1 in
//               a second LDS array, then per boundary pixel the code 1 + 2 n4 + 10 n8 from the flags.  An edge
//               neighbour with my byte is in my object; a diagonal one is for certain only when one of the two pixels
//               between us carries the byte too, otherwise the roots in `parent` decide.  One wave covers one tile row:
//               a run of equal bytes along it is one object, its first lane adds the run's three counts.
//   emit      : the n rows in the order of the measure call's `slots`
// The table is cleared by a kernel of its own, so that the call is one plain chain of launches under graph capture.
#include "sq_objects.h"

namespace {

constexpr int SHAPE_MAX_DIM = 65536;                            // a coordinate product stays below 2^32
constexpr int PT_W = 64, PT_H = 32;                             // perimeter tile: one wave per tile row, 8 rows per wave

// one object's shape accumulators, 104 bytes; rows of the table in shape_workspace, indexed by the measure call's slot
struct ShapeAcc {
    u64 m2[6];                                                 // pp, rr, cc, pr, pc, rc
    u64 faces[3];                                              // along plane, row, column
    u64 boundary;
    u64 per[3];                                                // straight, diagonal, mixed
};
static_assert(sizeof(ShapeAcc) == 104, "ShapeAcc layout");

inline int64_t shape_table_bytes(int max_out) { return ((int64_t)max_out * (int64_t)sizeof(ShapeAcc) + 15) / 16 * 16; }

__device__ __forceinline__ void add_nz(u64 *p, u64 v) {
    if (v) atomicAdd(p, v);
}

// 0^2 + 1^2 + ... + n^2, n <= 65535: n (n + 1) (2 n + 1) < 2^50
__device__ __forceinline__ u64 squares_upto(u64 n) { return n * (n + 1ULL) * (2ULL * n + 1ULL) / 6ULL; }

__global__ __launch_bounds__(256) void shape_clear_kernel(u64 *__restrict__ t, int64_t words) {
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < words; g += (int64_t)gridDim.x * blockDim.x) t[g] = 0ULL;
}

__global__ __launch_bounds__(256) void shape_runs_kernel(const uint8_t *__restrict__ mask, const int *__restrict__ parent,
                                                         const int *__restrict__ slot, ShapeAcc *__restrict__ acc,
                                                         int n_slots, int rows, int planes, int H, int W) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;                                      // whole waves leave: every ballot / shuffle below is full
    const uint8_t *row = mask + (size_t)r * W;
    const int base = r * W, rowi = r % H, plane = (r / H) % planes;
    const ptrdiff_t HW = (ptrdiff_t)H * W;
    const bool has_up = rowi > 0, has_down = rowi + 1 < H, has_before = plane > 0, has_behind = plane + 1 < planes;
    int prev_last = 0;
    for (int c0 = 0; c0 < W; c0 += 64) {
        const SegScan s = seg_scan(row, W, c0, lane, prev_last);
        const bool next_same = __shfl_down((int)s.same, 1) != 0 && lane != 63;
        const int col = c0 + lane;
        const bool on = s.v != 0;                               // col < W here
        int right = __shfl_down(s.v, 1);
        if (lane == 63) right = col + 1 < W ? (int)row[col + 1] : 0;
        int up = 0, down = 0, before = 0, behind = 0;
        if (on) {
            if (has_up) up = row[col - W];
            if (has_down) down = row[col + W];
            if (has_before) before = row[col - HW];
            if (has_behind) behind = row[col + HW];
        }
        const bool xl = on && !s.same, xr = on && right != s.v;  // a frame edge reads as byte 0
        const bool xu = on && up != s.v, xd = on && down != s.v;
        const bool xb = on && planes > 1 && before != s.v, xh = on && planes > 1 && behind != s.v;
        const u64 BL = __ballot(xl), BR = __ballot(xr), BU = __ballot(xu), BD = __ballot(xd);
        const u64 BB = __ballot(xb), BH = __ballot(xh), BANY = __ballot(xl || xr || xu || xd || xb || xh);
        if (on && !next_same) {                                 // last lane of a run segment
            const int j = s.j >= 0 ? s.j : 0;                   // the part of the run inside this segment starts at lane j
            const int root = parent[base + col];
            const int sl = root >= 0 && root < rows * W ? slot[root] : -1;     // a root is a pixel of the mask
            if (sl >= 0 && sl < n_slots) {
                ShapeAcc *a = acc + sl;
                const u64 upto = lane == 63 ? ~0ULL : ((2ULL << lane) - 1ULL);
                const u64 range = upto & (~0ULL << j);          // lanes j .. lane
                const u64 len = (u64)(lane - j + 1), lo = (u64)(c0 + j), hi = (u64)col;
                const u64 sc = len * (lo + hi) / 2ULL;          // sum of c over lo .. hi
                const u64 scc = squares_upto(hi) - (lo ? squares_upto(lo - 1ULL) : 0ULL);
                const u64 p = (u64)plane, q = (u64)rowi;
                add_nz(&a->m2[0], len * p * p);
                add_nz(&a->m2[1], len * q * q);
                add_nz(&a->m2[2], scc);
                add_nz(&a->m2[3], len * p * q);
                add_nz(&a->m2[4], p * sc);
                add_nz(&a->m2[5], q * sc);
                add_nz(&a->faces[0], (u64)(__popcll(BB & range) + __popcll(BH & range)));
                add_nz(&a->faces[1], (u64)(__popcll(BU & range) + __popcll(BD & range)));
                add_nz(&a->faces[2], (u64)(__popcll(BL & range) + __popcll(BR & range)));
                add_nz(&a->boundary, (u64)__popcll(BANY & range));
            }
        }
        prev_last = __shfl(s.v, 63);
    }
}

// which of the three counters a boundary pixel with n4 edge and n8 diagonal boundary neighbours of its object feeds:
// 1 straight (codes 5 7 15 17 25 27), 2 diagonal (21 33), 3 mixed (13 23), 0 none; code = 1 + 2 n4 + 10 n8
__device__ __forceinline__ int perimeter_kind(int n4, int n8) {
    if ((n4 == 2 || n4 == 3) && n8 <= 2) return 1;
    if ((n4 == 0 && n8 == 2) || (n4 == 1 && n8 == 3)) return 2;
    if (n4 == 1 && (n8 == 1 || n8 == 2)) return 3;
    return 0;
}

__global__ __launch_bounds__(256) void shape_perimeter_kernel(const uint8_t *__restrict__ mask, const int *__restrict__ parent,
                                                              const int *__restrict__ slot, ShapeAcc *__restrict__ acc,
                                                              int n_slots, int H, int W, int tiles_x, int tiles_y) {
    __shared__ uint8_t m[PT_H + 4][PT_W + 4];                   // the tile and a halo of 2; outside the frame: 0
    __shared__ uint8_t fl[PT_H + 2][PT_W + 2];                  // boundary flags of the tile and a halo of 1
    const int t = blockIdx.x;
    const int tx = t % tiles_x, ty = (t / tiles_x) % tiles_y, n = t / (tiles_x * tiles_y);
    const int r0 = ty * PT_H, c0 = tx * PT_W;
    const int base = n * H * W;                                 // fewer than 2^31 pixels in all
    const uint8_t *frame = mask + (size_t)base;
    for (int i = threadIdx.x; i < (PT_H + 4) * (PT_W + 4); i += 256) {
        const int y = i / (PT_W + 4), x = i % (PT_W + 4);
        const int r = r0 + y - 2, c = c0 + x - 2;
        m[y][x] = (r >= 0 && r < H && c >= 0 && c < W) ? frame[(size_t)r * W + c] : (uint8_t)0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < (PT_H + 2) * (PT_W + 2); i += 256) {
        const int y = i / (PT_W + 2), x = i % (PT_W + 2);       // flag (y, x) belongs to m[y + 1][x + 1]
        const uint8_t v = m[y + 1][x + 1];
        fl[y][x] = v != 0 && (m[y][x + 1] != v || m[y + 2][x + 1] != v || m[y + 1][x] != v || m[y + 1][x + 2] != v);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int y = threadIdx.x >> 6; y < PT_H; y += 4) {
        const int r = r0 + y;
        if (r >= H) break;                                      // the same for the whole wave
        const int v = m[y + 2][lane + 2];                       // 0 right of the frame
        const int g = base + r * W + c0 + lane;                 // read only where v != 0, inside the frame
        int kind = 0;
        if (v != 0 && fl[y + 1][lane + 1]) {
            const int n4 = (fl[y][lane + 1] && m[y + 1][lane + 2] == v) + (fl[y + 2][lane + 1] && m[y + 3][lane + 2] == v)
                         + (fl[y + 1][lane] && m[y + 2][lane + 1] == v) + (fl[y + 1][lane + 2] && m[y + 2][lane + 3] == v);
            int n8 = 0, root = -1;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const int dy = (d & 2) - 1, dx = 2 * (d & 1) - 1;
                if (!fl[y + 1 + dy][lane + 1 + dx] || m[y + 2 + dy][lane + 2 + dx] != v) continue;
                bool same = m[y + 2 + dy][lane + 2] == v || m[y + 2][lane + 2 + dx] == v;
                if (!same) {                                    // same byte, touching at a corner only: the roots decide
                    if (root < 0) root = parent[g];
                    same = parent[g + dy * W + dx] == root;
                }
                n8 += same;
            }
            kind = perimeter_kind(n4, n8);
        }
        const u64 K1 = __ballot(kind == 1), K2 = __ballot(kind == 2), K3 = __ballot(kind == 3);
        // runs of equal byte along the row are runs of one object: the first lane of each adds the run's counts
        const int prev = __shfl_up(v, 1);
        const bool start = lane == 0 || prev != v;
        const u64 starts = __ballot(start);
        if ((K1 | K2 | K3) == 0ULL || !start || v == 0) continue;
        const u64 after = lane == 63 ? 0ULL : (starts & (~0ULL << (lane + 1)));
        const int end = after ? __ffsll((long long)after) - 1 : 64;
        const u64 run = (end == 64 ? ~0ULL : ((1ULL << end) - 1ULL)) & (~0ULL << lane);
        const int k1 = __popcll(K1 & run), k2 = __popcll(K2 & run), k3 = __popcll(K3 & run);
        if ((k1 | k2 | k3) == 0) continue;
        const int root = parent[g];
        if (root < base || root - base >= H * W) continue;      // a root is a pixel of my frame
        const int sl = slot[root];
        if (sl < 0 || sl >= n_slots) continue;
        add_nz(&acc[sl].per[0], (u64)k1);
        add_nz(&acc[sl].per[1], (u64)k2);
        add_nz(&acc[sl].per[2], (u64)k3);
    }
}

__global__ __launch_bounds__(256) void shape_emit_kernel(const ObjAcc *__restrict__ acc, const ShapeAcc *__restrict__ shape,
                                                         const int *__restrict__ slots, int n, int n_slots,
                                                         long long *__restrict__ out) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        long long *o = out + 16 * (size_t)i;
        const int s = slots[i];
        if (s < 0 || s >= n_slots) {                            // not a slot of this workspace: an empty row
            for (int k = 0; k < 16; ++k) o[k] = 0;
            continue;
        }
        const ObjAcc a = acc[s];
        const ShapeAcc b = shape[s];
        o[0] = (long long)a.splane;
        o[1] = (long long)a.srow;
        o[2] = (long long)a.scol;
        for (int k = 0; k < 6; ++k) o[3 + k] = (long long)b.m2[k];
        for (int k = 0; k < 3; ++k) o[9 + k] = (long long)b.faces[k];
        o[12] = (long long)b.boundary;
        for (int k = 0; k < 3; ++k) o[13 + k] = (long long)b.per[k];
    }
}

}  // namespace

extern "C" int64_t sq_objects_shape_workspace(int max_out) {
    if (max_out <= 0) return -1;
    return shape_table_bytes(max_out);
}

extern "C" int sq_objects_shape(const uint8_t *mask, int N, int planes, int H, int W, const void *workspace, int n_slots,
                                const int32_t *slots, int n, void *shape_workspace, int64_t *shape_i, void *stream) {
    const char *who = "sq_objects_shape";
    SQ_REQUIRE(mask && workspace && slots && shape_workspace && shape_i, "%s: null pointer", who);
    SQ_REQUIRE(N > 0 && planes > 0 && H > 0 && W > 0 && (int64_t)N * planes * H * W < ((int64_t)1 << 31),
               "%s: the mask must have fewer than 2^31 elements", who);
    SQ_REQUIRE(planes <= SHAPE_MAX_DIM && H <= SHAPE_MAX_DIM && W <= SHAPE_MAX_DIM,
               "%s: planes, H and W may not exceed %d (the second-order sums must stay below 2^63), got (%d,%d,%d)", who,
               SHAPE_MAX_DIM, planes, H, W);
    SQ_REQUIRE(n_slots >= 1 && n >= 0 && n <= n_slots, "%s: n must lie in 0 .. n_slots, got n %d, n_slots %d", who, n, n_slots);
    SQ_REQUIRE((((uintptr_t)workspace) & 15u) == 0 && (((uintptr_t)shape_workspace) & 15u) == 0,
               "%s: workspace and shape_workspace must be 16-byte aligned", who);
    SqObjFilled f;
    SQ_REQUIRE(sq_obj_recall(workspace, &f), "%s: n_slots %d matches nothing: sq_objects_measure has not filled this workspace",
               who, n_slots);
    SQ_REQUIRE(f.N == N && f.planes == planes && f.H == H && f.W == W && f.max_out == n_slots,
               "%s: n_slots %d and mask (%d,%d,%d,%d) do not match the sq_objects_measure call that filled this workspace "
               "(max_out %d, mask (%d,%d,%d,%d))", who, n_slots, N, planes, H, W, f.max_out, f.N, f.planes, f.H, f.W);
    if (n == 0) return SQ_OK;
    hipStream_t st = (hipStream_t)stream;
    const int64_t total = (int64_t)N * planes * H * W;
    const ObjAcc *acc = reinterpret_cast<const ObjAcc *>(workspace);
    const int *parent = reinterpret_cast<const int *>(reinterpret_cast<const char *>(workspace) + obj_table_bytes(n_slots));
    const int *slot = parent + total;
    ShapeAcc *shape = reinterpret_cast<ShapeAcc *>(shape_workspace);
    const int rows = N * planes * H;
    const dim3 blk(256);
    const int64_t words = (int64_t)n_slots * (int64_t)(sizeof(ShapeAcc) / 8);
    hipLaunchKernelGGL(shape_clear_kernel, dim3(cc_grid(words)), blk, 0, st, reinterpret_cast<u64 *>(shape_workspace), words);
    hipLaunchKernelGGL(shape_runs_kernel, dim3((rows + 3) / 4), blk, 0, st, mask, parent, slot, shape, n_slots, rows, planes,
                       H, W);
    if (planes == 1) {
        const int tiles_x = (W + PT_W - 1) / PT_W, tiles_y = (H + PT_H - 1) / PT_H;
        hipLaunchKernelGGL(shape_perimeter_kernel, dim3((unsigned)((int64_t)N * tiles_x * tiles_y)), blk, 0, st, mask, parent,
                           slot, shape, n_slots, H, W, tiles_x, tiles_y);
    }
    hipLaunchKernelGGL(shape_emit_kernel, dim3(cc_grid(n)), blk, 0, st, acc, shape, slots, n, n_slots,
                       reinterpret_cast<long long *>(shape_i));
    return sq_check_launch(who);
}
