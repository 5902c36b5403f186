// Cell neighbourhoods on the GPU (include/sequitr_hip.h, "Label zones and the zone contact graph").
//
// sq_label_zones_i32: the exact Euclidean feature transform of a label image, separable as sq_edt_sq_f32 is; the row and
//   column passes live in sq_zones.h, which the volumetric call (sq_neighbors3d.hip) shares.
// sq_zone_graph: one wave per image row; runs of equal zone / equal (a, b) along the row make ONE atomic each.
// Integer work throughout: the same bits on every run, whatever order the atomics arrive in.
#include "sq_zones.h"

namespace {

// ---- graph ----------------------------------------------------------------------------------------------------------
// insert-and-add into the open-addressing table: the key is claimed with a 64-bit compare-and-swap, the count is a 32-bit add
__device__ __forceinline__ void table_add(u64 *__restrict__ keys, unsigned *__restrict__ counts, unsigned slots, u64 key,
                                          unsigned len, int *__restrict__ dropped) {
    unsigned s = (unsigned)mix64(key) & (slots - 1u);
    for (unsigned i = 0; i < slots; ++i) {
        u64 k = __atomic_load_n(&keys[s], __ATOMIC_RELAXED);
        if (k == 0ULL) {
            k = atomicCAS(&keys[s], 0ULL, key);
            if (k == 0ULL) k = key;
        }
        if (k == key) {
            atomicAdd(&counts[s], len);
            return;
        }
        s = (s + 1u) & (slots - 1u);
    }
    atomicAdd(dropped, 1);                                      // every slot holds another pair
}

__global__ __launch_bounds__(256) void zone_graph_kernel(const int *__restrict__ zones, long long *__restrict__ stats,
                                                         u64 *__restrict__ keys, unsigned *__restrict__ counts,
                                                         unsigned slots, int *__restrict__ dropped, int rows, int H, int W,
                                                         int max_label) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;                                      // whole waves leave
    const int n = r / H, y = r % H;
    const int *row = zones + (size_t)r * W;
    const bool edge_row = y == 0 || y == H - 1;
    long long *st = stats + (size_t)n * ((size_t)max_label + 1) * 2;
    for (int c0 = 0; c0 < W; c0 += 64) {
        const int col = c0 + lane;
        const bool in = col < W;
        int z = in ? row[col] : 0, zr = 0, zd = 0;
        if (z < 1 || z > max_label) z = 0;
        if (in && y + 1 < H) {
            zd = row[col + W];
            if (zd < 1 || zd > max_label) zd = 0;
        }
        int right = __shfl_down(z, 1);
        if (lane == 63) {
            right = col + 1 < W ? row[col + 1] : 0;
            if (right < 1 || right > max_label) right = 0;
        }
        zr = right;
        // areas and frame-border pixels: one 64-bit add per run of equal zone
        u64 mask = 0;
        const u64 E = __ballot(in && (edge_row || col == 0 || col == W - 1));
        int len = run_length((u64)z, lane, &mask);
        if (len) {
            atomicAdd((u64 *)&st[(size_t)z * 2], (u64)len);
            const int e = __popcll(E & mask);
            if (e) atomicAdd((u64 *)&st[(size_t)z * 2 + 1], (u64)e);
        }
        // pixel pairs (p, right neighbour) and (p, lower neighbour) whose zones differ, both > 0
        const u64 head = (u64)n << (2 * LABEL_BITS);
        const u64 kh = pair_key(head, z, zr);
        const u64 kv = pair_key(head, z, zd);
        len = run_length(kh, lane, &mask);
        if (len) table_add(keys, counts, slots, kh, (unsigned)len, dropped);
        len = run_length(kv, lane, &mask);
        if (len) table_add(keys, counts, slots, kv, (unsigned)len, dropped);
    }
}

__global__ __launch_bounds__(256) void zone_graph_compact_kernel(const u64 *__restrict__ keys,
                                                                 const unsigned *__restrict__ counts, unsigned slots,
                                                                 int *__restrict__ pairs, int max_pairs,
                                                                 int *__restrict__ count, int *__restrict__ dropped) {
    for (unsigned s = blockIdx.x * blockDim.x + threadIdx.x; s < slots; s += gridDim.x * blockDim.x) {
        const u64 k = keys[s];
        if (k == 0ULL) continue;
        const int idx = atomicAdd(count, 1);
        if (idx < 0 || idx >= max_pairs) {                      // only once max_pairs rows are written: count ends at max_pairs
            atomicSub(count, 1);
            atomicAdd(dropped, 1);
            continue;
        }
        int *row = pairs + (size_t)idx * 4;
        row[0] = (int)(k >> (2 * LABEL_BITS));
        row[1] = (int)((k >> LABEL_BITS) & LABEL_MASK);
        row[2] = (int)(k & LABEL_MASK);
        row[3] = (int)counts[s];
    }
}

}  // namespace

extern "C" int64_t sq_label_zones_workspace(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0 || H >= G_INF || W >= G_INF || (int64_t)N * H * W >= ((int64_t)1 << 31)) return -1;
    return ((int64_t)((N + 3) / 4) * 16 + (int64_t)N * H * W * 6 + 15) / 16 * 16;
}

extern "C" int sq_label_zones_i32(const int32_t *labels, int32_t *zones, int32_t *d2, int N, int H, int W, int max_label,
                                  int max_distance, void *workspace, void *stream) {
    SQ_REQUIRE(labels && zones && workspace, "sq_label_zones_i32: null pointer");
    SQ_REQUIRE(N > 0 && H > 0 && W > 0 && H < G_INF && W < G_INF && (int64_t)N * H * W < ((int64_t)1 << 31),
               "sq_label_zones_i32: need 0 < H, W < %d and N*H*W < 2^31", G_INF);
    SQ_REQUIRE(max_label >= 1 && max_label < (1 << LABEL_BITS), "sq_label_zones_i32: max_label %d is outside 1 .. 2^21 - 1",
               max_label);
    SQ_REQUIRE(max_distance >= 0 && max_distance <= MAX_REACH, "sq_label_zones_i32: max_distance %d is outside 0 .. %d",
               max_distance, MAX_REACH);
    SQ_REQUIRE((((uintptr_t)workspace) & 15u) == 0, "sq_label_zones_i32: workspace must be 16-byte aligned");
    const int64_t px = (int64_t)N * H * W, wsb = sq_label_zones_workspace(N, H, W);
    SQ_REQUIRE(!overlaps(workspace, wsb, labels, px * 4) && !overlaps(workspace, wsb, zones, px * 4) &&
                   !(d2 && overlaps(workspace, wsb, d2, px * 4)),
               "sq_label_zones_i32: the workspace must not overlap labels, zones or d2");
    SQ_REQUIRE(!(d2 && overlaps(d2, px * 4, zones, px * 4)), "sq_label_zones_i32: zones and d2 must not overlap");
    hipStream_t st = (hipStream_t)stream;
    int *flag = reinterpret_cast<int *>(workspace);
    int *gl = flag + ((N + 3) / 4) * 4;
    unsigned short *g = reinterpret_cast<unsigned short *>(gl + px);
    hipLaunchKernelGGL(clear_words_kernel, dim3(nb_grid(N)), dim3(256), 0, st, reinterpret_cast<unsigned *>(flag), (int64_t)N,
                       (unsigned *)nullptr, (int64_t)0, (int *)nullptr, (int *)nullptr);
    int rc = sq_check_launch("sq_label_zones_i32");
    if (rc) return rc;
    const int rows = N * H;
    hipLaunchKernelGGL(zone_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, labels, g, gl, flag, rows, H, W, max_label);
    rc = sq_check_launch("sq_label_zones_i32");
    if (rc) return rc;
    if (d2)
        hipLaunchKernelGGL(zone_cols_kernel<true>, dim3(nb_grid(px)), dim3(256), 0, st, g, gl, flag, zones, d2, N, H, W,
                           max_distance);
    else
        hipLaunchKernelGGL(zone_cols_kernel<false>, dim3(nb_grid(px)), dim3(256), 0, st, g, gl, flag, zones, (int *)nullptr, N,
                           H, W, max_distance);
    return sq_check_launch("sq_label_zones_i32");
}

extern "C" int64_t sq_zone_graph_workspace(int max_pairs) {
    if (max_pairs < 1 || max_pairs > (1 << 28)) return -1;
    return (graph_slots(max_pairs) * 12 + 15) / 16 * 16;
}

extern "C" int sq_zone_graph(const int32_t *zones, int N, int H, int W, int max_label, int64_t *stats, int32_t *pairs,
                             int max_pairs, int32_t *count, int32_t *dropped, void *workspace, void *stream) {
    SQ_REQUIRE(zones && stats && pairs && count && dropped && workspace, "sq_zone_graph: null pointer");
    SQ_REQUIRE(N > 0 && H > 0 && W > 0 && (int64_t)N * H * W < ((int64_t)1 << 31) && N < (1 << LABEL_BITS),
               "sq_zone_graph: need N, H, W > 0, N < 2^21 and N*H*W < 2^31");
    SQ_REQUIRE(max_label >= 1 && max_label < (1 << LABEL_BITS), "sq_zone_graph: max_label %d is outside 1 .. 2^21 - 1",
               max_label);
    SQ_REQUIRE(max_pairs >= 1 && max_pairs <= (1 << 28), "sq_zone_graph: max_pairs %d is outside 1 .. 2^28", max_pairs);
    SQ_REQUIRE((((uintptr_t)workspace) & 15u) == 0 && (((uintptr_t)stats) & 7u) == 0,
               "sq_zone_graph: workspace must be 16-byte and stats 8-byte aligned");
    const int64_t wsb = sq_zone_graph_workspace(max_pairs), stb = (int64_t)N * ((int64_t)max_label + 1) * 16;
    SQ_REQUIRE(!overlaps(workspace, wsb, zones, (int64_t)N * H * W * 4) && !overlaps(workspace, wsb, stats, stb) &&
                   !overlaps(workspace, wsb, pairs, (int64_t)max_pairs * 16) && !overlaps(workspace, wsb, count, 4) &&
                   !overlaps(workspace, wsb, dropped, 4),
               "sq_zone_graph: the workspace must not overlap zones or an output");
    hipStream_t st = (hipStream_t)stream;
    const unsigned slots = (unsigned)graph_slots(max_pairs);
    u64 *keys = reinterpret_cast<u64 *>(workspace);
    unsigned *counts = reinterpret_cast<unsigned *>(keys + slots);
    const int64_t table_words = (int64_t)slots * 3, stat_words = stb / 4;
    hipLaunchKernelGGL(clear_words_kernel, dim3(nb_grid(table_words > stat_words ? table_words : stat_words)), dim3(256), 0, st,
                       reinterpret_cast<unsigned *>(workspace), table_words, reinterpret_cast<unsigned *>(stats), stat_words,
                       count, dropped);
    int rc = sq_check_launch("sq_zone_graph");
    if (rc) return rc;
    const int rows = N * H;
    hipLaunchKernelGGL(zone_graph_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, zones, reinterpret_cast<long long *>(stats),
                       keys, counts, slots, dropped, rows, H, W, max_label);
    rc = sq_check_launch("sq_zone_graph");
    if (rc) return rc;
    hipLaunchKernelGGL(zone_graph_compact_kernel, dim3(nb_grid(slots)), dim3(256), 0, st, keys, counts, slots, pairs, max_pairs,
                       count, dropped);
    return sq_check_launch("sq_zone_graph");
}
