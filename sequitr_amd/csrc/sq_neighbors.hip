// Cell neighbourhoods on the GPU (include/sequitr_hip.h, "Label zones and the zone contact graph").
//
// sq_label_zones_i32: the exact Euclidean feature transform of a label image, separable as sq_edt_sq_f32 is; the row and
//   column passes live in sq_zones.h, which the volumetric call (sq_neighbors3d.hip) shares.
// sq_zone_graph: sq_zones.h's contact graph without depth, the program sq_zone_graph3d runs on volumes.
// Integer work throughout: the same bits on every run, whatever order the atomics arrive in.
#include "sq_zones.h"

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

extern "C" int64_t sq_zone_graph_workspace(int max_pairs) { return graph_bytes(max_pairs, 1); }

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
    return zone_graph_run<false>("sq_zone_graph", zones, N, 1, H, W, max_label, stats, stb / 4, pairs, max_pairs, count, dropped,
                                 workspace, (hipStream_t)stream);
}
