// Cell neighbourhoods in volumes (include/sequitr_hip.h, "Label zones and the contact graph in volumes").
//
// sq_label_zones3d_i32: the 3-D feature transform with a pinned tie rule, one more separable pass on top of the planar one:
//   planar half : zone_rows_kernel / zone_cols_kernel<true> (sq_zones.h) over the N*D slices, UNBOUNDED: per voxel P, the
//                 exact integer squared distance to the slice's nearest seed (P_INF: the slice holds none), and L, the
//                 smallest label among the slice's seeds at that distance
//   depth pass  : the lexicographic minimum over z' of (A(z - z') + P(z'), L(z')), A(k) = fl(fl(k dz) fl(k dz)), searched
//                 outwards from z while A(k) <= the best distance so far -- <=, not sq_edt3d_sq_f64's <: an equidistant
//                 seed with a smaller label further out must still be seen.  The products and the sum are explicit
//                 round-to-nearest operations (__dmul_rn / __dadd_rn), which the compiler may not contract into an fma.
// sq_zone_graph3d: sq_zones.h's contact graph with depth, the program sq_zone_graph runs on frames.
// A minimum of fixed expressions and sums of integers: the same bits on every run.
#include <cmath>
#include <cstdlib>

#include "sq_zones.h"

namespace {

constexpr int CS3 = 32;                // columns (w, the contiguous axis) of a block's strip: one 32-lane LDS group reads
                                       // 32 consecutive dwords of one slice -- no bank conflict, whatever k the other half is at

// ---- zones: depth ---------------------------------------------------------------------------------------------------
// LOADP(z') -> P and LOADL(z') -> L of slice z' at this (n, h, w); L is fetched only where it can matter.
// `limit`: +inf, or R*R when only the zone within the reach is wanted (a candidate beyond it cannot give a zone).
template <class LOADP, class LOADL>
__device__ __forceinline__ void zones3d_search(LOADP loadp, LOADL loadl, int z, int D, double dz, double limit,
                                               double *best_out, int *zone_out) {
    double best = (double)INFINITY;
    int zone = 0;
    const int p0 = loadp(z);
    if (p0 != P_INF) {
        best = (double)p0;
        zone = loadl(z);
    }
    for (int k = 1; k < D; ++k) {
        const int za = z - k, zb = z + k;
        if (za < 0 && zb >= D) break;
        const double t = __dmul_rn((double)k, dz);
        const double a = __dmul_rn(t, t);
        if (a > best || a > limit) break;                       // A is non-decreasing in k and the same on both sides
        if (za >= 0) {
            const int p = loadp(za);
            if (p != P_INF) {
                const double c = __dadd_rn(a, (double)p);
                if (c <= best) {
                    const int l = loadl(za);
                    if (c < best || l < zone) zone = l;
                    best = c;
                }
            }
        }
        if (zb < D) {
            const int p = loadp(zb);
            if (p != P_INF) {
                const double c = __dadd_rn(a, (double)p);
                if (c <= best) {
                    const int l = loadl(zb);
                    if (c < best || l < zone) zone = l;
                    best = c;
                }
            }
        }
    }
    *best_out = best;
    *zone_out = zone;
}

// LDS form: a block owns the strip of CS3 columns of one (n, h) row with (P, L) of ALL D slices in LDS, as two arrays
// [D][CS3] of 4 B (8 B x D x CS3 in all); lanes run along w, so the fill reads coalesced row segments
template <bool WANT_D2>
__global__ __launch_bounds__(256) void zones3d_depth_lds_kernel(const int *__restrict__ P, const int *__restrict__ L,
                                                                int *__restrict__ zones, double *__restrict__ d2out, int D,
                                                                int H, int W, double dz, double reach2, double limit) {
    extern __shared__ __attribute__((aligned(16))) int zs[];                  // P [D][CS3], then L [D][CS3]
    int *ps = zs, *ls = zs + D * CS3;
    const int strips = (W + CS3 - 1) / CS3;
    const int w0 = (int)(blockIdx.x % strips) * CS3, h = (int)((blockIdx.x / strips) % H);
    const int n = (int)(blockIdx.x / ((unsigned)strips * H));
    const size_t plane = (size_t)H * W, row0 = (size_t)n * D * plane + (size_t)h * W;
    for (int i = threadIdx.x; i < D * CS3; i += 256) {
        const int z = i / CS3, w = w0 + i % CS3;
        const size_t q = row0 + (size_t)z * plane + w;
        ps[i] = w < W ? P[q] : P_INF;
        ls[i] = w < W ? L[q] : 0;
    }
    __syncthreads();
    const int wl = threadIdx.x % CS3, w = w0 + wl;
    if (w >= W) return;
    const int *pc = ps + wl, *lc = ls + wl;
    for (int z = threadIdx.x / CS3; z < D; z += 256 / CS3) {
        double best;
        int zone;
        zones3d_search([&](int zz) { return pc[zz * CS3]; }, [&](int zz) { return lc[zz * CS3]; }, z, D, dz, limit, &best,
                       &zone);
        const size_t p = row0 + (size_t)z * plane + w;
        zones[p] = best <= reach2 ? zone : 0;
        if (WANT_D2) d2out[p] = best;
    }
}

// the same search on global memory, for depths whose strip does not fit in LDS (and SQ_ZONES3D_LDS=0)
template <bool WANT_D2>
__global__ __launch_bounds__(256) void zones3d_depth_kernel(const int *__restrict__ P, const int *__restrict__ L,
                                                            int *__restrict__ zones, double *__restrict__ d2out, int N, int D,
                                                            int H, int W, double dz, double reach2, double limit) {
    const int64_t plane = (int64_t)H * W, total = (int64_t)N * D * plane;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (int64_t)gridDim.x * blockDim.x) {
        const int z = (int)((p / plane) % D);
        const int64_t col = p - (int64_t)z * plane;             // slice 0 of this voxel's own volume
        const int *pc = P + col, *lc = L + col;
        double best;
        int zone;
        zones3d_search([&](int zz) { return pc[(int64_t)zz * plane]; }, [&](int zz) { return lc[(int64_t)zz * plane]; }, z, D,
                       dz, limit, &best, &zone);
        zones[p] = best <= reach2 ? zone : 0;
        if (WANT_D2) d2out[p] = best;
    }
}

struct Zones3dWs {
    int64_t flags, field, total;       // bytes: the per-slice flags, then P, L and gl (int32 each, `field` bytes), then g (u16)
};

inline bool zones3d_layout(int N, int D, int H, int W, Zones3dWs *l) {
    if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || D >= G_INF || H >= G_INF || W >= G_INF) return false;
    const int64_t vox = (int64_t)N * D * H * W;                 // < 2^31 * 30000: no overflow before the test
    if ((int64_t)N * D >= ((int64_t)1 << 31) || vox >= ((int64_t)1 << 31)) return false;
    l->flags = (((int64_t)N * D + 3) / 4) * 16;
    l->field = ((vox * 4 + 15) / 16) * 16;
    l->total = (l->flags + 3 * l->field + vox * 2 + 15) / 16 * 16;
    return true;
}

inline int zones3d_lds_limit() {
    static const int limit = [] {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || v <= 0)
            return 64 * 1024;
        return v;
    }();
    return limit;
}

template <bool WANT_D2>
int zones3d_depth(const int *P, const int *L, int *zones, double *d2, int N, int D, int H, int W, double dz, int R,
                  hipStream_t st) {
    const double reach2 = R > 0 ? (double)R * (double)R : (double)INFINITY;
    const double limit = WANT_D2 ? (double)INFINITY : reach2;   // d2 = D3 beyond the reach too: then the search runs on
    // SQ_ZONES3D_LDS=0: A/B switch to the global-memory form, read per launch
    const char *e = getenv("SQ_ZONES3D_LDS");
    const int64_t lds = (int64_t)D * CS3 * 8;
    if (!(e && e[0] == '0') && lds <= zones3d_lds_limit()) {
        auto kern = zones3d_depth_lds_kernel<WANT_D2>;
        if (lds > 48 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
            sq_set_error("sq_label_zones3d_i32: cannot reserve %d bytes of LDS", (int)lds);
            return SQ_ELAUNCH;
        }
        const int64_t blocks = (int64_t)N * H * ((W + CS3 - 1) / CS3);         // <= N*H*W < 2^31
        hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), (size_t)lds, st, P, L, zones, d2, D, H, W, dz, reach2,
                           limit);
    } else {
        hipLaunchKernelGGL(zones3d_depth_kernel<WANT_D2>, dim3(nb_grid((int64_t)N * D * H * W)), dim3(256), 0, st, P, L, zones,
                           d2, N, D, H, W, dz, reach2, limit);
    }
    return sq_check_launch("sq_label_zones3d_i32");
}

}  // namespace

extern "C" int64_t sq_label_zones3d_workspace(int N, int D, int H, int W) {
    Zones3dWs l;
    return zones3d_layout(N, D, H, W, &l) ? l.total : -1;
}

extern "C" int sq_label_zones3d_i32(const int32_t *labels, int32_t *zones, double *d2, int N, int D, int H, int W,
                                    int max_label, int max_distance, double dz, void *workspace, void *stream) {
    SQ_REQUIRE(labels && zones && workspace, "sq_label_zones3d_i32: null pointer");
    Zones3dWs l;
    SQ_REQUIRE(zones3d_layout(N, D, H, W, &l), "sq_label_zones3d_i32: need 0 < D, H, W < %d and N*D*H*W < 2^31", G_INF);
    SQ_REQUIRE(max_label >= 1 && max_label < (1 << LABEL_BITS), "sq_label_zones3d_i32: max_label %d is outside 1 .. 2^21 - 1",
               max_label);
    SQ_REQUIRE(max_distance >= 0 && max_distance <= MAX_REACH, "sq_label_zones3d_i32: max_distance %d is outside 0 .. %d",
               max_distance, MAX_REACH);
    SQ_REQUIRE(std::isfinite(dz) && dz > 0.0, "sq_label_zones3d_i32: the depth spacing must be finite and > 0");
    SQ_REQUIRE((((uintptr_t)workspace) & 15u) == 0, "sq_label_zones3d_i32: workspace must be 16-byte aligned");
    SQ_REQUIRE((((uintptr_t)d2) & 7u) == 0, "sq_label_zones3d_i32: d2 must be 8-byte aligned");
    const int64_t vox = (int64_t)N * D * H * W;
    SQ_REQUIRE(!overlaps(workspace, l.total, labels, vox * 4) && !overlaps(workspace, l.total, zones, vox * 4) &&
                   !(d2 && overlaps(workspace, l.total, d2, vox * 8)),
               "sq_label_zones3d_i32: the workspace must not overlap labels, zones or d2");
    SQ_REQUIRE(!(d2 && overlaps(d2, vox * 8, zones, vox * 4)), "sq_label_zones3d_i32: zones and d2 must not overlap");
    hipStream_t st = (hipStream_t)stream;
    char *base = reinterpret_cast<char *>(workspace);
    int *flag = reinterpret_cast<int *>(base);
    int *P = reinterpret_cast<int *>(base + l.flags);
    int *L = reinterpret_cast<int *>(base + l.flags + l.field);
    int *gl = reinterpret_cast<int *>(base + l.flags + 2 * l.field);
    unsigned short *g = reinterpret_cast<unsigned short *>(base + l.flags + 3 * l.field);
    // planar half over the N*D slices, unbounded: zones -> L, d2 -> P (P_INF and 0 in a slice without a seed)
    const int S = N * D;
    hipLaunchKernelGGL(clear_words_kernel, dim3(nb_grid(S)), dim3(256), 0, st, reinterpret_cast<unsigned *>(flag), (int64_t)S,
                       (unsigned *)nullptr, (int64_t)0, (int *)nullptr, (int *)nullptr);
    int rc = sq_check_launch("sq_label_zones3d_i32");
    if (rc) return rc;
    const int rows = S * H;                                     // <= voxels < 2^31
    hipLaunchKernelGGL(zone_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, labels, g, gl, flag, rows, H, W, max_label);
    rc = sq_check_launch("sq_label_zones3d_i32");
    if (rc) return rc;
    hipLaunchKernelGGL(zone_cols_kernel<true>, dim3(nb_grid(vox)), dim3(256), 0, st, g, gl, flag, L, P, S, H, W, 0);
    rc = sq_check_launch("sq_label_zones3d_i32");
    if (rc) return rc;
    return d2 ? zones3d_depth<true>(P, L, zones, d2, N, D, H, W, dz, max_distance, st)
              : zones3d_depth<false>(P, L, zones, nullptr, N, D, H, W, dz, max_distance, st);
}

extern "C" int64_t sq_zone_graph3d_workspace(int max_pairs) { return graph_bytes(max_pairs, 2); }

extern "C" int sq_zone_graph3d(const int32_t *zones, int N, int D, int H, int W, int max_label, int64_t *stats,
                               int32_t *pairs, int max_pairs, int32_t *count, int32_t *dropped, void *workspace,
                               void *stream) {
    SQ_REQUIRE(zones && stats && pairs && count && dropped && workspace, "sq_zone_graph3d: null pointer");
    SQ_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0 && N < (1 << LABEL_BITS) && (int64_t)N * D < ((int64_t)1 << 31) &&
                   (int64_t)N * D * H < ((int64_t)1 << 31) && (int64_t)N * D * H * W < ((int64_t)1 << 31),
               "sq_zone_graph3d: need N, D, H, W > 0, N < 2^21 and N*D*H*W < 2^31");
    SQ_REQUIRE(max_label >= 1 && max_label < (1 << LABEL_BITS), "sq_zone_graph3d: max_label %d is outside 1 .. 2^21 - 1",
               max_label);
    SQ_REQUIRE(max_pairs >= 1 && max_pairs <= (1 << 28), "sq_zone_graph3d: max_pairs %d is outside 1 .. 2^28", max_pairs);
    SQ_REQUIRE((((uintptr_t)workspace) & 15u) == 0 && (((uintptr_t)stats) & 7u) == 0,
               "sq_zone_graph3d: workspace must be 16-byte and stats 8-byte aligned");
    const int64_t wsb = sq_zone_graph3d_workspace(max_pairs), stb = (int64_t)N * ((int64_t)max_label + 1) * 16;
    SQ_REQUIRE(!overlaps(workspace, wsb, zones, (int64_t)N * D * H * W * 4) && !overlaps(workspace, wsb, stats, stb) &&
                   !overlaps(workspace, wsb, pairs, (int64_t)max_pairs * 20) && !overlaps(workspace, wsb, count, 4) &&
                   !overlaps(workspace, wsb, dropped, 4),
               "sq_zone_graph3d: the workspace must not overlap zones or an output");
    return zone_graph_run<true>("sq_zone_graph3d", zones, N, D, H, W, max_label, stats, stb / 4, pairs, max_pairs, count, dropped,
                                workspace, (hipStream_t)stream);
}
