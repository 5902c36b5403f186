// Linking objects from frame to frame (include/sequitr_hip.h, "Label overlap and relabelling").
//
// sq_label_overlap: the sparse contingency table of two label stacks.  A wave takes groups of 64 (one-lane form) or 256
//   (four-lane form) consecutive positions of one frame; runs of equal (la, lb) along memory make ONE insert-and-add each,
//   runs of equal label one 64-bit add each.  Integer work throughout: the same bits on every run, whatever order the
//   atomics arrive in.
// sq_relabel_lut_i32: label frames rewritten through a per-frame slice of one table; a streaming kernel.
#include <stdlib.h>
#include "sq_zones.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));

// insert-and-add into the open-addressing table, as in sq_zone_graph: the key is claimed with a 64-bit compare-and-swap,
// the count is a 32-bit add
__device__ __forceinline__ void overlap_add(u64 *__restrict__ keys, unsigned *__restrict__ counts, unsigned slots, u64 key,
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
    atomicAdd(dropped, 1);                                      // every slot holds another triple
}

__device__ __forceinline__ int in_range(int v, int max_label) { return (v < 1 || v > max_label) ? 0 : v; }

// the 64-bit key of (frame, la, lb); 0 = nothing to count (la > 0 makes every real key non-zero)
__device__ __forceinline__ u64 overlap_key(u64 head, int la, int lb) {
    return (la && lb) ? (head | ((u64)la << LABEL_BITS) | (u64)lb) : 0ULL;
}

struct OverlapArgs {
    const int *a, *b;
    long long *area_a, *area_b;                                 // may be null
    u64 *keys;
    unsigned *counts;
    unsigned slots;
    int *dropped;
    int N, max_label;
    int64_t P;
};

// Wave-chunk w = (frame n, chunk c of the frame's cpf chunks), walked as w, w + G, w + 2G, ... by the grid's G waves.  The
// two 64-bit divisions are made once; a step is two adds and a carry.  The wave's number goes through readfirstlane, so
// that n and c -- and with them the frame's base address -- are scalar values.
struct WaveWalk {
    int64_t w, n, c, step, dn, dc;
    __device__ __forceinline__ explicit WaveWalk(int64_t cpf) {
        const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        step = (int64_t)gridDim.x * 4;
        w = (int64_t)blockIdx.x * 4 + wave;
        n = w / cpf;
        c = w - n * cpf;
        dn = step / cpf;
        dc = step - dn * cpf;
    }
    __device__ __forceinline__ void next(int64_t cpf) {
        w += step;
        n += dn;
        c += dc;
        if (c >= cpf) {
            c -= cpf;
            ++n;
        }
    }
};

// ---- one lane per position ------------------------------------------------------------------------------------------
// wave-chunk = (frame n, LANE_U x 64 positions); every wave of the grid walks its chunks with a trip count that is uniform
// within the wave, so every ballot / shuffle below is full.  The chunk's 2 LANE_U loads are issued before any of them is
// used; a group of 64 positions without a label in either stack -- most of a frame is background -- is left at once.
constexpr int LANE_U = 4;
__global__ __launch_bounds__(256) void label_overlap_kernel(OverlapArgs g) {
    const int lane = threadIdx.x & 63;
    const int64_t cpf = (g.P + 64 * LANE_U - 1) / (64 * LANE_U), total = cpf * g.N;
    WaveWalk k(cpf);
    for (; k.w < total; k.next(cpf)) {
        const int64_t n = k.n, p0 = k.c * (64 * LANE_U) + lane;
        const int *fa = g.a + n * g.P, *fb = g.b + n * g.P;
        int va[LANE_U], vb[LANE_U];
#pragma unroll
        for (int u = 0; u < LANE_U; ++u) {
            const int64_t p = p0 + u * 64;
            va[u] = p < g.P ? fa[p] : 0;
            vb[u] = p < g.P ? fb[p] : 0;
        }
        const u64 head = (u64)n << (2 * LABEL_BITS);
        const size_t row = (size_t)n * ((size_t)g.max_label + 1);
#pragma unroll
        for (int u = 0; u < LANE_U; ++u) {
            const int la = in_range(va[u], g.max_label), lb = in_range(vb[u], g.max_label);
            if (__ballot((la | lb) != 0) == 0ULL) continue;     // wave-uniform
            u64 mask = 0;
            const u64 key = overlap_key(head, la, lb);
            int len = run_length(key, lane, &mask);
            if (len) overlap_add(g.keys, g.counts, g.slots, key, (unsigned)len, g.dropped);
            if (g.area_a) {                                     // uniform over the grid
                len = run_length((u64)la, lane, &mask);
                if (len) atomicAdd((u64 *)&g.area_a[row + la], (u64)len);
            }
            if (g.area_b) {
                len = run_length((u64)lb, lane, &mask);
                if (len) atomicAdd((u64 *)&g.area_b[row + lb], (u64)len);
            }
        }
    }
}

// ---- four positions per lane ----------------------------------------------------------------------------------------
// Runs are merged inside the lane first: a lane whose four keys are equal (nearly every lane: inside an object, or in the
// background) enters the wave's run search with that key and a weight of 4; a lane that sees a change leaves the search
// (key 0, which also ends its neighbours' runs) and adds its at most four runs itself.
template <class Add>
__device__ __forceinline__ void add_runs4(u64 k0, u64 k1, u64 k2, u64 k3, int lane, Add add) {
    const bool uniform = k0 == k1 && k1 == k2 && k2 == k3;
    u64 mask = 0;
    const int len = run_length(uniform ? k0 : 0ULL, lane, &mask);
    if (len) add(k0, 4u * (unsigned)len);
    if (!uniform) {
        u64 cur = k0;
        unsigned c = 1;
        const u64 k[3] = {k1, k2, k3};
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (k[i] == cur) {
                ++c;
            } else {
                if (cur) add(cur, c);
                cur = k[i];
                c = 1;
            }
        }
        if (cur) add(cur, c);
    }
}

// needs a, b 16-byte aligned and P % 4 == 0 (every frame then starts on 16 bytes and no quad straddles two frames);
// wave-chunk = (frame n, VEC_U x 256 positions), loads first and background left at once as in the one-lane form
constexpr int VEC_U = 2;
__global__ __launch_bounds__(256) void label_overlap_vec_kernel(OverlapArgs g) {
    const int lane = threadIdx.x & 63;
    const int64_t cpf = (g.P + 256 * VEC_U - 1) / (256 * VEC_U), total = cpf * g.N;
    WaveWalk k(cpf);
    for (; k.w < total; k.next(cpf)) {
        const int64_t n = k.n, p0 = k.c * (256 * VEC_U) + lane * 4;
        const int *fa = g.a + n * g.P, *fb = g.b + n * g.P;
        i32x4 va[VEC_U], vb[VEC_U];
#pragma unroll
        for (int u = 0; u < VEC_U; ++u) {
            const int64_t p = p0 + u * 256;
            va[u] = vb[u] = i32x4{0, 0, 0, 0};
            if (p < g.P) {                                      // P % 4 == 0: the quad lies inside the frame
                va[u] = *reinterpret_cast<const i32x4 *>(fa + p);
                vb[u] = *reinterpret_cast<const i32x4 *>(fb + p);
            }
        }
        const u64 head = (u64)n << (2 * LABEL_BITS);
        const size_t row = (size_t)n * ((size_t)g.max_label + 1);
#pragma unroll
        for (int u = 0; u < VEC_U; ++u) {
            int la[4], lb[4], any = 0;
            u64 key[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                la[i] = in_range(va[u][i], g.max_label);
                lb[i] = in_range(vb[u][i], g.max_label);
                key[i] = overlap_key(head, la[i], lb[i]);
                any |= la[i] | lb[i];
            }
            if (__ballot(any != 0) == 0ULL) continue;           // wave-uniform
            add_runs4(key[0], key[1], key[2], key[3], lane,
                      [&](u64 kk, unsigned len) { overlap_add(g.keys, g.counts, g.slots, kk, len, g.dropped); });
            if (g.area_a)
                add_runs4((u64)la[0], (u64)la[1], (u64)la[2], (u64)la[3], lane,
                          [&](u64 l, unsigned len) { atomicAdd((u64 *)&g.area_a[row + l], (u64)len); });
            if (g.area_b)
                add_runs4((u64)lb[0], (u64)lb[1], (u64)lb[2], (u64)lb[3], lane,
                          [&](u64 l, unsigned len) { atomicAdd((u64 *)&g.area_b[row + l], (u64)len); });
        }
    }
}

__global__ __launch_bounds__(256) void label_overlap_compact_kernel(const u64 *__restrict__ keys,
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

// the table, the two area arrays, count and dropped: cleared by a kernel of the call's own chain
__global__ __launch_bounds__(256) void label_overlap_clear_kernel(unsigned *__restrict__ t, int64_t nt, unsigned *__restrict__ a,
                                                                  unsigned *__restrict__ b, int64_t nab, int *__restrict__ count,
                                                                  int *__restrict__ dropped) {
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = i0; i < nt; i += step) t[i] = 0u;
    if (a)
        for (int64_t i = i0; i < nab; i += step) a[i] = 0u;
    if (b)
        for (int64_t i = i0; i < nab; i += step) b[i] = 0u;
    if (i0 == 0) {
        *count = 0;
        *dropped = 0;
    }
}

// ---- relabel --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int lut_value(int L, int64_t lo, int64_t cnt, const int *__restrict__ lut, int64_t lut_len) {
    if (L < 1 || (int64_t)L > cnt) return 0;
    const int64_t i = lo + L - 1;
    return (i >= 0 && i < lut_len) ? lut[i] : 0;                // an entry that points outside the table reads as 0
}

// block-chunk c = (frame n, 256 * V positions); V = 4: 16-byte loads and stores (labels, out aligned, P % 4 == 0).
// labels and out are not __restrict__: out == labels is allowed, every thread reads its positions before it writes them.
template <int V>
__global__ __launch_bounds__(256) void relabel_lut_kernel(const int *labels, int *out, int N, int64_t P,
                                                          const long long *__restrict__ offsets, const int *__restrict__ lut,
                                                          int64_t lut_len) {
    const int64_t cpf = (P + 256 * V - 1) / (256 * V), total = cpf * N;
    for (int64_t c = blockIdx.x; c < total; c += gridDim.x) {
        const int64_t n = c / cpf, p = (c - n * cpf) * (256 * V) + (int64_t)threadIdx.x * V;
        if (p >= P) continue;
        const int64_t lo = offsets[n], cnt = offsets[n + 1] - lo;
        if constexpr (V == 4) {
            i32x4 v = *reinterpret_cast<const i32x4 *>(labels + n * P + p);
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = lut_value(v[i], lo, cnt, lut, lut_len);
            *reinterpret_cast<i32x4 *>(out + n * P + p) = v;
        } else {
            out[n * P + p] = lut_value(labels[n * P + p], lo, cnt, lut, lut_len);
        }
    }
}

inline unsigned chunk_grid(int64_t chunks) { return (unsigned)(chunks < 1 ? 1 : (chunks > 32768 ? 32768 : chunks)); }

}  // namespace

extern "C" int64_t sq_label_overlap_workspace(int max_pairs) {
    if (max_pairs < 1 || max_pairs > (1 << 28)) return -1;
    return (graph_slots(max_pairs) * 12 + 15) / 16 * 16;
}

extern "C" int sq_label_overlap(const int32_t *a, const int32_t *b, int N, int64_t P, int max_label, int64_t *area_a,
                                int64_t *area_b, int32_t *pairs, int max_pairs, int32_t *count, int32_t *dropped,
                                void *workspace, void *stream) {
    SQ_REQUIRE(a && b && pairs && count && dropped && workspace, "sq_label_overlap: null pointer");
    SQ_REQUIRE(N >= 1 && N < (1 << LABEL_BITS) && P >= 1 && P < ((int64_t)1 << 31),
               "sq_label_overlap: need 1 <= N < 2^21 and 1 <= P < 2^31");      // hence N*P < 2^52 < 2^63
    SQ_REQUIRE(max_label >= 1 && max_label < (1 << LABEL_BITS), "sq_label_overlap: max_label %d is outside 1 .. 2^21 - 1",
               max_label);
    SQ_REQUIRE(max_pairs >= 1 && max_pairs <= (1 << 28), "sq_label_overlap: max_pairs %d is outside 1 .. 2^28", max_pairs);
    SQ_REQUIRE((((uintptr_t)workspace) & 15u) == 0, "sq_label_overlap: workspace must be 16-byte aligned");
    SQ_REQUIRE((((uintptr_t)area_a) & 7u) == 0 && (((uintptr_t)area_b) & 7u) == 0,
               "sq_label_overlap: the area arrays must be 8-byte aligned");
    const int64_t wsb = sq_label_overlap_workspace(max_pairs), inb = (int64_t)N * P * 4,
                  arb = (int64_t)N * ((int64_t)max_label + 1) * 8;
    SQ_REQUIRE(!overlaps(workspace, wsb, a, inb) && !overlaps(workspace, wsb, b, inb) &&
                   !overlaps(workspace, wsb, pairs, (int64_t)max_pairs * 16) && !overlaps(workspace, wsb, count, 4) &&
                   !overlaps(workspace, wsb, dropped, 4) && !(area_a && overlaps(workspace, wsb, area_a, arb)) &&
                   !(area_b && overlaps(workspace, wsb, area_b, arb)),
               "sq_label_overlap: the workspace must not overlap an input or an output");
    hipStream_t st = (hipStream_t)stream;
    const unsigned slots = (unsigned)graph_slots(max_pairs);
    OverlapArgs g;
    g.a = a;
    g.b = b;
    g.area_a = reinterpret_cast<long long *>(area_a);
    g.area_b = reinterpret_cast<long long *>(area_b);
    g.keys = reinterpret_cast<u64 *>(workspace);
    g.counts = reinterpret_cast<unsigned *>(g.keys + slots);
    g.slots = slots;
    g.dropped = dropped;
    g.N = N;
    g.max_label = max_label;
    g.P = P;
    const int64_t table_words = (int64_t)slots * 3, area_words = (area_a || area_b) ? arb / 4 : 0;
    hipLaunchKernelGGL(label_overlap_clear_kernel, dim3(nb_grid(table_words > area_words ? table_words : area_words)), dim3(256),
                       0, st, reinterpret_cast<unsigned *>(workspace), table_words, reinterpret_cast<unsigned *>(area_a),
                       reinterpret_cast<unsigned *>(area_b), area_words, count, dropped);
    int rc = sq_check_launch("sq_label_overlap");
    if (rc) return rc;
    // SQ_LINK_VEC=0|1: A/B switch between the one-lane and the four-lane form, read per call; the four-lane form needs
    // both bases on 16 bytes and P % 4 == 0, anything else takes the one-lane form
    const char *e = getenv("SQ_LINK_VEC");
    const bool want_vec = e && e[0] ? e[0] != '0' : SQ_LINK_VEC_DEFAULT != 0;
    if (want_vec && SQ_ALIGNED16(a) && SQ_ALIGNED16(b) && P % 4 == 0) {
        const int64_t waves = (P + 256 * VEC_U - 1) / (256 * VEC_U) * N;
        hipLaunchKernelGGL(label_overlap_vec_kernel, dim3(chunk_grid((waves + 3) / 4)), dim3(256), 0, st, g);
    } else {
        const int64_t waves = (P + 64 * LANE_U - 1) / (64 * LANE_U) * N;
        hipLaunchKernelGGL(label_overlap_kernel, dim3(chunk_grid((waves + 3) / 4)), dim3(256), 0, st, g);
    }
    rc = sq_check_launch("sq_label_overlap");
    if (rc) return rc;
    hipLaunchKernelGGL(label_overlap_compact_kernel, dim3(nb_grid(slots)), dim3(256), 0, st, g.keys, g.counts, slots, pairs,
                       max_pairs, count, dropped);
    return sq_check_launch("sq_label_overlap");
}

extern "C" int sq_relabel_lut_i32(const int32_t *labels, int32_t *out, int N, int64_t P, const int64_t *offsets,
                                  const int32_t *lut, int64_t lut_len, void *stream) {
    SQ_REQUIRE(labels && out && offsets, "sq_relabel_lut_i32: null pointer");
    SQ_REQUIRE(lut_len >= 0 && (lut || lut_len == 0), "sq_relabel_lut_i32: null lut with lut_len %lld", (long long)lut_len);
    SQ_REQUIRE(N >= 1 && N < (1 << LABEL_BITS) && P >= 1 && P < ((int64_t)1 << 31),
               "sq_relabel_lut_i32: need 1 <= N < 2^21 and 1 <= P < 2^31");
    SQ_REQUIRE((((uintptr_t)offsets) & 7u) == 0, "sq_relabel_lut_i32: offsets must be 8-byte aligned");
    const int64_t nb = (int64_t)N * P * 4;
    SQ_REQUIRE(out == labels || !overlaps(out, nb, labels, nb),
               "sq_relabel_lut_i32: out must be labels itself (in place) or not overlap it");
    SQ_REQUIRE(!overlaps(out, nb, offsets, ((int64_t)N + 1) * 8) && !(lut_len && overlaps(out, nb, lut, lut_len * 4)),
               "sq_relabel_lut_i32: out must not overlap offsets or lut");
    hipStream_t st = (hipStream_t)stream;
    const long long *off = reinterpret_cast<const long long *>(offsets);
    if (SQ_ALIGNED16(labels) && SQ_ALIGNED16(out) && P % 4 == 0)
        hipLaunchKernelGGL(relabel_lut_kernel<4>, dim3(chunk_grid((P + 1023) / 1024 * N)), dim3(256), 0, st, labels, out, N, P,
                           off, lut, lut_len);
    else
        hipLaunchKernelGGL(relabel_lut_kernel<1>, dim3(chunk_grid((P + 255) / 256 * N)), dim3(256), 0, st, labels, out, N, P,
                           off, lut, lut_len);
    return sq_check_launch("sq_relabel_lut_i32");
}
