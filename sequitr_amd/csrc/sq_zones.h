// What the planar and the volumetric neighbourhood calls share (sq_neighbors.hip, sq_neighbors3d.hip): the two planar
// passes of the feature transform, the clearing kernel, and the contact graph (its run / hash helpers serve sq_link.hip
// too).  Everything sits in an unnamed namespace: each translation unit gets its own copy, as with the other headers.
//   rows    : per pixel the distance g along its row to the nearest seed and the smaller label of the at most two
//             seeds at that distance; one wave per row over 64-pixel segments, the seed ballot, the nearest set bit
//             to the left / right (clz / ffs) with a carry between segments, the label fetched from that lane
//   columns : the lexicographic minimum over y' of (g(y',x)^2 + (y-y')^2, label(y',x)), searched outwards from y
//             while dy^2 <= the best distance so far (<=, not <: an equidistant seed with a smaller label further
//             out must still be seen); lanes run along x, every read is a coalesced row segment
#pragma once
#include "sq_common.h"

namespace {

typedef unsigned long long u64;
constexpr int G_INF = 30000;           // "no seed in this row": 30000^2 + 30000^2 < 2^31
constexpr int P_INF = 0x7fffffff;      // "no seed in this frame"
constexpr int MAX_REACH = 46340;       // R * R fits an int32

// ---- zones: rows ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void zone_rows_kernel(const int *__restrict__ labels, unsigned short *__restrict__ g,
                                                        int *__restrict__ gl, int *__restrict__ has_seed, int rows, int H,
                                                        int W, int max_label) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;                                      // whole waves leave: every ballot / shuffle below is full
    const int *row = labels + (size_t)r * W;
    unsigned short *grow = g + (size_t)r * W;
    int *lrow = gl + (size_t)r * W;
    // left-to-right: the nearest seed at or before this pixel
    int last = -G_INF, last_label = 0;                          // column and label of the last seed seen so far
    bool any = false;
    for (int c0 = 0; c0 < W; c0 += 64) {
        const int col = c0 + lane;
        int L = col < W ? row[col] : 0;
        if (L < 1 || L > max_label) L = 0;
        const u64 F = __ballot(L != 0);
        const u64 upto = lane == 63 ? ~0ULL : ((2ULL << lane) - 1ULL);
        const u64 m = F & upto;
        const int src = m ? 63 - __clzll((long long)m) : 0;
        const int fetched = __shfl(L, src);
        if (col < W) {
            const int d = col - (m ? c0 + src : last);
            grow[col] = (unsigned short)(d < G_INF ? d : G_INF);
            lrow[col] = m ? fetched : last_label;
        }
        if (F) {
            const int hi = 63 - __clzll((long long)F);
            last = c0 + hi;
            last_label = __shfl(L, hi);
            any = true;
        }
    }
    // right-to-left: combine with the nearest seed at or after this pixel; at equal distance the smaller label stays
    int next = 2 * G_INF, next_label = 0;
    const int nseg = (W + 63) / 64;
    for (int sgm = nseg - 1; sgm >= 0; --sgm) {
        const int c0 = sgm * 64, col = c0 + lane;
        int L = col < W ? row[col] : 0;
        if (L < 1 || L > max_label) L = 0;
        const u64 F = __ballot(L != 0);
        const u64 m = F & (~0ULL << lane);                      // lanes >= mine
        const int src = m ? __ffsll((long long)m) - 1 : 0;
        const int fetched = __shfl(L, src);
        if (col < W) {
            const int d = (m ? c0 + src : next) - col;
            const int lab = m ? fetched : next_label;
            const int old = grow[col];
            if (d < old) {
                grow[col] = (unsigned short)d;
                lrow[col] = lab;
            } else if (d == old && old < G_INF && lab < lrow[col]) {
                lrow[col] = lab;
            }
        }
        if (F) {
            const int lo = __ffsll((long long)F) - 1;
            next = c0 + lo;
            next_label = __shfl(L, lo);
        }
    }
    if (any && lane == 0) atomicOr(&has_seed[r / H], 1);
}

// ---- zones: columns -------------------------------------------------------------------------------------------------
// FULL: the search runs until no row can hold a candidate (d2 is wanted, and d2 = D beyond the reach too).  Otherwise it
// also stops at dy > R: a seed further than R rows away cannot give a zone.
template <bool FULL>
__global__ __launch_bounds__(256) void zone_cols_kernel(const unsigned short *__restrict__ g, const int *__restrict__ gl,
                                                        const int *__restrict__ has_seed, int *__restrict__ zones,
                                                        int *__restrict__ d2out, int N, int H, int W, int R) {
    const int64_t total = (int64_t)N * H * W;
    const int reach2 = R > 0 ? R * R : P_INF;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (int64_t)gridDim.x * blockDim.x) {
        const int x = (int)(p % W), y = (int)((p / W) % H), n = (int)(p / ((int64_t)H * W));
        int best = P_INF, zone = 0;
        if (has_seed[n]) {
            const size_t base = (size_t)n * H * W + x;
            const unsigned short *gc = g + base;
            const int *lc = gl + base;
            const int g0 = gc[(size_t)y * W];
            if (g0 < G_INF) {
                best = g0 * g0;
                zone = lc[(size_t)y * W];
            }
            const int dy_max = (!FULL && R > 0) ? R : H;
            for (int dy = 1; dy <= dy_max && dy * dy <= best; ++dy) {
                const int ya = y - dy, yb = y + dy;
                if (ya < 0 && yb >= H) break;
                if (ya >= 0) {
                    const int v = gc[(size_t)ya * W];
                    const int c = v * v + dy * dy;
                    if (v < G_INF && c <= best) {
                        const int l = lc[(size_t)ya * W];
                        if (c < best || l < zone) zone = l;
                        best = c;
                    }
                }
                if (yb < H) {
                    const int v = gc[(size_t)yb * W];
                    const int c = v * v + dy * dy;
                    if (v < G_INF && c <= best) {
                        const int l = lc[(size_t)yb * W];
                        if (c < best || l < zone) zone = l;
                        best = c;
                    }
                }
            }
        }
        zones[p] = best <= reach2 ? zone : 0;
        if (FULL) d2out[p] = best;
    }
}

// Everything a call accumulates into is cleared by a kernel of the call's own chain (a kernel node when the call is
// captured in a graph), not by memset nodes: two 32-bit word ranges and two single words.
__global__ __launch_bounds__(256) void clear_words_kernel(unsigned *__restrict__ a, int64_t na, unsigned *__restrict__ b,
                                                          int64_t nb, int *__restrict__ w0, int *__restrict__ w1) {
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = i0; i < na; i += step) a[i] = 0u;
    for (int64_t i = i0; i < nb; i += step) b[i] = 0u;
    if (i0 == 0) {
        if (w0) *w0 = 0;
        if (w1) *w1 = 0;
    }
}

inline unsigned nb_grid(int64_t items) {
    int64_t b = (items + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 16384 ? 16384 : b));
}

inline bool overlaps(const void *a, int64_t na, const void *b, int64_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

// ---- graph helpers --------------------------------------------------------------------------------------------------
constexpr int LABEL_BITS = 21;
constexpr u64 LABEL_MASK = (1ULL << LABEL_BITS) - 1ULL;

inline int64_t graph_slots(int64_t max_pairs) {
    int64_t s = 2;
    while (s < 2 * max_pairs) s *= 2;
    return s;
}

__device__ __forceinline__ u64 mix64(u64 k) {
    k ^= k >> 30; k *= 0xBF58476D1CE4E5B9ULL; k ^= k >> 27; k *= 0x94D049BB133111EBULL; k ^= k >> 31;
    return k;
}

// the 64-bit key of an unordered pair of zones of one frame / volume; 0 = no pair (equal zones, or one of them 0)
__device__ __forceinline__ u64 pair_key(u64 head, int a, int b) {
    return (a && b && a != b) ? (head | ((u64)min(a, b) << LABEL_BITS) | (u64)max(a, b)) : 0ULL;
}

// Runs of equal non-zero `key` over the 64 lanes: the leader lane of each run gets its length, every other lane 0.
// `mask_out` is the run's lane mask (leaders only).
__device__ __forceinline__ int run_length(u64 key, int lane, u64 *mask_out) {
    const u64 prev = __shfl_up(key, 1);
    const bool change = lane == 0 || prev != key;               // a run of any key, 0 included, starts here
    const u64 starts = __ballot(change);
    if (!change || key == 0ULL) return 0;
    const u64 after = lane == 63 ? 0ULL : (starts & (~0ULL << (lane + 1)));
    const int end = after ? __ffsll((long long)after) - 1 : 64;
    const u64 upto_end = end == 64 ? ~0ULL : ((1ULL << end) - 1ULL);
    *mask_out = upto_end & (~0ULL << lane);
    return end - lane;
}

// ---- graph ----------------------------------------------------------------------------------------------------------
// sq_zone_graph and sq_zone_graph3d: a frame is a volume with D = 1.  DEPTH (a volume's call) adds the deeper neighbour
// and a second count per pair: a slot of the table carries COUNTS = 1 (frames) or 2 ([lateral, axial]) 32-bit counts,
// and a row of `pairs` is [n, a, b] and the counts.

// insert-and-add into the open-addressing table: the key is claimed with a 64-bit compare-and-swap, the count -- the
// `which`-th of the slot's `stride` -- is a 32-bit add
__device__ __forceinline__ void table_add(u64 *__restrict__ keys, unsigned *__restrict__ counts, unsigned slots, u64 key,
                                          unsigned len, int stride, int which, int *__restrict__ dropped) {
    unsigned s = (unsigned)mix64(key) & (slots - 1u);
    for (unsigned i = 0; i < slots; ++i) {
        u64 k = __atomic_load_n(&keys[s], __ATOMIC_RELAXED);
        if (k == 0ULL) {
            k = atomicCAS(&keys[s], 0ULL, key);
            if (k == 0ULL) k = key;
        }
        if (k == key) {
            atomicAdd(&counts[(size_t)s * stride + which], len);
            return;
        }
        s = (s + 1u) & (slots - 1u);
    }
    atomicAdd(dropped, 1);                                      // every slot holds another pair
}

__device__ __forceinline__ int zone_value(int z, int max_label) { return (z < 1 || z > max_label) ? 0 : z; }

// one wave per (n, d, h) row; runs of equal zone / equal (a, b) per direction make ONE atomic each.  D comes last: a
// frame's launch never reads it, and with rows, H, W and max_label side by side a wave fetches them in one scalar load.
template <bool DEPTH>
__global__ __launch_bounds__(256) void zone_graph_kernel(const int *__restrict__ zones, long long *__restrict__ stats,
                                                         u64 *__restrict__ keys, unsigned *__restrict__ counts,
                                                         unsigned slots, int *__restrict__ dropped, int rows, int H, int W,
                                                         int max_label, int D) {
    constexpr int COUNTS = DEPTH ? 2 : 1;
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;                                      // whole waves leave
    const int h = r % H, d = DEPTH ? (r / H) % D : 0, n = DEPTH ? r / (H * D) : r / H;     // H * D <= rows < 2^31
    const int *row = zones + (size_t)r * W;
    const size_t plane = (size_t)H * W;
    const bool face_row = h == 0 || h == H - 1 || (DEPTH && (d == 0 || d == D - 1));
    long long *st = stats + (size_t)n * ((size_t)max_label + 1) * 2;
    const u64 head = (u64)n << (2 * LABEL_BITS);
    for (int c0 = 0; c0 < W; c0 += 64) {
        const int col = c0 + lane;
        const bool in = col < W;
        // the loads first, the range checks after: checked inside the conditionals, each load waits for the one before
        int z = in ? row[col] : 0;
        int zh = (in && h + 1 < H) ? row[col + W] : 0;                                     // the lower neighbour
        int zd = (DEPTH && in && d + 1 < D) ? row[col + plane] : 0;                        // the deeper neighbour
        z = zone_value(z, max_label), zh = zone_value(zh, max_label), zd = zone_value(zd, max_label);
        int zw = __shfl_down(z, 1);                                                        // the right neighbour
        if (lane == 63) zw = col + 1 < W ? zone_value(row[col + 1], max_label) : 0;
        // cells and cells on the frame's border / the volume's faces: one 64-bit add per run of equal zone
        u64 mask = 0;
        const u64 E = __ballot(in && (face_row || col == 0 || col == W - 1));
        int len = run_length((u64)z, lane, &mask);
        if (len) {
            atomicAdd((u64 *)&st[(size_t)z * 2], (u64)len);
            const int e = __popcll(E & mask);
            if (e) atomicAdd((u64 *)&st[(size_t)z * 2 + 1], (u64)e);
        }
        // pairs of cells along w and h (lateral) and along d (axial) whose zones differ, both > 0
        const u64 kw = pair_key(head, z, zw), kh = pair_key(head, z, zh);
        len = run_length(kw, lane, &mask);
        if (len) table_add(keys, counts, slots, kw, (unsigned)len, COUNTS, 0, dropped);
        len = run_length(kh, lane, &mask);
        if (len) table_add(keys, counts, slots, kh, (unsigned)len, COUNTS, 0, dropped);
        if (DEPTH) {
            const u64 kd = pair_key(head, z, zd);
            len = run_length(kd, lane, &mask);
            if (len) table_add(keys, counts, slots, kd, (unsigned)len, COUNTS, 1, dropped);
        }
    }
}

template <int COUNTS>
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
        int *row = pairs + (size_t)idx * (3 + COUNTS);
        row[0] = (int)(k >> (2 * LABEL_BITS));
        row[1] = (int)((k >> LABEL_BITS) & LABEL_MASK);
        row[2] = (int)(k & LABEL_MASK);
#pragma unroll
        for (int c = 0; c < COUNTS; ++c) row[3 + c] = (int)counts[(size_t)s * COUNTS + c];
    }
}

// bytes of the table for `max_pairs` pairs: 8 of key and 4 per count a slot
inline int64_t graph_bytes(int max_pairs, int counts) {
    if (max_pairs < 1 || max_pairs > (1 << 28)) return -1;
    return (graph_slots(max_pairs) * (8 + 4 * counts) + 15) / 16 * 16;
}

// clear -> graph -> compact, after the entry's own checks; `stat_words`: the 32-bit words of `stats`
template <bool DEPTH>
int zone_graph_run(const char *who, const int *zones, int N, int D, int H, int W, int max_label, int64_t *stats,
                   int64_t stat_words, int *pairs, int max_pairs, int *count, int *dropped, void *workspace, hipStream_t st) {
    constexpr int COUNTS = DEPTH ? 2 : 1;
    const unsigned slots = (unsigned)graph_slots(max_pairs);
    u64 *keys = reinterpret_cast<u64 *>(workspace);
    unsigned *counts = reinterpret_cast<unsigned *>(keys + slots);
    const int64_t table_words = (int64_t)slots * (2 + COUNTS);
    hipLaunchKernelGGL(clear_words_kernel, dim3(nb_grid(table_words > stat_words ? table_words : stat_words)), dim3(256), 0, st,
                       reinterpret_cast<unsigned *>(workspace), table_words, reinterpret_cast<unsigned *>(stats), stat_words,
                       count, dropped);
    int rc = sq_check_launch(who);
    if (rc) return rc;
    const int rows = N * D * H;
    hipLaunchKernelGGL(zone_graph_kernel<DEPTH>, dim3((rows + 3) / 4), dim3(256), 0, st, zones,
                       reinterpret_cast<long long *>(stats), keys, counts, slots, dropped, rows, H, W, max_label, D);
    rc = sq_check_launch(who);
    if (rc) return rc;
    hipLaunchKernelGGL(zone_graph_compact_kernel<COUNTS>, dim3(nb_grid(slots)), dim3(256), 0, st, keys, counts, slots, pairs,
                       max_pairs, count, dropped);
    return sq_check_launch(who);
}

}  // namespace
