// What the planar and the volumetric neighbourhood calls share (sq_neighbors.hip, sq_neighbors3d.hip): the two planar
// passes of the feature transform, the clearing kernel, and the run / hash helpers of the contact graphs.  Everything
// sits in an unnamed namespace: each translation unit gets its own copy, as with the other shared headers.
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

}  // namespace
