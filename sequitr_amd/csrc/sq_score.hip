// Scoring: confusion counts of predictions against labels, both in HBM (include/sequitr_hip.h "Scoring"; the reference's
// sequitr/confusion.py, a proxy to scikit-learn on host arrays).  One streaming pass over the two arrays and C*C + 1 integers
// per item out; nothing is downloaded and no mask is materialised for logits.
//
// Definition, per pixel p of item i (row = truth, column = prediction, scikit-learn's convention):
//
//     pc = SQ_PRED_MASK       : pred[i, p]                                               (uint8; >= C is "no class")
//          SQ_PRED_LOGITS_F32 : best = 0;  for c = 1 .. C-1: if (z[c] > z[best]) best = c   (sq_argmax_u8's loop, so NaN, +-inf
//                               and -0 rows give sq_argmax_u8's class)
//     tc = SQ_TRUTH_INDEX     : truth[i, p]                                              (uint8; >= C is "no class")
//          SQ_TRUTH_ONEHOT    : the lowest c with truth[i, p, c] != 0;  none: "no class"
//     tc < C and pc < C ?  counts[i, tc, pc] += 1  :  ignored[i] += 1
//
// Counting is private first: a block owns one CHUNK of one item and counts it into an LDS histogram of C*C + 1 bins, every
// bin REP = 32 counters wide with lane l adding into column l % 32, so that the 32 lanes of an LDS lane group sit on 32
// different banks whatever their bins are (lanes l and l + 32 are in different groups and never conflict).  The block then
// folds the columns and issues at most C*C + 1 global 64-bit integer atomic adds.  Integer adds commute: the result does not
// depend on any order and is the same bits on every run.
//
// The LDS counters are 32 bits.  A block visits at most one chunk between two flushes, and a chunk is at most 2^30 pixels
// (MAX_CHUNK), so no counter can wrap.
//
// Alignment.  Row bases are arbitrary byte addresses (n may be odd, tensors may be views).  The mask x index kernel, the hot
// pair, reads 16 pixels per lane: a block first takes the head pixels up to the first 16-byte boundary of its pred range one
// per thread, then whole 16-byte vectors of pred (aligned) with the matching 16 bytes of truth (aligned exactly when the two
// bases are congruent mod 16, as two tensors of one shape are; otherwise the same load instruction at an unaligned address,
// which global memory takes), then the tail one per thread.  No load touches a byte outside [base, base + items*n).  The
// other three pairs walk one pixel per lane: their traffic is the C floats or C bytes per pixel, read as the widest vector
// (16, 8 or 4 bytes for logits; 4, 2 or 1 for one-hot) that divides a pixel and that every row base is aligned to.
#include <algorithm>
#include "sq_common.h"

namespace {

constexpr int THREADS = 256;
constexpr int REP = 32;                                         // counters per bin: one per LDS bank of a 32-lane group
constexpr int MAXC = 16;
constexpr int64_t MIN_CHUNK = 16384;                            // pixels: 256 threads x 16 pixels x 4 rounds
constexpr int64_t MAX_CHUNK = (int64_t)1 << 30;                 // 32-bit LDS counters cannot wrap below 2^32 pixels
constexpr int64_t MAX_UNITS = (int64_t)1 << 22;                 // chunks of one call before the chunk doubles
constexpr int64_t MAX_GRID = 1 << 16;                           // blocks; the units beyond are a grid-stride loop

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
// the same 16 bytes at any byte address: one global_load_dwordx4 either way
typedef u32x4 u32x4_u __attribute__((aligned(1)));

__device__ __forceinline__ void count_one(unsigned *hist, int col, unsigned tc, unsigned pc, unsigned C, unsigned nocls) {
    const unsigned bin = (tc < C && pc < C) ? tc * C + pc : nocls;
    atomicAdd(&hist[bin * REP + col], 1u);                      // ds_add_u32, no return value
}

__device__ __forceinline__ void hist_clear(unsigned *hist, int cells) {
    for (int k = threadIdx.x; k < cells; k += THREADS) hist[k] = 0;
    __syncthreads();
}

// fold the REP columns of every bin; one 64-bit atomic per non-empty bin
__device__ __forceinline__ void hist_flush(unsigned *hist, int bins, unsigned long long *__restrict__ counts,
                                           unsigned long long *__restrict__ ignored, int64_t item) {
    __syncthreads();
    for (int b = threadIdx.x; b < bins; b += THREADS) {
        unsigned long long s = 0;
#pragma unroll 8
        for (int r = 0; r < REP; ++r) s += hist[b * REP + ((r + b) & (REP - 1))];
        if (s) {
            if (b == bins - 1) atomicAdd(&ignored[item], s);
            else atomicAdd(&counts[item * (int64_t)(bins - 1) + b], s);
        }
    }
    __syncthreads();                                            // the next unit clears the histogram
}

// ---- masks against index labels: 16 pixels per lane -----------------------------------------------------------------------

__global__ __launch_bounds__(THREADS) void confusion_mask_index_kernel(const uint8_t *__restrict__ pred,
                                                                       const uint8_t *__restrict__ truth,
                                                                       unsigned long long *__restrict__ counts,
                                                                       unsigned long long *__restrict__ ignored, int64_t n, int C,
                                                                       int64_t chunk, int64_t bpi, int64_t units) {
    extern __shared__ unsigned hist[];
    const int bins = C * C + 1, col = threadIdx.x & (REP - 1);
    const unsigned uc = (unsigned)C, nocls = (unsigned)(C * C);
    for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const int64_t item = u / bpi, start = (u % bpi) * chunk;
        const int64_t len = std::min(chunk, n - start);
        const uint8_t *p = pred + item * n + start, *t = truth + item * n + start;
        hist_clear(hist, bins * REP);
        const int64_t head = std::min<int64_t>(len, (int64_t)((16 - ((uintptr_t)p & 15)) & 15));
        const int64_t nvec = (len - head) >> 4, tail = head + (nvec << 4);
        if ((int64_t)threadIdx.x < head) count_one(hist, col, t[threadIdx.x], p[threadIdx.x], uc, nocls);
        const u32x4 *pv = reinterpret_cast<const u32x4 *>(p + head);
        const uint8_t *tv = t + head;
        for (int64_t v = threadIdx.x; v < nvec; v += THREADS) {
            const u32x4 a = __builtin_nontemporal_load(pv + v);
            const u32x4 b = *reinterpret_cast<const u32x4_u *>(tv + (v << 4));
#pragma unroll
            for (int w = 0; w < 4; ++w)
#pragma unroll
                for (int k = 0; k < 4; ++k) count_one(hist, col, (b[w] >> (8 * k)) & 255u, (a[w] >> (8 * k)) & 255u, uc, nocls);
        }
        if (tail + (int64_t)threadIdx.x < len) count_one(hist, col, t[tail + threadIdx.x], p[tail + threadIdx.x], uc, nocls);
        hist_flush(hist, bins, counts, ignored, item);
    }
}

// ---- the other pairs: one pixel per lane ----------------------------------------------------------------------------------

// sq_argmax_u8's loop over C floats read as vectors of VF
template <int VF>
__device__ __forceinline__ unsigned pred_logits(const float *__restrict__ z, int C) {
    typedef float V __attribute__((ext_vector_type(VF)));
    float bv = 0.f;
    unsigned best = 0;
    for (int c = 0; c < C; c += VF) {
        float v[VF];
        if constexpr (VF == 1) {
            v[0] = z[c];
        } else {
            const V q = *reinterpret_cast<const V *>(z + c);
#pragma unroll
            for (int k = 0; k < VF; ++k) v[k] = q[k];
        }
#pragma unroll
        for (int k = 0; k < VF; ++k) {
            if (c + k == 0) bv = v[0];
            else if (v[k] > bv) { bv = v[k]; best = (unsigned)(c + k); }
        }
    }
    return best;
}

// the lowest non-zero channel of C bytes read as words of VB bytes; 255: none
template <int VB>
__device__ __forceinline__ unsigned truth_onehot(const uint8_t *__restrict__ y, int C) {
    unsigned cls = 255u;
    for (int c = C - VB; c >= 0; c -= VB) {                     // downwards: the lowest channel is written last
        unsigned w;
        if constexpr (VB == 4) w = *reinterpret_cast<const unsigned *>(y + c);
        else if constexpr (VB == 2) w = *reinterpret_cast<const unsigned short *>(y + c);
        else w = y[c];
#pragma unroll
        for (int k = VB - 1; k >= 0; --k)
            if ((w >> (8 * k)) & 255u) cls = (unsigned)(c + k);
    }
    return cls;
}

template <bool LOGITS, bool ONEHOT, int VF, int VB>
__global__ __launch_bounds__(THREADS) void confusion_pixel_kernel(const void *__restrict__ pred, const uint8_t *__restrict__ truth,
                                                                  unsigned long long *__restrict__ counts,
                                                                  unsigned long long *__restrict__ ignored, int64_t n, int C,
                                                                  int64_t chunk, int64_t bpi, int64_t units) {
    extern __shared__ unsigned hist[];
    const int bins = C * C + 1, col = threadIdx.x & (REP - 1);
    const unsigned uc = (unsigned)C, nocls = (unsigned)(C * C);
    for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const int64_t item = u / bpi, start = (u % bpi) * chunk;
        const int64_t len = std::min(chunk, n - start), first = item * n + start;
        hist_clear(hist, bins * REP);
        for (int64_t q = threadIdx.x; q < len; q += THREADS) {
            const int64_t px = first + q;
            const unsigned pc = LOGITS ? pred_logits<VF>(reinterpret_cast<const float *>(pred) + px * C, C)
                                       : (unsigned)reinterpret_cast<const uint8_t *>(pred)[px];
            const unsigned tc = ONEHOT ? truth_onehot<VB>(truth + px * C, C) : (unsigned)truth[px];
            count_one(hist, col, tc, pc, uc, nocls);
        }
        hist_flush(hist, bins, counts, ignored, item);
    }
}

struct Launch {
    int64_t n, chunk, bpi, units;
    int C;
    unsigned grid;
    size_t lds;
    hipStream_t st;
};

template <bool LOGITS, bool ONEHOT, int VF, int VB>
void launch_pixel(const void *pred, const uint8_t *truth, unsigned long long *counts, unsigned long long *ignored,
                  const Launch &L) {
    hipLaunchKernelGGL((confusion_pixel_kernel<LOGITS, ONEHOT, VF, VB>), dim3(L.grid), dim3(THREADS), L.lds, L.st, pred, truth,
                       counts, ignored, L.n, L.C, L.chunk, L.bpi, L.units);
}

template <bool LOGITS, int VF>
void launch_truth(const void *pred, const uint8_t *truth, int truth_kind, int vb, unsigned long long *counts,
                  unsigned long long *ignored, const Launch &L) {
    if (truth_kind == SQ_TRUTH_INDEX) launch_pixel<LOGITS, false, VF, 1>(pred, truth, counts, ignored, L);
    else if (vb == 4) launch_pixel<LOGITS, true, VF, 4>(pred, truth, counts, ignored, L);
    else if (vb == 2) launch_pixel<LOGITS, true, VF, 2>(pred, truth, counts, ignored, L);
    else launch_pixel<LOGITS, true, VF, 1>(pred, truth, counts, ignored, L);
}

// the widest of the given vector sizes (bytes, descending) that divides a pixel and that every row base is aligned to
inline int vector_bytes(const void *base, int64_t pixel_bytes, int64_t row_bytes, int64_t items, int widest) {
    for (int v = widest; v > 1; v >>= 1)
        if (pixel_bytes % v == 0 && (uintptr_t)base % v == 0 && (items == 1 || row_bytes % v == 0)) return v;
    return 1;
}

}  // namespace

extern "C" int64_t sq_confusion_chunk(int64_t items, int64_t n) {
    if (items <= 0 || n <= 0) return 0;
    int64_t chunk = MIN_CHUNK;
    while (chunk < MAX_CHUNK && (n + chunk - 1) / chunk > MAX_UNITS / std::min(items, MAX_UNITS)) chunk *= 2;
    return chunk;
}

extern "C" int sq_confusion(const void *pred, int pred_kind, const uint8_t *truth, int truth_kind, int64_t *counts,
                            int64_t *ignored, int64_t items, int64_t n, int C, void *stream) {
    const char *what = "sq_confusion";
    SQ_REQUIRE(pred && truth && counts && ignored, "%s: null pointer", what);
    SQ_REQUIRE(pred_kind == SQ_PRED_MASK || pred_kind == SQ_PRED_LOGITS_F32, "%s: unknown pred_kind %d", what, pred_kind);
    SQ_REQUIRE(truth_kind == SQ_TRUTH_INDEX || truth_kind == SQ_TRUTH_ONEHOT, "%s: unknown truth_kind %d", what, truth_kind);
    SQ_REQUIRE(C >= 1 && C <= MAXC, "%s: %d classes not in 1 .. %d", what, C, MAXC);
    SQ_REQUIRE(items >= 0 && n >= 0, "%s: items and n must not be negative", what);
    SQ_REQUIRE(n <= ((int64_t)1 << 44) && items <= ((int64_t)1 << 40) &&
                   (n == 0 || items <= ((int64_t)1 << 56) / (n * C)),
               "%s: %lld items of %lld pixels are out of range", what, (long long)items, (long long)n);
    SQ_REQUIRE(((uintptr_t)counts | (uintptr_t)ignored) % 8 == 0, "%s: counts and ignored must be aligned to 8 bytes", what);
    SQ_REQUIRE(pred_kind != SQ_PRED_LOGITS_F32 || (uintptr_t)pred % 4 == 0, "%s: float32 logits must be aligned to 4 bytes", what);
    if (items == 0 || n == 0) return SQ_OK;

    Launch L;
    L.n = n, L.C = C, L.st = (hipStream_t)stream;
    L.chunk = sq_confusion_chunk(items, n);
    L.bpi = (n + L.chunk - 1) / L.chunk;
    L.units = items * L.bpi;
    L.grid = (unsigned)std::min(L.units, MAX_GRID);
    L.lds = (size_t)(C * C + 1) * REP * sizeof(unsigned);       // 33 KiB at C = 16
    unsigned long long *cn = reinterpret_cast<unsigned long long *>(counts);
    unsigned long long *ig = reinterpret_cast<unsigned long long *>(ignored);

    const int vb = truth_kind == SQ_TRUTH_ONEHOT ? vector_bytes(truth, C, n * C, items, 4) : 1;
    if (pred_kind == SQ_PRED_MASK) {
        if (truth_kind == SQ_TRUTH_INDEX)
            hipLaunchKernelGGL(confusion_mask_index_kernel, dim3(L.grid), dim3(THREADS), L.lds, L.st,
                               reinterpret_cast<const uint8_t *>(pred), truth, cn, ig, n, C, L.chunk, L.bpi, L.units);
        else
            launch_truth<false, 1>(pred, truth, truth_kind, vb, cn, ig, L);
    } else {
        const int vf = vector_bytes(pred, (int64_t)C * 4, n * C * 4, items, 16);
        if (vf == 16) launch_truth<true, 4>(pred, truth, truth_kind, vb, cn, ig, L);
        else if (vf == 8) launch_truth<true, 2>(pred, truth, truth_kind, vb, cn, ig, L);
        else launch_truth<true, 1>(pred, truth, truth_kind, vb, cn, ig, L);
    }
    return sq_check_launch(what);
}
