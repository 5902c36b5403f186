// Seam blending (include/sequitr_hip.h "Seam blending"): sq_stitch_probs with more than one tile per frame pixel.  Where
// tiles overlap, the merged logits of up to 3 x 3 of them are mixed with the integer tent weights of the header before the
// argmax and the softmax, so that the mask and the probabilities carry no step along the seam lines.
//
// One frame pixel per lane, 256 consecutive pixels a chunk, block-stride past the grid cap: stitch_probs_kernel's shape.
// A lane reads its row's and its column's three slots (two 8-byte words of (tile << 16 | local, weight) each; a wave's
// row slots are one or two cache lines) and counts its contributors ny * nx.  Nearly every pixel has one: the wave votes,
// and a wave with no seam pixel issues one load_pixel -- stitch_probs_kernel's traffic plus the slots.  A wave that
// touches a seam walks the 3 x 3 slots in order, each lane reading only where its weight is positive.  Both paths run
// blend_add / blend_divide, so the arithmetic is one text: S = +0; S = S + (float)(wy * wx) * v; b = S / (float)(Wy * Wx).
#include "sq_probs.h"

#pragma clang fp contract(off)

namespace {

constexpr int BLEND_THREADS = 256, BLEND_GRID_CAP = 16384;

struct BlendAxis {
    int2 s[3];                                                  // (tile << 16 | local, weight); contributors first
    __device__ __forceinline__ int count() const { return (s[0].y > 0) + (s[1].y > 0) + (s[2].y > 0); }
    __device__ __forceinline__ int weight() const { return s[0].y + s[1].y + s[2].y; }
};

__device__ __forceinline__ BlendAxis blend_axis(const int2 *__restrict__ slots, unsigned p) {
    BlendAxis a;
    const int2 *q = slots + 3 * (size_t)p;
    a.s[0] = q[0]; a.s[1] = q[1]; a.s[2] = q[2];
    return a;
}

// S <- S + (float)(wy * wx) * the K logits of tile (f, ky, kx) at (ly, lx)
template <int K>
__device__ __forceinline__ void blend_add(float (&S)[K], const float *__restrict__ logits, unsigned f, int2 ys, int2 xs,
                                          unsigned TR, unsigned TC, unsigned TS) {
    const size_t t = ((size_t)f * TR + ((unsigned)ys.x >> 16)) * TC + ((unsigned)xs.x >> 16);
    float z[K];
    load_pixel<K>(logits + ((t * TS + ((unsigned)ys.x & 0xffffu)) * TS + ((unsigned)xs.x & 0xffffu)) * K, z);
    const float w = (float)(ys.y * xs.y);
#pragma unroll
    for (int c = 0; c < K; ++c) S[c] = S[c] + w * z[c];
}

template <int K, typename P>
__global__ __launch_bounds__(BLEND_THREADS) void stitch_blend_kernel(const float *__restrict__ logits, const int2 *__restrict__ yslots,
                                                                     const int2 *__restrict__ xslots, uint8_t *__restrict__ mask,
                                                                     P *__restrict__ prob, float inv_n, unsigned H, unsigned W,
                                                                     unsigned TR, unsigned TC, unsigned TS, int64_t total) {
    const int64_t nchunks = (total + BLEND_THREADS - 1) / BLEND_THREADS;
    for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const int64_t base = chunk * BLEND_THREADS;
        if (base + threadIdx.x >= total) continue;
        const int64_t base_row = base / W;
        const unsigned l = (unsigned)(base - base_row * W) + threadIdx.x;
        const unsigned row = (unsigned)base_row + l / W, x = l % W;     // row < F * H < 2^31 (checked on the host)
        const unsigned y = row % H, f = row / H;
        const BlendAxis ya = blend_axis(yslots, y), xa = blend_axis(xslots, x);
        float z[K];
#pragma unroll
        for (int c = 0; c < K; ++c) z[c] = 0.f;
        if (!__any(ya.count() * xa.count() != 1)) {             // the wave's vote: no lane of it lies in a blend band
            blend_add<K>(z, logits, f, ya.s[0], xa.s[0], TR, TC, TS);
        } else {
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    if (ya.s[i].y * xa.s[j].y > 0) blend_add<K>(z, logits, f, ya.s[i], xa.s[j], TR, TC, TS);
        }
        const float wt = (float)(ya.weight() * xa.weight());    // exact: below 2^24
#pragma unroll
        for (int c = 0; c < K; ++c) z[c] = z[c] / wt;
        float bv;
        const int best = pixel_class<K>(z, bv);
        if (mask) mask[base + threadIdx.x] = (uint8_t)best;
        if (prob) {
            const float s = pixel_exps<K>(z, bv, inv_n);
            P *o = prob + ((size_t)f * K * H + y) * W + x;
            const size_t plane = (size_t)H * W;
#pragma unroll
            for (int c = 0; c < K; ++c, o += plane) store_prob(o, z[c] / s);
        }
    }
}

template <int K>
void blend_launch(const float *logits, const int32_t *yslots, const int32_t *xslots, uint8_t *mask, void *prob, int prob_dtype,
                  float inv_n, int F, int H, int W, int TR, int TC, int TS, hipStream_t st) {
    const int64_t total = (int64_t)F * H * W, chunks = (total + BLEND_THREADS - 1) / BLEND_THREADS;
    const dim3 grid((unsigned)(chunks > BLEND_GRID_CAP ? BLEND_GRID_CAP : chunks)), block(BLEND_THREADS);
    const int2 *ys = reinterpret_cast<const int2 *>(yslots), *xs = reinterpret_cast<const int2 *>(xslots);
    if (prob && prob_dtype == SQ_PIX_U8)
        hipLaunchKernelGGL((stitch_blend_kernel<K, uint8_t>), grid, block, 0, st, logits, ys, xs, mask,
                           reinterpret_cast<uint8_t *>(prob), inv_n, (unsigned)H, (unsigned)W, (unsigned)TR, (unsigned)TC,
                           (unsigned)TS, total);
    else
        hipLaunchKernelGGL((stitch_blend_kernel<K, float>), grid, block, 0, st, logits, ys, xs, mask,
                           reinterpret_cast<float *>(prob), inv_n, (unsigned)H, (unsigned)W, (unsigned)TR, (unsigned)TC,
                           (unsigned)TS, total);
}

}  // namespace

// Host only, no HIP call: the slot table of one axis, the header's per-axis rule.
extern "C" int sq_blend_axis_slots(int L, int T, int margin, int blend, int32_t *slots) {
    const char *what = "sq_blend_axis_slots";
    SQ_REQUIRE(slots, "%s: null pointer", what);
    SQ_REQUIRE(T >= 1 && T <= 65535 && L >= T, "%s: tile %d does not fit an axis of %d pixels (or is not 1 .. 65535)", what, T, L);
    SQ_REQUIRE(margin >= 0 && 2 * (int64_t)margin < T, "%s: margin %d too large for tile %d", what, margin, T);
    SQ_REQUIRE(blend >= 0 && blend <= margin && 2 * blend <= T - 2 * margin && blend <= 255,
               "%s: blend %d is not in 0 .. min(margin %d, (tile %d - 2 margin) / 2, 255)", what, blend, margin, T);
    const int stride = T - 2 * margin;
    const int64_t n64 = L == T ? 1 : ((int64_t)L - T + stride - 1) / stride + 1;   // origins 0, stride, ..., the last at L - T
    SQ_REQUIRE(n64 <= 65535, "%s: %lld tiles along an axis are more than 65535", what, (long long)n64);
    const int n = (int)n64;
    auto origin = [&](int k) { const int64_t o = (int64_t)k * stride; return (int)(o < L - T ? o : L - T); };
    auto start = [&](int k) { return k <= 0 ? 0 : (k >= n ? L : origin(k) + margin); };   // s[k]
    int k0 = 0;                                                 // the first tile whose weight can be positive at p
    for (int p = 0; p < L; ++p) {
        while (k0 < n - 1 && start(k0 + 1) + blend <= p) ++k0;  // tile k0 ends its band at s[k0 + 1] + blend
        int32_t *row = slots + 6 * (size_t)p;
        int used = 0;
        for (int k = k0; k < n && (k == 0 || start(k) - blend <= p); ++k) {
            const int far = 1 << 30;                            // +infinity: the frame border cuts no weight
            const int dl = k > 0 ? p - start(k) : far, dr = k < n - 1 ? start(k + 1) - 1 - p : far;
            int w = (dl < dr ? dl : dr) + blend + 1;
            w = w < 0 ? 0 : (w > 2 * blend + 1 ? 2 * blend + 1 : w);
            if (w == 0) continue;
            SQ_REQUIRE(used < 3, "%s: more than three tiles at coordinate %d (internal)", what, p);
            row[2 * used] = (int32_t)(((uint32_t)k << 16) | (uint32_t)(p - origin(k)));
            row[2 * used + 1] = w;
            ++used;
        }
        for (; used < 3; ++used) row[2 * used] = row[2 * used + 1] = 0;
    }
    return n;
}

extern "C" int sq_stitch_blend(const float *tile_logits, const int32_t *yslots, const int32_t *xslots, uint8_t *mask_out,
                               void *prob_out, int prob_dtype, float inv_n, int F, int H, int W, int TR, int TC, int TS, int K,
                               void *stream) {
    const char *what = "sq_stitch_blend";
    SQ_REQUIRE(tile_logits && yslots && xslots, "%s: null pointer", what);
    SQ_REQUIRE(mask_out || prob_out, "%s: null pointer: give mask_out, prob_out or both", what);
    SQ_REQUIRE(!prob_out || prob_dtype == SQ_PIX_U8 || prob_dtype == SQ_PIX_F32, "%s: prob_dtype %d is not SQ_PIX_U8 or SQ_PIX_F32",
               what, prob_dtype);
    SQ_REQUIRE(K >= 1 && K <= 16, "%s: %d classes are not 1 .. 16", what, K);
    SQ_REQUIRE(F > 0 && H > 0 && W > 0 && TR > 0 && TC > 0 && TS > 0 && TS < 65536, "%s: bad geometry", what);
    SQ_REQUIRE((int64_t)F * H <= 0x7fffffff, "%s: %d frames of %d rows are out of range", what, F, H);
    SQ_REQUIRE(inv_n > 0.f && inv_n <= 1.f, "%s: inv_n %g is not in (0, 1]", what, (double)inv_n);
    SQ_REQUIRE_ALIGNED(tile_logits);
    SQ_REQUIRE(((uintptr_t)yslots | (uintptr_t)xslots) % 8 == 0 && (!prob_out || prob_dtype == SQ_PIX_U8 || (uintptr_t)prob_out % 4 == 0),
               "%s: the slot tables must be 8-byte aligned (a slot is read as one word pair), prob_out to its elements", what);
    hipStream_t st = (hipStream_t)stream;
#define SQ_BLEND_K(k) case k: blend_launch<k>(tile_logits, yslots, xslots, mask_out, prob_out, prob_dtype, inv_n, F, H, W, TR, TC, TS, st); break;
    switch (K) {
        SQ_BLEND_K(1) SQ_BLEND_K(2) SQ_BLEND_K(3) SQ_BLEND_K(4) SQ_BLEND_K(5) SQ_BLEND_K(6) SQ_BLEND_K(7) SQ_BLEND_K(8)
        SQ_BLEND_K(9) SQ_BLEND_K(10) SQ_BLEND_K(11) SQ_BLEND_K(12) SQ_BLEND_K(13) SQ_BLEND_K(14) SQ_BLEND_K(15) SQ_BLEND_K(16)
    }
#undef SQ_BLEND_K
    return sq_check_launch(what);
}
