// One pixel's (or voxel's) K merged logits -> its class and its K probabilities, as include/sequitr_hip.h "Tile views and
// probability stitch" states them (MASK, PROBABILITIES): shared by sq_stitch_probs and sq_bricks_scatter_probs, so that
// the planar and the volumetric maps are one expression.  Include with contraction off.
#pragma once
#include "sq_common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

// the K floats of one interleaved pixel at p, in the widest pieces K allows (sq_store_pixel's rule)
template <int K>
__device__ __forceinline__ void load_pixel(const float *__restrict__ p, float (&z)[K]) {
    if constexpr (K % 4 == 0) {
#pragma unroll
        for (int q = 0; q < K; q += 4) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(p + q);
            z[q] = v.x; z[q + 1] = v.y; z[q + 2] = v.z; z[q + 3] = v.w;
        }
    } else if constexpr (K % 2 == 0) {
#pragma unroll
        for (int q = 0; q < K; q += 2) {
            const float2 v = *reinterpret_cast<const float2 *>(p + q);
            z[q] = v.x; z[q + 1] = v.y;
        }
    } else {
#pragma unroll
        for (int q = 0; q < K; ++q) z[q] = p[q];
    }
}

__device__ __forceinline__ void store_prob(float *p, float v) { *p = v; }
__device__ __forceinline__ void store_prob(uint8_t *p, float v) { *p = v != v ? (uint8_t)0 : (uint8_t)floorf(v * 255.0f + 0.5f); }

// sq_argmax_u8's loop: ties to the lowest class, NaN never wins; bv is the winner's value
template <int K>
__device__ __forceinline__ int pixel_class(const float (&z)[K], float &bv) {
    bv = z[0];
    int best = 0;
#pragma unroll
    for (int c = 1; c < K; ++c)
        if (z[c] > bv) { bv = z[c]; best = c; }
    return best;
}

// z <- e_k = expf(z_k * inv_n - m) with m = bv * inv_n; returns s = e_0 + ... + e_{K-1} in index order, or NaN for a row
// whose m is not finite or that holds a NaN (e / NaN: NaN in every class).  p_k = z[k] / s.
template <int K>
__device__ __forceinline__ float pixel_exps(float (&z)[K], float bv, float inv_n) {
    const float m = bv * inv_n;
    bool bad = !(fabsf(m) < INFINITY);                          // NaN or +-inf
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < K; ++c) {
        const float lc = z[c] * inv_n;
        bad = bad || lc != lc;
        z[c] = expf(lc - m);
        s = s + z[c];
    }
    return bad ? NAN : s;
}

}  // namespace
