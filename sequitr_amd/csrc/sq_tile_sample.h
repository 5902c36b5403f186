// What sq_tile_sample_affine (sq_tile_sampler.hip) and sq_tile_sample_affine_mc (sq_multichannel.hip) share: the patch
// geometry, the coordinate and interpolation expressions of include/sequitr_hip.h "Tile sampler" and the SQ_ROTATE_LDS
// switch.  One definition, so that channel c of the multi-channel sampler has the single-channel sampler's bits by
// construction.  Contraction is off here and in the including file from here on.
#pragma once
#include <stdlib.h>
#include "sq_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int PATCH = 32;                                       // output pixels per block along each axis
constexpr int ROWS = 8;                                         // blockDim.y: a thread takes PATCH / ROWS rows
constexpr int BOX = 48;                                         // largest staged box: 31 * sqrt(2) + 1 + the apron, rounded up
constexpr int PITCH = BOX + 1;                                  // odd pitch: a column walk touches every bank
constexpr float LIMIT = 8388608.f;                              // 2^23

struct TileGeom {
    int F, H, W, TH, TW, C, px;                                 // px: patches along a tile row
};

struct Affine {
    float a0, a1, a2, b0, b1, b2;
};

__device__ __forceinline__ void source_xy(const Affine &t, long long X, long long Y, float &sx, float &sy) {
#pragma clang fp contract(off)
    const float x = (float)X, y = (float)Y;
    const float p = t.a0 * x, q = t.a1 * y;
    sx = (p + q) + t.a2;
    const float u = t.b0 * x, v = t.b1 * y;
    sy = (u + v) + t.b2;
}

__device__ __forceinline__ bool in_range(float sx, float sy) {  // false for NaN
    return fabsf(sx) < LIMIT && fabsf(sy) < LIMIT;
}

__device__ __forceinline__ float bilinear(float sx, float sy, float fx0, float fy0, float v00, float v01, float v10, float v11) {
#pragma clang fp contract(off)
    const float fx1 = fx0 + 1.f, fy1 = fy0 + 1.f;
    const float wl = fx1 - sx, wr = sx - fx0;
    const float tl = wl * v00, tr = wr * v01;
    const float top = tl + tr;
    const float bl = wl * v10, br = wr * v11;
    const float bot = bl + br;
    const float a = (fy1 - sy) * top, b = (sy - fy0) * bot;
    return a + b;
}

__device__ __forceinline__ float norm_pixel(float r, bool norm, float m, float s) {
#pragma clang fp contract(off)
    return norm ? (r - m) / s : r;                              // tiles_norm_kernel's expression
}

// C bytes (label == q), q = 0 .. C-1, at p; `packed`: p is aligned to C, a power of two
__device__ __forceinline__ void store_onehot(uint8_t *p, unsigned label, int C, bool packed) {
    if (packed) {
        const uint64_t lo = label < 8u ? (uint64_t)1 << (8 * label) : 0;
        switch (C) {
        case 1: *p = (uint8_t)lo; return;
        case 2: *reinterpret_cast<uint16_t *>(p) = (uint16_t)lo; return;
        case 4: *reinterpret_cast<uint32_t *>(p) = (uint32_t)lo; return;
        case 8: *reinterpret_cast<uint64_t *>(p) = lo; return;
        default: {                                              // 16
            const uint64_t hi = (label >= 8u && label < 16u) ? (uint64_t)1 << (8 * (label - 8u)) : 0;
            uint64_t *d = reinterpret_cast<uint64_t *>(p);
            d[0] = lo;
            d[1] = hi;
            return;
        }
        }
    }
    for (int q = 0; q < C; ++q) p[q] = (uint8_t)(label == (unsigned)q);
}

// SQ_ROTATE_LDS, read per launch: 0 = the direct gather everywhere, 1 = the LDS form wherever the box fits.  Unset is the
// direct gather, the faster of the two as measured (tools/tile_sampler_bench.py: 0.77x the LDS form's time at theta = 0,
// 0.96-0.97x at pi/4 and at random angles -- a 32 x 32 patch's footprint is compact enough for L2 to serve the four
// corners, and staging costs a barrier and a second pass).
inline bool rotate_lds() {
    const char *e = getenv("SQ_ROTATE_LDS");
    return e && e[0] == '1';
}

}  // namespace
