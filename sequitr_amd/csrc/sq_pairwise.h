// numpy's float32 summation order on the GPU, shared by the tile front end (sq_frontend.hip) and the volume front end
// (sq_volume_frontend.hip).  np.mean / np.std reduce a contiguous float32 array in chunks of 8192 elements (the ufunc
// buffer size),
//     res = 0;  for every chunk: res = res + pairwise(chunk)
// and pairwise() splits recursively at n2 = n/2 - (n/2) % 8 down to blocks of <= 128 elements, each summed
// with 8 interleaved accumulators r[j] += a[8 i + j] combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)).
// A full chunk is a perfect binary tree over 64 blocks: one wave per chunk (lane = block, 16-byte loads feed
// the 8 accumulators directly), adjacent-pair shuffles for the tree.  The ragged last chunk follows the
// recursion literally on one thread.
#pragma once
#include "sq_common.h"

// every multiply and add below (and in the including file) is a separate, correctly rounded operation as in numpy: no
// fused contraction
#pragma clang fp contract(off)

namespace {

constexpr int CHUNK = 8192, LEAF = 128;

template <typename T> __device__ __forceinline__ float ld(const T *p, int64_t i) { return (float)p[i]; }

// element transform: plain value (mean pass) or squared deviation (variance pass), all in float32
template <bool SQ> __device__ __forceinline__ float xf(float v, float mean) {
    if (SQ) {
        const float d = v - mean;
        return d * d;
    }
    return v;
}

// numpy's pairwise block for n <= 128 (n >= 8 takes the 8-accumulator path)
template <typename T, bool SQ>
__device__ float pw_block(const T *a, int n, float mean) {
    if (n < 8) {
        float res = 0.f;
        for (int i = 0; i < n; ++i) res += xf<SQ>(ld(a, i), mean);
        return res;
    }
    float r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = xf<SQ>(ld(a, j), mean);
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] += xf<SQ>(ld(a, i + j), mean);
    }
    float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += xf<SQ>(ld(a, i), mean);
    return res;
}

template <typename T, bool SQ>
__device__ float pw_rec(const T *a, int n, float mean) {
    if (n <= LEAF) return pw_block<T, SQ>(a, n, mean);
    int n2 = n / 2;
    n2 -= n2 % 8;
    const float l = pw_rec<T, SQ>(a, n2, mean);
    const float r = pw_rec<T, SQ>(a + n2, n - n2, mean);
    return l + r;
}

// chunk_sums[f][c] for every 8192-element chunk c of frame (or volume) f.  blockDim = 256 = 4 waves = 4 chunks.
template <typename T, bool SQ>
__global__ __launch_bounds__(256) void frame_chunk_sums_kernel(const T *__restrict__ frames,
                                                               const float *__restrict__ mean,
                                                               float *__restrict__ chunk_sums, int64_t npix,
                                                               int nchunks) {
    const int f = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= nchunks) return;
    const T *a = frames + (size_t)f * npix + (size_t)c * CHUNK;
    const int64_t left = npix - (int64_t)c * CHUNK;
    const float m = SQ ? mean[f] : 0.f;
    float s;
    if (left >= CHUNK) {
        s = pw_block<T, SQ>(a + lane * LEAF, LEAF, m);         // lane = block of the perfect tree
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const float o = __shfl_down(s, d);
            s = s + o;                                          // only lanes that are multiples of 2d matter
        }
    } else {
        s = lane == 0 ? pw_rec<T, SQ>(a, (int)left, m) : 0.f;   // ragged tail: the recursion, literally
    }
    if (lane == 0) chunk_sums[(size_t)f * nchunks + c] = s;
}

}  // namespace
