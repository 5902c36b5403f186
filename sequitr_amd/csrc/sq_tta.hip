// Tile views and probability stitch (include/sequitr_hip.h "Tile views and probability stitch"): the two streaming steps
// that test-time augmentation and whole-frame class probabilities put around the network, both in HBM.
//
// sq_tiles_view_f32: dst (+)= one of the eight symmetries of the square applied to every (T, T, E) tile.  The inverse of an
// op is again one of the eight, so one kernel family serves both directions.
//   * un-transposed ops (0 .. 3) are row streams: a destination row is a source row, its pixels mirrored or not.  A lane
//     moves 16 bytes when the row length allows (E % 4 == 0: a quarter pixel or more, stored as read; E = 1, 2: a run of
//     4 or 2 mirrored pixels, read as one vector and permuted in registers; no mirror: a straight copy), one float
//     otherwise.
//   * transposed ops (4 .. 7) go through an LDS block of B x B pixels (B = 32 for E <= 4, 16 above: 17 KiB a block, so LDS
//     never limits the 8 blocks of 256 threads a CU holds): half-waves read runs of B pixels along the SOURCE rows, and
//     after the barrier write runs of B pixels along the DESTINATION rows.  The LDS row pitch is B * E plus a pad that
//     makes pitch = E (mod 32), so the 32 lanes of a transposed read -- element w = jl * E + e of a destination run --
//     hit bank (il * E + w) mod 32: 32 different banks.
//   * SQ_TTA_LDS=0 (read per call) takes the direct gather for the transposed ops instead: the row kernels with the
//     general index map, destination-contiguous, source strided by T * E floats.  The same bits.
// Every destination element is read (when accumulating), changed and written by exactly one thread, once.
//
// sq_stitch_probs: one frame pixel per lane; its K logits are one contiguous run in the owner tile, read as vectors; the
// argmax is sq_argmax_u8's loop, the softmax the header's expression with contraction off, and every class plane gets one
// coalesced store per wave.
//
// sq_bricks_view_f32 (include/sequitr_hip.h "Brick views and probability scatter") is the same kernel family: a brick
// batch (N, BZ, BX, BY, E) is N * BZ slices of BX rows of BY pixels; bit 0 of its op remaps the slice (z mirrored inside
// its brick), the other three bits are the in-plane op.  The row kernels take rectangular slices (BX != BY) for the
// un-transposed ops.  sq_tiles_view_f32 is the BZ = 1, BX = BY = T call of the same templates with VOL off: one slice size and
// no remap at compile time, because the run-time general form cost the planar merge 4 - 8 % (profiles/volume_tta_bench.json).
#include "sq_probs.h"
#include <stdlib.h>

#pragma clang fp contract(off)

namespace {

constexpr int TTA_THREADS = 256, TTA_GRID_CAP = 16384;
constexpr int VIEW_LDS_FLOATS = 4352;                           // 16 rows of 272 floats (E = 16), 32 rows of 132 (E = 4)

inline int view_block(int E) { return E <= 4 ? 32 : 16; }
inline int view_pitch(int B, int E) { return B * E + (((E - B * E) % 32) + 32) % 32; }

enum { ROWS_SCALAR = 0, ROWS_VEC_PIXEL = 1, ROWS_VEC_RUN = 2 };

// source pixel (a, b) of destination pixel (i, j) under the in-plane op; slices of TX rows of TY pixels, TX == TY under bit 2
__device__ __forceinline__ void view_source(int op, unsigned TX, unsigned TY, unsigned i, unsigned j, unsigned &a, unsigned &b) {
    const unsigned p = (op & 4) ? j : i, q = (op & 4) ? i : j;
    a = (op & 1) ? TX - 1 - p : p;
    b = (op & 2) ? TY - 1 - q : q;
}

// source slice of destination slice n: z mirrored inside its brick of BZ slices when fz (wave-uniform branch)
__device__ __forceinline__ unsigned view_slice(unsigned n, unsigned BZ, int fz) {
    return fz ? n + BZ - 1 - 2 * (n % BZ) : n;
}

// A block takes chunks of 256 consecutive units of the flat destination; UR units make a destination row.
//   ROWS_SCALAR    : a unit is one float, any op
//   ROWS_VEC_PIXEL : a unit is 4 floats inside one pixel (E % 4 == 0), any op
//   ROWS_VEC_RUN   : a unit is 4 floats of a row (TY * E % 4 == 0), ops 0 .. 3 with E = 1 or 2 when bit 1 mirrors
// VOL: brick slices -- TX x TY pixels, the source slice remapped under fz; without it the planar tile of the parent form,
// TY == TX and no remap, so that sq_tiles_view_f32 keeps the instruction stream it was measured with.
template <int MODE, bool ACC, bool VOL>
__global__ __launch_bounds__(TTA_THREADS) void view_rows_kernel(const float *__restrict__ src, float *__restrict__ dst,
                                                                unsigned TX, unsigned TYv, unsigned E, int op, unsigned BZ,
                                                                int fz, unsigned UR, int64_t total) {
    const unsigned TY = VOL ? TYv : TX;
    const int64_t nchunks = (total + TTA_THREADS - 1) / TTA_THREADS;
    const size_t R = (size_t)TY * E;
    for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const int64_t base = chunk * TTA_THREADS;
        if (base + threadIdx.x >= total) continue;
        const int64_t base_row = base / UR;                     // the one 64-bit division is the block's
        const unsigned l = (unsigned)(base - base_row * UR) + threadIdx.x;
        const unsigned row = (unsigned)base_row + l / UR, u = l % UR;   // row < slices * TX < 2^31 (checked on the host)
        const unsigned i = row % TX, n = VOL ? view_slice(row / TX, BZ, fz) : row / TX;
        if (MODE == ROWS_SCALAR) {
            const unsigned j = u / E, e = u % E;
            unsigned a, b;
            view_source(op, TX, TY, i, j, a, b);
            const float s = src[(((size_t)n * TX + a) * TY + b) * E + e];
            float *d = dst + (size_t)row * R + u;
            *d = ACC ? *d + s : s;
        } else {
            size_t from;
            bool mirrored = false;
            if (MODE == ROWS_VEC_PIXEL) {
                const unsigned f = 4 * u, j = f / E, e = f % E;
                unsigned a, b;
                view_source(op, TX, TY, i, j, a, b);
                from = (((size_t)n * TX + a) * TY + b) * E + e;
            } else {
                const unsigned a = (op & 1) ? TX - 1 - i : i;
                mirrored = (op & 2) != 0;
                from = ((size_t)n * TX + a) * R + (mirrored ? R - 4 - 4 * (size_t)u : 4 * (size_t)u);
            }
            f32x4 v = *reinterpret_cast<const f32x4 *>(src + from);
            if (MODE == ROWS_VEC_RUN && mirrored) {
                const f32x4 r1 = {v.w, v.z, v.y, v.x}, r2 = {v.z, v.w, v.x, v.y};
                v = E == 1 ? r1 : r2;
            }
            f32x4 *d = reinterpret_cast<f32x4 *>(dst + (size_t)row * R + 4 * (size_t)u);
            if (ACC) {
                const f32x4 o = *d;
                v = {o.x + v.x, o.y + v.y, o.z + v.z, o.w + v.w};
            }
            *d = v;
        }
    }
}

// Transposed ops: an item is the B x B pixel block (I0, J0) of destination slice n (square slices of T x T pixels).  Eight half-waves: half-wave g takes
// rows g, g + 8, ... of the block, its 32 lanes a run of floats.  ET: E at compile time, 0 = read E at run time.
template <int ET, bool ACC, bool VOL>
__global__ __launch_bounds__(TTA_THREADS) void view_tiles_kernel(const float *__restrict__ src, float *__restrict__ dst,
                                                                 unsigned T, unsigned Ert, int op, unsigned BZ, int fz,
                                                                 unsigned B, unsigned pitch, unsigned nb, int64_t items) {
    __shared__ float lds[VIEW_LDS_FLOATS];
    const unsigned E = ET ? (unsigned)ET : Ert;
    const unsigned g = threadIdx.x >> 5, lane = threadIdx.x & 31;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const unsigned n = (unsigned)(item / (nb * nb)), r = (unsigned)(item % (nb * nb));
        const unsigned I0 = (r / nb) * B, J0 = (r % nb) * B;
        const unsigned ni = min(B, T - I0), nj = min(B, T - J0);
        // lds[jl][il][e] = src[n, a(J0 + jl), b(I0 + il), e]: lanes along il, e -- the source row
        for (unsigned jl = g; jl < nj; jl += 8) {
            const unsigned a = (op & 1) ? T - 1 - (J0 + jl) : J0 + jl;
            const float *s = src + ((size_t)(VOL ? view_slice(n, BZ, fz) : n) * T + a) * T * E;
            for (unsigned w = lane; w < ni * E; w += 32) {
                const unsigned il = w / E, e = w - il * E;
                const unsigned b = (op & 2) ? T - 1 - (I0 + il) : I0 + il;
                lds[jl * pitch + w] = s[(size_t)b * E + e];
            }
        }
        __syncthreads();
        for (unsigned il = g; il < ni; il += 8) {
            float *d = dst + (((size_t)n * T + I0 + il) * T + J0) * E;
            for (unsigned w = lane; w < nj * E; w += 32) {
                const unsigned jl = w / E, e = w - jl * E;
                const float s = lds[jl * pitch + il * E + e];
                d[w] = ACC ? d[w] + s : s;
            }
        }
        __syncthreads();                                        // the next item overwrites the block
    }
}

inline unsigned tta_grid(int64_t blocks) { return (unsigned)(blocks < 1 ? 1 : (blocks > TTA_GRID_CAP ? TTA_GRID_CAP : blocks)); }

// SQ_TTA_LDS=0: A/B switch to the direct gather for the transposed ops; read per call
inline bool tta_lds() {
    const char *e = getenv("SQ_TTA_LDS");
    return !(e && e[0] == '0');
}

template <int MODE, bool VOL>
void rows_launch(const float *src, float *dst, int TX, int TY, int E, int op, int BZ, int fz, unsigned UR, int64_t total, bool acc,
                 hipStream_t st) {
    const dim3 grid(tta_grid((total + TTA_THREADS - 1) / TTA_THREADS)), block(TTA_THREADS);
    if (acc)
        hipLaunchKernelGGL((view_rows_kernel<MODE, true, VOL>), grid, block, 0, st, src, dst, (unsigned)TX, (unsigned)TY, (unsigned)E, op,
                           (unsigned)BZ, fz, UR, total);
    else
        hipLaunchKernelGGL((view_rows_kernel<MODE, false, VOL>), grid, block, 0, st, src, dst, (unsigned)TX, (unsigned)TY, (unsigned)E, op,
                           (unsigned)BZ, fz, UR, total);
}

template <int ET, bool VOL>
void tiles_launch(const float *src, float *dst, int64_t N, int T, int E, int op, int BZ, int fz, bool acc, hipStream_t st) {
    const unsigned B = (unsigned)view_block(E), pitch = (unsigned)view_pitch((int)B, E), nb = ((unsigned)T + B - 1) / B;
    const int64_t items = N * nb * nb;
    const dim3 grid(tta_grid(items)), block(TTA_THREADS);
    if (acc) hipLaunchKernelGGL((view_tiles_kernel<ET, true, VOL>), grid, block, 0, st, src, dst, (unsigned)T, (unsigned)E, op, (unsigned)BZ, fz, B, pitch, nb, items);
    else hipLaunchKernelGGL((view_tiles_kernel<ET, false, VOL>), grid, block, 0, st, src, dst, (unsigned)T, (unsigned)E, op, (unsigned)BZ, fz, B, pitch, nb, items);
}

// frame pixel (f, y, x) of the flat order, 256 consecutive pixels a chunk; P: float or uint8_t planes
template <int K, typename P>
__global__ __launch_bounds__(TTA_THREADS) void stitch_probs_kernel(const float *__restrict__ logits, const int *__restrict__ ymap,
                                                                   const int *__restrict__ xmap, uint8_t *__restrict__ mask,
                                                                   P *__restrict__ prob, float inv_n, unsigned H, unsigned W,
                                                                   unsigned TR, unsigned TC, unsigned TS, int64_t total) {
    const int64_t nchunks = (total + TTA_THREADS - 1) / TTA_THREADS;
    for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const int64_t base = chunk * TTA_THREADS;
        if (base + threadIdx.x >= total) continue;
        const int64_t base_row = base / W;
        const unsigned l = (unsigned)(base - base_row * W) + threadIdx.x;
        const unsigned row = (unsigned)base_row + l / W, x = l % W;     // row < F * H < 2^31 (checked on the host)
        const unsigned y = row % H, f = row / H;
        const int ym = ymap[y], xm = xmap[x];
        const size_t t = ((size_t)f * TR + (unsigned)(ym >> 16)) * TC + (unsigned)(xm >> 16);
        float z[K];
        load_pixel<K>(logits + ((t * TS + (unsigned)(ym & 0xffff)) * TS + (unsigned)(xm & 0xffff)) * K, z);
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
void stitch_launch(const float *logits, const int *ymap, const int *xmap, uint8_t *mask, void *prob, int prob_dtype, float inv_n,
                   int F, int H, int W, int TR, int TC, int TS, hipStream_t st) {
    const int64_t total = (int64_t)F * H * W;
    const dim3 grid(tta_grid((total + TTA_THREADS - 1) / TTA_THREADS)), block(TTA_THREADS);
    if (prob && prob_dtype == SQ_PIX_U8)
        hipLaunchKernelGGL((stitch_probs_kernel<K, uint8_t>), grid, block, 0, st, logits, ymap, xmap, mask,
                           reinterpret_cast<uint8_t *>(prob), inv_n, (unsigned)H, (unsigned)W, (unsigned)TR, (unsigned)TC,
                           (unsigned)TS, total);
    else
        hipLaunchKernelGGL((stitch_probs_kernel<K, float>), grid, block, 0, st, logits, ymap, xmap, mask,
                           reinterpret_cast<float *>(prob), inv_n, (unsigned)H, (unsigned)W, (unsigned)TR, (unsigned)TC,
                           (unsigned)TS, total);
}

}  // namespace

extern "C" int sq_tiles_view_block(int E) { return (E >= 1 && E <= 16) ? view_block(E) : -1; }

// dst (+)= the in-plane op (bit 0 mirrors the rows, bit 1 the pixels of a row, bit 2 transposes) of every slice, the source
// slice z-mirrored inside its brick of BZ when fz: what both entry points launch
template <bool VOL>
static int view_launch(const char *what, const float *src, float *dst, int64_t slices, int BZ, int TX, int TY, int E, int op, int fz,
                       bool acc, hipStream_t st) {
    if ((op & 4) && tta_lds()) {
        switch (E) {
        case 1: tiles_launch<1, VOL>(src, dst, slices, TX, E, op, BZ, fz, acc, st); break;
        case 2: tiles_launch<2, VOL>(src, dst, slices, TX, E, op, BZ, fz, acc, st); break;
        case 3: tiles_launch<3, VOL>(src, dst, slices, TX, E, op, BZ, fz, acc, st); break;
        case 4: tiles_launch<4, VOL>(src, dst, slices, TX, E, op, BZ, fz, acc, st); break;
        case 8: tiles_launch<8, VOL>(src, dst, slices, TX, E, op, BZ, fz, acc, st); break;
        case 16: tiles_launch<16, VOL>(src, dst, slices, TX, E, op, BZ, fz, acc, st); break;
        default: tiles_launch<0, VOL>(src, dst, slices, TX, E, op, BZ, fz, acc, st); break;
        }
        return sq_check_launch(what);
    }
    const int64_t R = (int64_t)TY * E, rows = slices * TX;
    if (E % 4 == 0 && ((op & 4) || (op & 2)))
        rows_launch<ROWS_VEC_PIXEL, VOL>(src, dst, TX, TY, E, op, BZ, fz, (unsigned)(R / 4), rows * (R / 4), acc, st);
    else if (!(op & 4) && R % 4 == 0 && (!(op & 2) || E <= 2))
        rows_launch<ROWS_VEC_RUN, VOL>(src, dst, TX, TY, E, op, BZ, fz, (unsigned)(R / 4), rows * (R / 4), acc, st);
    else
        rows_launch<ROWS_SCALAR, VOL>(src, dst, TX, TY, E, op, BZ, fz, (unsigned)R, rows * R, acc, st);
    return sq_check_launch(what);
}

extern "C" int sq_tiles_view_f32(const float *src, float *dst, int N, int T, int E, int op, int inverse, int accumulate,
                                 void *stream) {
    const char *what = "sq_tiles_view_f32";
    SQ_REQUIRE(src && dst, "%s: null pointer", what);
    SQ_REQUIRE(op >= 0 && op <= 7, "%s: op %d is not one of 0 .. 7", what, op);
    SQ_REQUIRE(E >= 1 && E <= 16, "%s: %d elements per pixel are not 1 .. 16", what, E);
    SQ_REQUIRE(T >= 1 && T <= 65535, "%s: tile %d is not 1 .. 65535", what, T);
    SQ_REQUIRE(N >= 1 && (int64_t)N * T <= 0x7fffffff, "%s: %d tiles of %d rows are out of range", what, N, T);
    const size_t bytes = (size_t)N * T * T * E * sizeof(float);
    const uintptr_t s0 = (uintptr_t)src, d0 = (uintptr_t)dst;
    SQ_REQUIRE(s0 + bytes <= d0 || d0 + bytes <= s0, "%s: src and dst overlap (a view is not made in place)", what);
    SQ_REQUIRE_ALIGNED(src);
    SQ_REQUIRE_ALIGNED(dst);
    static const int inverse_op[8] = {0, 1, 2, 3, 4, 6, 5, 7};   // unview_op == view_op'
    if (inverse) op = inverse_op[op];
    return view_launch<false>(what, src, dst, N, 1, T, T, E, op, 0, accumulate != 0, (hipStream_t)stream);
}

extern "C" int sq_bricks_view_f32(const float *src, float *dst, int N, int BZ, int BX, int BY, int E, int op, int inverse,
                                  int accumulate, void *stream) {
    const char *what = "sq_bricks_view_f32";
    SQ_REQUIRE(src && dst, "%s: null pointer", what);
    SQ_REQUIRE(op >= 0 && op <= 15, "%s: op %d is not one of 0 .. 15", what, op);
    SQ_REQUIRE(E >= 1 && E <= 16, "%s: %d elements per voxel are not 1 .. 16", what, E);
    SQ_REQUIRE(N >= 1 && BZ >= 1 && BX >= 1 && BY >= 1, "%s: sizes must be positive", what);
    SQ_REQUIRE(BX <= 65535 && BY <= 65535, "%s: brick rows %d x %d are not 1 .. 65535", what, BX, BY);
    SQ_REQUIRE(!(op & 8) || BX == BY, "%s: op %d transposes x and y, the brick is %d x %d", what, op, BX, BY);
    SQ_REQUIRE((int64_t)N * BZ * BX <= 0x7fffffff, "%s: %d bricks of %d x %d rows are out of range", what, N, BZ, BX);
    const size_t bytes = (size_t)N * BZ * BX * BY * E * sizeof(float);
    const uintptr_t s0 = (uintptr_t)src, d0 = (uintptr_t)dst;
    SQ_REQUIRE(s0 + bytes <= d0 || d0 + bytes <= s0, "%s: src and dst overlap (a view is not made in place)", what);
    SQ_REQUIRE_ALIGNED(src);
    SQ_REQUIRE_ALIGNED(dst);
    // unview_op == view_op': under the transpose the x and y mirrors change places
    static const int inverse_op[16] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 10, 11, 14, 15};
    if (inverse) op = inverse_op[op];
    // The brick op transposes first and mirrors the result (the volume sampler's order): dst[x, y] = src[fy(y), fx(x)].
    // The in-plane op of the kernels mirrors first: dst[i, j] = src[f0(j), f1(i)].  So under the transpose f0 is the y
    // mirror and f1 the x mirror; without it f0 mirrors x and f1 mirrors y.
    const int fx = (op >> 1) & 1, fy = (op >> 2) & 1, t = (op >> 3) & 1;
    const int plane_op = t ? (fy | fx << 1 | 4) : (fx | fy << 1);
    return view_launch<true>(what, src, dst, (int64_t)N * BZ, BZ, BX, BY, E, plane_op, op & 1, accumulate != 0, (hipStream_t)stream);
}

extern "C" int sq_stitch_probs(const float *tile_logits, const int32_t *ymap, const int32_t *xmap, uint8_t *mask_out,
                               void *prob_out, int prob_dtype, float inv_n, int F, int H, int W, int TR, int TC, int TS, int K,
                               void *stream) {
    const char *what = "sq_stitch_probs";
    SQ_REQUIRE(tile_logits && ymap && xmap, "%s: null pointer", what);
    SQ_REQUIRE(mask_out || prob_out, "%s: null pointer: give mask_out, prob_out or both", what);
    SQ_REQUIRE(!prob_out || prob_dtype == SQ_PIX_U8 || prob_dtype == SQ_PIX_F32, "%s: prob_dtype %d is not SQ_PIX_U8 or SQ_PIX_F32",
               what, prob_dtype);
    SQ_REQUIRE(K >= 1 && K <= 16, "%s: %d classes are not 1 .. 16", what, K);
    SQ_REQUIRE(F > 0 && H > 0 && W > 0 && TR > 0 && TC > 0 && TS > 0 && TS < 65536, "%s: bad geometry", what);
    SQ_REQUIRE((int64_t)F * H <= 0x7fffffff, "%s: %d frames of %d rows are out of range", what, F, H);
    SQ_REQUIRE(inv_n > 0.f && inv_n <= 1.f, "%s: inv_n %g is not in (0, 1]", what, (double)inv_n);
    SQ_REQUIRE_ALIGNED(tile_logits);
    SQ_REQUIRE(((uintptr_t)ymap | (uintptr_t)xmap) % 4 == 0 && (!prob_out || prob_dtype == SQ_PIX_U8 || (uintptr_t)prob_out % 4 == 0),
               "%s: arrays must be aligned to their elements", what);
    hipStream_t st = (hipStream_t)stream;
#define SQ_STITCH_K(k) case k: stitch_launch<k>(tile_logits, ymap, xmap, mask_out, prob_out, prob_dtype, inv_n, F, H, W, TR, TC, TS, st); break;
    switch (K) {
        SQ_STITCH_K(1) SQ_STITCH_K(2) SQ_STITCH_K(3) SQ_STITCH_K(4) SQ_STITCH_K(5) SQ_STITCH_K(6) SQ_STITCH_K(7) SQ_STITCH_K(8)
        SQ_STITCH_K(9) SQ_STITCH_K(10) SQ_STITCH_K(11) SQ_STITCH_K(12) SQ_STITCH_K(13) SQ_STITCH_K(14) SQ_STITCH_K(15) SQ_STITCH_K(16)
    }
#undef SQ_STITCH_K
    return sq_check_launch(what);
}
