// Class masks and class probability maps of whole volumes from merged brick logits (include/sequitr_hip.h "Brick views and
// probability scatter"): the volumetric sibling of sq_stitch_probs.  The brick views themselves are sq_tta.hip's kernels
// (a brick is BZ slices).
//
// sq_bricks_scatter_probs: bricks_scatter_kernel's grid -- (x groups, BZ, count), lanes along y -- over every brick's owned
// box, clamped into brick and volume.  A lane owns one voxel: its K logits are one contiguous run in the brick, read as
// vectors; the class is sq_argmax_u8's loop, the softmax the header's expression with contraction off (sq_probs.h: the
// code sq_stitch_probs runs), and the mask and every class plane get one store per lane, consecutive lanes consecutive y.
#include "sq_probs.h"

#pragma clang fp contract(off)

namespace {

// The brick geometry as sq_volume_frontend.hip carries it (VolGeom, brick_at, row_block, geom_ok), restated: that file's
// helpers are local to it.
struct VolGeom {
    int V, Z, X, Y, KZ, KX, KY, BZ, BX, BY;
};

// brick b of the whole stack -> volume and brick indices along the axes (wave-uniform)
struct BrickAt {
    int v, kz, kx, ky;
};
__device__ __forceinline__ BrickAt brick_at(const VolGeom &g, int64_t b) {
    const int per = g.KZ * g.KX * g.KY;
    BrickAt a;
    a.v = (int)(b / per);
    int r = (int)(b - (int64_t)a.v * per);
    a.ky = r % g.KY;
    r /= g.KY;
    a.kx = r % g.KX;
    a.kz = r / g.KX;
    return a;
}

// block (TX lanes along a row, 256 / TX rows): TX = the power of two that covers a row's 16-byte pieces, 4 .. 64
inline dim3 row_block(int64_t row_bytes) {
    const int64_t pieces = (row_bytes + 15) / 16 + 1;
    unsigned tx = 4;
    while (tx < 64 && tx < pieces) tx *= 2;
    return dim3(tx, 256 / tx);
}

inline int geom_ok(const char *what, int V, int Z, int X, int Y, int KZ, int KX, int KY, int BZ, int BX, int BY, int64_t first,
                   int count) {
    SQ_REQUIRE(V > 0 && Z > 0 && X > 0 && Y > 0 && KZ > 0 && KX > 0 && KY > 0 && BZ > 0 && BX > 0 && BY > 0,
               "%s: sizes must be positive", what);
    SQ_REQUIRE((int64_t)KZ * KX * KY < (1 << 30) && BZ <= 65535 && (int64_t)BY < (1 << 24), "%s: geometry out of range", what);
    SQ_REQUIRE(count > 0 && count <= 65535, "%s: count %d not in 1 .. 65535", what, count);
    SQ_REQUIRE(first >= 0 && first + count <= (int64_t)V * KZ * KX * KY, "%s: bricks %lld .. %lld of %lld", what,
               (long long)first, (long long)(first + count - 1), (long long)((int64_t)V * KZ * KX * KY));
    return SQ_OK;
}

template <int K, typename P>
__global__ __launch_bounds__(256) void bricks_scatter_probs_kernel(const float *__restrict__ logits, const int *__restrict__ geom,
                                                                   uint8_t *__restrict__ mask, P *__restrict__ prob, float inv_n,
                                                                   VolGeom g, int64_t first) {
    const int bl = blockIdx.z;
    const BrickAt a = brick_at(g, first + bl);
    const int NK = g.KZ + g.KX + g.KY, iz = a.kz, ix = g.KZ + a.kx, iy = g.KZ + g.KX + a.ky;
    const int oz = geom[iz], ox = geom[ix], oy = geom[iy];
    // the owned box, held inside both the brick and the volume whatever the table says: no store or load can leave them
    const int lz = max(geom[NK + iz], max(oz, 0)), hz = min(geom[2 * NK + iz], min(oz + g.BZ, g.Z));
    const int lx = max(geom[NK + ix], max(ox, 0)), hx = min(geom[2 * NK + ix], min(ox + g.BX, g.X));
    const int ly = max(geom[NK + iy], max(oy, 0)), hy = min(geom[2 * NK + iy], min(oy + g.BY, g.Y));
    const int gz = lz + blockIdx.y;
    const int gx = lx + blockIdx.x * blockDim.y + threadIdx.y;
    if (gz >= hz || gx >= hx || hy <= ly) return;
    const float *src = logits + ((((size_t)bl * g.BZ + (gz - oz)) * g.BX + (gx - ox)) * g.BY + (ly - oy)) * K;
    const size_t plane = (size_t)g.Z * g.X * g.Y, row = ((size_t)gz * g.X + gx) * g.Y + ly;
    uint8_t *mrow = mask ? mask + (size_t)a.v * plane + row : nullptr;
    P *prow = prob ? prob + (size_t)a.v * K * plane + row : nullptr;
    const int n = hy - ly;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        float z[K], bv;
        load_pixel<K>(src + (size_t)i * K, z);
        const int best = pixel_class<K>(z, bv);
        if (mrow) mrow[i] = (uint8_t)best;
        if (prow) {
            const float s = pixel_exps<K>(z, bv, inv_n);
            P *o = prow + i;
#pragma unroll
            for (int c = 0; c < K; ++c, o += plane) store_prob(o, z[c] / s);
        }
    }
}

template <int K>
void scatter_probs_launch(const float *logits, const int *geom, uint8_t *mask, void *prob, int prob_dtype, float inv_n,
                          const VolGeom &g, int64_t first, int count, hipStream_t st) {
    const dim3 block = row_block((int64_t)g.BY * 16);           // a lane per voxel: up to 64 lanes along y
    const dim3 grid((g.BX + block.y - 1) / block.y, g.BZ, count);
    if (prob && prob_dtype == SQ_PIX_U8)
        hipLaunchKernelGGL((bricks_scatter_probs_kernel<K, uint8_t>), grid, block, 0, st, logits, geom, mask,
                           reinterpret_cast<uint8_t *>(prob), inv_n, g, first);
    else
        hipLaunchKernelGGL((bricks_scatter_probs_kernel<K, float>), grid, block, 0, st, logits, geom, mask,
                           reinterpret_cast<float *>(prob), inv_n, g, first);
}

}  // namespace

extern "C" int sq_bricks_scatter_probs(const float *brick_logits, const int32_t *geom, uint8_t *mask_out, void *prob_out,
                                       int prob_dtype, float inv_n, int V, int Z, int X, int Y, int KZ, int KX, int KY, int BZ,
                                       int BX, int BY, int K, int64_t first, int count, void *stream) {
    const char *what = "sq_bricks_scatter_probs";
    SQ_REQUIRE(brick_logits && geom, "%s: null pointer", what);
    SQ_REQUIRE(mask_out || prob_out, "%s: null pointer: give mask_out, prob_out or both", what);
    SQ_REQUIRE(!prob_out || prob_dtype == SQ_PIX_U8 || prob_dtype == SQ_PIX_F32, "%s: prob_dtype %d is not SQ_PIX_U8 or SQ_PIX_F32",
               what, prob_dtype);
    SQ_REQUIRE(K >= 1 && K <= 16, "%s: %d classes are not 1 .. 16", what, K);
    SQ_REQUIRE(inv_n > 0.f && inv_n <= 1.f, "%s: inv_n %g is not in (0, 1]", what, (double)inv_n);
    if (int rc = geom_ok(what, V, Z, X, Y, KZ, KX, KY, BZ, BX, BY, first, count)) return rc;
    SQ_REQUIRE_ALIGNED(brick_logits);
    SQ_REQUIRE((uintptr_t)geom % 4 == 0 && (!prob_out || prob_dtype == SQ_PIX_U8 || (uintptr_t)prob_out % 4 == 0),
               "%s: arrays must be aligned to their elements", what);
    const VolGeom g = {V, Z, X, Y, KZ, KX, KY, BZ, BX, BY};
    hipStream_t st = (hipStream_t)stream;
#define SQ_SCATTER_K(k) case k: scatter_probs_launch<k>(brick_logits, geom, mask_out, prob_out, prob_dtype, inv_n, g, first, count, st); break;
    switch (K) {
        SQ_SCATTER_K(1) SQ_SCATTER_K(2) SQ_SCATTER_K(3) SQ_SCATTER_K(4) SQ_SCATTER_K(5) SQ_SCATTER_K(6) SQ_SCATTER_K(7) SQ_SCATTER_K(8)
        SQ_SCATTER_K(9) SQ_SCATTER_K(10) SQ_SCATTER_K(11) SQ_SCATTER_K(12) SQ_SCATTER_K(13) SQ_SCATTER_K(14) SQ_SCATTER_K(15) SQ_SCATTER_K(16)
    }
#undef SQ_SCATTER_K
    return sq_check_launch(what);
}
