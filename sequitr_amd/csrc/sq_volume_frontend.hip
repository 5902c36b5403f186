// Volume front end on the GPU: raw volumes (V, Z, X, Y; uint8 / uint16 / float32, single channel) -> ImageNorm per volume
// (sequitr/pipeline.py:350-356) -> network bricks (count, BZ, BX, BY, 1) f32, and the brick-shaped network output (uint8
// masks, float32 logits) scattered back into full-volume arrays.  Geometry: include/sequitr_hip.h "Volume front end".
//
// Statistics: the chunk sums are the tile front end's (sq_pairwise.h: numpy's float32 summation order); what differs is the
// end.  numpy divides the float32 sum by an INTEGER count, which is a float64 division rounded to float32; a float32
// division gives the same bits only while the count is exact in float32 (<= 2^24), and a volume has more voxels than that.
//
// The three copy kernels stream rows: the block's indices give (brick, z) and a group of x rows, (volume, kz, kx, ky) and
// the row's base pointers are wave-uniform arithmetic done once, the lanes of a row run along y.  A row's destination is
// written with 16-byte stores from its first 16-byte-aligned element on, scalar stores before it and after the last whole
// 16 bytes (an owned run starts at any y).  No per-element index arithmetic beyond an add.
#include "sq_pairwise.h"

namespace {

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

// elements before the first 16-byte boundary of p, at most n
template <typename E> __device__ __forceinline__ int head_elems(const E *p, int n) {
    const int h = (int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) / sizeof(E));
    return h < n ? h : n;
}

// res = 0; res += chunk (in order), one wave per volume: each lane fetches one chunk sum, the sums are added in chunk
// order out of the lanes (64 loads in flight instead of one dependent load per add); then
// mean = (float)((double)res / n)   or   std = sqrtf((float)((double)res / n))
__global__ __launch_bounds__(64) void volume_stats_finish_kernel(const float *__restrict__ chunk_sums,
                                                                 float *__restrict__ out, int nchunks, double n,
                                                                 int take_sqrt) {
    const int v = blockIdx.x, lane = threadIdx.x;
    const float *p = chunk_sums + (size_t)v * nchunks;
    float res = 0.f;
    for (int base = 0; base < nchunks; base += 64) {
        const int c = base + lane;
        const float s = c < nchunks ? p[c] : 0.f;
        const int m = nchunks - base < 64 ? nchunks - base : 64;
        if (m == 64) {
#pragma unroll
            for (int j = 0; j < 64; ++j) res = res + __shfl(s, j);
        } else {
            for (int j = 0; j < m; ++j) res = res + __shfl(s, j);
        }
    }
    if (lane == 0) {
        const float q = (float)((double)res / n);
        out[v] = take_sqrt ? sqrtf(q) : q;
    }
}

// out[bl][z][x][y] = (vol[v][oz+z][ox+x][oy+y] - mean[v]) / std[v], 0.0f beyond the volume.
// grid (x groups, BZ, count), block (lanes along y, x rows)
template <typename T>
__global__ __launch_bounds__(256) void volume_to_bricks_kernel(const T *__restrict__ vols, const float *__restrict__ mean,
                                                               const float *__restrict__ stdv,
                                                               const int *__restrict__ geom, float *__restrict__ out,
                                                               VolGeom g, int64_t first) {
    const int bl = blockIdx.z, z = blockIdx.y;
    const int x = blockIdx.x * blockDim.y + threadIdx.y;
    if (x >= g.BX) return;
    const BrickAt a = brick_at(g, first + bl);
    const int oz = geom[a.kz], ox = geom[g.KZ + a.kx], oy = geom[g.KZ + g.KX + a.ky];
    const bool norm = mean != nullptr;
    const float m = norm ? mean[a.v] : 0.f, s = norm ? stdv[a.v] : 1.f;
    const int gz = oz + z, gx = ox + x;
    const bool row_in = (unsigned)gz < (unsigned)g.Z && (unsigned)gx < (unsigned)g.X;
    const T *src = vols + (((size_t)a.v * g.Z + (row_in ? gz : 0)) * g.X + (row_in ? gx : 0)) * g.Y;
    float *dst = out + (((size_t)bl * g.BZ + z) * g.BX + x) * g.BY;
    const unsigned Y = row_in ? (unsigned)g.Y : 0u;            // a row outside the volume is all fill
    auto val = [&](int i) -> float {
        const int gy = oy + i;
        if ((unsigned)gy >= Y) return 0.f;
        const float r = (float)src[gy];
        return norm ? (r - m) / s : r;
    };
    const int n = g.BY, tx = threadIdx.x, TX = blockDim.x;
    const int head = head_elems(dst, n), nvec = (n - head) >> 2;
    for (int i = tx; i < head; i += TX) dst[i] = val(i);
    for (int j = tx; j < nvec; j += TX) {
        const int i = head + 4 * j;
        f32x4 o;
        o.x = val(i), o.y = val(i + 1), o.z = val(i + 2), o.w = val(i + 3);
        *reinterpret_cast<f32x4 *>(dst + i) = o;
    }
    for (int i = head + 4 * nvec + tx; i < n; i += TX) dst[i] = val(i);
}

// out[v][gz][gx][ly .. hy) = bricks[bl][gz-oz][gx-ox][ly-oy ..) for every (gz, gx) of the brick's owned box; C values
// per voxel.  grid (x groups, BZ, count), block (lanes along y, x rows); rows beyond the owned box leave at once.
template <typename E>
__global__ __launch_bounds__(256) void bricks_scatter_kernel(const E *__restrict__ bricks, const int *__restrict__ geom,
                                                             E *__restrict__ out, VolGeom g, int C, int64_t first) {
    constexpr int VE = 16 / sizeof(E);
    const int bl = blockIdx.z;
    const BrickAt a = brick_at(g, first + bl);
    const int K = g.KZ + g.KX + g.KY, iz = a.kz, ix = g.KZ + a.kx, iy = g.KZ + g.KX + a.ky;
    const int oz = geom[iz], ox = geom[ix], oy = geom[iy];
    // the owned box, held inside both the brick and the volume whatever the table says: no store or load can leave them
    const int lz = max(geom[K + iz], max(oz, 0)), hz = min(geom[2 * K + iz], min(oz + g.BZ, g.Z));
    const int lx = max(geom[K + ix], max(ox, 0)), hx = min(geom[2 * K + ix], min(ox + g.BX, g.X));
    const int ly = max(geom[K + iy], max(oy, 0)), hy = min(geom[2 * K + iy], min(oy + g.BY, g.Y));
    const int gz = lz + blockIdx.y;
    const int gx = lx + blockIdx.x * blockDim.y + threadIdx.y;
    if (gz >= hz || gx >= hx || hy <= ly) return;
    const E *src = bricks + ((((size_t)bl * g.BZ + (gz - oz)) * g.BX + (gx - ox)) * g.BY + (ly - oy)) * C;
    E *dst = out + ((((size_t)a.v * g.Z + gz) * g.X + gx) * g.Y + ly) * C;
    const int n = (hy - ly) * C, tx = threadIdx.x, TX = blockDim.x;
    const int head = head_elems(dst, n), nvec = (n - head) / VE;
    for (int i = tx; i < head; i += TX) dst[i] = src[i];
    for (int j = tx; j < nvec; j += TX) {
        const int i = head + VE * j;
        uint4 t;
        __builtin_memcpy(&t, src + i, 16);                      // the source run is aligned to its element only
        *reinterpret_cast<uint4 *>(dst + i) = t;
    }
    for (int i = head + VE * nvec + tx; i < n; i += TX) dst[i] = src[i];
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

template <typename T>
int vstats_launch(const T *vols, float *mean, float *stdv, float *ws, int V, int64_t nvox, hipStream_t st) {
    const int nchunks = (int)((nvox + CHUNK - 1) / CHUNK);
    dim3 grid((nchunks + 3) / 4, V);
    hipLaunchKernelGGL((frame_chunk_sums_kernel<T, false>), grid, dim3(256), 0, st, vols, (const float *)nullptr, ws, nvox,
                       nchunks);
    hipLaunchKernelGGL(volume_stats_finish_kernel, dim3(V), dim3(64), 0, st, ws, mean, nchunks, (double)nvox, 0);
    hipLaunchKernelGGL((frame_chunk_sums_kernel<T, true>), grid, dim3(256), 0, st, vols, mean, ws, nvox, nchunks);
    hipLaunchKernelGGL(volume_stats_finish_kernel, dim3(V), dim3(64), 0, st, ws, stdv, nchunks, (double)nvox, 1);
    return sq_check_launch("sq_volume_stats");
}

template <typename T>
int to_bricks_launch(const T *vols, const float *mean, const float *stdv, const int *geom, float *out, const VolGeom &g,
                     int64_t first, int count, hipStream_t st) {
    const dim3 block = row_block((int64_t)g.BY * 4);
    const dim3 grid((g.BX + block.y - 1) / block.y, g.BZ, count);
    hipLaunchKernelGGL(volume_to_bricks_kernel<T>, grid, block, 0, st, vols, mean, stdv, geom, out, g, first);
    return sq_check_launch("sq_volume_to_bricks");
}

template <typename E>
int scatter_launch(const char *what, const E *bricks, const int *geom, E *out, const VolGeom &g, int C, int64_t first,
                   int count, hipStream_t st) {
    const dim3 block = row_block((int64_t)g.BY * C * sizeof(E));
    const dim3 grid((g.BX + block.y - 1) / block.y, g.BZ, count);
    hipLaunchKernelGGL(bricks_scatter_kernel<E>, grid, block, 0, st, bricks, geom, out, g, C, first);
    return sq_check_launch(what);
}

}  // namespace

extern "C" int64_t sq_volume_stats_workspace(int V, int64_t nvox) {
    if (V <= 0 || V > 65535 || nvox <= 0 || nvox > ((int64_t)1 << 40)) return -1;
    return (int64_t)V * ((nvox + CHUNK - 1) / CHUNK) * 4;
}

extern "C" int sq_volume_stats(const void *vols, int dtype, float *mean, float *stdv, void *workspace, int V, int64_t nvox,
                               void *stream) {
    SQ_REQUIRE(vols && mean && stdv && workspace, "sq_volume_stats: null pointer");
    SQ_REQUIRE(sq_volume_stats_workspace(V, nvox) > 0, "sq_volume_stats: need 0 < V <= 65535 and 0 < nvox <= 2^40");
    SQ_REQUIRE_ALIGNED(vols);
    hipStream_t st = (hipStream_t)stream;
    float *ws = reinterpret_cast<float *>(workspace);
    switch (dtype) {
    case SQ_PIX_U8: return vstats_launch(reinterpret_cast<const uint8_t *>(vols), mean, stdv, ws, V, nvox, st);
    case SQ_PIX_U16: return vstats_launch(reinterpret_cast<const uint16_t *>(vols), mean, stdv, ws, V, nvox, st);
    case SQ_PIX_F32: return vstats_launch(reinterpret_cast<const float *>(vols), mean, stdv, ws, V, nvox, st);
    }
    sq_set_error("sq_volume_stats: unknown voxel type %d", dtype);
    return SQ_EINVAL;
}

extern "C" int sq_volume_to_bricks(const void *vols, int dtype, const float *mean, const float *stdv, const int32_t *geom,
                                   float *out, int V, int Z, int X, int Y, int KZ, int KX, int KY, int BZ, int BX, int BY,
                                   int64_t first, int count, void *stream) {
    SQ_REQUIRE(vols && geom && out, "sq_volume_to_bricks: null pointer");
    SQ_REQUIRE((mean == nullptr) == (stdv == nullptr), "sq_volume_to_bricks: give both mean and std, or neither");
    if (int rc = geom_ok("sq_volume_to_bricks", V, Z, X, Y, KZ, KX, KY, BZ, BX, BY, first, count)) return rc;
    const VolGeom g = {V, Z, X, Y, KZ, KX, KY, BZ, BX, BY};
    hipStream_t st = (hipStream_t)stream;
    switch (dtype) {
    case SQ_PIX_U8: return to_bricks_launch(reinterpret_cast<const uint8_t *>(vols), mean, stdv, geom, out, g, first, count, st);
    case SQ_PIX_U16: return to_bricks_launch(reinterpret_cast<const uint16_t *>(vols), mean, stdv, geom, out, g, first, count, st);
    case SQ_PIX_F32: return to_bricks_launch(reinterpret_cast<const float *>(vols), mean, stdv, geom, out, g, first, count, st);
    }
    sq_set_error("sq_volume_to_bricks: unknown voxel type %d", dtype);
    return SQ_EINVAL;
}

extern "C" int sq_bricks_scatter_u8(const uint8_t *bricks, const int32_t *geom, uint8_t *out, int V, int Z, int X, int Y,
                                    int KZ, int KX, int KY, int BZ, int BX, int BY, int64_t first, int count, void *stream) {
    SQ_REQUIRE(bricks && geom && out, "sq_bricks_scatter_u8: null pointer");
    if (int rc = geom_ok("sq_bricks_scatter_u8", V, Z, X, Y, KZ, KX, KY, BZ, BX, BY, first, count)) return rc;
    const VolGeom g = {V, Z, X, Y, KZ, KX, KY, BZ, BX, BY};
    return scatter_launch("sq_bricks_scatter_u8", bricks, geom, out, g, 1, first, count, (hipStream_t)stream);
}

extern "C" int sq_bricks_scatter_f32(const float *bricks, const int32_t *geom, float *out, int V, int Z, int X, int Y, int KZ,
                                     int KX, int KY, int BZ, int BX, int BY, int C, int64_t first, int count, void *stream) {
    SQ_REQUIRE(bricks && geom && out, "sq_bricks_scatter_f32: null pointer");
    SQ_REQUIRE(C > 0 && C <= 64, "sq_bricks_scatter_f32: %d channels not in 1 .. 64", C);
    if (int rc = geom_ok("sq_bricks_scatter_f32", V, Z, X, Y, KZ, KX, KY, BZ, BX, BY, first, count)) return rc;
    const VolGeom g = {V, Z, X, Y, KZ, KX, KY, BZ, BX, BY};
    return scatter_launch("sq_bricks_scatter_f32", bricks, geom, out, g, C, first, count, (hipStream_t)stream);
}
