// Volume sampler: augmented training bricks cut out of volumes that stay in HBM (include/sequitr_hip.h "Volume sampler";
// the reference's ImageSample + ImageFlip + the quarter turns of ImageRotate, sequitr/pipeline.py).  A plan row
// [v, oz, ox, oy, op] gives the volume, the origin of a (BZ, BX, BY) box and a symmetry: bit 0 flips z, bit 1 flips x, bit 2
// flips y, bit 3 transposes x and y.  Output voxel (z, x, y) of a brick is box voxel (fz(z), a, b), (a, b) = (fx(x), fy(y))
// or, transposed, (fy(y), fx(x)), f the identity or the mirror of its axis; a box voxel outside the volume is fill.
//
// One kernel body serves the three entry points through a policy: how a voxel is loaded into a staging word W, and how
// the K output units U of a voxel come out of that word (images: one float; copies: the element, or three bytes of it;
// one-hot: C bytes (label == c)).
//
// sample_rows_kernel streams output rows like the volume front end's kernels: the block's indices give (brick, z) and a
// group of x rows, the plan row, the symmetry and the source base are wave-uniform arithmetic done once, the lanes of a
// row run along y.  A row is written with 16-byte stores from its first 16-byte-aligned unit on, scalar stores before and
// after.  Along the row the source index is base + t * stride, t = o + y or o + BY-1 - y: stride 1 for the plain and
// flipped ops (a y flip reads the same row backwards), stride Y for the transposed ones (the direct gather).
//
// sample_tiles_kernel takes the transposed ops instead (default; SQ_SAMPLE_LDS=0 leaves them to the gather): a 64 x 64
// tile of the plane is loaded with the lanes along the source's contiguous axis into LDS rows padded by one word, and
// written with the lanes along the output's contiguous axis -- a column read of the tile, 65 words apart, conflict-free.
// Both paths evaluate the same expression per voxel, so they produce the same bits.
//
// The plan is data: coordinates are formed in unsigned arithmetic (exact modulo 2^32, and a true coordinate lies in
// [0, L) exactly when the wrapped one does), every load is guarded by coordinate < length, v by v < V.
#include <stdlib.h>
#include <type_traits>
#include "sq_common.h"

namespace {

struct SampGeom {
    int V, Z, X, Y, BZ, BX, BY;
};

constexpr int TILE = 64;

template <typename T> struct ImagePolicy {
    using U = float;
    using W = float;
    static constexpr int KT = 1;
    const T *src;
    const float *mean, *stdv;
    struct Ctx {
        float m, s;
        bool norm;
    };
    __device__ __forceinline__ Ctx ctx(int v) const {
        Ctx c;
        c.norm = mean != nullptr;
        c.m = c.norm ? mean[v] : 0.f;
        c.s = c.norm ? stdv[v] : 1.f;
        return c;
    }
    __device__ __forceinline__ W load(size_t i, const Ctx &c) const {
        const float r = (float)src[i];
        return c.norm ? (r - c.m) / c.s : r;                    // volume_to_bricks_kernel's expression
    }
    __device__ __forceinline__ static U unit(W w, int) { return w; }
    __device__ __forceinline__ static W fill() { return 0.f; }
};

// voxels of K_ units of type E (K_ = 3 with E = uint8_t: three-byte voxels), moved verbatim
template <typename E, int K_> struct CopyPolicy {
    using U = E;
    using W = typename std::conditional<sizeof(E) == 8, uint64_t, uint32_t>::type;
    static constexpr int KT = K_;
    const E *src;
    struct Ctx {};
    __device__ __forceinline__ Ctx ctx(int) const { return Ctx(); }
    __device__ __forceinline__ W load(size_t i, const Ctx &) const {
        if (K_ == 1) return (W)src[i];
        const E *p = src + i * K_;
        return (W)p[0] | ((W)p[1] << 8) | ((W)p[2] << 16);
    }
    __device__ __forceinline__ static U unit(W w, int sub) { return K_ == 1 ? (U)w : (U)(w >> (8 * sub)); }
    __device__ __forceinline__ static W fill() { return 0; }
};

struct OnehotPolicy {
    using U = uint8_t;
    using W = uint32_t;
    static constexpr int KT = 0;                                // C units per voxel, known at run time
    const uint8_t *src;
    struct Ctx {};
    __device__ __forceinline__ Ctx ctx(int) const { return Ctx(); }
    __device__ __forceinline__ W load(size_t i, const Ctx &) const { return src[i]; }
    __device__ __forceinline__ static U unit(W w, int sub) { return (U)(w == (W)sub); }
    __device__ __forceinline__ static W fill() { return 0xffffffffu; }   // equals no class
};

// units before the first 16-byte boundary of p, at most n
template <typename E> __device__ __forceinline__ int head_units(const E *p, int n) {
    const int h = (int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) / sizeof(E));
    return h < n ? h : n;
}

// grid (x groups, BZ, count), block (lanes along y, x rows).  skip_transposed: those bricks are sample_tiles_kernel's.
template <typename P>
__global__ __launch_bounds__(256) void sample_rows_kernel(P p, const int *__restrict__ plan, typename P::U *__restrict__ out,
                                                          SampGeom g, int Krt, int opmask, int skip_transposed) {
    using U = typename P::U;
    using W = typename P::W;
    constexpr int VE = 16 / sizeof(U);
    const int bl = blockIdx.z, z = blockIdx.y;
    const int x = blockIdx.x * blockDim.y + threadIdx.y;
    if (x >= g.BX) return;
    const int *row = plan + (size_t)bl * 5;
    const int op = row[4] & opmask;
    const bool tr = (op & 8) != 0;
    if (tr && skip_transposed) return;
    const unsigned v = (unsigned)row[0], oz = (unsigned)row[1], ox = (unsigned)row[2], oy = (unsigned)row[3];
    const unsigned gz = oz + (unsigned)((op & 1) ? g.BZ - 1 - z : z);
    const unsigned fixed = (tr ? oy : ox) + (unsigned)((op & 2) ? g.BX - 1 - x : x);   // gy when transposed, else gx
    const bool ok = v < (unsigned)g.V && gz < (unsigned)g.Z && fixed < (unsigned)(tr ? g.Y : g.X);
    const unsigned L = ok ? (unsigned)(tr ? g.X : g.Y) : 0u;    // a row outside the volume is all fill
    const size_t plane = ok ? ((size_t)v * g.Z + gz) * g.X : 0;
    const size_t base = ok ? (tr ? plane * g.Y + fixed : (plane + fixed) * g.Y) : 0;
    const size_t stride = tr ? (size_t)g.Y : 1;
    const unsigned t0 = (tr ? ox : oy) + (unsigned)((op & 4) ? g.BY - 1 : 0);
    const bool back = (op & 4) != 0;
    const typename P::Ctx c = p.ctx(ok ? (int)v : 0);
    auto voxel = [&](int vox) -> W {
        const unsigned t = back ? t0 - (unsigned)vox : t0 + (unsigned)vox;
        return t < L ? p.load(base + (size_t)t * stride, c) : P::fill();
    };
    const int K = P::KT ? P::KT : Krt;
    const int n = g.BY * K, tx = threadIdx.x, TX = blockDim.x;
    U *dst = out + (((size_t)bl * g.BZ + z) * g.BX + x) * n;
    auto val = [&](int i) -> U {
        const int vox = i / K;
        return P::unit(voxel(vox), i - vox * K);
    };
    const int head = head_units(dst, n), nvec = (n - head) / VE;
    for (int i = tx; i < head; i += TX) dst[i] = val(i);
    for (int j = tx; j < nvec; j += TX) {
        const int i = head + VE * j;
        int vox = i / K, sub = i - vox * K;
        W w = voxel(vox);
        U o[VE];
#pragma unroll
        for (int u = 0; u < VE; ++u) {
            o[u] = P::unit(w, sub);
            if (++sub == K) {
                sub = 0;
                ++vox;
                if (u + 1 < VE) w = voxel(vox);                 // vox < BY here: unit i + u + 1 is inside the row
            }
        }
        uint4 t;
        __builtin_memcpy(&t, o, 16);
        *reinterpret_cast<uint4 *>(dst + i) = t;
    }
    for (int i = head + VE * nvec + tx; i < n; i += TX) dst[i] = val(i);
}

// transposed bricks only (BX == BY = B): grid (tiles of the plane, BZ, count), block (64, 4)
template <typename P>
__global__ __launch_bounds__(256) void sample_tiles_kernel(P p, const int *__restrict__ plan, typename P::U *__restrict__ out,
                                                           SampGeom g, int Krt) {
    using U = typename P::U;
    using W = typename P::W;
    __shared__ W tile[TILE][TILE + 1];
    const int bl = blockIdx.z, z = blockIdx.y;
    const int *row = plan + (size_t)bl * 5;
    const int op = row[4];
    if (!(op & 8)) return;
    const int B = g.BX, nt = (B + TILE - 1) / TILE;
    const int x0 = (int)(blockIdx.x % nt) * TILE, y0 = (int)(blockIdx.x / nt) * TILE;   // the OUTPUT tile's corner
    const unsigned v = (unsigned)row[0], oz = (unsigned)row[1], ox = (unsigned)row[2], oy = (unsigned)row[3];
    const unsigned gz = oz + (unsigned)((op & 1) ? g.BZ - 1 - z : z);
    const bool ok = v < (unsigned)g.V && gz < (unsigned)g.Z;
    const size_t plane = ok ? ((size_t)v * g.Z + gz) * g.X * g.Y : 0;
    const typename P::Ctx c = p.ctx(ok ? (int)v : 0);
    const int tx = threadIdx.x, ty = threadIdx.y;
    // tile[j][i] = box voxel (fy(y0 + j), fx(x0 + i)): lanes along i, the source's contiguous axis
    {
        const int xo = x0 + tx;
        const unsigned gy = oy + (unsigned)((op & 2) ? B - 1 - xo : xo);
        const bool col_ok = ok && xo < B && gy < (unsigned)g.Y;
#pragma unroll 4
        for (int j = ty; j < TILE; j += 4) {
            const int yo = y0 + j;
            const unsigned gx = ox + (unsigned)((op & 4) ? B - 1 - yo : yo);
            W w = P::fill();
            if (col_ok && yo < B && gx < (unsigned)g.X) w = p.load(plane + (size_t)gx * g.Y + gy, c);
            tile[j][tx] = w;
        }
    }
    __syncthreads();
    const int K = P::KT ? P::KT : Krt;
    const int ni = min(TILE, B - x0), n = min(TILE, B - y0) * K;
    for (int i = ty; i < ni; i += 4) {
        U *dst = out + ((((size_t)bl * g.BZ + z) * B + (x0 + i)) * B + y0) * K;
        for (int k = tx; k < n; k += TILE) {
            const int vox = k / K;
            dst[k] = P::unit(tile[vox][i], k - vox * K);
        }
    }
}

// block (TX lanes along a row, 256 / TX rows): TX = the power of two that covers a row's 16-byte pieces, 4 .. 64
inline dim3 row_block(int64_t row_bytes) {
    const int64_t pieces = (row_bytes + 15) / 16 + 1;
    unsigned tx = 4;
    while (tx < 64 && tx < pieces) tx *= 2;
    return dim3(tx, 256 / tx);
}

// SQ_SAMPLE_LDS=0: A/B switch back to the direct gather for the transposed ops; read per launch
inline bool sample_lds() {
    const char *e = getenv("SQ_SAMPLE_LDS");
    return !(e && e[0] == '0');
}

inline int sample_ok(const char *what, int V, int Z, int X, int Y, int BZ, int BX, int BY, int count, int allow_transpose) {
    SQ_REQUIRE(V > 0 && Z > 0 && X > 0 && Y > 0 && BZ > 0 && BX > 0 && BY > 0, "%s: sizes must be positive", what);
    SQ_REQUIRE(BZ <= 65535 && BX < (1 << 24) && BY < (1 << 24), "%s: box %d x %d x %d out of range", what, BZ, BX, BY);
    SQ_REQUIRE(count > 0 && count <= 65535, "%s: count %d not in 1 .. 65535", what, count);
    SQ_REQUIRE(!allow_transpose || BX == BY, "%s: the transposed ops need a square box in the plane, got BX=%d BY=%d "
               "(allow_transpose = 0 ignores bit 3)", what, BX, BY);
    return SQ_OK;
}

template <typename P>
int sample_launch(const char *what, const P &p, const int32_t *plan, typename P::U *out, const SampGeom &g, int K, int count,
                  int allow_transpose, hipStream_t st) {
    const bool lds = allow_transpose && sample_lds();
    const dim3 block = row_block((int64_t)g.BY * K * sizeof(typename P::U));
    const dim3 grid((g.BX + block.y - 1) / block.y, g.BZ, count);
    hipLaunchKernelGGL(sample_rows_kernel<P>, grid, block, 0, st, p, plan, out, g, K, allow_transpose ? 15 : 7, (int)lds);
    if (lds) {
        const int nt = (g.BX + TILE - 1) / TILE;
        hipLaunchKernelGGL(sample_tiles_kernel<P>, dim3(nt * nt, g.BZ, count), dim3(TILE, 4), 0, st, p, plan, out, g, K);
    }
    return sq_check_launch(what);
}

template <typename E, int K_>
int copy_launch(const void *src, const int32_t *plan, void *out, const SampGeom &g, int count, int allow_transpose,
                hipStream_t st) {
    SQ_REQUIRE(((uintptr_t)src | (uintptr_t)out) % sizeof(E) == 0, "sq_volume_sample_copy: src and out must be aligned to %d bytes",
               (int)sizeof(E));
    const CopyPolicy<E, K_> p = {reinterpret_cast<const E *>(src)};
    return sample_launch("sq_volume_sample_copy", p, plan, reinterpret_cast<E *>(out), g, K_, count, allow_transpose, st);
}

}  // namespace

extern "C" int sq_volume_sample_f32(const void *vols, int dtype, const float *mean, const float *stdv, const int32_t *plan,
                                    float *out, int V, int Z, int X, int Y, int BZ, int BX, int BY, int count,
                                    int allow_transpose, void *stream) {
    SQ_REQUIRE(vols && plan && out, "sq_volume_sample_f32: null pointer");
    SQ_REQUIRE((mean == nullptr) == (stdv == nullptr), "sq_volume_sample_f32: give both mean and std, or neither");
    if (int rc = sample_ok("sq_volume_sample_f32", V, Z, X, Y, BZ, BX, BY, count, allow_transpose)) return rc;
    SQ_REQUIRE(dtype == SQ_PIX_U8 || dtype == SQ_PIX_U16 || dtype == SQ_PIX_F32, "sq_volume_sample_f32: unknown voxel type %d",
               dtype);
    SQ_REQUIRE((uintptr_t)out % 4 == 0 && (uintptr_t)vols % (dtype == SQ_PIX_U8 ? 1 : dtype == SQ_PIX_U16 ? 2 : 4) == 0,
               "sq_volume_sample_f32: vols and out must be aligned to their elements");
    const SampGeom g = {V, Z, X, Y, BZ, BX, BY};
    hipStream_t st = (hipStream_t)stream;
    const char *what = "sq_volume_sample_f32";
    switch (dtype) {
    case SQ_PIX_U8: {
        const ImagePolicy<uint8_t> p = {reinterpret_cast<const uint8_t *>(vols), mean, stdv};
        return sample_launch(what, p, plan, out, g, 1, count, allow_transpose, st);
    }
    case SQ_PIX_U16: {
        const ImagePolicy<uint16_t> p = {reinterpret_cast<const uint16_t *>(vols), mean, stdv};
        return sample_launch(what, p, plan, out, g, 1, count, allow_transpose, st);
    }
    default: {
        const ImagePolicy<float> p = {reinterpret_cast<const float *>(vols), mean, stdv};
        return sample_launch(what, p, plan, out, g, 1, count, allow_transpose, st);
    }
    }
}

extern "C" int sq_volume_sample_copy(const void *src, int elem_bytes, const int32_t *plan, void *out, int V, int Z, int X,
                                     int Y, int BZ, int BX, int BY, int count, int allow_transpose, void *stream) {
    SQ_REQUIRE(src && plan && out, "sq_volume_sample_copy: null pointer");
    SQ_REQUIRE(elem_bytes == 1 || elem_bytes == 2 || elem_bytes == 3 || elem_bytes == 4 || elem_bytes == 8,
               "sq_volume_sample_copy: elem_bytes %d not one of 1, 2, 3, 4, 8", elem_bytes);
    if (int rc = sample_ok("sq_volume_sample_copy", V, Z, X, Y, BZ, BX, BY, count, allow_transpose)) return rc;
    const SampGeom g = {V, Z, X, Y, BZ, BX, BY};
    hipStream_t st = (hipStream_t)stream;
    switch (elem_bytes) {
    case 1: return copy_launch<uint8_t, 1>(src, plan, out, g, count, allow_transpose, st);
    case 2: return copy_launch<uint16_t, 1>(src, plan, out, g, count, allow_transpose, st);
    case 3: return copy_launch<uint8_t, 3>(src, plan, out, g, count, allow_transpose, st);
    case 4: return copy_launch<uint32_t, 1>(src, plan, out, g, count, allow_transpose, st);
    default: return copy_launch<uint64_t, 1>(src, plan, out, g, count, allow_transpose, st);
    }
}

extern "C" int sq_volume_sample_onehot_u8(const uint8_t *labels, int C, const int32_t *plan, uint8_t *out, int V, int Z, int X,
                                          int Y, int BZ, int BX, int BY, int count, int allow_transpose, void *stream) {
    SQ_REQUIRE(labels && plan && out, "sq_volume_sample_onehot_u8: null pointer");
    SQ_REQUIRE(C >= 1 && C <= 16, "sq_volume_sample_onehot_u8: %d classes not in 1 .. 16", C);
    if (int rc = sample_ok("sq_volume_sample_onehot_u8", V, Z, X, Y, BZ, BX, BY, count, allow_transpose)) return rc;
    const SampGeom g = {V, Z, X, Y, BZ, BX, BY};
    const OnehotPolicy p = {labels};
    return sample_launch("sq_volume_sample_onehot_u8", p, plan, out, g, C, count, allow_transpose, (hipStream_t)stream);
}
