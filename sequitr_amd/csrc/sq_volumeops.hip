// Volume clean-up between "mask" and "objects" (include/sequitr_hip.h, "Volume clean-up"): the 3-D counterpart of
// sq_maskops.hip for (N, D, H, W) uint8 masks.  Cavity filling and border-object removal are sq_component_ops.hip.
//   morph        : one block per 8 x 32 x 128 brick.  Per class the bit plane of the brick and its halo is built straight
//                  from global memory -- a wave loads four rows as dwords into its own small LDS buffer and packs each
//                  64-voxel row segment with one __ballot -- every elementary step is shifts, carries and AND / OR with the
//                  rows and planes around it between two LDS copies of the plane, and each class's plane is merged into the
//                  brick in `out` against the brick's own bytes of the mask.
#include "sq_cleanup.h"

namespace {

constexpr int VT_D = SQ_MORPH3D_TILE_D, VT_H = SQ_MORPH3D_TILE_H, VT_W = SQ_MORPH3D_TILE_W;
constexpr int VT_HALO = 2 * SQ_MORPH3D_MAX_ITER;               // open / close at the largest r: planes and rows
constexpr int VT_XHALO = 32;                                   // columns: the staged row starts at a word-friendly offset
constexpr int VS_D = VT_D + 2 * VT_HALO, VS_H = VT_H + 2 * VT_HALO, VS_W = VT_W + 2 * VT_XHALO;   // the staged region
constexpr int VS_WORDS = VS_W / 64;                            // 64-bit words per staged row
constexpr int VS_DWORDS = VS_W / 4;                            // dwords of bytes per staged row
constexpr int VT_QUADS = VT_D * VT_H * VT_W / 4 / 256;         // 4-voxel groups of the brick per thread
constexpr int VB_ROWS = 4;                                     // rows a wave loads before it packs them
static_assert(VS_W % 64 == 0 && VT_XHALO % 4 == 0 && VT_XHALO >= VT_HALO && VT_W % 4 == 0, "staged rows are whole words");
static_assert(VS_WORDS == 3 && VS_DWORDS <= 64, "one lane per dword of a staged row");
static_assert(VT_D * VT_H * VT_W / 4 % 256 == 0 && (VT_HALO + 3) / 4 * 4 <= VT_XHALO, "the brick divides among 256 threads");
static_assert(2 * VS_D * VS_H * VS_WORDS * 8 + 2 * 4 * VB_ROWS * VS_DWORDS * 4 <= 64 * 1024, "static LDS stays under 64 KiB");

// the word (plane p, row r, word k) of bit plane P; outside the planes [P0, P1), the rows [R0, R1) or the staged row: 0
struct Region {
    int P0, P1, R0, R1;
};

__device__ __forceinline__ u64 vrd(const u64 *P, const Region &g, int p, int r, int k) {
    return (p >= g.P0 && p < g.P1 && r >= g.R0 && r < g.R1 && k >= 0 && k < VS_WORDS) ? P[(p * VS_H + r) * VS_WORDS + k] : 0ULL;
}

// the voxel with its left and right neighbours in its row
template <bool DILATE>
__device__ __forceinline__ u64 vhoriz(const u64 *P, const Region &g, int p, int r, int w) {
    const u64 c = vrd(P, g, p, r, w);
    const u64 l = (c << 1) | (vrd(P, g, p, r, w - 1) >> 63), h = (c >> 1) | (vrd(P, g, p, r, w + 1) << 63);
    return DILATE ? (c | l | h) : (c & l & h);
}

// one elementary step of the word (p, r, w): CUBE takes the horizontal triple of all nine rows (p +- 1, r +- 1), the cross
// the triple of its own row and the same word of the rows above and below and of the planes before and after
template <bool DILATE, bool CUBE>
__device__ __forceinline__ u64 vmorph_word(const u64 *P, const Region &g, int p, int r, int w) {
    if (CUBE) {
        u64 acc = DILATE ? 0ULL : ~0ULL;
#pragma unroll
        for (int dp = -1; dp <= 1; ++dp)
#pragma unroll
            for (int dr = -1; dr <= 1; ++dr) {
                const u64 v = vhoriz<DILATE>(P, g, p + dp, r + dr, w);
                acc = DILATE ? (acc | v) : (acc & v);
            }
        return acc;
    }
    const u64 m = vhoriz<DILATE>(P, g, p, r, w);
    const u64 a = vrd(P, g, p, r - 1, w), b = vrd(P, g, p, r + 1, w), c = vrd(P, g, p - 1, r, w), d = vrd(P, g, p + 1, r, w);
    return DILATE ? (m | a | b | c | d) : (m & a & b & c & d);
}

// VEC: W % 4 == 0 and both bases 4-byte aligned, so a 4-voxel group is one dword that lies wholly inside or outside a row
template <bool VEC>
__global__ __launch_bounds__(256, 2) void volume_morph_kernel(const uint8_t *__restrict__ mask, uint8_t *__restrict__ out, int D,
                                                           int H, int W, int C, int op, int cube, int iters, int tiles_x,
                                                           int tiles_y, int tiles_z) {
    __shared__ u64 pl[2][VS_D * VS_H * VS_WORDS];               // the bit plane of one class, before and after a step
    __shared__ uint32_t wb[2][4][VB_ROWS][VS_DWORDS];           // per wave: the bytes of the rows it packs, two generations
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int bid = blockIdx.x;
    const int tx = bid % tiles_x;
    bid /= tiles_x;
    const int ty = bid % tiles_y;
    bid /= tiles_y;
    const int tz = bid % tiles_z, n = bid / tiles_z;
    const bool two = op == SQ_MORPH_OPEN || op == SQ_MORPH_CLOSE;
    const bool extensive = op == SQ_MORPH_DILATE || op == SQ_MORPH_CLOSE;
    const int steps = two ? 2 * iters : iters, halo = steps;   // <= VT_HALO
    const int x0 = tx * VT_W - VT_XHALO, y0 = ty * VT_H - VT_HALO, z0 = tz * VT_D - VT_HALO;   // volume coordinates of staged (0, 0, 0)
    // staged planes and rows that matter: inside the halo AND inside the volume (outside it everything is zero for ever)
    Region g;
    g.P0 = max(VT_HALO - halo, -z0);
    g.P1 = min(VT_HALO + VT_D + halo, D - z0);
    g.R0 = max(VT_HALO - halo, -y0);
    g.R1 = min(VT_HALO + VT_H + halo, H - y0);
    const int nplanes = g.P1 - g.P0, nrows = g.R1 - g.R0, lines = nplanes * nrows;
    const int h4 = (halo + 3) & ~3;
    const int D0 = (VT_XHALO - h4) / 4, D1 = (VT_XHALO + VT_W + h4) / 4;   // staged dword columns that matter
    const int64_t HW = (int64_t)H * W;
    const uint8_t *vol = mask + (int64_t)n * D * HW;

    // columns of the volume in each word column: a dilation must not leave the volume
    u64 valid[VS_WORDS];
#pragma unroll
    for (int w = 0; w < VS_WORDS; ++w) {
        const int c0 = x0 + w * 64, lo = max(0, -c0), hi = min(64, W - c0);
        valid[w] = hi <= lo ? 0ULL : ((hi == 64 ? ~0ULL : ((1ULL << hi) - 1ULL)) & ~((1ULL << lo) - 1ULL));
    }
    const int col = x0 + 4 * lane;                              // this lane's dword of a staged row
    const bool dcol = lane >= D0 && lane < D1 && lane < VS_DWORDS;

    // Merge the finished plane P of class c into the brick, one 4-voxel group at a time: the thread's own voxels are read
    // again from the mask (and, from the second class on, from `out`, where this same thread wrote them), never kept in
    // registers.  fresh: nothing has been written yet -- extensive operations start from the mask, the others from its
    // bytes >= C alone.  P == nullptr writes that start value and nothing else.
    uint8_t *dst = out + (int64_t)n * D * HW;
    auto merge = [&](const u64 *P, int c, bool fresh) {
#pragma unroll 4
        for (int k = 0; k < VT_QUADS; ++k) {
            const int item = t + 256 * k;
            const int qx = 4 * (item % (VT_W / 4)), qy = (item / (VT_W / 4)) % VT_H, qz = item / (VT_W / 4 * VT_H);
            const int x = tx * VT_W + qx, y = ty * VT_H + qy, z = tz * VT_D + qz;
            if (z >= D || y >= H || x >= W) continue;
            const int64_t at = (int64_t)z * HW + (int64_t)y * W + x;
            uint32_t m = 0, r = 0;
            if (VEC) {
                m = *reinterpret_cast<const uint32_t *>(vol + at);
                if (!fresh) r = *reinterpret_cast<const uint32_t *>(dst + at);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (x + j < W) {
                        m |= (uint32_t)vol[at + j] << (8 * j);
                        if (!fresh) r |= (uint32_t)dst[at + j] << (8 * j);
                    }
            }
            if (fresh) {
                r = m;
                if (!extensive) {                               // classes start from nothing, bytes >= C stay
                    r = 0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const uint32_t b = (m >> (8 * j)) & 255u;
                        if ((int)b >= C) r |= b << (8 * j);
                    }
                }
            }
            if (P) {
                const int sc = VT_XHALO + qx;
                const uint32_t bits = (uint32_t)(P[((VT_HALO + qz) * VS_H + VT_HALO + qy) * VS_WORDS + sc / 64] >> (sc % 64)) & 15u;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (!((bits >> j) & 1u)) continue;
                    const uint32_t sh = 8 * j;
                    if (extensive) {
                        if (((r >> sh) & 255u) == 0u) r |= (uint32_t)c << sh;
                    } else if ((int)((m >> sh) & 255u) == c) {
                        r |= (uint32_t)c << sh;
                    }
                }
            }
            if (VEC) {
                *reinterpret_cast<uint32_t *>(dst + at) = r;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (x + j < W) dst[at + j] = (uint8_t)(r >> (8 * j));
            }
        }
    };

    bool fresh = true;
    for (int c = 1; c < C; ++c) {
        // the bit plane of class c: every pass the four waves take VB_ROWS lines each; all threads run every pass, so the
        // barrier between a wave's dword stores and its byte loads is one the whole block reaches
        int any = 0;
        int gen = 0;
        for (int first = 0; first < lines; first += 4 * VB_ROWS, gen ^= 1) {
            uint32_t v[VB_ROWS];
#pragma unroll
            for (int u = 0; u < VB_ROWS; ++u) {
                const int line = first + wave * VB_ROWS + u;
                v[u] = 0;
                if (line < lines && dcol) {
                    const int p = g.P0 + line / nrows, r = g.R0 + line % nrows;
                    const uint8_t *src = vol + (int64_t)(z0 + p) * HW + (int64_t)(y0 + r) * W;
                    if (VEC) {
                        if (col >= 0 && col < W) v[u] = *reinterpret_cast<const uint32_t *>(src + col);
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (col + j >= 0 && col + j < W) v[u] |= (uint32_t)src[col + j] << (8 * j);
                    }
                }
            }
            if (lane < VS_DWORDS) {
#pragma unroll
                for (int u = 0; u < VB_ROWS; ++u) wb[gen][wave][u][lane] = v[u];
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < VB_ROWS; ++u) {
                const int line = first + wave * VB_ROWS + u;      // depends on the wave only: every ballot sees 64 lanes
                if (line >= lines) continue;
                const int p = g.P0 + line / nrows, r = g.R0 + line % nrows;
                const uint8_t *bytes = reinterpret_cast<const uint8_t *>(wb[gen][wave][u]);
                u64 b[VS_WORDS];
#pragma unroll
                for (int w = 0; w < VS_WORDS; ++w) {
                    b[w] = __ballot((int)bytes[w * 64 + lane] == c);
                    any |= b[w] != 0ULL;
                }
                if (lane < VS_WORDS) pl[0][(p * VS_H + r) * VS_WORDS + lane] = lane == 0 ? b[0] : (lane == 1 ? b[1] : b[2]);
            }
        }
        if (__syncthreads_or(any)) {                           // a class absent from the staged region gives an empty plane
            for (int s = 0; s < steps; ++s) {
                const bool dil = op == SQ_MORPH_DILATE || (op == SQ_MORPH_OPEN && s >= iters) || (op == SQ_MORPH_CLOSE && s < iters);
                const u64 *P = pl[s & 1];
                u64 *Q = pl[(s + 1) & 1];
                for (int item = t; item < lines * VS_WORDS; item += 256) {
                    const int w = item % VS_WORDS, line = item / VS_WORDS;
                    const int p = g.P0 + line / nrows, r = g.R0 + line % nrows;
                    u64 q;
                    if (dil) {
                        q = cube ? vmorph_word<true, true>(P, g, p, r, w) : vmorph_word<true, false>(P, g, p, r, w);
                        q &= w == 0 ? valid[0] : (w == 1 ? valid[1] : valid[2]);
                    } else {
                        q = cube ? vmorph_word<false, true>(P, g, p, r, w) : vmorph_word<false, false>(P, g, p, r, w);
                    }
                    Q[(p * VS_H + r) * VS_WORDS + w] = q;
                }
                __syncthreads();
            }
            merge(pl[steps & 1], c, fresh);
            fresh = false;
            __syncthreads();                                    // the next class writes pl[0]
        }
    }

    if (fresh) merge(nullptr, 0, true);                         // no class in the region: the brick is copied through
}

}  // namespace

extern "C" int sq_volume_morph_u8(const uint8_t *mask, uint8_t *out, int N, int D, int H, int W, int C, int op, int structure,
                                  int iterations, void *stream) {
    const char *who = "sq_volume_morph_u8";
    SQ_CLEANUP_COMMON(who, D, "(%d,%d,%d,%d)", N, D, H, W);
    SQ_REQUIRE(op == SQ_MORPH_ERODE || op == SQ_MORPH_DILATE || op == SQ_MORPH_OPEN || op == SQ_MORPH_CLOSE,
               "%s: op must be SQ_MORPH_ERODE, DILATE, OPEN or CLOSE, got %d", who, op);
    SQ_REQUIRE(structure == SQ_MORPH3D_CROSS || structure == SQ_MORPH3D_CUBE,
               "%s: structure must be SQ_MORPH3D_CROSS or SQ_MORPH3D_CUBE, got %d", who, structure);
    SQ_REQUIRE(iterations >= 1 && iterations <= SQ_MORPH3D_MAX_ITER, "%s: iterations must be 1 .. %d, got %d", who,
               SQ_MORPH3D_MAX_ITER, iterations);
    const int tiles_x = (W + VT_W - 1) / VT_W, tiles_y = (H + VT_H - 1) / VT_H, tiles_z = (D + VT_D - 1) / VT_D;
    const int64_t blocks = (int64_t)N * tiles_x * tiles_y * tiles_z;   // at most one per voxel: < 2^31
    const bool vec = W % 4 == 0 && (((uintptr_t)mask | (uintptr_t)out) & 3u) == 0;
    if (vec)
        hipLaunchKernelGGL(volume_morph_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, mask, out, D, H,
                           W, C, op, structure == SQ_MORPH3D_CUBE, iterations, tiles_x, tiles_y, tiles_z);
    else
        hipLaunchKernelGGL(volume_morph_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, mask, out, D, H,
                           W, C, op, structure == SQ_MORPH3D_CUBE, iterations, tiles_x, tiles_y, tiles_z);
    return sq_check_launch(who);
}
