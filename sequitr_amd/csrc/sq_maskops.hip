// Mask clean-up between "mask" and "objects" (include/sequitr_hip.h, "Mask clean-up"): binary morphology per class on
// bit planes in LDS.  Planar (N, H, W) uint8 masks.  Hole filling and border-object removal are sq_component_ops.hip.
//   morph        : one block per 64 x 192 tile.  The tile and its halo are staged as bytes in LDS once; per class one
//                  __ballot per 64-pixel row segment packs a row into 64-bit words, every 3x3 step is shifts, carries and
//                  AND / OR between two LDS copies of the plane, the classes are merged in registers, the tile is stored.
#include "sq_cleanup.h"

namespace {

constexpr int MT_ROWS = SQ_MORPH_TILE_ROWS, MT_COLS = SQ_MORPH_TILE_COLS;
constexpr int MT_HALO = 2 * SQ_MORPH_MAX_ITER;                 // open / close at the largest r
constexpr int MS_ROWS = MT_ROWS + 2 * MT_HALO, MS_COLS = MT_COLS + 2 * MT_HALO;   // the staged region
constexpr int MS_WORDS = MS_COLS / 64;                         // 64-bit words per staged row
constexpr int MT_QUADS = MT_ROWS * MT_COLS / 4 / 256;          // 4-pixel groups of the tile per thread
static_assert(MS_COLS % 64 == 0 && MT_HALO % 4 == 0 && MT_COLS % 4 == 0, "staged rows are whole words and dwords");
static_assert(MS_WORDS == 4, "a thread keeps one word column: 256 threads = 64 rows x 4 words per pass");
static_assert(MT_ROWS * MT_COLS / 4 % 256 == 0, "the tile's 4-pixel groups divide among 256 threads");

// one 3x3 step of the word (row, w) of plane P; rows outside [R0, R1) and words outside the staged row read as 0
template <bool DILATE, bool SQUARE>
__device__ __forceinline__ u64 morph_word(const u64 *P, int row, int w, int R0, int R1) {
    auto rd = [&](int r, int k) -> u64 { return (r >= R0 && r < R1 && k >= 0 && k < MS_WORDS) ? P[r * MS_WORDS + k] : 0ULL; };
    auto horiz = [&](int r) -> u64 {                            // the pixel with its left and right neighbours
        const u64 c = rd(r, w);
        const u64 l = (c << 1) | (rd(r, w - 1) >> 63), g = (c >> 1) | (rd(r, w + 1) << 63);
        return DILATE ? (c | l | g) : (c & l & g);
    };
    if (SQUARE) {
        const u64 a = horiz(row - 1), b = horiz(row), c = horiz(row + 1);
        return DILATE ? (a | b | c) : (a & b & c);
    }
    const u64 m = horiz(row), u = rd(row - 1, w), d = rd(row + 1, w);
    return DILATE ? (m | u | d) : (m & u & d);
}

// VEC: W % 4 == 0 and both bases 4-byte aligned, so a 4-pixel group is one dword that lies wholly inside or outside a row
template <bool VEC>
__global__ __launch_bounds__(256) void morph_kernel(const uint8_t *__restrict__ mask, uint8_t *__restrict__ out, int H, int W,
                                                    int C, int op, int square, int iters, int tiles_x, int tiles_y) {
    __shared__ uint32_t sb[MS_ROWS * MS_COLS / 4];              // the staged bytes, 4 pixels per dword
    __shared__ u64 pl[2][MS_ROWS * MS_WORDS];                  // the bit plane of one class, before and after a step
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int bid = blockIdx.x;
    const int tx = bid % tiles_x, ty = (bid / tiles_x) % tiles_y, n = bid / (tiles_x * tiles_y);
    const bool two = op == SQ_MORPH_OPEN || op == SQ_MORPH_CLOSE;
    const bool extensive = op == SQ_MORPH_DILATE || op == SQ_MORPH_CLOSE;
    const int steps = two ? 2 * iters : iters, halo = steps;   // <= MT_HALO
    const int x0 = tx * MT_COLS - MT_HALO, y0 = ty * MT_ROWS - MT_HALO;   // frame coordinates of staged (0, 0)
    // staged rows that matter: inside the halo AND inside the frame (rows outside the frame are zero for ever)
    const int R0 = max(MT_HALO - halo, -y0), R1 = min(MT_HALO + MT_ROWS + halo, H - y0);
    const int h4 = (halo + 3) & ~3;
    const int D0 = (MT_HALO - h4) / 4, D1 = (MT_HALO + MT_COLS + h4) / 4;   // staged dword columns that matter
    const uint8_t *frame = mask + (size_t)n * H * W;
    const int nrows = R1 - R0;

    // eight rows' loads in flight per thread before the first LDS store waits for one (one at a time, a block spent its
    // time in 17 .. 33 serial round trips to memory); a thread's dword column d is the same in every pass
    constexpr int LOADS = 8;
    const int d = t % (MS_COLS / 4), col = x0 + 4 * d;
    const bool dcol = d >= D0 && d < D1;
    for (int row0 = R0 + t / (MS_COLS / 4); row0 < R1; row0 += LOADS * (256 / (MS_COLS / 4))) {
        uint32_t v[LOADS];
#pragma unroll
        for (int u = 0; u < LOADS; ++u) {
            const int row = row0 + u * (256 / (MS_COLS / 4));
            v[u] = 0;
            if (row < R1 && dcol) {
                const uint8_t *src = frame + (size_t)(y0 + row) * W;
                if (VEC) {
                    if (col >= 0 && col < W) v[u] = *reinterpret_cast<const uint32_t *>(src + col);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (col + j >= 0 && col + j < W) v[u] |= (uint32_t)src[col + j] << (8 * j);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < LOADS; ++u) {
            const int row = row0 + u * (256 / (MS_COLS / 4));
            if (row < R1) sb[row * (MS_COLS / 4) + d] = v[u];
        }
    }

    // the thread's 4-pixel groups of the tile: staged dword index, or -1 below the frame
    uint32_t res[MT_QUADS], m4[MT_QUADS];
#pragma unroll
    for (int k = 0; k < MT_QUADS; ++k) { res[k] = 0; m4[k] = 0; }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < MT_QUADS; ++k) {
        const int item = t + 256 * k, row = MT_HALO + item / (MT_COLS / 4), d = MT_HALO / 4 + item % (MT_COLS / 4);
        if (row < R1) {
            const uint32_t m = sb[row * (MS_COLS / 4) + d];
            m4[k] = m;
            uint32_t r = m;
            if (!extensive) {                                   // classes start from nothing, bytes >= C stay
                r = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t b = (m >> (8 * j)) & 255u;
                    if ((int)b >= C) r |= b << (8 * j);
                }
            }
            res[k] = r;
        }
    }

    // columns of the frame in this thread's word column (it is t & 3 in every pass): a dilation must not leave the frame
    const int myw = t & (MS_WORDS - 1);
    u64 valid;
    {
        const int c0 = x0 + myw * 64, lo = max(0, -c0), hi = min(64, W - c0);
        valid = hi <= lo ? 0ULL : ((hi == 64 ? ~0ULL : ((1ULL << hi) - 1ULL)) & ~((1ULL << lo) - 1ULL));
    }
    const uint8_t *sbytes = reinterpret_cast<const uint8_t *>(sb);

    for (int c = 1; c < C; ++c) {
        int any = 0;
        for (int p = wave; p < nrows * MS_WORDS; p += 4) {      // p depends on the wave only: every ballot sees 64 lanes
            const int row = R0 + p / MS_WORDS, w = p % MS_WORDS;
            const u64 b = __ballot((int)sbytes[row * MS_COLS + w * 64 + lane] == c);
            if (lane == 0) pl[0][row * MS_WORDS + w] = b;
            any |= b != 0ULL;
        }
        if (__syncthreads_or(any)) {                           // a class absent from the staged region gives an empty plane
            for (int s = 0; s < steps; ++s) {
                const bool dil = op == SQ_MORPH_DILATE || (op == SQ_MORPH_OPEN && s >= iters) || (op == SQ_MORPH_CLOSE && s < iters);
                const u64 *P = pl[s & 1];
                u64 *Q = pl[(s + 1) & 1];
                for (int item = t; item < nrows * MS_WORDS; item += 256) {
                    const int row = R0 + item / MS_WORDS;
                    u64 q;
                    if (dil) q = (square ? morph_word<true, true>(P, row, myw, R0, R1) : morph_word<true, false>(P, row, myw, R0, R1)) & valid;
                    else q = square ? morph_word<false, true>(P, row, myw, R0, R1) : morph_word<false, false>(P, row, myw, R0, R1);
                    Q[row * MS_WORDS + myw] = q;
                }
                __syncthreads();
            }
            const u64 *P = pl[steps & 1];
#pragma unroll
            for (int k = 0; k < MT_QUADS; ++k) {
                const int item = t + 256 * k, row = MT_HALO + item / (MT_COLS / 4), col = MT_HALO + 4 * (item % (MT_COLS / 4));
                if (row < R1) {
                    const uint32_t bits = (uint32_t)(P[row * MS_WORDS + col / 64] >> (col % 64)) & 15u;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (!((bits >> j) & 1u)) continue;
                        const uint32_t sh = 8 * j;
                        if (extensive) {
                            if (((res[k] >> sh) & 255u) == 0u) res[k] |= (uint32_t)c << sh;
                        } else if ((int)((m4[k] >> sh) & 255u) == c) {
                            res[k] |= (uint32_t)c << sh;
                        }
                    }
                }
            }
            __syncthreads();                                    // the next class writes pl[0]
        }
    }

    uint8_t *dst = out + (size_t)n * H * W;
#pragma unroll
    for (int k = 0; k < MT_QUADS; ++k) {
        const int item = t + 256 * k;
        const int y = ty * MT_ROWS + item / (MT_COLS / 4), x = tx * MT_COLS + 4 * (item % (MT_COLS / 4));
        if (y >= H) continue;
        if (VEC) {
            if (x < W) *reinterpret_cast<uint32_t *>(dst + (size_t)y * W + x) = res[k];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x + j < W) dst[(size_t)y * W + x + j] = (uint8_t)(res[k] >> (8 * j));
        }
    }
}

}  // namespace

extern "C" int sq_mask_morph_u8(const uint8_t *mask, uint8_t *out, int N, int H, int W, int C, int op, int structure,
                                int iterations, void *stream) {
    const char *who = "sq_mask_morph_u8";
    SQ_CLEANUP_COMMON(who, 1, "(%d,%d,%d)", N, H, W);
    SQ_REQUIRE(op == SQ_MORPH_ERODE || op == SQ_MORPH_DILATE || op == SQ_MORPH_OPEN || op == SQ_MORPH_CLOSE,
               "%s: op must be SQ_MORPH_ERODE, DILATE, OPEN or CLOSE, got %d", who, op);
    SQ_REQUIRE(structure == SQ_MORPH_CROSS || structure == SQ_MORPH_SQUARE,
               "%s: structure must be SQ_MORPH_CROSS or SQ_MORPH_SQUARE, got %d", who, structure);
    SQ_REQUIRE(iterations >= 1 && iterations <= SQ_MORPH_MAX_ITER, "%s: iterations must be 1 .. %d, got %d", who,
               SQ_MORPH_MAX_ITER, iterations);
    const int tiles_x = (W + MT_COLS - 1) / MT_COLS, tiles_y = (H + MT_ROWS - 1) / MT_ROWS;
    const int64_t blocks = (int64_t)N * tiles_x * tiles_y;      // < 2^31 / 1 as the mask has fewer than 2^31 pixels
    const bool vec = W % 4 == 0 && (((uintptr_t)mask | (uintptr_t)out) & 3u) == 0;
    if (vec)
        hipLaunchKernelGGL(morph_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, mask, out, H, W, C, op,
                           structure == SQ_MORPH_SQUARE, iterations, tiles_x, tiles_y);
    else
        hipLaunchKernelGGL(morph_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, mask, out, H, W, C, op,
                           structure == SQ_MORPH_SQUARE, iterations, tiles_x, tiles_y);
    return sq_check_launch(who);
}
