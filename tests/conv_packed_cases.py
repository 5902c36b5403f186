"""Shared by the packed-filter tests: the fragment-order pack of include/sequitr_hip.h ("Fragment-order filter pack") restated in
numpy from its definition, and the 64-channel-block plan a packed case must reach.

    wp[((((cb * Cin/16 + c) * 9 + tap) * 4 + s) * 64 + 16 kk + li) * 4 + nb] = w[tap][16 c + 4 s + kk][64 cb + 16 nb + li]
"""
import collections

import numpy as np

from tests import f32_walk_cases as wc


def pack_index(Cin, Cout):
    """flat index into w.reshape(-1) of every element of the pack, in pack order (int64, 9 Cin Cout entries)"""
    nchunk, cblocks = Cin // 16, Cout // 64
    cb, c, tap, s, kk, li, nb = np.meshgrid(np.arange(cblocks), np.arange(nchunk), np.arange(9), np.arange(4), np.arange(4),
                                            np.arange(16), np.arange(4), indexing="ij")
    # the pack's axes in storage order: cb, c, tap, s, lane = (kk, li), nb
    src = (tap * Cin + 16 * c + 4 * s + kk) * Cout + 64 * cb + 16 * nb + li
    return src.reshape(-1).astype(np.int64)


def pack_numpy(w):
    """the pack of a (3,3,Cin,Cout) float32 filter: a gather, so every bit pattern survives"""
    K, K2, Cin, Cout = w.shape
    assert (K, K2) == (3, 3) and Cin % 16 == 0 and Cout % 64 == 0
    return np.ascontiguousarray(w).reshape(-1)[pack_index(Cin, Cout)]


def on_64_blocks(form, N, H, W, Cin, Cout, act="relu"):
    """(taken, walk): does the tile-walk plan put the call on 64-channel blocks of the generic kernel -- ntiles x Cout / 64 >= 512 --
    the only plan a pack is read at (sq_conv_walk_plan; wc.PLAIN or wc.POOL)"""
    p = wc.walk(form, N, H, W, Cin, Cout, 3, act)
    return (p["kernel"] == wc.V2 and Cout % 64 == 0 and p["cblocks"] == Cout // 64 and p["items"] * p["cblocks"] >= 512), p


# ---- the walk sweep of the packed kernel (tests/test_gpu_conv_packed.py; the regimes are checked on the CPU by
# tests/test_conv_packed_cpu.py).  form: wc.PLAIN or wc.POOL; bias: "rand" or None; tags: the regimes the case is there for, as
# packed_tags() recomputes them from sq_conv_walk_plan and the shape.
WalkCase = collections.namedtuple("WalkCase", "form N H W Cin Cout act bias tags")

PACKED_NEEDED = {
    "chunks=1", "chunks=3",            # an odd chunk count: consecutive tiles start in alternating halo buffers; tmax >= 2, uneven
    "chunks>=4",                       # the A ring wraps across a tile boundary from the fourth chunk or later; tmax >= 2
    "cblocks=2", "cblocks=4",          # a channel block other than 0 (a pack offset) on a walk of two or more tiles
    "tmax>=4",
    "every_carry",                     # a block with a step without carry, one column -> row and one row -> image; tiles_x != tiles_y,
                                       # N >= 2, G no whole number of images
    "G%8!=0", "G%8==0",                # the residue sq_xcd_remap sees
    "rx=1", "rx=15", "ry=1", "ry=15", "ragged_x_only", "ragged_y_only",
    "mixed_epilogues",                 # ReLU, and a block whose walk holds a whole tile (fast epilogue) and a partial one (masked)
    "tiles_x=1",                       # with W < 16
    "tiles_y=1",
    "tiles_x=2",                       # a carry of the column at every step or every other one
    "pool_ragged",                     # H, W even, neither a multiple of 16, one of them = 2 (mod 4): a wave's rows straddle the edge
    "pool_tmax>=3",
    "pool_leaky",                      # the pooled epilogue without the fast path, on two or more tiles
    "relu_nobias", "none_bias",
}


def whole_tile(c, t):
    """does tile t lie inside the image (the kernel's fast-epilogue condition, but for ReLU)"""
    tiles_x, tiles_y = wc.tiles_xy(c)
    return (t % tiles_x) * 16 + 16 <= c.W and (t // tiles_x) % tiles_y * 16 + 16 <= c.H


def blocks_mixing_epilogues(c, p):
    """blocks whose walk holds both a whole tile and a partial one"""
    return [b for b in range(p["G"]) if len({whole_tile(c, t) for t in range(b, p["items"], p["G"])}) == 2]


def packed_walk(c):
    return wc.walk(c.form, c.N, c.H, c.W, c.Cin, c.Cout, 3, c.act)


def packed_tags(c):
    """the regimes of PACKED_NEEDED the case reaches, from the walk sq_conv_walk_plan reports and the shape"""
    p = packed_walk(c)
    tiles_x, tiles_y = wc.tiles_xy(c)
    chunks, rx, ry = c.Cin // 16, c.W % 16, c.H % 16
    multi, uneven = p["tmax"] >= 2, p["tmin"] < p["tmax"]
    t = {"G%8==0" if p["G"] % 8 == 0 else "G%8!=0"}
    if chunks in (1, 3) and multi and uneven:
        t.add("chunks=%d" % chunks)
    if chunks >= 4 and multi:
        t.add("chunks>=4")
    if p["cblocks"] in (2, 4) and multi:
        t.add("cblocks=%d" % p["cblocks"])
    if p["tmax"] >= 4:
        t.add("tmax>=4")
    if tiles_x != tiles_y and c.N >= 2 and p["G"] % (tiles_x * tiles_y) != 0 and wc.blocks_with_every_carry(p, tiles_x, tiles_y):
        t.add("every_carry")
    if rx in (1, 15):
        t.add("rx=%d" % rx)
    if ry in (1, 15):
        t.add("ry=%d" % ry)
    if rx and not ry:
        t.add("ragged_x_only")
    if ry and not rx:
        t.add("ragged_y_only")
    if c.act == "relu" and blocks_mixing_epilogues(c, p):
        t.add("mixed_epilogues")
    if tiles_x == 1 and c.W < 16:
        t.add("tiles_x=1")
    if tiles_y == 1:
        t.add("tiles_y=1")
    if tiles_x == 2:
        t.add("tiles_x=2")
    if c.form == wc.POOL:
        if c.H % 2 == 0 and c.W % 2 == 0 and rx and ry and 2 in (c.H % 4, c.W % 4):
            t.add("pool_ragged")
        if p["tmax"] >= 3:
            t.add("pool_tmax>=3")
        if c.act == "leaky" and multi:
            t.add("pool_leaky")
    if c.act == "relu" and c.bias is None:
        t.add("relu_nobias")
    if c.act is None and c.bias is not None:
        t.add("none_bias")
    return t


def packed_case_id(c):
    return "%s-%dx%dx%d-%d-%d-%s-bias_%s" % ("pool" if c.form == wc.POOL else "plain", c.N, c.H, c.W, c.Cin, c.Cout, c.act, c.bias)


# Every (tile, channel block) count is at least 512, below which the plan leaves the 64-channel blocks.  The walks are those
# sq_conv_walk_plan reports (G blocks of tmin .. tmax tiles, stride G = gn images + gy rows + gx columns of tiles):
#   2 x 145 x 193, 16 -> 256   13 x 10 tiles, G = 87 = 6 rows + 9 columns, 2 or 3 tiles; one-pixel last row and column
#   2 x 145 x 207, 48 -> 256   the same walk at three chunks per tile, a 15-pixel last column
#   2 x 193 x 319, 48 -> 128   20 x 13 tiles, G = 174 = 8 rows + 14 columns, 2 or 3 tiles
#   4 x 207 x 305, 16 -> 64    20 x 13 tiles, G = 347 = 1 image + 4 rows + 7 columns, 2 or 3 tiles; a 15-pixel last row
#   3 x 130 x 336, 32 -> 256   21 x 9 tiles, G = 114 = 5 rows + 9 columns, 4 or 5 tiles; ragged at the bottom only
#   3 x 224 x 193, 64 -> 64    13 x 14 tiles, G = 273 = 1 image + 7 rows, 2 tiles, four chunks; ragged on the right only
#   2 x 250 x 278, 32 -> 128   pooled, 18 x 16 tiles, G = 192 = 10 rows + 12 columns, 3 tiles; 250 = 278 = 2 (mod 4)
#   2 x 242 x 270, 48 -> 128   pooled, 17 x 16 tiles, G = 182 = 10 rows + 12 columns, 2 or 3 tiles, leaky: no fast epilogue
#   3 x 1045 x 31, 16 -> 256   2 x 66 tiles, G = 99 = 49 rows + 1 column, 4 tiles: the column carries at every other step and
#                              every block mixes whole tiles of the left column with partial ones of the right
#   1 x 2048 x 7, 1 x 15 x 2048, 1 x 16 x 2048, 16 -> 256: one column / one row of 128 tiles, one tile per block
PACKED_WALKS = [
    WalkCase(wc.PLAIN, 2, 145, 193, 16, 256, "relu", "rand",
             ("G%8!=0", "cblocks=4", "chunks=1", "every_carry", "mixed_epilogues", "rx=1", "ry=1")),
    WalkCase(wc.PLAIN, 2, 145, 207, 48, 256, "leaky", "rand", ("G%8!=0", "cblocks=4", "chunks=3", "every_carry", "rx=15", "ry=1")),
    WalkCase(wc.PLAIN, 2, 193, 319, 48, 128, "relu", None,
             ("G%8!=0", "cblocks=2", "chunks=3", "every_carry", "mixed_epilogues", "relu_nobias", "rx=15", "ry=1")),
    WalkCase(wc.PLAIN, 4, 207, 305, 16, 64, None, "rand", ("G%8!=0", "chunks=1", "every_carry", "none_bias", "rx=1", "ry=15")),
    WalkCase(wc.PLAIN, 3, 130, 336, 32, 256, "relu", "rand",
             ("G%8!=0", "cblocks=4", "every_carry", "mixed_epilogues", "ragged_y_only", "tmax>=4")),
    WalkCase(wc.PLAIN, 3, 224, 193, 64, 64, "relu", "rand", ("G%8!=0", "chunks>=4", "ragged_x_only", "rx=1")),
    WalkCase(wc.POOL, 2, 250, 278, 32, 128, "relu", "rand",
             ("G%8==0", "cblocks=2", "every_carry", "mixed_epilogues", "pool_ragged", "pool_tmax>=3")),
    WalkCase(wc.POOL, 2, 242, 270, 48, 128, "leaky", "rand",
             ("G%8!=0", "cblocks=2", "chunks=3", "every_carry", "pool_leaky", "pool_ragged", "pool_tmax>=3")),
    WalkCase(wc.PLAIN, 3, 1045, 31, 16, 256, "relu", "rand",
             ("G%8!=0", "cblocks=4", "every_carry", "mixed_epilogues", "rx=15", "tiles_x=2", "tmax>=4")),
    WalkCase(wc.PLAIN, 1, 2048, 7, 16, 256, "relu", "rand", ("G%8==0", "ragged_x_only", "tiles_x=1")),
    WalkCase(wc.PLAIN, 1, 15, 2048, 16, 256, "relu", "rand", ("G%8==0", "ragged_y_only", "ry=15", "tiles_y=1")),
    WalkCase(wc.PLAIN, 1, 16, 2048, 16, 256, "relu", None, ("G%8==0", "relu_nobias", "tiles_y=1")),
]
# the non-finite test's case: ReLU, a bias, three tiles per block, even sides so that it also runs pooled
NONFINITE_CASE = PACKED_WALKS[6]


# ---- shared with the tests of the 32 -> 32 kernel (tests/test_gpu_conv_r32.py) ----------------------------------------------
SENTINEL = -12345.678


class Guarded(object):
    """an (N, H, W, C) float32 device tensor inside sentinel bands of one image row (W * C floats) each, itself filled with the
    sentinel: a store outside the tensor lands in a band, an element never stored keeps the sentinel"""

    def __init__(self, N, H, W, C=32):
        import torch
        self.band = W * C
        self.buf = torch.full((N * H * W * C + 2 * self.band,), SENTINEL, dtype=torch.float32, device="cuda")
        self.t = self.buf[self.band:self.band + N * H * W * C].view(N, H, W, C)

    def bands_intact(self):
        import torch
        s = torch.tensor(SENTINEL, dtype=torch.float32, device="cuda")
        return bool((self.buf[:self.band] == s).all()) and bool((self.buf[-self.band:] == s).all())

    def all_stored(self):
        return not bool((self.t == SENTINEL).any())


def mismatch(got, ref, p, H, W, name="y", bn=64):
    """None where the float32 arrays `got` and `ref` (N, h, w, C) hold the same bits.  Otherwise the report: how many elements
    differ, the first of them as (n, y, x, channel) with the pixel tile they lie in, that tile's block (gridDim.x index after the
    remap, and the channel block of `bn` channels), its position in the block's walk and the walk's length -- from the walk `p`
    of sq_conv_walk_plan -- and how the differing elements spread over walk positions: a seam fault shows at positions >= 1 only
    (or at the last one only).  name "pooled": the arrays are the 2x2-pooled output, a pixel lies in the tile of those it pools."""
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.float32, (name, got.shape, ref.shape, got.dtype, ref.dtype)
    gb, rb = got.view(np.uint32), ref.view(np.uint32)
    if np.array_equal(gb, rb):
        return None
    bad = np.argwhere(gb != rb)
    sub = 2 if name == "pooled" else 1
    tiles_x, tiles_y = -(-W // 16), -(-H // 16)
    lines = ["%s: %d of %d elements differ in bits" % (name, len(bad), got.size)]
    spread = collections.Counter()
    for k, idx in enumerate(bad[:20000]):
        n, y, x, ch = (int(v) for v in idx)
        tyi, txi = y * sub // 16, x * sub // 16
        b, pos, cnt = wc.tile_position(p, tiles_x, tiles_y, n, tyi, txi)
        spread[(pos, cnt)] += 1
        if k < 5:
            lines.append("  %s (n %d, y %d, x %d, channel %d): %r (0x%08x) vs %r (0x%08x) -- tile (n %d, ty %d, tx %d), item %d of %d "
                         "of block %d (of %d blocks), channel block %d" % (name, n, y, x, ch, got[n, y, x, ch], gb[n, y, x, ch],
                                                                          ref[n, y, x, ch], rb[n, y, x, ch], n, tyi, txi, pos, cnt,
                                                                          b, p["G"], ch // bn))
    lines.append("  differing elements by (position in the walk, items of the walk): %s" % sorted(spread.items()))
    return "\n".join(lines)


def nonfinite_plants(N, H, W, Cin):
    """[(n, y, x, channel, value)]: NaN, +inf and -inf at the first and the last pixel of an inner tile, in halo pixels of the
    last (border) tile column and row -- the pixels left of and above them -- at the corners of the last image, in the first and
    the last channel"""
    nan, inf = float("nan"), float("inf")
    tiles_x, tiles_y = -(-W // 16), -(-H // 16)
    ty, tx = min(3, tiles_y - 1), min(4, tiles_x - 1)
    y0, x0 = 16 * ty, 16 * tx
    hx, hy = max(16 * (tiles_x - 1) - 1, 0), max(16 * (tiles_y - 1) - 1, 0)
    return [(0, y0, x0, 0, nan), (0, min(y0 + 15, H - 1), min(x0 + 15, W - 1), Cin - 1, inf),
            (0, min(y0 + 40, H - 1), hx, 0, -inf), (0, hy, min(x0 + 40, W - 1), Cin - 1, nan),
            (N - 1, 0, 0, 0, inf), (N - 1, H - 1, W - 1, Cin - 1, nan), (N - 1, H - 1, 0, Cin - 1, -inf),
            (N - 1, 0, W - 1, 0, nan), (N - 1, min(y0 + 8, H - 1), min(x0 + 8, W - 1), Cin // 2, inf),
            (N - 1, min(y0 + 8, H - 1), min(x0 + 9, W - 1), 0, -inf)]


def neighbourhoods(x):
    """(finite, has_nan), bool (N, H, W): is every value of the 3x3 x Cin neighbourhood of the pixel finite / is one of them a
    NaN -- a max-pool of the per-pixel maps, on the CPU"""
    import torch
    x = torch.as_tensor(x).cpu()

    def near(m):
        return torch.nn.functional.max_pool2d(m.float().unsqueeze(1), 3, stride=1, padding=1).squeeze(1) > 0

    return ~near(~torch.isfinite(x).all(dim=-1)), near(torch.isnan(x).any(dim=-1))
