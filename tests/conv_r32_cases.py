"""Case tables of the 32 -> 32 filter-in-registers conv (conv_r32_kernel, sq_conv_f32_r32.hip), shared by the CPU plan tests
(tests/test_conv_r32_plan.py) and the GPU bit-identity tests (tests/test_gpu_conv_r32.py).

The kernel takes a call only on the plan that ran conv_mfma_f32_v2_kernel<32,3,32,0> before it (32-channel blocks, 32 staged
channels: at least 512 pixel tiles) and walks that kernel's grid, so sq_conv_walk_plan / sq_conv_plan report the same values with
the switch SQ_CONV_R32 on and off."""
import collections
import ctypes

from sequitr_amd import _lib
from tests import conv_sweep_cases as cs
from tests import f32_walk_cases as wc

# pooled: through conv3x3_pool (y and pooled).  bias: "rand" or None.  weights: "normal", or "denormal" (a filter at the denormal
# scale with negative zeros in it).
Case = collections.namedtuple("Case", "N H W pooled bias weights")

# (2, 256, 256): 512 tiles, the smallest on-plan call -- every block exactly one tile (no seam), 60 of every 256 tiles on a border.
# (5, 256, 272): 1360 tiles on 454 blocks -- blocks walk 2 or 3 tiles, the tile grid is non-square (17 x 16), and the stride
# (454 = 1 image + 10 rows + 12 columns) carries from the column into the row into the image.
SHAPES = [(2, 256, 256), (5, 256, 272)]
CASES = [Case(N, H, W, pooled, bias, "normal") for (N, H, W) in SHAPES for pooled in (False, True) for bias in ("rand", None)]
CASES.append(Case(5, 256, 272, True, "rand", "denormal"))

# calls the kernel declines, one departure each from (2, 256, 256, relu, wscale 1): (H, act, wscale)
FALLBACKS = [(256, None, 1.0), (256, "relu", 0.5), (250, "relu", 1.0)]


def case_id(c):
    return "%dx%dx%d-%s-bias_%s-%s" % (c.N, c.H, c.W, "pool" if c.pooled else "plain", c.bias, c.weights)


def takes(N, H, W, Cin=32, Cout=32, K=3, act="relu", pooled=False):
    """sq_conv_r32_takes_f32 (host only)"""
    return _lib.load().sq_conv_r32_takes_f32(N, H, W, Cin, Cout, K, cs.ACT[act], 1 if pooled else 0)


WALK_FIELDS = ("kernel", "G", "tmin", "tmax", "gx", "gy", "gn", "mtiles", "cblocks", "items", "tilepx")


def walk(N, H, W, pooled, act="relu"):
    """dict of WALK_FIELDS: sq_conv_walk_plan of the 32 -> 32 call (form PLAIN = 0 / POOL = 2)"""
    lib = _lib.load()
    out = (ctypes.c_int * len(WALK_FIELDS))()
    rc = lib.sq_conv_walk_plan(cs.POOL if pooled else cs.PLAIN, N, H, W, 32, 32, 3, cs.ACT[act], 0, 0,
                               ctypes.cast(out, ctypes.c_void_p))
    if rc != 0:
        raise _lib.SequitrHipError("sq_conv_walk_plan: %s" % lib.sq_last_error().decode())
    return dict(zip(WALK_FIELDS, out))


def plan(N, H, W, pooled, act="relu"):
    """sq_conv_plan of the 32 -> 32 call"""
    return cs.plan(cs.F32, cs.POOL if pooled else cs.PLAIN, N, H, W, 32, 32, 3, act)


# ---- the walk sweep (tests/test_gpu_conv_r32.py against the C oracle; the regimes are checked on the CPU by
# tests/test_conv_r32_plan.py).  The stores of a tile ride in the MFMA phase of the block's next tile and only the last tile has an
# epilogue of its own, so the walk lengths 1, 2, 3 and 4 or more are different code paths, as is a one-tile block beside longer ones.
# tags: the regimes the case is there for, each as "<regime>/plain" or "<regime>/pooled", as r32_tags() recomputes them.
WalkCase = collections.namedtuple("WalkCase", "N H W pooled bias tags")

R32_REGIMES = ("tmax>=4",              # with tmin < tmax
               "every_carry",          # a block with a step without carry, one column -> row and one row -> image; tiles_x != tiles_y,
                                       # N >= 2, G no whole number of images
               "tmin=1<tmax",          # blocks of one tile (no deferred store at all) beside blocks of two
               "tiles_x=1", "tiles_y=1", "tiles_x=2",
               "G%8!=0")               # the residue sq_xcd_remap sees
R32_NEEDED = {"%s/%s" % (r, k) for r in R32_REGIMES for k in ("plain", "pooled")} | {"nobias/plain", "nobias/pooled"}


def r32_tags(c):
    """the regimes of R32_NEEDED the case reaches, from the walk sq_conv_walk_plan reports and the shape"""
    p = walk(c.N, c.H, c.W, c.pooled)
    tiles_x, tiles_y = c.W // 16, c.H // 16
    t = set()
    if p["tmax"] >= 4 and p["tmin"] < p["tmax"]:
        t.add("tmax>=4")
    if tiles_x != tiles_y and c.N >= 2 and p["G"] % (tiles_x * tiles_y) != 0 and wc.blocks_with_every_carry(p, tiles_x, tiles_y):
        t.add("every_carry")
    if p["tmin"] == 1 and p["tmax"] >= 2:
        t.add("tmin=1<tmax")
    if tiles_x in (1, 2):
        t.add("tiles_x=%d" % tiles_x)
    if tiles_y == 1:
        t.add("tiles_y=1")
    if p["G"] % 8 != 0:
        t.add("G%8!=0")
    if c.bias is None:
        t.add("nobias")
    return {"%s/%s" % (r, "pooled" if c.pooled else "plain") for r in t}


def walk_case_id(c):
    return "%dx%dx%d-%s-bias_%s" % (c.N, c.H, c.W, "pool" if c.pooled else "plain", c.bias)


# The walks sq_conv_walk_plan reports (G blocks of tmin .. tmax tiles, stride G = gn images + gy rows + gx columns of tiles):
#   7 x 208 x 272     17 x 13 tiles, 1547 in all, G = 387 = 1 image + 9 rows + 13 columns, 3 or 4 tiles
#   1 x 17600 x 16    one column of 1100 tiles, G = 367 rows, 2 or 3 tiles
#   1 x 16 x 17600    one row of 1100 tiles, G = 367 columns, 2 or 3 tiles
#   3 x 5872 x 32     2 x 367 tiles, 2202 in all, G = 441 = 220 rows + 1 column, 4 or 5 tiles: the column carries at every other step
#   3 x 304 x 144     9 x 19 tiles, 513 in all, G = 257 = 1 image + 9 rows + 5 columns: block 256 has one tile, the others two
_WALK_SHAPES = [((7, 208, 272), ("G%8!=0", "every_carry", "tmax>=4")), ((1, 17600, 16), ("G%8!=0", "tiles_x=1")),
                ((1, 16, 17600), ("G%8!=0", "tiles_y=1")), ((3, 5872, 32), ("G%8!=0", "every_carry", "tiles_x=2", "tmax>=4")),
                ((3, 304, 144), ("G%8!=0", "tmin=1<tmax"))]
# no bias: the widest walk plain, the single tile row pooled
_NOBIAS = {(7, 208, 272, False), (1, 16, 17600, True)}
R32_WALKS = [WalkCase(*_s, _pooled, None if _s + (_pooled,) in _NOBIAS else "rand",
                      tuple("%s/%s" % (_r, "pooled" if _pooled else "plain")
                            for _r in _regimes + (("nobias",) if _s + (_pooled,) in _NOBIAS else ())))
             for _s, _regimes in _WALK_SHAPES for _pooled in (False, True)]
# the non-finite test's shape: ReLU, a bias, blocks of two tiles (plain and pooled)
NONFINITE_SHAPE = (3, 304, 144)
