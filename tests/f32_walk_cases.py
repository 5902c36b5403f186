"""Case tables of the f32 tile-walk sweep (tests/test_gpu_f32_walk_sweep.py) and the walks they reach.

A plain module: the CPU suite reads the same tables through sq_conv_walk_plan (tests/test_f32_walk_plan.py) to check that every
case reaches the regime it is there for -- a block that walks three or more tiles, blocks that walk unevenly, every carry of the
tile stride, every row-tile count of the transpose conv.  The persistent f32 inference kernels give block b the items b, b + G,
b + 2G, ...; the seam between two items (prefetch one or two items ahead, double-buffered patches) only runs where G < items."""
import collections
import ctypes

from sequitr_amd import _lib
from tests import conv_sweep_cases as cs

PLAIN, POOL, CONCAT, FIRST, UP, HEAD, CONVT = 0, 2, 10, 8, 11, 12, 13          # SQ_PLAN_* forms of sq_conv_walk_plan
POOLED = 2                                                                     # SQ_PLAN_POOLED
NONE, L0, V2, CT = 0, 1, 2, 3                                                  # SQ_WALK_* kernels
FIELDS = ("kernel", "G", "tmin", "tmax", "gx", "gy", "gn", "mtiles", "cblocks", "items", "tilepx")
BRIDGES = ("eltwise_mul", "eltwise_add", "eltwise_sub", None)

# opt: FIRST -- also pool; UP, CONVT -- the bridge; HEAD -- head_c.  bias: "rand", "zero" or None (of the 3x3 conv).
# CONVT: (N, H, W) is the low-resolution input, everything else the output.
Case = collections.namedtuple("Case", "form N H W Cin Cout act opt bias")


def walk(form, N, H, W, Cin, Cout, K=3, act=None, pooled=False, head_c=0, wscale_one=True):
    """dict of FIELDS: the walk the call would launch with (sq_conv_walk_plan); raises where the entry point refuses the call"""
    lib = _lib.load()
    out = (ctypes.c_int * len(FIELDS))()
    flags = (0 if wscale_one else cs.WSCALE) | (POOLED if pooled else 0)
    rc = lib.sq_conv_walk_plan(form, N, H, W, Cin, Cout, K, cs.ACT[act], flags, head_c, ctypes.cast(out, ctypes.c_void_p))
    if rc != 0:
        raise _lib.SequitrHipError("sq_conv_walk_plan: %s" % lib.sq_last_error().decode())
    return dict(zip(FIELDS, out))


def walk_of(c):
    return walk(c.form, c.N, c.H, c.W, c.Cin, c.Cout, 3, c.act, pooled=c.form == FIRST and c.opt,
                head_c=c.opt if c.form == HEAD else 0)


def case_id(c):
    name = {PLAIN: "plain", POOL: "pool", CONCAT: "concat", FIRST: "first", UP: "up", HEAD: "head", CONVT: "convT"}[c.form]
    opt = {FIRST: "pool" if c.opt else "nopool", UP: str(c.opt), CONVT: str(c.opt), HEAD: "c%s" % c.opt}.get(c.form, "")
    return "%s-%s-%dx%dx%d-%d-%d-%s-bias_%s" % (name, opt, c.N, c.H, c.W, c.Cin, c.Cout, c.act, c.bias)


def tiles_xy(c):
    return -(-c.W // 16), -(-c.H // 16)


def block_count(p, b):
    """items block b walks"""
    return (p["items"] - b + p["G"] - 1) // p["G"]


def carries_of_block(p, tiles_x, tiles_y, b):
    """[(column carried into the row, row carried into the image)] of every advance() of block b, with the tile it lands on
    checked against b + k G: advance() as the kernels do it, by carries from the stride triple"""
    tx, ty, n = b % tiles_x, (b // tiles_x) % tiles_y, b // (tiles_x * tiles_y)
    steps = []
    for k in range(1, block_count(p, b)):
        tx += p["gx"]
        cx = tx >= tiles_x
        if cx:
            tx, ty = tx - tiles_x, ty + 1
        ty += p["gy"]
        cy = ty >= tiles_y
        if cy:
            ty, n = ty - tiles_y, n + 1
        n += p["gn"]
        t = b + k * p["G"]
        assert (tx, ty, n) == (t % tiles_x, (t // tiles_x) % tiles_y, t // (tiles_x * tiles_y)), (b, k, tx, ty, n)
        steps.append((cx, cy))
    return steps


def blocks_with_every_carry(p, tiles_x, tiles_y):
    """blocks whose walk has a step without a carry (the column moves alone), one where the column carries into the row and
    one where the row carries into the image"""
    out = []
    for b in range(p["G"]):
        s = carries_of_block(p, tiles_x, tiles_y, b)
        if any(not cx and not cy for cx, cy in s) and any(cx for cx, _ in s) and any(cy for _, cy in s):
            out.append(b)
    return out


def tile_position(p, tiles_x, tiles_y, n, ty, tx):
    """(block, position in its walk, tiles of its walk) of pixel tile (n, ty, tx); the block is the remapped index vb"""
    t = (n * tiles_y + ty) * tiles_x + tx
    b = t % p["G"]
    return b, t // p["G"], block_count(p, b)


def convT_position(p, c, n, oy, ox, ch):
    """(row tile, pixel tile, block, position in its walk, items of its walk) of output element (n, oy, ox, ch)"""
    rt = (((oy & 1) * 2 + (ox & 1)) * c.Cout + ch) // 128
    pt = ((n * c.H + oy // 2) * c.W + ox // 2) // p["tilepx"]
    item = pt * p["mtiles"] + rt
    b = item % p["G"]
    return rt, pt, b, item // p["G"], block_count(p, b)


# ---- the level-0 family: every instantiation at two shapes.  Both keep G < tiles / 2 at G = 1024 (plain 16 -> 16, pool, head,
# FIRST) and at G = 512 (16 -> 32, UP), leave tiles % G != 0, have tiles_x != tiles_y and N >= 2.  The same cases run the generic
# kernel under SQ_CONV_L0=0 (tiles % 3 != 0 keeps its grid uneven as well).
L0_SHAPES = [(4, 320, 416), (2, 368, 736)]
_L0_FORMS = [(PLAIN, 16, 16, None), (PLAIN, 16, 32, None), (POOL, 16, 16, None), (HEAD, 16, 16, 2), (FIRST, 1, 16, True),
             (FIRST, 1, 16, False)] + [(UP, 16, 16, b) for b in BRIDGES]
_L0_BIAS = {(PLAIN, 16, None, 0): None, (PLAIN, 32, None, 0): "zero", (POOL, 16, None, 1): None, (HEAD, 16, 2, 1): "zero",
            (FIRST, 16, False, 1): "zero", (UP, 16, "eltwise_add", 0): "zero", (UP, 16, None, 1): None}   # the kernel branches on a.bias
L0_CASES = [Case(_form, _N, _H, _W, _cin, _cout, "relu", _opt, _L0_BIAS.get((_form, _cout, _opt, _i), "rand"))
            for _i, (_N, _H, _W) in enumerate(L0_SHAPES) for (_form, _cin, _cout, _opt) in _L0_FORMS]

# ---- the generic kernel at a wide ragged shape the level-0 kernel declines by itself: 23 x 46 x 2 tiles with a partial last
# row and column of tiles, even sides for pool and UP; the forms that take an activation also run without ReLU
RAGGED = (2, 366, 730)
RAGGED_CASES = [
    Case(UP, *RAGGED, 16, 16, "leaky", "eltwise_mul", "rand"), Case(UP, *RAGGED, 16, 16, None, "eltwise_add", "rand"),
    Case(UP, *RAGGED, 16, 16, "relu", "eltwise_sub", None), Case(UP, *RAGGED, 16, 16, "leaky", None, "rand"),
    Case(FIRST, *RAGGED, 1, 16, "relu", True, "rand"), Case(FIRST, *RAGGED, 1, 16, "relu", False, "rand"),
    Case(HEAD, *RAGGED, 16, 16, "leaky", 1, "rand"), Case(HEAD, *RAGGED, 16, 16, None, 2, "rand"),
    Case(HEAD, *RAGGED, 16, 16, "relu", 3, None),
    Case(PLAIN, *RAGGED, 32, 16, "leaky", None, "rand"),        # 16-channel blocks, two input chunks
]

# ---- the generic kernel on wide channel blocks: (case, BN, KC, channel blocks) as sq_conv_plan reports them
WIDE_CASES = [
    (Case(PLAIN, 2, 250, 262, 32, 80, "relu", None, "rand"), 64, 16, 2),       # 64-channel blocks, two chunks, fast + masked epilogue
    (Case(PLAIN, 4, 250, 264, 16, 48, "leaky", None, "rand"), 32, 16, 2),      # 32-channel blocks, unstaged
    (Case(PLAIN, 2, 250, 264, 32, 48, "relu", None, "rand"), 32, 32, 2),       # 32-channel blocks, stage-32
    (Case(CONCAT, 2, 250, 262, 32, 80, None, None, "rand"), 64, 16, 2),        # concat at 64-channel blocks
    (Case(POOL, 4, 250, 264, 16, 48, "relu", None, "rand"), 32, 16, 2),        # pooled at 32-channel blocks
]

# ---- the transpose conv at the default 32-pixel tiles: row tiles 1 .. 5 (Cout 32 .. 160), more than 2 G work items, a ragged
# last pixel tile, two or more chunks; every bridge at 3 and 4 row tiles (3: the grid is trimmed to a multiple of the row tiles)
_CT = [(64, 32, 2, 181, 183, ("eltwise_mul", None)), (64, 64, 3, 61, 181, ("eltwise_mul", None)), (64, 96, 2, 60, 183, BRIDGES),
       (256, 128, 1, 90, 183, BRIDGES), (96, 160, 2, 36, 183, ("eltwise_mul", None))]
CONVT_CASES = [Case(CONVT, n, h, w, cin, cout, None, b, "rand" if (cin, b) != (64, None) else None)
               for (cin, cout, n, h, w, bridges) in _CT for b in bridges]
