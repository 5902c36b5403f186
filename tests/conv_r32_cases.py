"""Case tables of the 32 -> 32 filter-in-registers conv (conv_r32_kernel, sq_conv_f32_r32.hip), shared by the CPU plan tests
(tests/test_conv_r32_plan.py) and the GPU bit-identity tests (tests/test_gpu_conv_r32.py).

The kernel takes a call only on the plan that ran conv_mfma_f32_v2_kernel<32,3,32,0> before it (32-channel blocks, 32 staged
channels: at least 512 pixel tiles) and walks that kernel's grid, so sq_conv_walk_plan / sq_conv_plan report the same values with
the switch SQ_CONV_R32 on and off."""
import collections
import ctypes

from sequitr_amd import _lib
from tests import conv_sweep_cases as cs

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
