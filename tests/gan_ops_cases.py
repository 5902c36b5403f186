"""Shared by the GAN operator tests: case tables, fp64 definitions, exact replays and the bounds of the GPU sweep
(tests/test_gpu_gan_ops_sweep.py), whose regime coverage, references and bounds tests/test_gan_ops_definitions.py checks
without a GPU.  No HIP call, no import of the library.  The kernels are those of sequitr_amd/csrc/sq_gan_ops.hip,
sq_gan_bf16.hip, sq_dense.hip and pixelnorm_f32_kernel of sq_pointwise.hip, reached through sequitr_amd/ops.py,
ops_gan_bf16.py and functional.py.

Every table is a list of (case, declared tags); beside it a *_tags(case) that recomputes the tags from the launch
arithmetic restated from the .hip source, and a *_NEEDED set the table has to reach.

Three kinds of check:
  EXACT cases.  Sums and dot products (the small weight gradients and asum, dot_per_sample, dense forward and weight
    gradient, the dy-sum of the mbstd backward) run on small integers (bf16-exact where the operand is bf16) with power-of-two
    scales: every partial sum in any order is an integer below 2^24, so the GPU result must EQUAL the fp64 one.  A dropped or
    doubled term shows at any size.
  BOUNDED cases.  randn-type inputs against the fp64 definition, |got - ref| <= k u sum |terms| per output, u = 2^-24, k the
    largest number of f32 roundings a term passes on its way to the output (lane chain + fold + finish), counted from the
    code without contraction (a fused multiply-add only removes a rounding).  A bf16 output adds half a bf16 ulp of the
    exact value (2^-8 relative), one more where an activation gate rounds a second time.  k is derived next to each table.
  EXACT REPLAYS.  Index maps and single-rounding operators equal a numpy / torch replay, compared as numbers.

Layouts: activations NHWC, 1x1 filters (1,1,Cin,Cout), dense weights (K,N)."""
import numpy as np
import torch

from tests.bf16_ops_cases import SLOPE, _gen, _randn, group_size
from tests.f32_ops_cases import U, _butterfly, _fma32

BF16 = torch.bfloat16
F32 = torch.float32
HALF_BF16_ULP = 2.0 ** -8                                      # relative: half a unit in the last of 8 significant bits
ACTS = (None, "relu", "leaky")

# the launch constants, by source file
GRID_CAP_F32 = 2048                                             # grid_for of sq_gan_ops.hip and sq_pointwise.hip: blocks of 256
GRID_CAP_BF16 = 4096                                            # grid_for of sq_gan_bf16.hip
SMALL_CAP_F32 = 256                                             # small_blocks of sq_gan_ops.hip (wgrad1x1_small_kernel)
SMALL_CAP_BF16 = 1024                                           # small_blocks of sq_gan_bf16.hip
DOT_SLICES = 32                                                 # sq_gan_ops.hip
MB_B, MB_BT, MB_T = 64, 256, 1024                               # sq_gan_ops.hip: statistic blocks per group, their threads; loss block
DK, DM, WK = 64, 32, 32                                         # sq_dense.hip: reduction slice, rows per block; wgrad rows of dW


def _cdiv(a, b):
    return -(-a // b)


def _pow2(v):
    return v & (v - 1) == 0


def regime(items, cap_blocks):
    """stream_regime's idea with the cap as an argument: how a 256-thread grid-stride kernel capped at cap_blocks walks `items`"""
    if items < 256:
        return "below_256"
    if items <= cap_blocks * 256:
        return "one_trip_ragged" if items % 256 else "one_trip_whole"
    return "above_cap_ragged" if items % (cap_blocks * 256) else "above_cap_whole"


STREAM_NEEDED = {"below_256", "one_trip_ragged", "above_cap_ragged"}


def _ints(g, shape, bound):
    """integers in [-bound, bound] as f32: exact in bf16 for bound <= 256"""
    return torch.randint(-bound, bound + 1, shape, generator=g).to(F32)


def _signed_with_zeros(g, shape):
    """randn with exact +0.0 and -0.0 planted: the gates read `x > 0`"""
    x = _randn(g, shape)
    x.view(-1)[::7] = 0.0
    x.view(-1)[7::14] = -0.0
    return x


def act64(v, act):
    return v if SLOPE[act] == 1.0 else torch.where(v > 0, v, v * float(np.float32(SLOPE[act])))


# ==== 1. image-side small weight gradients =================================================================================
# wgrad1x1_small_kernel (f32, unit = 4 channels per thread) and wgrad1x1_small_bf16_kernel (unit = 8):
#   groups = C / unit, gpp = min(256, groups) channel groups per pass, pl = 256 // gpp pixel lanes per block,
#   nb = min(cap, ceil(npix / 256)) blocks, step = nb * pl: lane (block, tp) walks pixels block * pl + tp + i * step with one
#   fmaf per pixel and output (the bf16 kernel four pixels per trip while p + 3 step < npix, then a tail: the same order).
#   The block folds its pl lanes in LDS: a halving tree where pl is a power of two, one thread adding the pl lanes in order
#   otherwise.  The finish is sq_group_reduce over the nb block partials: G = group_size(nb) lanes, lane g adds partials
#   g, g + G, ... in order, then a butterfly.  The bf16 entry multiplies by `scale` when it is not 1.
# k: roundings on the longest path of a term
#   lane chain   ceil(npix / step)       one fmaf per pixel
#   fold         log2(pl) | pl           tree | serial (the first add of the serial fold is to 0: counted all the same)
#   finish       ceil(nb / G) + log2(G)
#   scale        1 where scale != 1
# asum (bf16 entry): the lanes of channel group 0 add a[p][c] in the same pixel order (chain), always the serial fold (pl), the
# same finish, no scale.
class SmallLaunch(object):
    def __init__(self, npix, C, unit, cap):
        self.npix, self.C, self.unit = npix, C, unit
        self.groups = C // unit
        self.gpp = min(256, self.groups)
        self.pl = 256 // self.gpp
        self.nb = min(cap, max(1, _cdiv(npix, 256)))
        self.step = self.nb * self.pl
        self.G = group_size(self.nb)
        self.trips = _cdiv(npix, self.step)                     # pixels of the busiest lane
        self.capped = _cdiv(npix, 256) > cap
        self.tree = _pow2(self.pl)

    def fold_adds(self):
        return int(np.log2(self.pl)) if self.tree else self.pl

    def finish_adds(self):
        return _cdiv(self.nb, self.G) + int(np.log2(self.G))

    def k(self, scale=1.0):
        return self.trips + self.fold_adds() + self.finish_adds() + (1 if scale != 1.0 else 0)

    def k_asum(self):
        return self.trips + self.pl + self.finish_adds()

    def lane_counts(self):
        """the two pixel counts lanes have: (count of the first npix % step lanes, count of the others)"""
        full, part = divmod(self.npix, self.step)
        return (full + 1 if part else full), full


def _g_tag(G):
    return "G=1" if G == 1 else ("G=64" if G == 64 else "G=mid")


def wg32_launch(c):
    npix, Ca, Cb = c
    return SmallLaunch(npix, Cb, 4, SMALL_CAP_F32)


def wg32_tags(c):
    npix, Ca, Cb = c
    L = wg32_launch(c)
    tags = {"Ca=%d" % Ca, _g_tag(L.G)}
    if L.groups > 256:
        tags.add("multi_pass")
    elif L.pl == 1:
        tags.add("one_lane")
    elif L.tree:
        tags.add("tree_fold" if L.pl * L.gpp == 256 else "tree_fold_idle_threads")
    else:
        tags.add("serial_fold")
    if npix < L.step:
        tags.add("fewer_pixels_than_lanes")
    if npix % L.step:
        tags.add("ragged")
    if L.capped and L.trips > 1:
        tags.add("block_stride")
    return tags


WG32_NEEDED = {"Ca=%d" % c for c in range(1, 8)} | {"tree_fold", "tree_fold_idle_threads", "serial_fold", "one_lane",
                                                      "multi_pass", "fewer_pixels_than_lanes", "ragged", "block_stride",
                                                      "G=1", "G=mid", "G=64"}
# (npix, Ca, Cb).  one_lane is pl == 1 in one pass: 129 <= Cb / 4 <= 256 (at Cb / 4 = 128 the kernel still has two lanes).
WG32_CASES = [((300, ca, 16), {"Ca=%d" % ca, "tree_fold", "ragged", "G=mid"}) for ca in range(1, 8)] + [
    ((100, 2, 400), {"Ca=2", "tree_fold_idle_threads", "G=1"}),                     # q4 100: 2 lanes, 56 threads idle
    ((50, 3, 12), {"Ca=3", "serial_fold", "fewer_pixels_than_lanes", "ragged", "G=1"}),     # q4 3: 85 lanes
    ((1300, 4, 20), {"Ca=4", "serial_fold", "ragged", "G=mid"}),                    # q4 5: 51 lanes, 6 blocks, G 4
    ((700, 2, 192), {"Ca=2", "serial_fold", "ragged", "G=mid"}),                    # q4 48: 5 lanes
    ((40, 1, 520), {"Ca=1", "one_lane", "G=1"}),                                    # q4 130
    ((33, 2, 1028), {"Ca=2", "multi_pass", "G=1"}),                                 # q4 257: a second pass of one quad
    ((256 * 256 + 5, 3, 8), {"Ca=3", "tree_fold", "ragged", "block_stride", "G=64"}),   # 257 blocks of pixels on 256
]


def wgbf_launch(c):
    npix, Ca, C = c[:3]
    return SmallLaunch(npix, C, 8, SMALL_CAP_BF16)


def wgbf_tags(c):
    npix, Ca, C, a_none, want_asum, scale = c
    L = wgbf_launch(c)
    tags = {"Ca=%d" % Ca, "scale=1" if scale == 1.0 else "scale!=1"}
    if a_none:
        tags.add("a_none")
    if want_asum:
        tags.add("asum")
    tags.add("multi_pass" if L.groups > 256 else ("pow2" if _pow2(L.groups) else "non_pow2"))
    for cnt in set(L.lane_counts()):                            # four pixels per trip while p + 3 step < npix, then the tail
        n4, rem = divmod(cnt, 4)
        if n4 and not rem:
            tags.add("unroll4_only")
        if n4 and rem:
            tags.add("unroll4_plus_remainder")
        if not n4 and rem:
            tags.add("remainder_only")
    if L.capped:
        tags.add("block_cap")
    return tags


NON_POW2_C = (24, 40, 48, 56, 72, 120, 192, 320)              # C / 8 = 3, 5, 6, 7, 9, 15, 24, 40
WGBF_NEEDED = {"Ca=1", "Ca=2", "Ca=3", "Ca=4", "a_none", "asum", "scale=1", "scale!=1", "pow2", "non_pow2", "multi_pass",
               "unroll4_only", "unroll4_plus_remainder", "remainder_only", "block_cap"}
# (npix, Ca, C, a is None, want_asum, scale)
WGBF_CASES = [
    ((300, 1, 8, False, False, 1.0), {"Ca=1", "scale=1", "pow2", "remainder_only"}),
    ((1024, 2, 512, False, True, 0.5), {"Ca=2", "scale!=1", "asum", "pow2", "unroll4_only"}),
    ((1030, 3, 512, False, False, 1.0), {"Ca=3", "scale=1", "pow2", "unroll4_only", "unroll4_plus_remainder"}),
    ((700, 4, 32, False, True, 1.0), {"Ca=4", "scale=1", "asum", "pow2", "unroll4_only", "remainder_only"}),
    ((500, 1, 64, True, False, 0.5), {"Ca=1", "scale!=1", "a_none", "pow2", "unroll4_only", "unroll4_plus_remainder"}),
    ((777, 2, 24, False, True, 0.5), {"Ca=2", "scale!=1", "asum", "non_pow2", "remainder_only"}),
    ((777, 3, 40, False, False, 1.0), {"Ca=3", "scale=1", "non_pow2", "unroll4_only", "remainder_only"}),
    ((130, 1, 40, True, False, 1.0), {"Ca=1", "scale=1", "a_none", "non_pow2", "remainder_only"}),
    ((777, 2, 48, False, True, 1.0), {"Ca=2", "scale=1", "asum", "non_pow2", "unroll4_only", "unroll4_plus_remainder"}),
    ((2000, 1, 56, False, False, 0.5), {"Ca=1", "scale!=1", "non_pow2", "unroll4_plus_remainder"}),
    ((777, 4, 72, False, True, 1.0), {"Ca=4", "scale=1", "asum", "non_pow2", "unroll4_plus_remainder"}),
    ((777, 1, 120, True, False, 1.0), {"Ca=1", "scale=1", "a_none", "non_pow2", "unroll4_only", "unroll4_plus_remainder"}),
    ((777, 2, 192, False, False, 0.5), {"Ca=2", "scale!=1", "non_pow2", "unroll4_only", "unroll4_plus_remainder"}),
    ((600, 3, 320, False, True, 1.0), {"Ca=3", "scale=1", "asum", "non_pow2", "unroll4_plus_remainder"}),
    ((300, 2, 2056, False, True, 0.5), {"Ca=2", "scale!=1", "asum", "multi_pass", "unroll4_plus_remainder"}),
    ((1024 * 256 + 77, 2, 8, False, True, 1.0), {"Ca=2", "scale=1", "asum", "pow2", "remainder_only", "block_cap"}),
]
A_BOUND, B_BOUND = 2, 4                                         # exact inputs: |a| <= 2, |b| <= 4 (integers)


def wg_inputs(npix, Ca, C, exact, bf, a_none=False):
    """(a (npix, Ca) f32 or None, b (npix, C) f32 -- bf16-valued where bf)"""
    g = _gen(41, npix, Ca, C, exact, bf)
    if exact:
        a, b = _ints(g, (npix, Ca), A_BOUND), _ints(g, (npix, C), B_BOUND)
    else:
        a, b = _randn(g, (npix, Ca)), _randn(g, (npix, C))
        if bf:
            b = b.to(BF16).to(F32)
    return (None if a_none else a), b


def wg_ref64(a, b, scale=1.0):
    """fp64: (m, sum |terms| of m, asum, sum |terms| of asum); a None = ones (npix, 1)"""
    b64 = b.double()
    a64 = torch.ones((b.shape[0], 1), dtype=torch.float64) if a is None else a.double()
    s = float(np.float32(scale))
    return a64.t() @ b64 * s, a64.abs().t() @ b64.abs() * abs(s), a64.sum(0), a64.abs().sum(0)


def wg_restated(a, b, unit, cap, fold="fixed", scale=1.0, drop=None):
    """the two kernels and their finish in numpy float32, in the kernels' own order: (m (Ca, C), asum (Ca)).
    fold: "fixed" -- the halving tree where pl is a power of two, the serial fold otherwise;
          "tree"  -- the halving tree `for (st = pl >> 1; st > 0; st >>= 1) if (tp < st) v[tp] += v[tp + st]` whatever pl.
    drop: ("lane", i) zeroes lane i's accumulators before the fold; ("pixel", p) skips pixel p."""
    f = np.float32
    B = b.numpy()
    npix, C = B.shape
    A = np.ones((npix, 1), f) if a is None else a.numpy()
    Ca = A.shape[1]
    L = SmallLaunch(npix, C, unit, cap)
    acc = np.zeros((L.step, Ca, C), f)                          # lane block * pl + tp holds pixels lane + i * step, in order
    asl = np.zeros((L.step, Ca), f)
    for i in range(L.trips):
        lo = i * L.step
        n = min(L.step, npix - lo)
        Ai, Bi = A[lo:lo + n].copy(), B[lo:lo + n]
        if drop is not None and drop[0] == "pixel" and lo <= drop[1] < lo + n:
            Ai[drop[1] - lo] = 0.0                              # fmaf(0, b, acc) = acc, acc + 0 = acc: the pixel is skipped
        acc[:n] = _fma32(Ai[:, :, None], Bi[:, None, :], acc[:n])
        asl[:n] = asl[:n] + Ai
    if drop is not None and drop[0] == "lane":
        acc[drop[1]] = 0.0
        asl[drop[1]] = 0.0
    v = acc.reshape(L.nb, L.pl, Ca * C)

    def serial(w):
        s = np.zeros((L.nb,) + w.shape[2:], f)
        for kk in range(L.pl):
            s = s + w[:, kk]
        return s

    if fold == "tree" or L.tree:
        v = v.copy()
        st = L.pl >> 1
        while st > 0:
            v[:, :st] = v[:, :st] + v[:, st:2 * st]
            st >>= 1
        part = v[:, 0]
    else:
        part = serial(v)
    part = np.concatenate([part, serial(asl.reshape(L.nb, L.pl, Ca))], 1)       # [block][Ca C + Ca]
    lanes = np.zeros((L.G, part.shape[1]), f)
    for blk in range(L.nb):                                     # sq_group_reduce: lane g adds partials g, g + G, ... in order
        lanes[blk % L.G] = lanes[blk % L.G] + part[blk]
    out = _butterfly(lanes, L.G)
    m = out[:Ca * C].reshape(Ca, C)
    if scale != 1.0:
        m = m * f(scale)
    return torch.from_numpy(m.astype(f)), torch.from_numpy(out[Ca * C:].astype(f))


def tree_lanes_reached(pl):
    """how many of pl lanes that all hold 1 end up in lane 0 of the halving tree"""
    v = np.ones(pl)
    st = pl >> 1
    while st > 0:
        v[:st] += v[st:2 * st]
        st >>= 1
    return int(v[0])


# ---- image-side forward convolutions (sq_conv1x1_smallin_fwd_bf16, sq_conv1x1_smallout_fwd_bf16) ---------------------------
# smallin:  y[p][c] = bf16(act(chain_a fmaf(fl(w[a][c] wscale), x[p][a]) + bias[c])), x f32 with CA <= 4 channels; thread =
#           (pixel, 8 channels), grid-stride over npix C / 8 items, grid_for of sq_gan_bf16.hip.
#           k = 1 (w wscale) + CA (chain) + 1 (bias) + 1 (leaky's product) = CA + 3, then the bf16 rounding.
# smallout: y[p][o] = act(chain_c fmaf(fl(w[c][o] wscale), x[p][c]) + bias[o]), x bf16; ONE thread per pixel, ceil(npix / 256)
#           blocks, no cap.   k = 1 + C + 1 + 1 = C + 3, f32 output.
# Both activations are 1-Lipschitz, so the bound of the pre-activation carries over.
def smallin_k(CA):
    return CA + 3


def smallout_k(C):
    return C + 3


def smallin_tags(c):
    npix, CA, C, bias, act = c
    return {"CA=%d" % CA, "C=%d" % C, "bias" if bias else "no_bias", "act=%s" % act, regime(npix * (C // 8), GRID_CAP_BF16)}


def smallout_tags(c):
    npix, CO, C, bias, act = c
    tags = {"CO=%d" % CO, "C=%d" % C, "bias" if bias else "no_bias", "act=%s" % act}
    tags.add("below_256" if npix < 256 else ("blocks_ragged" if npix % 256 else "blocks_whole"))
    return tags


IMAGE_C = (8, 24, 40, 512)
SMALLIN_NEEDED = {"CA=%d" % k for k in (1, 2, 3, 4)} | {"C=%d" % c for c in IMAGE_C} | {"bias", "no_bias"} | {
    "act=%s" % a for a in ACTS} | STREAM_NEEDED
SMALLOUT_NEEDED = {"CO=%d" % k for k in (1, 2, 3, 4)} | {"C=%d" % c for c in IMAGE_C} | {"bias", "no_bias"} | {
    "act=%s" % a for a in ACTS} | {"below_256", "blocks_ragged"}
# (npix, CA, C, bias, act); npix is even: the sweep hands conv2d the image (1, 2, npix / 2, .), a spatial map to its dispatch
SMALLIN_CASES = [
    ((26, 1, 8, True, None), {"CA=1", "C=8", "bias", "act=None", "below_256"}),
    ((1000, 2, 24, False, "leaky"), {"CA=2", "C=24", "no_bias", "act=leaky", "one_trip_ragged"}),
    ((1000, 3, 40, True, "relu"), {"CA=3", "C=40", "bias", "act=relu", "one_trip_ragged"}),
    ((30, 4, 512, True, "leaky"), {"CA=4", "C=512", "bias", "act=leaky", "one_trip_ragged"}),
    ((4096 * 4 + 6, 2, 512, False, "leaky"), {"CA=2", "C=512", "no_bias", "act=leaky", "above_cap_ragged"}),
]
SMALLOUT_CASES = [
    ((26, 1, 8, True, None), {"CO=1", "C=8", "bias", "act=None", "below_256"}),
    ((1000, 2, 24, False, "leaky"), {"CO=2", "C=24", "no_bias", "act=leaky", "blocks_ragged"}),
    ((1000, 3, 40, True, "relu"), {"CO=3", "C=40", "bias", "act=relu", "blocks_ragged"}),
    ((300, 4, 512, True, "leaky"), {"CO=4", "C=512", "bias", "act=leaky", "blocks_ragged"}),
]
IMAGE_WSCALE = 0.37


def image_conv_inputs(c, out):
    """smallin (out False): x f32 (npix, CA), w (CA, C); smallout: x bf16-valued (npix, C), w (C, CO)"""
    npix, Cs, C, bias, act = c
    g = _gen(42, npix, Cs, C, out)
    ci, co = (C, Cs) if out else (Cs, C)
    x = _randn(g, (npix, ci))
    if out:
        x = x.to(BF16).to(F32)
    return {"x": x, "w": _randn(g, (ci, co)), "bias": _randn(g, (co,)) if bias else None}


def image_conv_ref64(i, act, wscale=IMAGE_WSCALE):
    """(act(x (w wscale) + bias), sum |terms| of the pre-activation) with the filter scaled in f32 as the kernel holds it"""
    ws = (i["w"] * torch.tensor(wscale, dtype=F32)).double()
    x = i["x"].double()
    pre, terms = x @ ws, x.abs() @ ws.abs()
    if i["bias"] is not None:
        pre, terms = pre + i["bias"].double(), terms + i["bias"].double().abs()
    return act64(pre, act), terms


# ==== 2. pixel norm ========================================================================================================
# y = x r, r = 1 / sqrt(mean_c x^2 + eps); one GL-lane group per pixel, 64 / GL pixels per wave.
#   f32 (pixelnorm_f32_kernel, pixelnorm_bwd_kernel): GL = 1, 2, 4, 8, 16 for C <= 4, 8, 16, 32, else; a lane owns channels
#        4 l + 4 GL k + {0..3}; grid_for(npix GL) with the 2048-block cap.
#   bf16 (pixelnorm_bf16_kernel): 8 channels per lane and pass; the register path at C = 8 GL NCH for C in {8, ..., 512},
#        otherwise GL = 1, 2, 4, 8, 16 for C <= 8, 16, 32, 64, else; the 4096-block cap.
# Roundings of a channel sum (x^2, g x, v x, v g): products 1, the lane's chain `passes * per` adds (per = 4 or 8 channels),
# the butterfly log2(GL):  k_sum = 1 + passes per + log2(GL).   r: the sum, * 1/C (1; 1/C itself 1), + eps (1), sqrt (1),
# the division (1):  k_r = k_sum + 5  (the square root halves what comes before it; not used).
#   forward   y = x r                              |err| <= (k_r + 1) u |y|
#   backward  dx = r g - r^3 s x, s = mean(g x)    terms t1 = r g, t2 = r^3 s x; s carries ABSOLUTE error k_sum u mean|g x|:
#             |err| <= u ((k_r + 2) |t1| + (3 k_r + 6) |t2| + k_sum r^3 |x| mean|g x|)
#             gated (x the output of an activation): dx slope where x <= 0 -- one more product: + u |out|
#   2nd backward  dg as the backward with v for g;
#             dx2 = -r^3 u x + 3 r^5 s t x - r^3 t g - r^3 s v, t = mean(v x), u = mean(v g): four terms A1..A4, each with
#             at most 5 k_r + 10 relative roundings, and the absolute errors of s, t, u:
#             |err| <= u ((5 k_r + 10)(|A1| + |A2| + |A3| + |A4|)
#                         + k_sum (r^3 |x| mean|v g| + 3 r^5 |x| (|t| mean|g x| + |s| mean|v x|) + r^3 |g| mean|v x| + r^3 |v| mean|g x|))
# bf16 outputs: + 2^-8 (|exact| + the f32 bound) per stored rounding (two for the gated backward).
PN_EPS = 1e-8
PN_REGS = {8: (1, 1), 16: (2, 1), 32: (4, 1), 64: (8, 1), 128: (16, 1), 256: (16, 2), 512: (16, 4)}    # C: (GL, NCH)


def pn_launch(bf, C):
    """(GL, passes of the busiest lane, channels per lane and pass, register path)"""
    per = 8 if bf else 4
    if bf and C in PN_REGS:
        GL, nch = PN_REGS[C]
        return GL, nch, per, True
    GL = 1
    while GL < 16 and C > per * GL:
        GL *= 2
    return GL, _cdiv(C, per * GL), per, False


def pn_k_sum(bf, C):
    GL, passes, per, _ = pn_launch(bf, C)
    return 1 + passes * per + int(np.log2(GL))


def pn_tags(c):
    bf, C, npix = c
    GL, passes, per, regs = pn_launch(bf, C)
    cap = GRID_CAP_BF16 if bf else GRID_CAP_F32
    tags = {"gl%d" % GL}
    if bf:
        tags.add("regs_nch%d" % passes if regs else "generic")
    if C < per * GL:
        tags.add("idle_lanes")
    if not regs and passes >= 2:
        tags.add("second_pass")
    if not regs and passes >= 3:
        tags.add("third_pass")
    ppw = 64 // GL
    if npix < ppw:
        tags.add("below_one_wave")
    if npix % ppw:
        tags.add("ragged_wave")
    if npix * GL > cap * 256:
        tags.add("above_cap")
    return tags


PN32_NEEDED = {"gl1", "gl2", "gl4", "gl8", "gl16", "idle_lanes", "second_pass", "third_pass", "below_one_wave", "ragged_wave",
               "above_cap"}
PN32_CASES = [
    ((False, 4, 77), {"gl1", "ragged_wave"}),
    ((False, 8, 77), {"gl2", "ragged_wave"}),
    ((False, 12, 3), {"gl4", "idle_lanes", "below_one_wave", "ragged_wave"}),
    ((False, 16, 77), {"gl4", "ragged_wave"}),
    ((False, 20, 77), {"gl8", "idle_lanes", "ragged_wave"}),
    ((False, 32, 5), {"gl8", "below_one_wave", "ragged_wave"}),
    ((False, 36, 77), {"gl16", "idle_lanes", "ragged_wave"}),
    ((False, 64, 77), {"gl16", "ragged_wave"}),
    ((False, 68, 77), {"gl16", "second_pass", "ragged_wave"}),                      # lane 0 alone takes a second quad
    ((False, 132, 3), {"gl16", "second_pass", "third_pass", "below_one_wave", "ragged_wave"}),
    ((False, 36, 32768 + 5), {"gl16", "idle_lanes", "ragged_wave", "above_cap"}),  # the smallest above the 2048-block cap
]
PNBF_NEEDED = {"regs_nch1", "regs_nch2", "regs_nch4", "generic", "gl1", "gl2", "gl4", "gl8", "gl16", "idle_lanes",
               "second_pass", "third_pass", "below_one_wave", "ragged_wave", "above_cap"}
PNBF_CASES = [
    ((True, 8, 77), {"gl1", "regs_nch1", "ragged_wave"}),
    ((True, 16, 77), {"gl2", "regs_nch1", "ragged_wave"}),
    ((True, 32, 77), {"gl4", "regs_nch1", "ragged_wave"}),
    ((True, 64, 5), {"gl8", "regs_nch1", "below_one_wave", "ragged_wave"}),
    ((True, 128, 77), {"gl16", "regs_nch1", "ragged_wave"}),
    ((True, 256, 3), {"gl16", "regs_nch2", "below_one_wave", "ragged_wave"}),
    ((True, 512, 77), {"gl16", "regs_nch4", "ragged_wave"}),
    ((True, 24, 77), {"gl4", "generic", "idle_lanes", "ragged_wave"}),
    ((True, 40, 77), {"gl8", "generic", "idle_lanes", "ragged_wave"}),
    ((True, 48, 5), {"gl8", "generic", "idle_lanes", "below_one_wave", "ragged_wave"}),
    ((True, 56, 77), {"gl8", "generic", "idle_lanes", "ragged_wave"}),
    ((True, 72, 77), {"gl16", "generic", "idle_lanes", "ragged_wave"}),
    ((True, 136, 77), {"gl16", "generic", "second_pass", "ragged_wave"}),
    ((True, 264, 3), {"gl16", "generic", "second_pass", "third_pass", "below_one_wave", "ragged_wave"}),
    ((True, 72, 65536 + 5), {"gl16", "generic", "idle_lanes", "ragged_wave", "above_cap"}),
]


def pn_inputs(c):
    """x with both signs and exact zeros (the gate reads x > 0); g, v upstream gradients; bf16-valued where bf"""
    bf, C, npix = c
    g = _gen(43, bf, C, npix)
    i = {"x": _signed_with_zeros(g, (npix, C)), "g": _randn(g, (npix, C)), "v": _randn(g, (npix, C))}
    if bf:
        i = {k: t.to(BF16).to(F32) for k, t in i.items()}
    return i


def pn_ref64(i, bf, eps=PN_EPS):
    """fp64 definitions and their f32 bounds (see the derivation above): {name: (exact, bound)}; bf16 roundings are added by
    pn_store_bound"""
    x, g, v = (i[k].double() for k in ("x", "g", "v"))
    C = x.shape[1]
    ks = pn_k_sum(bf, C)
    kr = ks + 5
    eps = float(np.float32(eps))
    m = lambda t: t.mean(1, keepdim=True)                       # noqa: E731
    r = 1.0 / torch.sqrt(m(x * x) + eps)
    r3, r5 = r ** 3, r ** 5
    s, t, uu = m(g * x), m(v * x), m(v * g)
    sa, ta, ua = m((g * x).abs()), m((v * x).abs()), m((v * g).abs())
    out = {"fwd": (x * r, (kr + 1) * U * (x * r).abs())}

    def bwd(gg, ss, ssa):
        t1, t2 = r * gg, r3 * ss * x
        return t1 - t2, U * ((kr + 2) * t1.abs() + (3 * kr + 6) * t2.abs() + ks * r3 * x.abs() * ssa)

    out["bwd"] = bwd(g, s, sa)
    out["dg"] = bwd(v, t, ta)
    A1, A2, A3, A4 = r3 * uu * x, 3 * r5 * s * t * x, r3 * t * g, r3 * s * v
    rel = (5 * kr + 10) * (A1.abs() + A2.abs() + A3.abs() + A4.abs())
    ab = ks * (r3 * x.abs() * ua + 3 * r5 * x.abs() * (t.abs() * sa + s.abs() * ta) + r3 * g.abs() * ta + r3 * v.abs() * sa)
    out["dx2"] = (-A1 + A2 - A3 - A4, U * (rel + ab))
    return out


def pn_gate(exact, bound, x, act, bf):
    """the backward leaving through the activation whose output x is: (exact, bound), for bf16 with every stored rounding"""
    if bf:                                                      # bf16: the ungated value is rounded to bf16 first
        bound = pn_store_bound(exact, bound)
    if SLOPE[act] == 1.0:
        return exact, bound
    sl = float(np.float32(SLOPE[act]))
    pos = x.double() > 0
    e = torch.where(pos, exact, exact * sl)
    gated = bound * sl + U * e.abs()
    return e, torch.where(pos, bound, pn_store_bound(e, gated) if bf else gated)    # bf16: the gated value is rounded again


def pn_store_bound(exact, bound):
    return bound + HALF_BF16_ULP * (exact.abs() + bound)


def _rb(t):
    """round an f32 numpy array to bf16 (nearest even) and back"""
    return torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)).to(BF16).to(F32).numpy()


def pn_restated(i, bf=False, act=None, eps=PN_EPS, drop_piece=None, store=True):
    """pixelnorm_f32_kernel, pixelnorm_bwd_kernel (f32) or pixelnorm_bf16_kernel in numpy float32, in the kernels' order -- a
    lane's chain over its channel pieces (4 channels, or 8 for bf16), then the butterfly over the lane group: {fwd, bwd, dg, dx2}
    (bwd through the gate of `act`; bf16 results rounded where the kernel stores them).  drop_piece: that 4- / 8-channel piece
    is left out of every channel sum.  store=False: the f32 values before the bf16 kernel rounds them (act None only)."""
    f = np.float32
    x, g, v = (i[k].numpy() for k in ("x", "g", "v"))
    npix, C = x.shape
    GL, _, per, _ = pn_launch(bf, C)
    assert store or act is None
    sums = {k: np.zeros((GL, npix), f) for k in ("xx_fwd", "xx", "gx", "vx", "vg")}
    for q in range(C // per):
        if q == drop_piece:
            continue
        l = q % GL
        sl = slice(per * q, per * q + per)
        pairs = {"xx": (x[:, sl], x[:, sl]), "gx": (g[:, sl], x[:, sl]), "vx": (v[:, sl], x[:, sl]), "vg": (v[:, sl], g[:, sl])}
        if bf:                                                  # dot8: an fmaf chain from 0, added to the lane's sum
            for k, (a, b) in pairs.items():
                d = np.zeros(npix, f)
                for j in range(per):
                    d = _fma32(a[:, j], b[:, j], d)
                sums[k][l] = sums[k][l] + d
            sums["xx_fwd"][l] = sums["xx"][l]
        else:
            for j in range(per):                                # forward kernel: one fmaf chain through the lane's channels
                sums["xx_fwd"][l] = _fma32(x[:, sl][:, j], x[:, sl][:, j], sums["xx_fwd"][l])
            for k, (a, b) in pairs.items():                     # backward kernel: s += ((p0 + p1) + p2) + p3
                pr = a * b
                sums[k][l] = sums[k][l] + (((pr[:, 0] + pr[:, 1]) + pr[:, 2]) + pr[:, 3])
    S = {k: _butterfly(t, GL)[:, None] for k, t in sums.items()}
    invC = f(1.0) / f(C)
    if bf:
        r_fwd = f(1.0) / np.sqrt(S["xx"] * invC + f(eps))
    else:
        r_fwd = f(1.0) / np.sqrt(S["xx_fwd"] / f(C) + f(eps))
    r = f(1.0) / np.sqrt(S["xx"] * invC + f(eps))
    r3 = r * r * r
    s_, t_, u_ = S["gx"] * invC, S["vx"] * invC, S["vg"] * invC
    out = {"fwd": x * r_fwd, "bwd": r * g - r3 * s_ * x, "dg": r * v - r3 * t_ * x}
    a = -r3 * u_ + f(3.0) * r3 * r * r * s_ * t_
    out["dx2"] = (a * x + (-r3 * t_) * g) + (-r3 * s_) * v
    if bf and store:
        out = {k: _rb(t) for k, t in out.items()}
    if SLOPE[act] != 1.0:
        gated = out["bwd"] * f(SLOPE[act])
        out["bwd"] = np.where(x > 0, out["bwd"], _rb(gated) if bf else gated)
    return {k: torch.from_numpy(np.ascontiguousarray(t, dtype=f)) for k, t in out.items()}


# ==== 3. minibatch stdev ===================================================================================================
# x (groups n, P): s_g = sqrt(mean_j var_j), var_j the population variance of position j over the group's n samples.
# mbstd_stats_kernel: grid (64, groups) blocks of 256; a thread walks positions block 256 + t + i 16384; per position the mean
# (n adds, eight samples per trip, one division), the variance (an fmaf chain of n, one division), added to the thread's sum;
# the block's tree (8), then every consumer folds the 64 partials in order, divides by P and takes the root.
#   var_j:   relative (n + 3) u, and through d = x - mu (mu carries (n + 1) u mean_i |x_ij|):  2 mean_i|d_ij| (n + 1) u mean_i|x_ij|
#   s^2:     + (trips + 8 + 64 + 1) u s^2, trips = ceil(P / 16384);   s: half of that relative, + u
# backward  dx_ij = k d_ij, k = ds / (P n) / s, ds = the sum of dy over the group: a thread's chain ceil(n cells / 256), the
#   tree 8:  |err ds| <= K_ds u sum|dy|;  k: + 3 roundings;  d_ij: u |d| + (n + 1) u mean|x|.
# 2nd backward, cotangent V of dx:  A = sum_ij V_ij d_ij (chain n trips, tree 8, fold 64), ddy = A / (P n) / s on every cell,
#   dx2_ij = (ds / (P n) / s) ((V_ij - Vbar_j) - (A / (P n) / s^2) d_ij).
# The bounds below are these, first order, evaluated in fp64 on the case's inputs.
MB_NEEDED = {"n=%d" % n for n in (2, 7, 8, 9, 17)} | {"groups=1", "groups=2", "groups=3", "idle_blocks", "ragged",
                                                      "position_stride", "cells=1", "cells=16", "cells=40", "fill_loop"}


def mb_tags(c):
    bf, groups, n, P, cells = c
    tags = {"n=%d" % n, "groups=%d" % groups, "cells=%d" % cells}
    if P < MB_BT:
        tags.add("idle_blocks")                                 # blocks 1..63 have no position
    if P % MB_BT:
        tags.add("ragged")
    if P > MB_B * MB_BT:
        tags.add("position_stride")
    if n * cells > MB_BT:
        tags.add("fill_loop")                                   # the fill and the dy-sum take a second trip
    if bf and P % 2 == 0 and P >= 2:
        tags.add("both_halves")                                 # idx = i P + p with P even: every row reads low and high halves
    return tags


def _mb_cases(bf):
    h = {"both_halves"} if bf else set()
    return [
        ((bf, 1, 2, 16, 1), {"n=2", "groups=1", "cells=1", "idle_blocks", "ragged"} | h),
        ((bf, 2, 7, 1000, 16), {"n=7", "groups=2", "cells=16", "ragged"} | h),
        ((bf, 3, 8, 16400, 40), {"n=8", "groups=3", "cells=40", "ragged", "position_stride", "fill_loop"} | h),
        ((bf, 1, 9, 300, 40), {"n=9", "groups=1", "cells=40", "ragged", "fill_loop"} | h),
        ((bf, 2, 17, 600, 16), {"n=17", "groups=2", "cells=16", "ragged", "fill_loop"} | h),
    ]


MB32_CASES, MBBF_CASES = _mb_cases(False), _mb_cases(True)
# the dy-sum on exact inputs: x = +1 / -1 on alternate samples (mu = 0, var = 1, s = 1 exactly), P and n powers of two, dy
# integers: dx = (sum dy) / (P n) x exactly.  (groups, n, P, cells)
MB_EXACT_CASES = [(1, 2, 16, 16), (2, 8, 512, 40), (3, 8, 32768, 40)]
# sq_mbstd_fwd_f32 (the scalar form): (N, P); min(256, ceil(P / 256)) blocks
MBSTD_SCALAR_CASES = [(2, 16), (7, 1000), (3, 256 * 256 + 9)]


def mb_inputs(c):
    bf, groups, n, P, cells = c
    g = _gen(44, *c)
    N = groups * n
    i = {"x": 0.3 + _randn(g, (N, P)), "v": _randn(g, (N, P)), "dy": _randn(g, (N, cells))}
    if bf:
        i["x"], i["v"] = i["x"].to(BF16).to(F32), i["v"].to(BF16).to(F32)
    return i


def mb_exact_inputs(c):
    groups, n, P, cells = c
    g = _gen(45, *c)
    x = torch.ones((groups * n, P))
    x[1::2] = -1.0                                              # n is even: samples alternate within every group
    return {"x": x, "dy": _ints(g, (groups * n, cells), 8)}


def mb_stat64(x, groups):
    """fp64: (s per group (groups,), d = x - mu (groups, n, P))"""
    X = x.double().reshape(groups, -1, x.shape[1])
    d = X - X.mean(1, keepdim=True)
    return torch.sqrt((d * d).mean(1).mean(1)), d


def mb_ref64(i, groups):
    """the map, its gradient and the gradient's adjoint in fp64 by automatic differentiation of the definition"""
    x = i["x"].double().requires_grad_(True)
    dy = i["dy"].double().requires_grad_(True)
    N, cells = dy.shape
    s, _ = mb_stat64(x, groups)
    y = s.reshape(groups, 1, 1).expand(groups, N // groups, cells).reshape(N, cells)
    (dx,) = torch.autograd.grad((y * dy).sum(), x, create_graph=True)
    ddy, dx2 = torch.autograd.grad((dx * i["v"].double()).sum(), (dy, x))
    return {"y": y.detach(), "dx": dx.detach(), "ddy": ddy, "dx2": dx2}


def mb_bounds(i, groups, blocks=MB_B):
    """first-order f32 bounds of y, dx, ddy, dx2 (the derivation above), fp64 tensors of the outputs' shapes.  blocks: how many
    block partials the statistic is folded from (sq_mbstd_fwd_f32, the scalar form, has min(256, ceil(P / 256)))"""
    x, v, dy = i["x"].double(), i["v"].double(), i["dy"].double()
    N, P = x.shape
    n, cells = N // groups, dy.shape[1]
    X, V = x.reshape(groups, n, P), v.reshape(groups, n, P)
    s, d = mb_stat64(x, groups)
    s = s.reshape(groups, 1, 1)
    trips = _cdiv(P, blocks * MB_BT)
    dmu = (n + 1) * U * X.abs().mean(1, keepdim=True)           # (groups, 1, P)
    dd = U * d.abs() + dmu                                      # error of d_ij
    var = (d * d).mean(1, keepdim=True)
    dvar = (n + 3) * U * var + 2 * d.abs().mean(1, keepdim=True) * dmu
    ds2 = dvar.mean(2, keepdim=True) + (trips + 8 + blocks + 1) * U * s * s
    dS = ds2 / (2 * s) + U * s                                  # error of s, (groups, 1, 1)
    out = {"y": dS.expand(groups, n, cells).reshape(N, cells)}
    k_ds = _cdiv(n * cells, MB_BT) + 8
    DY = dy.reshape(groups, -1)
    dsum, dsum_abs = DY.sum(1).reshape(groups, 1, 1), DY.abs().sum(1).reshape(groups, 1, 1)
    c = 1.0 / (P * n)
    k1 = dsum * c / s
    dk1 = k_ds * U * dsum_abs * c / s + k1.abs() * (dS / s + 3 * U)
    out["dx"] = (dk1 * d.abs() + k1.abs() * dd + U * (k1 * d).abs()).reshape(N, P)
    A = (V * d).sum((1, 2), keepdim=True)
    dA = (n * trips + 8 + MB_B) * U * (V * d).abs().sum((1, 2), keepdim=True) + (V.abs() * dd).sum((1, 2), keepdim=True)
    ddy = c * A / s
    out["ddy"] = (c * dA / s + ddy.abs() * (dS / s + 3 * U)).expand(groups, n, cells).reshape(N, cells)
    k2 = A * c / (s * s)
    dk2 = dA * c / (s * s) + k2.abs() * (2 * dS / s + 3 * U)
    w = V - V.mean(1, keepdim=True)
    dw = U * w.abs() + (n + 1) * U * V.abs().mean(1, keepdim=True)
    inner = w - k2 * d
    dinner = dw + dk2 * d.abs() + k2.abs() * dd + U * (k2 * d).abs() + U * inner.abs()
    out["dx2"] = (dk1 * inner.abs() + k1.abs() * dinner + U * (k1 * inner).abs()).reshape(N, P)
    return out


def _block_tree(t):
    """mb_block_sum / the trees of dot_per_sample_kernel along the last axis (a power of two): element 0"""
    t = t.copy()
    kk = t.shape[-1] >> 1
    while kk:
        t[..., :kk] = t[..., :kk] + t[..., kk:2 * kk]
        kk >>= 1
    return t[..., 0]


def mb_restated(i, groups, drop_position=None, drop_dy=None, bf=False):
    """mbstd_stats_kernel + mbstd_map_fill_kernel / mbstd_map_bwd_kernel / mbstd_map_bwd2_kernel in numpy float32, in the
    kernels' order: {y, dx, ddy, dx2} (bf: dx and dx2 rounded to bf16 as stored).  drop_position: that position is left out of
    the statistic and of A; drop_dy: that element of dy out of its sum."""
    f = np.float32
    x, dy = i["x"].numpy(), i["dy"].numpy()
    N, P = x.shape
    n, cells = N // groups, dy.shape[1]
    X = x.reshape(groups, n, P)
    V = i["v"].numpy().reshape(groups, n, P) if "v" in i else np.zeros_like(X)
    mu, vb = np.zeros((groups, P), f), np.zeros((groups, P), f)
    for s in range(n):
        mu = mu + X[:, s]
        vb = vb + V[:, s]
    mu, vb = mu / f(n), vb / f(n)
    T = MB_B * MB_BT
    acc, aa = np.zeros((groups, T), f), np.zeros((groups, T), f)
    for base in range(0, P, T):                                 # thread (block, t) walks positions block 256 + t + i 16384
        w = min(T, P - base)
        var = np.zeros((groups, w), f)
        keep = np.ones(w, bool)
        if drop_position is not None and base <= drop_position < base + w:
            keep[drop_position - base] = False
        for s in range(n):                                      # var and A advance together, sample by sample
            d = X[:, s, base:base + w] - mu[:, base:base + w]
            var = _fma32(d, d, var)
            aa[:, :w] = np.where(keep, _fma32(V[:, s, base:base + w], d, aa[:, :w]), aa[:, :w])
        acc[:, :w] = acc[:, :w] + np.where(keep, var / f(n), f(0.0))
    sv, A = np.zeros(groups, f), np.zeros(groups, f)
    pv, pa = _block_tree(acc.reshape(groups, MB_B, MB_BT)), _block_tree(aa.reshape(groups, MB_B, MB_BT))
    for blk in range(MB_B):                                     # mb_fold: the 64 partials in index order
        sv, A = sv + pv[:, blk], A + pa[:, blk]
    s = np.sqrt(sv / f(P))
    dyg = dy.reshape(groups, n * cells).copy()
    if drop_dy is not None:
        dyg[:, drop_dy] = 0.0
    th = np.zeros((groups, MB_BT), f)
    for base in range(0, n * cells, MB_BT):
        w = min(MB_BT, n * cells - base)
        th[:, :w] = th[:, :w] + dyg[:, base:base + w]
    ds = _block_tree(th)
    k = ds / (f(P) * f(n)) / s
    c = f(1.0) / (f(P) * f(n))
    k1, k2 = (ds * c / s)[:, None, None], (A * c / (s * s))[:, None, None]
    d = X - mu[:, None, :]
    out = {"y": np.repeat(s, n * cells).reshape(N, cells), "dx": (k[:, None, None] * d).reshape(N, P),
           "ddy": np.repeat(c * A / s, n * cells).reshape(N, cells),
           "dx2": (k1 * ((V - vb[:, None, :]) - k2 * d)).reshape(N, P)}
    if bf:
        out["dx"], out["dx2"] = _rb(out["dx"]), _rb(out["dx2"])
    return {name: torch.from_numpy(np.ascontiguousarray(t, dtype=f)) for name, t in out.items()}


# ==== 4. per-sample algebra and index maps =================================================================================
# lerp: y = al a + be b, be = fl(1 - al): t1 = al a passes its product and the sum (2), t2 = be b also be's rounding (3).
# scale: y = k x, k = s or fl(1 - s): one rounding -- a replay.  al in {0, 1}: y = a or b exactly -- a replay.
# (n elements, per-sample size); n / 4 items under the 2048-block cap
ALGEBRA_CASES = [((4 * 37, 4), {"below_256", "per_sample=4"}), ((4 * 1000, 800), {"one_trip_ragged"}),
                 ((4 * (GRID_CAP_F32 * 256 + 1234), 4 * (GRID_CAP_F32 * 256 + 1234) // 2), {"above_cap_ragged"})]
ALGEBRA_NEEDED = STREAM_NEEDED | {"per_sample=4"}
LERP_ALPHA = 0.3


def algebra_tags(c):
    n, per = c
    tags = {regime(n // 4, GRID_CAP_F32)}
    if per == 4:
        tags.add("per_sample=4")                                # i / per_sample4 changes on every item
    return tags


def algebra_inputs(c):
    n, per = c
    g = _gen(46, n, per)
    N = n // per
    return {"a": _randn(g, (N, per)), "b": _randn(g, (N, per)), "per": torch.rand((N,), generator=g, dtype=F32)}


def lerp_ref64(a, b, al):
    """al: an f32 scalar or an (N,) f32 tensor.  (exact, bound)"""
    al = (al.double().reshape(-1, 1) if isinstance(al, torch.Tensor) else float(np.float32(al)))
    t1, t2 = al * a.double(), (1.0 - al) * b.double()
    return t1 + t2, U * (2 * t1.abs() + 3 * t2.abs())


def scale_replay(x, s, one_minus):
    k = s.reshape(-1, 1) if isinstance(s, torch.Tensor) else torch.tensor(s, dtype=F32)
    if one_minus:
        k = torch.tensor(1.0, dtype=F32) - k
    return k * x


def act_replay(x, act, bf=False):
    """sq_act on the f32 value; a bf16 tensor is rounded once after it"""
    xf = x.to(F32)
    y = xf if SLOPE[act] == 1.0 else torch.where(xf > 0, xf, xf * torch.tensor(SLOPE[act], dtype=F32))
    return y.to(BF16) if bf else y


# dot_per_sample: block (slice sl, sample n) covers float4 items [per4 sl / 32, per4 (sl + 1) / 32); a thread's chain adds one
# item's ((p0 + p1) + p2) + p3 per trip: products 1, the three adds 3, the chain ceil(slice / 256), the block tree 8, the finish 32.
DOT_NEEDED = {"empty_slices", "per4%32", "N=1", "N=3", "N=70", "second_trip"}
DOT_CASES = [((1, 4 * 7), {"N=1", "empty_slices", "per4%32"}), ((3, 4 * 100), {"N=3", "per4%32"}),
             ((70, 4 * 40), {"N=70", "per4%32"}), ((3, 4 * 20001), {"N=3", "per4%32", "second_trip"})]


def dot_tags(c):
    N, per = c
    per4 = per // 4
    tags = {"N=%d" % N}
    if per4 < DOT_SLICES:
        tags.add("empty_slices")
    if per4 % DOT_SLICES:
        tags.add("per4%32")
    if _cdiv(per4, DOT_SLICES) > 256:
        tags.add("second_trip")
    return tags


def dot_k(per):
    return 1 + 3 + _cdiv(_cdiv(per // 4, DOT_SLICES), 256) + 8 + DOT_SLICES


def dot_inputs(c, exact):
    N, per = c
    g = _gen(47, N, per, exact)
    if exact:
        return _ints(g, (N, per), A_BOUND), _ints(g, (N, per), B_BOUND)
    return _randn(g, (N, per)), _randn(g, (N, per))


def dot_restated(a, b, drop_slice=None):
    """dot_per_sample_kernel + dot_finish_kernel in numpy float32, in the kernels' order"""
    f = np.float32
    A, B = a.numpy(), b.numpy()
    N, per = A.shape
    per4 = per // 4
    P = (A * B).reshape(N, per4, 4)
    item = ((P[:, :, 0] + P[:, :, 1]) + P[:, :, 2]) + P[:, :, 3]
    out = np.zeros(N, f)
    for sl in range(DOT_SLICES):
        lo, hi = per4 * sl // DOT_SLICES, per4 * (sl + 1) // DOT_SLICES
        th = np.zeros((N, 256), f)
        for base in range(lo, hi, 256):
            w = min(256, hi - base)
            th[:, :w] = th[:, :w] + item[:, base:base + w]
        kk = 128
        while kk:
            th[:, :kk] = th[:, :kk] + th[:, kk:2 * kk]
            kk >>= 1
        if sl != drop_slice:
            out = out + th[:, 0]
    return torch.from_numpy(out)


# resize_nearest (align_corners): source row = round-half-away(yo * fl((Hi - 1) / (Ho - 1))), the product in f32, clamped to Hi - 1
RESIZE_CASES = [((2, 8, 8, 4, 4, 3), {"halving", "odd_C"}), ((1, 16, 16, 8, 8, 4), {"halving"}), ((1, 32, 32, 16, 16, 1), {"halving", "odd_C"}),
                ((2, 6, 10, 4, 7, 3), {"non_square", "odd_C", "half_coordinates"}), ((1, 4, 4, 9, 9, 2), {"upsizing", "half_coordinates"}),
                ((2, 5, 7, 1, 3, 4), {"Ho=1", "non_square"}), ((1, 4, 4, 3, 3, 5), {"half_coordinates", "odd_C"}),
                ((1, 6, 6, 11, 11, 2), {"half_coordinates", "upsizing"})]
RESIZE_NEEDED = {"halving", "non_square", "upsizing", "Ho=1", "odd_C", "half_coordinates"}


def _resize_src(Hi, Ho):
    f = np.float32
    sc = f(Hi - 1) / f(Ho - 1) if Ho > 1 else f(0.0)
    v = np.arange(Ho, dtype=f) * sc                             # the f32 product
    r = np.floor(np.abs(v.astype(np.float64)) + 0.5) * np.sign(v)       # roundf: half away from zero
    return np.minimum(r.astype(np.int64), Hi - 1), v


def resize_tags(c):
    N, Hi, Wi, Ho, Wo, C = c
    tags = set()
    if Hi == 2 * Ho and Wi == 2 * Wo:
        tags.add("halving")
    if Hi != Wi or Ho != Wo:
        tags.add("non_square")
    if Ho > Hi and Wo > Wi:
        tags.add("upsizing")
    if Ho == 1:
        tags.add("Ho=1")
    if C % 2:
        tags.add("odd_C")
    if any(bool((v - np.floor(v) == 0.5).any()) for v in (_resize_src(Hi, Ho)[1], _resize_src(Wi, Wo)[1])):
        tags.add("half_coordinates")
    return tags


def resize_input(c):
    N, Hi, Wi, Ho, Wo, C = c
    return torch.arange(N * Hi * Wi * C, dtype=F32).reshape(N, Hi, Wi, C)


def resize_replay(x, Ho, Wo):
    ys, xs = _resize_src(x.shape[1], Ho)[0], _resize_src(x.shape[2], Wo)[0]
    return torch.from_numpy(np.ascontiguousarray(x.numpy()[:, ys][:, :, xs]))


def resize_loop(x, Ho, Wo):
    N, Hi, Wi, C = x.shape
    y = torch.empty((N, Ho, Wo, C))
    sy = np.float32(Hi - 1) / np.float32(Ho - 1) if Ho > 1 else np.float32(0)
    sx = np.float32(Wi - 1) / np.float32(Wo - 1) if Wo > 1 else np.float32(0)

    def rnd(t):
        t = float(t)
        return int(np.floor(t + 0.5)) if t >= 0 else -int(np.floor(-t + 0.5))
    for n in range(N):
        for i in range(Ho):
            for j in range(Wo):
                y[n, i, j] = x[n, min(rnd(np.float32(i) * sy), Hi - 1), min(rnd(np.float32(j) * sx), Wi - 1)]
    return y


# WGAN-GP losses: one block of 1024 threads.  Per sample d_i = ((-Dx + Dz) + 10 ex^2) + 0.001 Dx^2, ex = max(sqrt(gn2) - 1, 0):
# at most 8 roundings on a term, and ex carries the root's u sqrt(gn2) on top of its own: 10 (2 ex) (2 u sqrt(gn2)) on the penalty.
# The sum: a thread's chain ceil(N / 1024), the tree 10, the division 1.
WGAN_N = (1, 32, 1500)


def wgan_inputs(N):
    g = _gen(48, N)
    gn2 = (1.0 + 0.5 * _randn(g, (N,))) ** 2
    gn2[0] = 1.0
    if N > 2:
        gn2[1], gn2[2] = 0.0, 0.25
    return {"Dz": _randn(g, (N,)), "Dx": _randn(g, (N,)), "gn2": gn2}


def wgan_ref64(i, generator_only=False):
    """(d_loss, its bound, g_loss, its bound)"""
    Dz = i["Dz"].double()
    N = Dz.numel()
    ksum = _cdiv(N, MB_T) + 10 + 1
    gl, gl_b = (-Dz).mean(), (ksum + 1) * U * Dz.abs().mean()
    if generator_only:
        return None, None, gl, gl_b
    Dx, nrm = i["Dx"].double(), i["gn2"].double().sqrt()
    ex = (nrm - 1.0).clamp(min=0.0)
    k10, k001 = float(np.float32(10.0)), float(np.float32(0.001))
    pen, epsv = k10 * ex * ex, k001 * Dx * Dx
    mag = Dx.abs() + Dz.abs() + pen + epsv
    per = (8 + ksum) * U * mag + k10 * 2 * ex * 2 * U * nrm
    return (-Dx + Dz + pen + epsv).mean(), per.mean(), gl, gl_b


def wgan_bwd_ref64(i, gd, gg, generator_only=False):
    """gd, gg: upstream gradients (python floats or None = 0).  {name: (exact, bound)}"""
    Dz = i["Dz"].double()
    N = Dz.numel()
    ud = 0.0 if (gd is None or generator_only) else float(np.float32(gd)) / N
    ug = 0.0 if gg is None else float(np.float32(gg)) / N
    out = {"dDz": (torch.full((N,), ud - ug, dtype=torch.float64), torch.full((N,), 2 * U * (abs(ud) + abs(ug)), dtype=torch.float64))}
    if generator_only:
        return out
    Dx, nrm = i["Dx"].double(), i["gn2"].double().sqrt()
    ex = (nrm - 1.0).clamp(min=0.0)
    k10, k002 = float(np.float32(10.0)), float(np.float32(0.002))
    out["dDx"] = (ud * (-1.0 + k002 * Dx), 4 * U * abs(ud) * (1.0 + k002 * Dx.abs()))
    safe = torch.where(nrm > 0, nrm, torch.ones_like(nrm))
    dg = torch.where(ex > 0, ud * k10 * ex / safe, torch.zeros_like(ex))
    out["dgn2"] = (dg, torch.where(ex > 0, 5 * U * dg.abs() + abs(ud) * k10 * 3 * U, torch.zeros_like(ex)))
    return out


# mosaic: N images (H, W, C) into R x Cc cells of pitch (H + 1, W + 1); the seam row / column after every image and the cells
# past N are +0.0.  (N, H, W, C, R, Cc)
MOSAIC_CASES = [((5, 4, 4, 8, 2, 3), {"empty_cells", "non_square_grid"}), ((4, 8, 8, 4, 2, 2), set()),
                ((7, 4, 6, 12, 4, 2), {"empty_cells", "non_square_grid"})]
MOSAIC_NEEDED = {"empty_cells", "non_square_grid"}


def mosaic_tags(c):
    N, H, W, C, R, Cc = c
    return {t for t, on in (("empty_cells", R * Cc > N), ("non_square_grid", R != Cc)) if on}


def mosaic_input(c):
    N, H, W, C, R, Cc = c
    return 1.0 + torch.arange(N * H * W * C, dtype=F32).reshape(N, H, W, C)        # no zero: a zero in the mosaic is a seam


def mosaic_replay(x, R, Cc):
    N, H, W, C = x.shape
    cells = np.zeros((R * Cc, H + 1, W + 1, C), np.float32)
    cells[:N, :H, :W] = x.numpy()
    m = cells.reshape(R, Cc, H + 1, W + 1, C).transpose(0, 2, 1, 3, 4)
    return torch.from_numpy(np.ascontiguousarray(m).reshape(1, R * (H + 1), Cc * (W + 1), C))


def mosaic_loop(x, R, Cc):
    N, H, W, C = x.shape
    m = torch.zeros((1, R * (H + 1), Cc * (W + 1), C))
    for n in range(N):
        for yy in range(H):
            for xx in range(W):
                m[0, (n // Cc) * (H + 1) + yy, (n % Cc) * (W + 1) + xx] = x[n, yy, xx]
    return m


def mosaic_seam_mask(c):
    """True where the mosaic holds no image pixel"""
    N, H, W, C, R, Cc = c
    return mosaic_replay(torch.ones((N, H, W, C)), R, Cc) == 0


# head_concat: flat[p] = [float(conv[p, :C]), mb[p]]; its adjoint rounds dflat[..., :C] to bf16.  (N, P, C); npix (C + 1) items
HEAD_CONCAT_CASES = [((2, 5, 8), {"C=8", "below_256"}), ((4, 16, 40), {"C=40", "one_trip_ragged"}),
                     ((3, 16, 8), {"C=8", "one_trip_ragged"}), ((5, 5117, 40), {"C=40", "above_cap_ragged"})]
HEAD_CONCAT_NEEDED = {"C=8", "C=40"} | STREAM_NEEDED


def head_concat_tags(c):
    N, P, C = c
    return {"C=%d" % C, regime(N * P * (C + 1), GRID_CAP_BF16)}


def head_concat_inputs(c):
    N, P, C = c
    g = _gen(49, *c)
    return {"conv": _randn(g, (N, P, C)).to(BF16), "mb": _randn(g, (N, P)), "dflat": _randn(g, (N, P * (C + 1)))}


def head_concat_replay(conv, mb):
    N = conv.shape[0]
    return torch.cat([conv.to(F32), mb.unsqueeze(-1)], -1).reshape(N, -1)


def head_split_replay(dflat, N, P, C):
    d = dflat.reshape(N, P, C + 1)
    return d[..., :C].contiguous().to(BF16), d[..., C].contiguous()


# ==== 5. dense =============================================================================================================
# forward: S = ceil(K / 64) slices; part[s][m][n] an fmaf chain over the slice's k (ascending) of fl(w wscale) x; the finish has
# G = min(8, group_size(S)) groups: group g adds slices g, g + G, ... in order, an LDS tree folds the groups, + bias, activation.
#   k = 1 (w wscale) + 64 (chain) + ceil(S / G) + log2(G) + 1 (bias) + 1 (leaky)
# weight gradient: dW[k][n] = scale * chain over m of fmaf(x[m][k], dy[m][n]) (+ what dw holds with accumulate bit 0);
# db[n] = the sum over m of dy (+ db with bit 1).   k = M (chain) + 1 (scale) + 1 (accumulate)
def dense_launch(K):
    S = _cdiv(K, DK)
    return S, min(8, group_size(S))


def dense_k(K):
    S, G = dense_launch(K)
    return 1 + DK + _cdiv(S, G) + int(np.log2(G)) + 2


def dense_wgrad_k(M):
    return M + 2


def dense_tags(c):
    M, K, N, bias, act, wscale = c
    S, G = dense_launch(K)
    tags = {"M=%d" % M, "N=%d" % N, "K=%d" % K, "G=%d" % G, "act=%s" % act, "bias" if bias else "no_bias",
            "wscale=1" if wscale == 1.0 else "wscale!=1"}
    if K % DK and K % 4 == 0:
        tags.add("K%64")
    if S == 1:
        tags.add("S=1")
    return tags


DENSE_NEEDED = {"M=%d" % m for m in (1, 5, 32, 33, 96)} | {"N=%d" % n for n in (64, 260, 512)} | {
    "K=8208", "K=68", "K=300", "K%64", "S=1", "G=1", "G=2", "G=4", "G=8", "bias", "no_bias", "wscale=1", "wscale!=1"} | {
    "act=%s" % a for a in ACTS}
# (M, K, N, bias, act, wscale); S = 1, 2, 3, 5, 129
DENSE_CASES = [
    ((1, 60, 64, True, None, 1.0), {"M=1", "K=60", "N=64", "K%64", "S=1", "G=1", "bias", "act=None", "wscale=1"}),
    ((5, 68, 260, False, "relu", 0.5), {"M=5", "K=68", "N=260", "K%64", "G=2", "no_bias", "act=relu", "wscale!=1"}),
    ((32, 132, 64, True, "leaky", 0.5), {"M=32", "K=132", "N=64", "K%64", "G=2", "bias", "act=leaky", "wscale!=1"}),
    ((33, 300, 260, True, "relu", 1.0), {"M=33", "K=300", "N=260", "K%64", "G=4", "bias", "act=relu", "wscale=1"}),
    ((96, 8208, 512, True, "leaky", 0.5), {"M=96", "K=8208", "N=512", "K%64", "G=8", "bias", "act=leaky", "wscale!=1"}),
]
DENSE_BOUNDED_WSCALE = 0.37                                     # exact cases use the case's (power-of-two) scale; bounded ones this


def dense_inputs(c, exact):
    M, K, N, bias, act, wscale = c
    g = _gen(50, M, K, N, exact)
    if exact:
        return {"x": _ints(g, (M, K), A_BOUND), "w": _ints(g, (K, N), B_BOUND), "bias": _ints(g, (N,), 8) if bias else None}
    return {"x": _randn(g, (M, K)), "w": _randn(g, (K, N)), "bias": _randn(g, (N,)) if bias else None}


def dense_ref64(i, act, wscale):
    ws = (i["w"] * torch.tensor(wscale, dtype=F32)).double()
    x = i["x"].double()
    pre, terms = x @ ws, x.abs() @ ws.abs()
    if i["bias"] is not None:
        pre, terms = pre + i["bias"].double(), terms + i["bias"].double().abs()
    return act64(pre, act), terms


def dense_restated(i, act, wscale, drop_slice=None):
    """dense_partial_kernel + dense_finish_kernel in numpy float32, in the kernels' order"""
    f = np.float32
    x, w = i["x"].numpy(), i["w"].numpy() * f(wscale)
    M, K = x.shape
    N = w.shape[1]
    S, G = dense_launch(K)
    xp, wp = np.zeros((M, S * DK), f), np.zeros((S * DK, N), f)   # zero taps past K: fmaf(0, 0, acc) = acc, as in the kernel
    xp[:, :K], wp[:K] = x, w
    xp, wp = xp.reshape(M, S, DK).transpose(1, 0, 2), wp.reshape(S, DK, N)
    part = np.zeros((S, M, N), f)
    for j in range(DK):                                         # every slice's chain advances one k
        part = _fma32(xp[:, :, j, None], wp[:, j, None, :], part)
    if drop_slice is not None:
        part[drop_slice] = 0.0
    grp = np.zeros((G, M, N), f)
    for s in range(S):
        grp[s % G] = grp[s % G] + part[s]
    m = G >> 1
    while m:
        grp[:m] = grp[:m] + grp[m:2 * m]
        m >>= 1
    v = grp[0]
    if i["bias"] is not None:
        v = v + i["bias"].numpy()
    if SLOPE[act] != 1.0:
        v = np.where(v > 0, v, v * f(SLOPE[act]))
    return torch.from_numpy(v.astype(f))


def dense_wgrad_tags(c):
    M, K, N, accumulate, scale, want_db = c
    tags = {"M=%d" % M, "accumulate=%d" % accumulate, "scale=1" if scale == 1.0 else "scale!=1", "db" if want_db else "no_db"}
    if K % WK:
        tags.add("K%32")
    if N % 256:
        tags.add("N%256")
    return tags


DENSE_WGRAD_NEEDED = {"M=1", "M=5", "M=128", "K%32", "N%256", "scale=1", "scale!=1", "db", "no_db"} | {
    "accumulate=%d" % a for a in range(4)}
# (M, K, N, accumulate, scale, db wanted)
DENSE_WGRAD_CASES = [
    ((1, 33, 64, 0, 1.0, True), {"M=1", "K%32", "N%256", "accumulate=0", "scale=1", "db"}),
    ((5, 68, 260, 3, 0.5, True), {"M=5", "K%32", "N%256", "accumulate=3", "scale!=1", "db"}),
    ((128, 100, 300, 1, 0.5, True), {"M=128", "K%32", "N%256", "accumulate=1", "scale!=1", "db"}),
    ((5, 40, 64, 2, 1.0, True), {"M=5", "K%32", "N%256", "accumulate=2", "scale=1", "db"}),
    ((128, 8208, 512, 1, 0.5, False), {"M=128", "K%32", "accumulate=1", "scale!=1", "no_db"}),
]


def dense_wgrad_inputs(c, exact):
    """x, dy and what the destinations hold before the call"""
    M, K, N, accumulate, scale, want_db = c
    g = _gen(51, M, K, N, exact)
    if exact:
        return {"x": _ints(g, (M, K), A_BOUND), "dy": _ints(g, (M, N), B_BOUND), "dw0": _ints(g, (K, N), 16), "db0": _ints(g, (N,), 16)}
    return {"x": _randn(g, (M, K)), "dy": _randn(g, (M, N)), "dw0": _randn(g, (K, N)), "db0": _randn(g, (N,))}


def dense_wgrad_ref64(i, accumulate, scale):
    """(dW, sum |terms|, db, sum |terms|) with the destinations' earlier contents where accumulate says so"""
    x, dy, s = i["x"].double(), i["dy"].double(), float(np.float32(scale))
    dw, dwt = x.t() @ dy * s, x.abs().t() @ dy.abs() * abs(s)
    db, dbt = dy.sum(0), dy.abs().sum(0)
    if accumulate & 1:
        dw, dwt = dw + i["dw0"].double(), dwt + i["dw0"].double().abs()
    if accumulate & 2:
        db, dbt = db + i["db0"].double(), dbt + i["db0"].double().abs()
    return dw, dwt, db, dbt


def dense_wgrad_restated(i, accumulate, scale, drop_row=None):
    f = np.float32
    x, dy = i["x"].numpy(), i["dy"].numpy()
    M = x.shape[0]
    a = np.zeros((x.shape[1], dy.shape[1]), f)
    bs = np.zeros(dy.shape[1], f)
    for m in range(M):
        if m == drop_row:
            continue
        a = _fma32(x[m][:, None], dy[m][None, :], a)
        bs = bs + dy[m]
    v = a if scale == 1.0 else a * f(scale)
    if accumulate & 1:
        v = i["dw0"].numpy() + v
    if accumulate & 2:
        bs = i["db0"].numpy() + bs
    return torch.from_numpy(v.astype(f)), torch.from_numpy(bs.astype(f))


# ==== refusals =============================================================================================================
# (name, the operand that is wrong, its element count, what a launch sized by the well-formed operands would have covered).
# Every wrong operand is the LARGER one, or the call is refused on a property (a channel count, an alignment, a parity, M) that
# the entry point checks before any launch with all buffers at their full size; the definitions file asserts it from these
# numbers alone.
REFUSALS = [
    ("pixelnorm f32: C = 6", "x", 5 * 6, 5 * 6),
    ("pixelnorm bf16: C = 12", "x", 5 * 12, 5 * 12),
    ("pixelnorm_bwd f32: C = 6", "x", 5 * 6, 5 * 6),
    ("wgrad1x1_small f32: Cb = 6", "b", 10 * 6, 10 * 6),
    ("wgrad1x1_small bf16: C = 12", "b", 10 * 12, 10 * 12),
    ("wgrad1x1_small f32: b covers more pixels", "b", 12 * 8, 10 * 8),
    ("wgrad1x1_small bf16: a covers more pixels", "a", 12 * 2, 10 * 2),      # the bf16 entry sizes its launch by b
    ("pixelnorm f32: misaligned view", "x", 5 * 8, 5 * 8),
    ("pixelnorm bf16: misaligned view", "x", 5 * 8, 5 * 8),
    ("lerp: misaligned view", "a", 64, 64),
    ("mbstd_map bf16: odd P", "x", 4 * 7, 4 * 7),
    ("mbstd_map_bwd bf16: odd P", "x", 4 * 7, 4 * 7),
    ("dense_wgrad: M = 129", "x", 129 * 8, 129 * 8),
    ("dense: K = 6", "x", 2 * 6, 2 * 6),
]
