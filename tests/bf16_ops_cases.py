"""Shared by the bf16 operator tests (sequitr_amd/csrc/sq_ops_bf16.hip through sequitr_amd/ops_bf16.py): CPU references and
the case tables of the GPU sweep (tests/test_gpu_bf16_ops_sweep.py), whose regime coverage
tests/test_bf16_ops_definitions.py checks without a GPU.  No HIP call, no import of the library.

EMULATIONS (torch CPU, bf16 in, bf16 out).  Every streaming kernel computes an output as: bf16 operands widened to f32, ONE
IEEE f32 operation, one round-to-nearest-even to bf16 (the gated forms: a second f32 multiply and a second rounding).  Torch
on the CPU in float32 followed by .to(bfloat16) is that arithmetic, so the GPU results must EQUAL these, compared as numbers
(+0.0 == -0.0), no tolerance.  The emulations themselves are anchored on the CPU to fp64 / torch autograd.
The pool tie rule is the kernels': the first maximum in the order (0,0), (0,1), (1,0), (1,1) wins.  The keep rate is divided
out as v * (1.0f / (1.0f - rate)), the reciprocal formed in f32.

MASK: dropout_mask() restates sq_dropout_key / sq_dropout_thr16 / sq_dropout_keep4 (sq_common.h) in numpy uint32.

fp64 DEFINITIONS for what has no replayable chain: the transpose conv (MFMA order) and the head's dW / db / loss.

Layouts: activations NHWC, transpose-conv kernel (2,2,Cout,Cin), head kernel (1,1,Cin,Cout)."""
import numpy as np
import torch

BF16 = torch.bfloat16
CAP = 2048 * 256                                                # items one trip of the capped grid covers
RATE = 0.4                                                      # the workload's dropout rate; its gate scale is 1 / 0.6
GATE = 1.0 / 0.6
SLOPE = {"relu": 0.0, "leaky": 0.2, "none": 1.0, None: 1.0}
ACTS = ("relu", "leaky", "none")
KINDS = ("eltwise_add", "eltwise_mul", "eltwise_sub")


def _s(v):
    """a scalar as the kernel holds it: f32"""
    return torch.tensor(float(v), dtype=torch.float32)


def _inv_keep(rate):
    return _s(1.0) / (_s(1.0) - _s(rate))                       # 1.0f / (1.0f - rate)


def _zero_like(t):
    return torch.zeros((), dtype=BF16).expand(t.shape)


# ---- emulations ----------------------------------------------------------------------------------------------------------
def to_bf16(x):
    return x.to(BF16)


def to_f32(x):
    return x.to(torch.float32)


def _windows(t):
    """(N,H,W,C) -> (N,H/2,W/2,C,4), last axis the window positions (0,0), (0,1), (1,0), (1,1)"""
    N, H, W, C = t.shape
    return t.reshape(N, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(N, H // 2, W // 2, C, 4)


def _unwindows(v):
    N, Ho, Wo, C, _ = v.shape
    return v.reshape(N, Ho, Wo, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(N, 2 * Ho, 2 * Wo, C).contiguous()


def _first_max(xw):
    """(max, position) per window; a later position replaces the running maximum only when strictly greater"""
    m = xw[..., 0].clone()
    k = torch.zeros(m.shape, dtype=torch.int8)
    for j in (1, 2, 3):
        gt = xw[..., j] > m
        m = torch.where(gt, xw[..., j], m)
        k = torch.where(gt, torch.tensor(j, dtype=torch.int8), k)
    return m, k


def _scatter(xw, dy):
    """f32 (N,Ho,Wo,C,4): dy at the window's first maximum, 0 elsewhere"""
    _, k = _first_max(xw)
    sel = k.unsqueeze(-1) == torch.arange(4, dtype=torch.int8)
    return torch.where(sel, dy.float().unsqueeze(-1), _s(0.0))


def maxpool(x):
    return _first_max(_windows(x.float()))[0].to(BF16)


def maxpool_bwd(x, dy):
    return _unwindows(_scatter(_windows(x.float()), dy).to(BF16))


def maxpool_bwd_add(x, dy, add, gate_scale=0.0):
    """bf16(scatter(dy) + add); gate_scale > 0: then x > 0 ? bf16(that * gate_scale) : 0"""
    xw = _windows(x.float())
    s = (_scatter(xw, dy) + _windows(add.float())).to(BF16)
    if gate_scale > 0:
        s = torch.where(xw > 0, (s.float() * _s(gate_scale)).to(BF16), _zero_like(s))
    return _unwindows(s)


def act_bwd(dy, y, act):
    if SLOPE[act] == 1.0:
        return dy
    return torch.where(y.float() > 0, dy, (dy.float() * _s(SLOPE[act])).to(BF16))


def bridge(a, b, kind):
    p, q = a.float(), b.float()
    return {"eltwise_add": p + q, "eltwise_mul": p * q, "eltwise_sub": p - q}[kind].to(BF16)


def bridge_bwd(dy, a, b, kind):
    """(d a, d b) of bridge(a, b)"""
    if kind == "eltwise_mul":
        return (dy.float() * b.float()).to(BF16), (dy.float() * a.float()).to(BF16)
    return dy, ((-dy.float()).to(BF16) if kind == "eltwise_sub" else dy)


def space_to_depth(t):
    """g[n,i,j,(2a+b)*C + c] = t[n,2i+a,2j+b,c]"""
    N, H2, W2, C = t.shape
    return t.reshape(N, H2 // 2, 2, W2 // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, H2 // 2, W2 // 2, 4 * C).contiguous()


def bridge_bwd_s2d(dy, up, skip, kind):
    """(d up in space-to-depth layout, d skip) of merged = bridge(up, skip)"""
    da, db = bridge_bwd(dy, up, skip, kind)
    return space_to_depth(da), db


def dropout_fwd(x, mask, rate):
    return torch.where(mask != 0, (x.float() * _inv_keep(rate)).to(BF16), _zero_like(x))


dropout_bwd = dropout_fwd                                       # the same expression on dy


def relu_scale_bwd(dy, y, scale):
    return torch.where(y.float() > 0, (dy.float() * _s(scale)).to(BF16), _zero_like(dy))


def act_dropout_bwd(dy, mask, y, rate, act):
    d = dropout_bwd(dy, mask, rate)                             # rounded as the stand-alone pass rounds it
    return torch.where(y.float() > 0, d, (d.float() * _s(SLOPE[act])).to(BF16))


# ---- the dropout mask, restated from the comment block of sq_common.h ----------------------------------------------------
def _u32(v):
    return np.asarray(v, dtype=np.uint64).astype(np.uint32)


def dropout_key(seed, step=None):
    """(s1, s2): the key carries (seed, step) into the hash at two places"""
    seed = _u32([int(seed) & 0xFFFFFFFF])
    if step is not None:
        seed = seed + _u32([int(step) & 0xFFFFFFFF]) * np.uint32(0x9E3779B9)
    s1 = seed * np.uint32(0x9E3779B1) + np.uint32(0x7F4A7C15)
    s2 = (seed ^ np.uint32(0x68E31DA4)) * np.uint32(0x85EBCA6B)
    s2 = s2 ^ (s2 >> np.uint32(13))
    return s1, s2


def dropout_thr16(rate):
    return np.uint32(int(np.float32(rate) * np.float32(65536.0)))


def dropout_keep4(key, q, thr16):
    """(len(q), 4) bool: element 4q + j is kept; one 32-bit hash per quad, two words = four 16-bit uniforms"""
    s1, s2 = key
    h = _u32(q) + s1
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x7FEB352D)
    h = h ^ (h >> np.uint32(15)) ^ s2
    h = h * np.uint32(0x846CA68B)
    h = h ^ (h >> np.uint32(16))
    g = (h ^ np.uint32(0x5BD1E995)) * np.uint32(0x2C1B3C6D)
    g = g ^ (g >> np.uint32(15))
    u = np.stack([h & np.uint32(0xFFFF), h >> np.uint32(16), g & np.uint32(0xFFFF), g >> np.uint32(16)], -1)
    return u >= thr16


def dropout_mask(n, rate, seed, step=None):
    """the byte mask the dropout kernels write for n elements: one byte (0 / 1) per element, quad q = elements 4q .. 4q+3"""
    assert n % 4 == 0
    keep = dropout_keep4(dropout_key(seed, step), np.arange(n // 4, dtype=np.uint64), dropout_thr16(rate))
    return keep.astype(np.uint8).reshape(-1)


def keep_probability(rate):
    return 1.0 - float(dropout_thr16(rate)) / 65536.0


# ---- fp64 definitions ----------------------------------------------------------------------------------------------------
def convT64(x, w, bias):
    """y[n,2i+a,2j+b,o] = sum_c x[n,i,j,c] * w[a,b,o,c] + bias[o] on the operands as given (bf16-rounded), in fp64"""
    y = torch.nn.functional.conv_transpose2d(x.double().permute(0, 3, 1, 2), w.double().permute(3, 2, 0, 1),
                                             None if bias is None else bias.double(), stride=2)
    return y.permute(0, 2, 3, 1).contiguous()


def head_logits64(x, w, bias):
    N, H, W, Cin = x.shape
    z = x.double().reshape(-1, Cin) @ w.double().reshape(Cin, -1)
    if bias is not None:
        z = z + bias.double()
    return z.reshape(N, H, W, -1)


def head_wgrad64(x, dz):
    """(dW (Cin,Cout), db, sum |terms| of dW, sum |terms| of db)"""
    X, G = x.double().reshape(-1, x.shape[-1]), dz.double().reshape(-1, dz.shape[-1])
    return X.T @ G, G.sum(0), X.abs().T @ G.abs(), G.abs().sum(0)


def wce64(z, onehot, wgt):
    """loss = mean_p w_p (lse(z_p) sum(y_p) - <y_p, z_p>), dz = w_p / npix (softmax(z_p) sum(y_p) - y_p)"""
    z, y = z.double(), onehot.double()
    w = wgt.double().reshape(z.shape[:-1] + (1,))
    npix = z.numel() // z.shape[-1]
    lse = torch.logsumexp(z, -1, keepdim=True)
    yt = y.sum(-1, keepdim=True)
    loss = (w * (lse * yt - (y * z).sum(-1, keepdim=True))).sum() / npix
    return loss, w / npix * (torch.exp(z - lse) * yt - y)


# ---- case tables ---------------------------------------------------------------------------------------------------------
def stream_regime(items):
    """which way a 256-thread grid-stride kernel with the grid capped at 2048 blocks walks `items`"""
    if items < 256:
        return "below_256"
    if items <= CAP:
        return "one_trip_ragged" if items % 256 else "one_trip_whole"
    return "above_cap_ragged" if items % CAP else "above_cap_whole"


STREAM_NEEDED = {"below_256", "one_trip_ragged", "above_cap_ragged"}

# flat ops: (elements, regime).  8 elements per item; the casts take 4 per item, i.e. twice the items
FLAT_CASES = [
    (8 * 37, "below_256"),
    (8 * 1000, "one_trip_ragged"),
    (8 * (CAP + 1234), "above_cap_ragged"),
]
CAST_CASES = [(4 * 61, "below_256"), (4 * 3001, "one_trip_ragged"), (4 * (CAP + 4321), "above_cap_ragged")]


def flat_regime(n, per_item=8):
    return stream_regime(n // per_item)


def spatial_tags(shape):
    """pool ops on x (N,H,W,C): one item = 8 channels of one pooled pixel"""
    N, H, W, C = shape
    tags = {stream_regime(N * (H // 2) * (W // 2) * (C // 8)), "C8=%d" % (C // 8)}
    tags |= {t for t, on in (("odd_Ho", (H // 2) % 2), ("odd_Wo", (W // 2) % 2), ("N>1", N > 1), ("H=2", H == 2),
                             ("W=2", W == 2)) if on}
    return tags


SPATIAL_NEEDED = STREAM_NEEDED | {"odd_Ho", "odd_Wo", "C8=1", "C8=2", "C8=3", "N>1", "H=2", "W=2"}
POOL_CASES = [
    ((1, 2, 2, 8), {"below_256", "H=2", "W=2", "C8=1", "odd_Ho", "odd_Wo"}),
    ((1, 2, 12, 16), {"below_256", "H=2", "C8=2"}),
    ((2, 10, 2, 8), {"below_256", "W=2", "N>1", "odd_Ho"}),
    ((3, 14, 22, 24), {"one_trip_ragged", "C8=3", "odd_Ho", "odd_Wo", "N>1"}),
    ((2, 362, 366, 64), {"above_cap_ragged", "odd_Ho", "odd_Wo", "N>1"}),     # 529 968 pooled items
]
BIG_POOL = (2, 362, 366, 64)


def s2d_tags(shape):
    """bridge_bwd_s2d on dy (N,2H,2W,C): one item = 8 channels of one HIGH-resolution pixel; H, W the low side"""
    N, H2, W2, C = shape
    tags = {stream_regime(N * H2 * W2 * (C // 8)), "C8=%d" % (C // 8)}
    tags |= {t for t, on in (("odd_Ho", (H2 // 2) % 2), ("odd_Wo", (W2 // 2) % 2), ("N>1", N > 1), ("H=2", H2 == 2),
                             ("W=2", W2 == 2)) if on}
    return tags


S2D_CASES = [
    ((1, 2, 2, 8), {"below_256", "H=2", "W=2", "C8=1", "odd_Ho", "odd_Wo"}),
    ((1, 2, 12, 16), {"below_256", "H=2", "C8=2"}),
    ((2, 10, 2, 8), {"below_256", "W=2", "N>1", "odd_Ho"}),
    ((3, 14, 22, 24), {"one_trip_ragged", "C8=3", "odd_Ho", "odd_Wo", "N>1"}),
    ((2, 182, 186, 64), {"above_cap_ragged", "odd_Ho", "odd_Wo", "N>1"}),     # 541 632 items
]

# hand-made ties, one case per window position k: x (1,2,2,8), channel c holds the maximum 2.0 at position k AND at
# TIE_PARTNER[k][c] (positive, tied), 1.0 elsewhere; channel 6 is an all-equal positive window, channel 7 all zero
TIE_PARTNER = {0: (1, 2, 3, 1, 2, 3), 1: (0, 2, 3, 0, 2, 3), 2: (0, 1, 3, 0, 1, 3), 3: (0, 1, 2, 0, 1, 2)}


def tie_case(k):
    """(x (1,2,2,8) bf16, the winning position per channel)"""
    xw = torch.ones((1, 1, 1, 8, 4))
    win = []
    for c, j in enumerate(TIE_PARTNER[k]):
        xw[0, 0, 0, c, k] = xw[0, 0, 0, c, j] = 2.0
        win.append(min(k, j))
    xw[0, 0, 0, 6] = 3.0
    xw[0, 0, 0, 7] = 0.0
    return _unwindows(xw).to(BF16), win + [0, 0]


# transpose conv: (N, H, W, Cin, Cout); P = N*H*W input pixels, a block takes 64 of them and 64 of the 4*Cout rows
CONVT_NEEDED = {"Cout=16", "Cout=32", "Cout=48", "Cout=64", "Cin=32", "Cin=96", "P<64", "P>64_ragged",
                "three_images_in_a_block", "W=1", "H=1"}
CONVT_CASES = [
    ((3, 5, 3, 32, 16), {"Cout=16", "Cin=32", "P<64", "three_images_in_a_block"}),
    ((3, 5, 3, 96, 48), {"Cout=48", "Cin=96", "P<64", "three_images_in_a_block"}),
    ((2, 9, 13, 32, 48), {"Cout=48", "Cin=32", "P>64_ragged"}),
    ((2, 9, 13, 96, 64), {"Cout=64", "Cin=96", "P>64_ragged"}),
    ((4, 7, 1, 32, 32), {"Cout=32", "Cin=32", "W=1", "P<64", "three_images_in_a_block"}),
    ((1, 1, 75, 96, 16), {"Cout=16", "Cin=96", "H=1", "P>64_ragged"}),
    ((2, 4, 8, 32, 64), {"Cout=64", "Cin=32"}),                 # P = 64: one whole block
]


def convT_tags(c):
    N, H, W, Cin, Cout = c
    P = N * H * W
    tags = {"Cout=%d" % Cout, "Cin=%d" % Cin}
    tags |= {t for t, on in (("P<64", P < 64), ("P>64_ragged", P > 64 and P % 64), ("W=1", W == 1), ("H=1", H == 1),
                             ("three_images_in_a_block", 2 * H * W < min(P, 64))) if on}
    return tags


# head: (N, H, W, Cin, Cout).  nblk = min(2048, ceil(npix / 256)) block partials, G = sq_group_size(nblk) finish lanes.
# k = f32 additions on the longest path from a term of dW / db to the output, counted from head_bwd_bf16_kernel and
# head_finish2_kernel: the per-thread fmaf loop (one per trip through the pixel loop: `trips`), wave_sum (6), the three block
# adds (3), sq_group_reduce: a lane's serial sum (ceil(nblk / G)) and its butterfly (log2 G).
#   nblk    1: trips 1, G  1: k = 1 + 6 + 3 +  1 + 0 = 11
#   nblk    5: trips 1, G  4: k = 1 + 6 + 3 +  2 + 2 = 14
#   nblk  600: trips 1, G 64: k = 1 + 6 + 3 + 10 + 6 = 26   (lanes 0..23 sum 10 partials: 8 in the 8-deep loop, run once, + 2)
#   nblk 2048: trips 2, G 64: k = 2 + 6 + 3 + 32 + 6 = 49
HEAD_K = {1: 11, 5: 14, 600: 26, 2048: 49}
HEAD_NEEDED = {"pair=%dx%d" % (ci, co) for ci in (16, 32) for co in (1, 2, 3, 4, 5)} | {
    "%s/Cin=%d" % (r, ci) for r in ("nblk=1", "nblk=5", "nblk=600", "second_trip_partial") for ci in (16, 32)}
HEAD_CASES = [((1, 9, 13, ci, co), {"pair=%dx%d" % (ci, co), "nblk=1/Cin=%d" % ci}) for ci in (16, 32) for co in (1, 2, 3, 4, 5)] + [
    ((2, 23, 25, 16, 2), {"nblk=5/Cin=16"}),
    ((2, 23, 25, 32, 3), {"nblk=5/Cin=32"}),
    ((1, 200, 767, 16, 5), {"nblk=600/Cin=16"}),
    ((1, 200, 767, 32, 4), {"nblk=600/Cin=32"}),
    ((1, 725, 724, 16, 3), {"second_trip_partial/Cin=16"}),     # 524 900 pixels: 2048 blocks, 612 pixels in a second trip
    ((1, 725, 724, 32, 2), {"second_trip_partial/Cin=32"}),
]


def head_blocks(npix):
    return min(2048, -(-npix // 256))


def group_size(nblk):
    G = 1
    while G < 64 and G * 2 <= nblk:
        G *= 2
    return G


def head_chain_adds(npix):
    """k of the table above, recomputed from the launch arithmetic"""
    nblk = head_blocks(npix)
    G = group_size(nblk)
    trips = -(-npix // (nblk * 256))
    return trips + 6 + 3 + -(-nblk // G) + int(np.log2(G))


def head_tags(c):
    N, H, W, Cin, Cout = c
    npix = N * H * W
    nblk, tags = head_blocks(npix), {"pair=%dx%d" % (Cin, Cout)}
    G = group_size(nblk)
    if nblk == 1:
        tags.add("nblk=1/Cin=%d" % Cin)
    if nblk == 5 and G == 4 and nblk % G:
        tags.add("nblk=5/Cin=%d" % Cin)
    per_lane = -(-nblk // G)
    if nblk == 600 and G == 64 and 8 <= per_lane < 16 and per_lane % 8:       # the 8-deep loop runs once and leaves a tail
        tags.add("nblk=600/Cin=%d" % Cin)
    if nblk == 2048 and 2048 * 256 < npix < 2 * 2048 * 256 and npix % 256:
        tags.add("second_trip_partial/Cin=%d" % Cin)
    return tags


# dropout masks the GPU file asks for: (rate, seed, step or None)
MASK_CASES = [(0.4, 3, None), (0.4, 3, 7), (0.4, 4, 7), (0.1, 12345, 2), (0.75, 0xDEADBEEF, 1000003), (0.0, 1, None)]
# and every (rate, seed, step) the inputs below draw a mask with: the CPU file checks the kept share of all of them
MASK_SHARE_CASES = MASK_CASES + [(RATE, 11, 5), (RATE, 21, None), (RATE, 31, None)]


# ---- inputs --------------------------------------------------------------------------------------------------------------
def _gen(*key):
    g = torch.Generator()
    g.manual_seed(abs(hash(tuple(int(k) for k in key))) % (2 ** 31))
    return g


def _randn(g, shape):
    return torch.randn(shape, generator=g, dtype=torch.float32)


def block_output(g, shape, seed):
    """what a conv block hands on in the workload: bf16 of relu(randn) through a 0.4-rate dropout (zeros where gated)"""
    n = int(np.prod(shape))
    y = torch.relu(_randn(g, shape)).to(BF16)
    mask = torch.from_numpy(dropout_mask(n, RATE, seed)).reshape(shape)
    return dropout_fwd(y, mask, RATE)


def flat_inputs(n):
    g = _gen(1, n)
    y = _randn(g, (n,)).to(BF16)
    y[::7] = 0.0                                                # exact zeros: the gates are `> 0`
    return {"dy": _randn(g, (n,)).to(BF16), "y": y, "a": _randn(g, (n,)).to(BF16), "b": _randn(g, (n,)).to(BF16),
            "mask": torch.from_numpy(dropout_mask(n, RATE, 11, 5))}


def flat_expected(i):
    """name -> expected bf16 tensor (or pair) of every flat op on flat_inputs()"""
    e = {}
    for act in ACTS:
        e["act_bwd/" + act] = act_bwd(i["dy"], i["y"], act)
        e["act_dropout_bwd/" + act] = act_dropout_bwd(i["dy"], i["mask"], i["y"], RATE, act)
    for kind in KINDS:
        e["bridge/" + kind] = bridge(i["a"], i["b"], kind)
        e["bridge_bwd/" + kind] = bridge_bwd(i["dy"], i["a"], i["b"], kind)
    e["dropout_fwd"] = dropout_fwd(i["a"], i["mask"], RATE)
    e["dropout_bwd"] = dropout_bwd(i["dy"], i["mask"], RATE)
    e["relu_scale_bwd"] = relu_scale_bwd(i["dy"], i["y"], GATE)
    return e


def pool_inputs(shape):
    N, H, W, C = shape
    g = _gen(2, *shape)
    return {"x": block_output(g, shape, 21), "dy": _randn(g, (N, H // 2, W // 2, C)).to(BF16), "add": _randn(g, shape).to(BF16)}


def pool_expected(i):
    return {"maxpool": maxpool(i["x"]), "maxpool_bwd": maxpool_bwd(i["x"], i["dy"]),
            "maxpool_bwd_add": maxpool_bwd_add(i["x"], i["dy"], i["add"]),
            "maxpool_bwd_add/gate": maxpool_bwd_add(i["x"], i["dy"], i["add"], GATE)}


def pool_input_statistics(x):
    """(share of all-zero windows, number of windows whose positive maximum is held by more than one position)"""
    xw = _windows(x.float())
    m = xw.max(-1, keepdim=True).values
    tied = ((xw == m).sum(-1) > 1) & (m[..., 0] > 0)
    return float((m == 0).float().mean()), int(tied.sum())


def s2d_inputs(shape):
    g = _gen(3, *shape)
    return {"dy": _randn(g, shape).to(BF16), "up": _randn(g, shape).to(BF16), "skip": _randn(g, shape).to(BF16)}


def convT_inputs(c):
    N, H, W, Cin, Cout = c
    g = _gen(4, *c)
    return {"x": _randn(g, (N, H, W, Cin)).to(BF16), "w": 0.2 * _randn(g, (2, 2, Cout, Cin)), "bias": 0.1 * _randn(g, (Cout,)),
            "skip": _randn(g, (N, 2 * H, 2 * W, Cout)).to(BF16)}


def convT_expected(i):
    """fp64, before the final rounding: {None: up, kind: bridge(bf16(up), skip)} -- the up-scaled value is stored as bf16
    first, as test_convT_bf16 has it"""
    up = convT64(i["x"], i["w"].to(BF16), i["bias"])
    u, s = up.to(BF16).double(), i["skip"].double()
    return {None: up, "eltwise_add": u + s, "eltwise_mul": u * s, "eltwise_sub": u - s}


def head_inputs(c):
    """x: a block output (zeros where gated), pixel 0 all zero so that its logits are the bias: bias[0] == bias[-1] is the
    largest, an exact tie the lowest index must win (without bias: all logits 0, the same).  dz is of the size the loss
    hands down (weights up to 10, divided by npix), which is what keeps the summation bound under the existing test's"""
    N, H, W, Cin, Cout = c
    g = _gen(5, *c)
    npix = N * H * W
    x = block_output(g, (N, H, W, Cin), 31)
    x[0, 0, 0] = 0.0
    bias = 0.5 * _randn(g, (Cout,)).clamp(-2, 2)
    bias[0] = bias[-1] = 2.0
    lab = torch.randint(0, Cout, (N, H, W), generator=g)
    return {"x": x, "w": 0.3 * _randn(g, (1, 1, Cin, Cout)), "bias": bias, "dz": _randn(g, (N, H, W, Cout)) * (4.0 / npix),
            "onehot": (lab.unsqueeze(-1) == torch.arange(Cout)).to(torch.uint8),
            "wgt": 1 + 9 * torch.rand((N, H, W, 1), generator=g, dtype=torch.float32), "dloss": torch.tensor(0.61)}


def head_expected(i):
    """everything the GPU file compares the head with; the chains through oracle.c_oracle (c ascending, bias added last)"""
    from oracle import c_oracle as co
    x, w, dz = i["x"], i["w"], i["dz"]
    Cin, Cout = w.shape[2], w.shape[3]
    xf = x.float().numpy()
    e = {}
    for name, b in (("bias", i["bias"]), ("nobias", None)):
        z = co.conv2d(xf, w.numpy(), None if b is None else b.numpy())
        e["logits/" + name] = torch.from_numpy(z)
        e["mask/" + name] = torch.from_numpy(co.argmax_u8(z))
        z64 = head_logits64(x, w, b)
        e["loss64/" + name], e["dz64/" + name] = wce64(z64, i["onehot"], i["wgt"])
    wt = w.reshape(Cin, Cout).t().contiguous().reshape(1, 1, Cout, Cin)       # dx[c] = chain over o of dz[o] * w[c][o]
    e["dx"] = torch.from_numpy(co.conv2d(dz.numpy(), wt.numpy())).to(BF16)
    e["dx/gate"] = relu_scale_bwd(e["dx"], x, GATE)
    e["dw64"], e["db64"], e["dw_abs"], e["db_abs"] = head_wgrad64(x, dz)
    return e
