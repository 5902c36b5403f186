"""Shared by the f32 operator tests: CPU references and the case tables of the GPU sweeps (tests/test_gpu_f32_ops_sweep.py,
tests/test_gpu_bn_sweep.py), whose regime coverage and references tests/test_f32_ops_definitions.py checks without a GPU.
No HIP call, no import of the library.  The kernels are those of sequitr_amd/csrc/sq_backward_misc.hip, sq_pointwise.hip,
sq_batchnorm.hip and the loss of sq_convt_loss.hip, reached through sequitr_amd/ops.py.

REPLAYS (torch / numpy on the CPU in float32).  Every streaming kernel computes an output with one or two IEEE f32
operations in a fixed order, so the GPU results must EQUAL these, compared as numbers (+0.0 == -0.0), no tolerance.  The pool
tie rule is the kernels': the first maximum in the order (0,0), (0,1), (1,0), (1,1) wins, replaced only when strictly
greater.  The keep rate is divided out as v * (1.0f / (1.0f - rate)).  Sums of a window are ((a+b)+(d+e)).  Index maps are
written twice: as a numpy reshape / transpose (used by the sweep) and as a naive loop (the definitions file compares the two).

fp64 DEFINITIONS, with bounds counted from the code (u = 2^-24, one f32 rounding):
  axpy_ with a general alpha: one correctly rounded fmaf, |got - exact| <= u |exact|.
  Adam: ADAM_K below.   Head dW / db: head_chain_adds() below.   Loss: wce_k() below.
  BN statistics and gradients: the tolerances of tests/test_gpu_batchnorm.py.

Layouts: activations NHWC, conv kernel HWIO (K,K,Cin,Cout), head kernel (1,1,Cin,Cout)."""
import numpy as np
import torch

from tests.bf16_ops_cases import (ACTS, CAP, KINDS, RATE, SLOPE, STREAM_NEEDED, _first_max, _gen, _inv_keep, _randn, _s,
                                  _scatter, _unwindows, _windows, dropout_mask, group_size, head_wgrad64, stream_regime,
                                  wce64)

U = 2.0 ** -24
F32 = torch.float32


# ---- replays: flat ops ---------------------------------------------------------------------------------------------------
def act_bwd(dy, y, act):
    if SLOPE[act] == 1.0:
        return dy                                               # `none` hands dy itself on
    return torch.where(y > 0, dy, dy * _s(SLOPE[act]))


def bridge(a, b, kind):
    return {"eltwise_add": a + b, "eltwise_mul": a * b, "eltwise_sub": a - b}[kind]


def bridge_bwd(dy, a, b, kind):
    """(d a, d b) of bridge(a, b); a, b are read by eltwise_mul only"""
    if kind == "eltwise_mul":
        return dy * b, dy * a
    return dy, (-dy if kind == "eltwise_sub" else dy)


def dropout_fwd(x, mask, rate):
    return torch.where(mask != 0, x * _inv_keep(rate), _s(0.0))


dropout_bwd = dropout_fwd                                       # the same expression on dy


def axpy(y, x, alpha):
    """alpha in {1, 0.5, -2}: alpha * x is exact in f32, so fmaf(alpha, x, y) is the rounded sum"""
    return y + _s(alpha) * x


def axpy64(y, x, alpha):
    return float(np.float32(alpha)) * x.double() + y.double()


# ---- replays: 2x2 spatial ops --------------------------------------------------------------------------------------------
def maxpool(x):
    return _first_max(_windows(x))[0]


def _sum4(xw):
    return (xw[..., 0] + xw[..., 1]) + (xw[..., 2] + xw[..., 3])


def avgpool(x):
    return _sum4(_windows(x)) * _s(0.25)


def sumpool(x, scale):
    return _sum4(_windows(x)) * _s(scale)


def maxpool_bwd(x, dy):
    return _unwindows(_scatter(_windows(x), dy))


def upsample_nn2x(x):
    """y[n,i,j,c] = x[n,i//2,j//2,c]"""
    return torch.from_numpy(np.repeat(np.repeat(x.numpy(), 2, axis=1), 2, axis=2))


def broadcast2x2(src, scale):
    return upsample_nn2x(src * _s(scale))


def broadcast2x2_act_bwd(src, gate, scale, act):
    g = broadcast2x2(src, scale)
    return torch.where(gate > 0, g, g * _s(SLOPE[act]))


def space_to_depth2(t):
    """g[n,i,j,(2a+b)*C + c] = t[n,2i+a,2j+b,c]"""
    N, H2, W2, C = t.shape
    a = t.numpy().reshape(N, H2 // 2, 2, W2 // 2, 2, C).transpose(0, 1, 3, 2, 4, 5)
    return torch.from_numpy(np.ascontiguousarray(a).reshape(N, H2 // 2, W2 // 2, 4 * C))


def zero_insert2x(x):
    """u[n,2i+1,2j+1,:] = x[n,i,j,:], 0 elsewhere"""
    N, H, W, C = x.shape
    u = np.zeros((N, 2 * H, 2 * W, C), np.float32)
    u[:, 1::2, 1::2] = x.numpy()
    return torch.from_numpy(u)


def gather_odd2x(du):
    """dx[n,i,j,:] = du[n,2i+1,2j+1,:]"""
    return torch.from_numpy(np.ascontiguousarray(du.numpy()[:, 1::2, 1::2]))


def conv_weight_transform(w):
    """wt[ky,kx,co,ci] = w[K-1-ky,K-1-kx,ci,co]"""
    return torch.from_numpy(np.ascontiguousarray(w.numpy()[::-1, ::-1].transpose(0, 1, 3, 2)))


def argmax_u8(z):
    """the lowest index wins ties (numpy's argmax returns the first occurrence)"""
    return torch.from_numpy(np.argmax(z.numpy(), axis=-1).astype(np.uint8))


# the same index maps as naive loops over pixels (channels stay a vector); the definitions file compares them with the above
def upsample_loop(x):
    N, H, W, C = x.shape
    y = torch.empty((N, 2 * H, 2 * W, C))
    for n in range(N):
        for i in range(2 * H):
            for j in range(2 * W):
                y[n, i, j] = x[n, i // 2, j // 2]
    return y


def space_to_depth_loop(t):
    N, H2, W2, C = t.shape
    g = torch.empty((N, H2 // 2, W2 // 2, 4 * C))
    for n in range(N):
        for i in range(H2 // 2):
            for j in range(W2 // 2):
                for a in range(2):
                    for b in range(2):
                        g[n, i, j, (2 * a + b) * C:(2 * a + b + 1) * C] = t[n, 2 * i + a, 2 * j + b]
    return g


def zero_insert_loop(x):
    N, H, W, C = x.shape
    u = torch.empty((N, 2 * H, 2 * W, C))
    for n in range(N):
        for i in range(2 * H):
            for j in range(2 * W):
                u[n, i, j] = x[n, i // 2, j // 2] if (i % 2 == 1 and j % 2 == 1) else 0.0
    return u


def gather_odd_loop(du):
    N, H2, W2, C = du.shape
    dx = torch.empty((N, H2 // 2, W2 // 2, C))
    for n in range(N):
        for i in range(H2 // 2):
            for j in range(W2 // 2):
                dx[n, i, j] = du[n, 2 * i + 1, 2 * j + 1]
    return dx


def weight_transform_loop(w):
    K, _, Cin, Cout = w.shape
    wt = torch.empty((K, K, Cout, Cin))
    for ky in range(K):
        for kx in range(K):
            for co in range(Cout):
                for ci in range(Cin):
                    wt[ky, kx, co, ci] = w[K - 1 - ky, K - 1 - kx, ci, co]
    return wt


# ---- flat cases ----------------------------------------------------------------------------------------------------------
# (elements, regime); one item = one float4
FLAT_CASES = [(4 * 37, "below_256"), (4 * 1000, "one_trip_ragged"), (4 * (CAP + 1234), "above_cap_ragged")]
AXPY_ALPHAS = (1.0, 0.5, -2.0)
AXPY_GENERAL_ALPHA = 0.3


def flat_regime(n):
    return stream_regime(n // 4)


def flat_inputs(n):
    g = _gen(11, n)
    y = _randn(g, (n,))
    y[::7] = 0.0                                                # exact zeros and -0.0: the gates are `> 0`
    y[7::14] = -0.0
    return {"dy": _randn(g, (n,)), "y": y, "a": _randn(g, (n,)), "b": _randn(g, (n,)),
            "mask": torch.from_numpy(dropout_mask(n, RATE, 11, 5))}


def flat_expected(i):
    e = {}
    for act in ACTS:
        e["act_bwd/" + act] = act_bwd(i["dy"], i["y"], act)
    for kind in KINDS:
        e["bridge/" + kind] = bridge(i["a"], i["b"], kind)
        e["bridge_bwd/" + kind] = bridge_bwd(i["dy"], i["a"], i["b"], kind)
    e["dropout_fwd"] = dropout_fwd(i["a"], i["mask"], RATE)
    e["dropout_bwd"] = dropout_bwd(i["dy"], i["mask"], RATE)
    return e


# axpy_: (n, offset, tags).  offset 1: the views y[1:], x[1:] of buffers of n + 1 floats, which are not 16-byte aligned, so the
# kernel takes its scalar loop for every element.  The grid is grid_for(ceil(n / 4)); the regime is that of ceil(n / 4) items.
def axpy_tags(n, offset):
    tags = {stream_regime(-(-n // 4))}
    if offset:
        tags.add("all_scalar")
    elif n >= 4:
        tags.add("vector_body")
        if n % 4:
            tags.add("scalar_tail=%d" % (n % 4))
    if n < 4:
        tags.add("n<4")
    return tags


AXPY_NEEDED = STREAM_NEEDED | {"all_scalar", "vector_body", "scalar_tail=1", "scalar_tail=2", "scalar_tail=3", "n<4"}
AXPY_CASES = [(n, 0, axpy_tags(n, 0)) for n, _ in FLAT_CASES] + [(n - 1, 1, axpy_tags(n - 1, 1)) for n, _ in FLAT_CASES] + [
    (4 * 1000 + 1, 0, {"one_trip_ragged", "vector_body", "scalar_tail=1"}),
    (4 * 1000 + 2, 0, {"one_trip_ragged", "vector_body", "scalar_tail=2"}),
    (4 * 1000 + 3, 0, {"one_trip_ragged", "vector_body", "scalar_tail=3"}),
    (1, 0, {"below_256", "n<4"}),
    (3, 0, {"below_256", "n<4"}),
]


def axpy_inputs(n, offset):
    """(y buffer, x buffer) of n + offset floats; the operands are buffer[offset:]"""
    g = _gen(12, n, offset)
    return _randn(g, (n + offset,)), _randn(g, (n + offset,))


# ---- Adam ----------------------------------------------------------------------------------------------------------------
# adam_update (sq_backward_misc.hip), every operation an f32 rounding of relative size u:
#   gi = g * gscale                                    1
#   mi = b1 * m + (1 - b1) * gi                        terms t1 = b1 m, t2 = (1 - b1) g gscale
#        t1: its product 1, the sum 1 = 2;  t2: gi 1, its product 1, the sum 1 = 3            ->  k_m = 3
#   vi = b2 * v + ((1 - b2) * gi) * gi                 terms t1 = b2 v, t2 = (1 - b2) (g gscale)^2
#        t1: 2;  t2: gi enters twice 2, two products 2, the sum 1 = 5                         ->  k_v = 5
#   p  = p - lr_t * mi / (sqrt(vi) + eps)              on the STORED mi, vi (f32), terms p and q = lr_t mi / (sqrt(vi) + eps)
#        q: lr_t * mi 1, sqrt 1, + eps 1, the division 1 = 4; the difference 1 on both terms  ->  k_p = 5
# 1 - b1 and 1 - b2 are exact in f32 (Sterbenz: 0.5 <= b <= 1).  The compiler may contract a product and the sum that follows
# into one fma, which removes a rounding; the counts are for the looser, uncontracted case.  Division and square root are
# correctly rounded (the build passes no fast-math flag).
# adam_step forms lr_t on the host in double and rounds it once; numpy's pow may differ from the C library's in the last
# double bit, so its lr_t may be one f32 ulp (2 u) from ours: 2 more on q for that form alone.  The device forms store their
# lr_t in state[1], which the reference reads back after checking it to one f32 ulp.
ADAM_K = {"m": 3, "v": 5, "p": 5}
ADAM_HOST_LR_SLACK = 2
LR, B1, B2, EPS, GSCALE = 1e-3, 0.9, 0.999, 1e-8, 0.37
ADAM_CASES = [(37, "below_256"), (1000, "one_trip_ragged"), (CAP + 1234, "above_cap_ragged")]      # one item = one element
ADAM_MULTI_COUNTS = (1, 2047, 2048, 2049, 3 * 2048 + 5, 300)   # sq_adam_multi_chunk() = 2048 elements per block
ADAM_WARMUPS, ADAM_STEPS = (0, 3), (1, 2, 3, 4, 5)


def adam_multi_tags(n, chunk=2048):
    tags = {"chunks=%d" % min(-(-n // chunk), 2)}
    if n % chunk:
        tags.add("last_chunk_partial")
    if n % chunk == 0:
        tags.add("last_chunk_whole")
    if n < 256:
        tags.add("below_one_sweep")
    return tags


ADAM_MULTI_NEEDED = {"chunks=1", "chunks=2", "last_chunk_partial", "last_chunk_whole", "below_one_sweep"}


def adam_inputs(n, key=0):
    g = _gen(13, n, key)
    return {"p": _randn(g, (n,)), "g": _randn(g, (n,)), "m": 0.1 * _randn(g, (n,)), "v": 1e-3 * _randn(g, (n,)) ** 2}


def adam_lr_t(step, warmup=0, lr=LR, b1=B1, b2=B2):
    """adam_prepare_kernel / sq_adam_step_f32 in Python doubles on the f32 arguments"""
    lr, b1, b2 = float(np.float32(lr)), float(np.float32(b1)), float(np.float32(b2))
    ramp = step / warmup if (warmup > 0 and step < warmup) else 1.0
    return lr * ramp * np.sqrt(1.0 - b2 ** step) / (1.0 - b1 ** step)


def adam_ref(i, got_m, got_v, lr_t, b1=B1, b2=B2, eps=EPS, gscale=GSCALE):
    """fp64 on the f32 state: {name: (reference, sum |terms|)}; p's path starts at the stored got_m, got_v"""
    b1, b2, eps, gs = (float(np.float32(t)) for t in (b1, b2, eps, gscale))
    p, g, m, v = (i[k].double() for k in ("p", "g", "m", "v"))
    gi = g * gs
    m1, m2 = b1 * m, (1.0 - b1) * gi
    v1, v2 = b2 * v, (1.0 - b2) * gi * gi
    q = float(lr_t) * got_m.double() / (got_v.double().sqrt() + eps)
    return {"m": (m1 + m2, m1.abs() + m2.abs()), "v": (v1 + v2, v1 + v2), "p": (p - q, p.abs() + q.abs()), "q": q.abs()}


def adam_f32(i, lr_t, b1=B1, b2=B2, eps=EPS, gscale=GSCALE):
    """adam_update restated in numpy float32, no contraction: (p, m, v)"""
    f = np.float32
    p, g, m, v = (i[k].numpy() for k in ("p", "g", "m", "v"))
    gi = g * f(gscale)
    mi = f(b1) * m + (f(1.0) - f(b1)) * gi
    vi = f(b2) * v + (f(1.0) - f(b2)) * gi * gi
    pn = p - f(lr_t) * mi / (np.sqrt(vi) + f(eps))
    return torch.from_numpy(pn), torch.from_numpy(mi), torch.from_numpy(vi)


def adam_check(what, got, i, lr_t, host_lr=False):
    """asserts |got - ref| <= k u sum |terms| for m, v, p (got = (p, m, v) CPU tensors); returns the worst fractions"""
    gp, gm, gv = got
    r = adam_ref(i, gm, gv, lr_t)
    worst = {}
    for name, g in (("m", gm), ("v", gv), ("p", gp)):
        ref, terms = r[name]
        tol = ADAM_K[name] * U * terms
        if name == "p" and host_lr:
            tol = tol + ADAM_HOST_LR_SLACK * U * r["q"]
        err = (g.double() - ref).abs()
        worst[name] = float((err / tol.clamp(min=1e-300)).max())
        assert bool((err <= tol).all()), "%s: %s has %d elements past %d u sum |terms|, worst %.3f of the bound" % (
            what, name, int((err > tol).sum()), ADAM_K[name], worst[name])
    return worst


# ---- 2x2 spatial cases ---------------------------------------------------------------------------------------------------
# one item = one float4.  Which side of the shape a kernel counts its items on differs by operator:
#   "pooled": N (H/2) (W/2) C4 -- maxpool, avgpool, maxpool_bwd, sumpool (x = the shape);  gather_odd2x (du = the shape)
#   "full"  : N H W C4         -- broadcast2x2, broadcast2x2_act_bwd, upsample_nn2x, zero_insert2x (OUTPUT = the shape),
#                                 space_to_depth2 (dy = the shape)
def spatial_items(shape, side):
    N, H, W, C = shape
    return N * (H // 2) * (W // 2) * (C // 4) if side == "pooled" else N * H * W * (C // 4)


def spatial_tags(shape, side="pooled"):
    N, H, W, C = shape
    tags = {stream_regime(spatial_items(shape, side)), "C4=%d" % (C // 4)}
    tags |= {t for t, on in (("odd_Ho", (H // 2) % 2), ("odd_Wo", (W // 2) % 2), ("N>1", N > 1), ("H=2", H == 2),
                             ("W=2", W == 2)) if on}
    return tags


SPATIAL_NEEDED = STREAM_NEEDED | {"odd_Ho", "odd_Wo", "C4=1", "C4=2", "C4=3", "N>1", "H=2", "W=2"}
SPATIAL_CASES = [
    ((1, 2, 2, 4), {"below_256", "H=2", "W=2", "C4=1", "odd_Ho", "odd_Wo"}),
    ((1, 2, 12, 8), {"below_256", "H=2", "C4=2", "odd_Ho"}),
    ((2, 10, 2, 4), {"below_256", "W=2", "N>1", "odd_Ho", "odd_Wo", "C4=1"}),
    ((3, 14, 22, 12), {"one_trip_ragged", "C4=3", "odd_Ho", "odd_Wo", "N>1"}),
    ((2, 362, 366, 32), {"above_cap_ragged", "C4=8", "odd_Ho", "odd_Wo", "N>1"}),    # 529 968 pooled items
]
BIG_SPATIAL = (2, 362, 366, 32)
SUMPOOL_SCALES = (1.0, 0.25, 4.0)


def large_side(shape):
    """the (N,H,W,C) the up-sampling operators WRITE: x's shape is their small side in the small cases, their large side
    in the big one (whose doubled form would be four times the size limit)"""
    N, H, W, C = shape
    return shape if shape == BIG_SPATIAL else (N, 2 * H, 2 * W, C)


def small_side(shape):
    N, H, W, C = large_side(shape)
    return (N, H // 2, W // 2, C)


def spatial_inputs(shape):
    """x, gate: the shape; dy: the pooled shape; small / large: the operands of the up-sampling operators and their adjoints"""
    N, H, W, C = shape
    g = _gen(14, *shape)
    x = _randn(g, shape)
    gate = _randn(g, shape)
    gate.view(-1)[::7] = 0.0
    gate.view(-1)[7::14] = -0.0
    return {"x": x, "gate": gate, "dy": _randn(g, (N, H // 2, W // 2, C)), "small": _randn(g, small_side(shape)),
            "large": _randn(g, large_side(shape))}


# the scalar path of broadcast2x2 / sumpool2x2: C % 4 != 0, or C % 4 == 0 on a view that is not 16-byte aligned
SCALAR_PATH_C = (1, 2, 3, 6)
SCALAR_PATH_SHAPE = (2, 6, 10)                                  # + (C,)
MISALIGNED_C = 8                                                # on a view that starts one float into a larger buffer


def pool_window_case(kind):
    """x (1,2,2,4) for the max-pool edge cases, and the winning position per channel"""
    if kind == "signed_zeros":                                  # +0.0 == -0.0: nothing is strictly greater, position 0 wins
        xw = torch.tensor([[0.0, -0.0, 0.0, -0.0], [-0.0, 0.0, 0.0, -0.0], [-0.0, -0.0, -0.0, 0.0], [0.0, 0.0, -0.0, -0.0]])
    else:                                                       # all equal, negative
        xw = torch.full((4, 4), -1.5)
    return _unwindows(xw.reshape(1, 1, 1, 4, 4)), [0, 0, 0, 0]


# conv_weight_transform: (K, Cin, Cout); one item = one element
def wt_tags(c):
    K, Cin, Cout = c
    return {stream_regime(K * K * Cin * Cout), "K=%d" % K}


WT_NEEDED = {"K=1", "K=2", "K=3", "below_256", "one_trip_ragged", "above_cap_ragged"}
WT_CASES = [((K, ci, co), wt_tags((K, ci, co))) for K in (1, 2, 3) for ci, co in ((4, 8), (3, 5), (16, 32))] + [
    ((3, 256, 256), {"K=3", "above_cap_ragged"})]              # 589 824 elements


def wt_input(c):
    K, Cin, Cout = c
    return torch.arange(K * K * Cin * Cout, dtype=F32).reshape(K, K, Cin, Cout)    # distinct, exact in f32 (< 2^24)


# ---- head backward -------------------------------------------------------------------------------------------------------
# (N, H, W, Cin, Cout).  nblk = min(512, ceil(npix / 256)) block partials (head_blocks of sq_backward_misc.hip), G =
# sq_group_size(nblk) finish lanes.  k = f32 additions on the longest path from a term of dW / db to the output, counted from
# head_bwd_kernel and head_finish_kernel as bf16_ops_cases.HEAD_K counts them: the per-thread fmaf (one per trip through the
# pixel loop), wave_sum (6), the three block adds (3), sq_group_reduce: a lane's serial sum (ceil(nblk / G)), its butterfly
# (log2 G).
#   nblk   1: trips 1, G  1: k = 1 + 6 + 3 + 1 + 0 = 11
#   nblk   5: trips 1, G  4: k = 1 + 6 + 3 + 2 + 2 = 14
#   nblk 300: trips 1, G 64: k = 1 + 6 + 3 + 5 + 6 = 21   (no lane reaches the 8-deep loop: g + 7 * 64 >= 300)
#   nblk 500: trips 1, G 64: k = 1 + 6 + 3 + 8 + 6 = 24   (lanes 0..51 run the 8-deep loop once, lanes 52..63 the tail 7 times)
#   nblk 512: trips 2, G 64: k = 2 + 6 + 3 + 8 + 6 = 25   (131 684 pixels: 612 of them in a second trip)
HEAD_CAP = 512
HEAD_K = {1: 11, 5: 14, 300: 21, 500: 24, 512: 25}
HEAD_REGIMES = ("nblk=1", "nblk=5", "nblk=300", "nblk=500", "second_trip_partial")
HEAD_NEEDED = {"pair=%dx%d" % (ci, co) for ci in (8, 16, 32) for co in (1, 2, 3, 4)} | set(HEAD_REGIMES)
HEAD_CASES = [((1, 9, 13, ci, co), {"pair=%dx%d" % (ci, co), "nblk=1"}) for ci in (8, 16, 32) for co in (1, 2, 3, 4)] + [
    ((2, 23, 25, 16, 2), {"pair=16x2", "nblk=5"}),
    ((2, 23, 25, 32, 3), {"pair=32x3", "nblk=5"}),
    ((1, 260, 295, 8, 4), {"pair=8x4", "nblk=300"}),
    ((1, 260, 295, 32, 1), {"pair=32x1", "nblk=300"}),
    ((1, 100, 1279, 16, 3), {"pair=16x3", "nblk=500"}),
    ((1, 4, 32921, 8, 2), {"pair=8x2", "second_trip_partial"}),
    ((1, 4, 32921, 32, 4), {"pair=32x4", "second_trip_partial"}),
]


def head_blocks(npix):
    return min(HEAD_CAP, -(-npix // 256))


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
    per_lane = -(-nblk // G)
    if nblk == 1:
        tags.add("nblk=1")
    if nblk == 5 and G == 4 and nblk % G:
        tags.add("nblk=5")
    if nblk == 300 and G == 64 and 63 + 7 * G >= nblk and 0 + 7 * G >= nblk:           # no lane enters the 8-deep loop
        tags.add("nblk=300")
    if nblk == 500 and G == 64 and 0 + 7 * G < nblk <= 63 + 7 * G and per_lane == 8:   # some lanes enter it, some do not
        tags.add("nblk=500")
    if nblk == HEAD_CAP and HEAD_CAP * 256 < npix < 2 * HEAD_CAP * 256 and npix % 256:
        tags.add("second_trip_partial")
    return tags


def head_inputs(c):
    """the recipe of bf16_ops_cases.head_inputs in f32: x a block output (relu, then a 0.4-rate dropout: zeros where gated),
    dz of the size the loss hands down (weights up to 10, divided by npix)"""
    N, H, W, Cin, Cout = c
    g = _gen(15, *c)
    npix = N * H * W
    x = torch.relu(_randn(g, (N, H, W, Cin)))
    x = dropout_fwd(x, torch.from_numpy(dropout_mask(x.numel(), RATE, 31)).reshape(x.shape), RATE)
    return {"x": x, "w": 0.3 * _randn(g, (1, 1, Cin, Cout)), "dz": _randn(g, (N, H, W, Cout)) * (4.0 / npix)}


def head_expected(i):
    """dx: the fmaf chain over o ascending through oracle.c_oracle.conv2d on the transposed filter; dW / db: fp64"""
    from oracle import c_oracle as co
    x, w, dz = i["x"], i["w"], i["dz"]
    Cin, Cout = w.shape[2], w.shape[3]
    wt = w.reshape(Cin, Cout).t().contiguous().reshape(1, 1, Cout, Cin)       # dx[c] = chain over o of dz[o] * w[c][o]
    e = {"dx": torch.from_numpy(co.conv2d(dz.numpy(), wt.numpy()))}
    e["dw64"], e["db64"], e["dw_abs"], e["db_abs"] = head_wgrad64(x, dz)
    return e


def _fma32(a, b, c):
    """fmaf on float32 arrays: the product of two f32 is exact in fp64; the fp64 sum is rounded once more to f32 (a double
    rounding differs from fmaf only when the fp64 sum lands on an f32 tie, and then by less than u)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _butterfly(v, width):
    """lane 0 of `v += shfl_xor(v, m)` for m = width/2 .. 1 along axis 0 (every lane holds the same tree)"""
    lanes = np.arange(width)
    m = width >> 1
    while m:
        v = v + v[lanes ^ m]
        m >>= 1
    return v[0]


def head_wgrad_f32(i):
    """head_bwd_kernel + head_finish_kernel restated in numpy float32, in the kernel's own order: (dW (Cin,Cout), db)"""
    x, dz = i["x"].numpy(), i["dz"].numpy()
    Cin, Cout = x.shape[-1], dz.shape[-1]
    X, G = x.reshape(-1, Cin), dz.reshape(-1, Cout)
    npix = X.shape[0]
    nblk = head_blocks(npix)
    stride = nblk * 256
    gw = np.zeros((stride, Cin, Cout), np.float32)
    gb = np.zeros((stride, Cout), np.float32)
    for base in range(0, npix, stride):                         # one trip of the grid: thread t of block b holds pixel b*256+t
        n = min(stride, npix - base)
        gw[:n] = _fma32(X[base:base + n, :, None], G[base:base + n, None, :], gw[:n])
        gb[:n] = gb[:n] + G[base:base + n]
    vals = np.concatenate([gw.reshape(stride, -1), gb], 1).reshape(nblk, 4, 64, -1)      # [block][wave][lane][value]
    wave = _butterfly(np.ascontiguousarray(vals.transpose(2, 0, 1, 3)), 64)              # wave_sum: (nblk, 4, NVAL)
    part = ((wave[:, 0] + wave[:, 1]) + wave[:, 2]) + wave[:, 3]                        # (nblk, NVAL)
    Gs = group_size(nblk)
    lanes = np.zeros((Gs, part.shape[1]), np.float32)
    for b in range(nblk):                                       # lane g sums partials g, g + G, ... in order
        lanes[b % Gs] = lanes[b % Gs] + part[b]
    out = _butterfly(lanes, Gs)
    return torch.from_numpy(out[:Cin * Cout].reshape(Cin, Cout)), torch.from_numpy(out[Cin * Cout:])


# ---- loss ----------------------------------------------------------------------------------------------------------------
# (C, npix, kind); the grid is min(2048, ceil(npix / 256)) blocks of 256 pixels, i.e. stream_regime(npix)
# sq_wce_pixel, roundings that scale with the logits (the extreme case): lse = m + logf(s) 1, lse * yt 1, the dot chain C, the
# subtraction 1, the product with w 1  ->  k = C + 4
def wce_k(C):
    return C + 4


LOSS_C = (1, 2, 3, 5, 8)
LOSS_NEEDED = STREAM_NEEDED | {"C=%d" % c for c in LOSS_C} | {"extreme", "zero_rows"}
LOSS_CASES = [((C, npix, "plain"), {"C=%d" % C, stream_regime(npix), "zero_rows"}) for C in LOSS_C for npix in (37, 1000)] + [
    ((2, CAP + 1234, "plain"), {"C=2", "above_cap_ragged", "zero_rows"}),
    ((3, 1000, "extreme"), {"C=3", "one_trip_ragged", "zero_rows", "extreme"}),
]
LOSS_GRAD_SCALES = (1.0, 0.37)


def loss_inputs(c):
    """logits 4 randn (extreme: 60 randn clamped to +-80), labels with all-zero one-hot rows (class C), weights in [1, 10]"""
    C, npix, kind = c
    g = _gen(16, C, npix, kind == "extreme")
    z = 4.0 * _randn(g, (npix, C))
    if kind == "extreme":
        z = (15.0 * z).clamp(-80.0, 80.0)
    lab = torch.randint(0, C + 1, (npix,), generator=g)
    lab[:3] = torch.tensor([C, 0, C])[:3]
    return {"z": z, "onehot": (lab.unsqueeze(-1) == torch.arange(C)).to(torch.uint8),
            "wgt": 1 + 9 * torch.rand((npix, 1), generator=g, dtype=F32)}


def loss_tags(c):
    C, npix, kind = c
    i = loss_inputs(c)
    tags = {"C=%d" % C, stream_regime(npix)}
    if bool((i["onehot"].sum(-1) == 0).any()):
        tags.add("zero_rows")
    if kind == "extreme" and float(i["z"].abs().max()) == 80.0 and float(i["z"].abs().median()) > 20.0:
        tags.add("extreme")
    return tags


def loss_bounds(c, i, grad_scale=1.0):
    """(fp64 loss, its tolerance, fp64 dz at grad_scale, its tolerance): tests/test_gpu_ops.py::test_wsoftmax_ce_loss_and_grad's
    1e-6 relative and 2e-6 max|w| / npix |grad_scale|; the extreme case adds k u mean_p(w_p sum(y_p) max_c |z_pc|)"""
    C, npix, kind = c
    l64, dz64 = wce64(i["z"], i["onehot"], i["wgt"])
    tol = 1e-6 * abs(float(l64))
    if kind == "extreme":
        scale = i["wgt"].double().reshape(-1) * i["onehot"].double().sum(-1) * i["z"].double().abs().max(-1).values
        tol += wce_k(C) * U * float(scale.mean())
    return float(l64), tol, dz64 * grad_scale, 2e-6 * float(i["wgt"].max()) / npix * abs(grad_scale)


def wce_f32(i, grad_scale=1.0):
    """sq_wce_pixel + the fp64 accumulation restated in numpy float32: (loss, dz)"""
    f = np.float32
    z, y, w = i["z"].numpy(), i["onehot"].numpy().astype(np.float32), i["wgt"].numpy().reshape(-1)
    npix, C = z.shape
    m = z.max(-1)
    yt, dot, s = np.zeros(npix, f), np.zeros(npix, f), np.zeros(npix, f)
    for c in range(C):
        yt = yt + y[:, c]
        dot = _fma32(y[:, c], z[:, c], dot)
    for c in range(C):
        s = s + np.exp(z[:, c] - m)
    ls = np.log(s)
    lse = m + ls
    g = w * (f(grad_scale) / f(npix))
    dz = g[:, None] * (np.exp((z - m[:, None]) - ls[:, None]) * yt[:, None] - y)     # the softmax as exp((z - m) - log s)
    per_pixel = w * (lse * yt - dot)
    return float(per_pixel.astype(np.float64).sum() / npix), torch.from_numpy(dz.astype(f))


# ---- batch normalisation -------------------------------------------------------------------------------------------------
# (N, H, W, C).  bn_reduce_kernel: cg = C / 4 threads per pixel, rows = 256 // cg pixels per block and pass, the grid is
# min(1024, ceil(npix / rows)) (bn_grid); bn_apply / bn_bwd_apply: one quad per thread, min(4096, ceil(npix cg / 256)) blocks
# (stream_grid).
BN_EPS = 1e-3
BN_CONST = 1.25                                                 # channel 0: n * 1.25 and n * 1.25^2 are exact in fp64, so the
#                                                                 kernel's q / n - m * m is exactly 0
BN_MEAN, BN_STD = 100.0, 0.5                                    # channel 1: the cancellation case of E[x^2] - m^2
BN_VAR_SPARE = 4.0                                              # the restated kernel keeps the variance tolerance with this factor
#                                                                 to spare at BN_MEAN = 100 (test_f32_ops_definitions.py), so the
#                                                                 planted mean did not have to be lowered


def bn_tags(shape):
    N, H, W, C = shape
    npix, cg = N * H * W, C // 4
    rows = 256 // cg
    nb = -(-npix // rows)
    tags = {"C=%d" % C}
    tags |= {t for t, on in (
        ("fewer_pixels_than_rows", npix < rows), ("idle_threads", 256 % cg != 0), ("one_row_per_block", rows == 1),
        ("bn_grid_capped", nb > 1024), ("bn_grid_capped_ragged", nb > 1024 and npix % (1024 * rows) != 0),
        ("stream_grid_capped", -(-npix * cg // 256) > 4096), ("reduce_five_trips", -(-npix // (1024 * rows)) == 5),
        ("npix=1", npix == 1)) if on}
    return tags


BN_NEEDED = {"C=4", "C=12", "C=48", "C=256", "C=1024", "C=8", "fewer_pixels_than_rows", "idle_threads", "one_row_per_block",
             "bn_grid_capped", "bn_grid_capped_ragged", "stream_grid_capped", "reduce_five_trips", "npix=1"}
BN_CASES = [
    ((1, 1, 7, 4), {"C=4", "fewer_pixels_than_rows"}),
    ((3, 9, 7, 12), {"C=12", "idle_threads"}),
    ((3, 9, 7, 48), {"C=48", "idle_threads"}),
    ((1, 50, 100, 256), {"C=256", "bn_grid_capped", "bn_grid_capped_ragged"}),                      # 5000 pixels, 4 per block
    ((1, 30, 50, 1024), {"C=1024", "one_row_per_block", "bn_grid_capped", "bn_grid_capped_ragged"}),  # 1500 pixels
    ((1, 600, 1000, 8), {"C=8", "bn_grid_capped", "bn_grid_capped_ragged", "stream_grid_capped", "reduce_five_trips"}),
    ((1, 1, 1, 16), {"C=16", "npix=1", "fewer_pixels_than_rows"}),
]
BN_MOVING_NPIX = (1, 100)


def bn_inputs(shape):
    N, H, W, C = shape
    g = _gen(17, *shape)
    x = 1.7 * _randn(g, shape) + 0.3
    x[..., 0] = BN_CONST
    x[..., 1] = BN_MEAN + BN_STD * _randn(g, (N, H, W))
    return {"x": x, "dy": _randn(g, shape), "gamma": 1 + 0.3 * _randn(g, (C,)), "beta": _randn(g, (C,))}


def bn_stats64(x):
    """two-pass fp64: (mean, population variance)"""
    X = x.double().reshape(-1, x.shape[-1])
    mu = X.mean(0)
    return mu, ((X - mu) ** 2).mean(0)


def bn_stats_restated(x):
    """bn_reduce_kernel<false> + bn_stats_finish_kernel in numpy, in the kernel's order: per-thread fp64 sums over the thread's
    pixels (row + k * grid * rows), the block's rows in order, the blocks in order, then q / n - m * m clamped at 0"""
    C = x.shape[-1]
    X = x.numpy().reshape(-1, C)
    npix, cg = X.shape[0], C // 4
    rows = 256 // cg
    nblk = min(1024, -(-npix // rows))
    span = nblk * rows
    s = np.zeros((span, C))
    q = np.zeros((span, C))
    for base in range(0, npix, span):                           # thread (block b, row r) holds pixel b * rows + r of each pass
        n = min(span, npix - base)
        v = X[base:base + n].astype(np.float64)
        s[:n] += v
        q[:n] += v * v
    s, q = s.reshape(nblk, rows, C), q.reshape(nblk, rows, C)
    ps, pq = np.zeros((nblk, C)), np.zeros((nblk, C))
    for r in range(rows):
        ps += s[:, r]
        pq += q[:, r]
    S, Q = np.zeros(C), np.zeros(C)
    for b in range(nblk):
        S += ps[b]
        Q += pq[b]
    m = S / npix
    v = Q / npix - m * m
    return m.astype(np.float32), np.where(v > 0, v, 0.0).astype(np.float32), v


def bn_dact(dy, y, act, dtype=torch.float64):
    """d = act'(.) dy in `dtype`, decided from the activation OUTPUT y as the kernels do (bn_dact of sq_batchnorm.hip): a
    pre-activation within rounding of zero then gates the reference the way it gates the kernel"""
    d = dy.to(dtype)
    if SLOPE[act] == 1.0:
        return d
    return torch.where(y.float() > 0, d, d * torch.tensor(SLOPE[act], dtype=dtype))


def bn_bwd64(x, d, gamma, eps=BN_EPS):
    """(dx, dgamma, dbeta) of gamma * (x - mu) / sqrt(var + eps) + beta with batch statistics, upstream gradient d, in fp64
    closed form (the definitions file checks it against autograd)"""
    C = x.shape[-1]
    X, D = x.double().reshape(-1, C), d.double().reshape(-1, C)
    mu, var = bn_stats64(x)
    r = 1.0 / torch.sqrt(var + eps)
    xh = (X - mu) * r
    dbeta, dgamma = D.sum(0), (D * xh).sum(0)
    dx = gamma.double() * r * (D - (dbeta + xh * dgamma) / X.shape[0])
    return dx.reshape(x.shape), dgamma, dbeta


def bn_bwd_f32(x, d, mean, var, gamma, eps=BN_EPS):
    """bn_reduce_kernel<true> (fp64 sums of f32 terms) + bn_bwd_apply_kernel restated in numpy float32; d = bn_dact(...) as f32"""
    f = np.float32
    C = x.shape[-1]
    X, D = x.numpy().reshape(-1, C), d.numpy().reshape(-1, C)
    mean, var, gamma = mean.numpy(), var.numpy(), gamma.numpy()
    r = f(1.0) / np.sqrt(var + f(eps))
    xh = (X - mean) * r
    dbeta = D.astype(np.float64).sum(0).astype(f)
    dgamma = (D * xh).astype(np.float64).sum(0).astype(f)
    inv_m = f(1.0 / X.shape[0])
    dx = gamma * r * (D - (dbeta + xh * dgamma) * inv_m)
    return torch.from_numpy(dx.reshape(x.shape)), torch.from_numpy(dgamma), torch.from_numpy(dbeta)


def grad_close(got, ref, what):
    """the gradient tolerance of tests/test_gpu_batchnorm.py: max |got - ref| <= 2e-5 max |ref| + 1e-6; returns the fraction used"""
    err = float((got.double() - ref).abs().max())
    tol = 2e-5 * float(ref.abs().max()) + 1e-6
    assert err <= tol, "%s: max error %.3g past %.3g" % (what, err, tol)
    return err / tol


def bn_moving_ref(mm, mv, mean, var, npix, momentum):
    """tf.layers.batch_normalization: moving -= (moving - batch) * (1 - momentum), the batch variance unbiased by n / (n - 1)
    (1 at npix = 1); fp64"""
    unbias = npix / (npix - 1.0) if npix > 1 else 1.0
    k = 1.0 - float(np.float32(momentum))
    return mm.double() - (mm.double() - mean.double()) * k, mv.double() - (mv.double() - var.double() * unbias) * k


# ---- refusals ------------------------------------------------------------------------------------------------------------
# one entry per host-side hole that sequitr_amd/ops.py now closes: (name, the operand that is wrong, its element count or
# shape, what the launch would have covered).  EVERY mismatched operand is the larger one, so that if a check were missing the
# launch that followed would still stay inside every buffer; the definitions file asserts it from these numbers alone.
REFUSAL_N = 64                                                  # elements of the well-formed operands of the flat cases
REFUSAL_SHAPE = (2, 4, 4, 8)
HOLES = [
    ("bridge_bwd: a longer", "a", REFUSAL_N + 4, REFUSAL_N),
    ("bridge_bwd: b float64", "b", REFUSAL_N * 2, REFUSAL_N),                # float64, equal element count: twice the bytes
    ("maxpool2x2_bwd: dy oversize", "dy", 2 * 3 * 2 * 8, 2 * 2 * 2 * 8),     # (2,3,2,8) against (2,2,2,8)
    ("dropout_fwd: mask longer", "mask", REFUSAL_N + 4, REFUSAL_N),
    ("dropout_bwd: mask longer", "mask", REFUSAL_N + 4, REFUSAL_N),
    ("space_to_depth2: odd H", "dy", 2 * 5 * 4 * 8, 2 * 4 * 4 * 8),          # floored: the launch reads (2,4,4,8) of (2,5,4,8)
    ("space_to_depth2: odd W", "dy", 2 * 4 * 5 * 8, 2 * 4 * 4 * 8),
    ("gather_odd2x: odd H", "du", 2 * 5 * 4 * 8, 2 * 4 * 4 * 8),
    ("gather_odd2x: odd W", "du", 2 * 4 * 5 * 8, 2 * 4 * 4 * 8),
    ("conv1x1_small_bwd: w (1,1,16,2) for Cin 8", "w", 16 * 2, 8 * 2),
    ("conv1x1_small_bwd: dz with 4 channels for Cout 2", "dz", 2 * 4 * 4 * 4, 2 * 4 * 4 * 2),
    ("adam_step_dev: g longer", "g", REFUSAL_N + 4, REFUSAL_N),
    ("adam_step_dev: m longer", "m", REFUSAL_N + 4, REFUSAL_N),
    ("adam_apply_dev: v longer", "v", REFUSAL_N + 4, REFUSAL_N),
    ("bn_apply: scale longer", "scale", 12, 8),
    ("bn_apply: shift longer", "shift", 12, 8),
    ("bn_bwd: mean longer", "mean", 12, 8),
    ("bn_bwd: var longer", "var", 12, 8),
    ("bn_bwd: gamma longer", "gamma", 12, 8),
    ("bn_bwd: dy oversize", "dy", 2 * 5 * 4 * 8, 2 * 4 * 4 * 8),
    ("bn_bwd: y oversize", "y", 2 * 5 * 4 * 8, 2 * 4 * 4 * 8),
]
