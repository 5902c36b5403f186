"""GPU: the 32 -> 32 f32 3x3 conv with the filter held in registers (conv_r32_kernel) against the generic kernel on the same
tensors -- the same call with SQ_CONV_R32=0 (read per call), which the existing sweeps pin to the C oracle.  Every comparison is
torch.equal: the kernel keeps every output's fmaf chain.  Each case first asserts through sq_conv_r32_takes_f32 that the kernel
takes the call, so that a silent fall-back cannot make the comparison vacuous.  Outputs are written between sentinel-filled guard
bands one image row wide, and the bands are checked afterwards: a wrong store bound must not be repaired by a neighbour.
The walk sweep (rc.R32_WALKS) compares the kernel itself with the C oracle at every walk length and on degenerate tile grids."""
import os
import zlib

import numpy as np
import pytest
import torch

from oracle import c_oracle as co
from sequitr_amd import _lib, ops
from sequitr_amd.networks.unet import GraphedPredict, UNet2D, init_unet_weights
from tests import conv_r32_cases as rc
from tests.conv_packed_cases import SENTINEL, Guarded, mismatch, neighbourhoods, nonfinite_plants

pytestmark = pytest.mark.gpu

C = 32


class generic(object):
    """`with generic():` -- SQ_CONV_R32=0: the same call runs conv_mfma_f32_v2_kernel<32,3,32,0>"""

    def __enter__(self):
        self.prev = os.environ.get("SQ_CONV_R32")
        os.environ["SQ_CONV_R32"] = "0"

    def __exit__(self, *exc):
        if self.prev is None:
            del os.environ["SQ_CONV_R32"]
        else:
            os.environ["SQ_CONV_R32"] = self.prev
        return False


@pytest.fixture(autouse=True)
def _switch_unset(monkeypatch):
    monkeypatch.delenv("SQ_CONV_R32", raising=False)


def _inputs(N, H, W, bias, weights, key):
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32(repr(key).encode()))
    x = torch.randn((N, H, W, C), generator=g)                   # standard normal
    w = torch.randn((3, 3, C, C), generator=g) / float(np.sqrt(9 * C))
    if weights == "denormal":                                    # a filter at the denormal scale, negative zeros in it
        w = w * 1e-39
        w[:, :, ::3, ::5] = -0.0
    b = torch.randn((C,), generator=g) * 0.1
    if weights == "denormal":
        b = b * 1e-39                                            # outputs stay at the filter's scale: ReLU still splits them
    return x, w, (b if bias else None)


def _run(x, w, b, pooled, act="relu", wscale=1.0, into=None):
    """(y, pooled or None) through the C entry points on guarded outputs; asserts the bands afterwards.  into: the (y, pooled)
    Guarded buffers of an earlier call, written again"""
    N, H, W, _ = x.shape
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    y = into[0] if into else Guarded(N, H, W)
    bp = b.data_ptr() if b is not None else None
    if pooled:
        assert wscale == 1.0
        p = into[1] if into else Guarded(N, H // 2, W // 2)
        _lib.check(lib.sq_conv3x3_pool_fwd_f32(x.data_ptr(), w.data_ptr(), bp, y.t.data_ptr(), p.t.data_ptr(), N, H, W, C, C,
                                               ops.ACT[act], st), "sq_conv3x3_pool_fwd_f32")
    else:
        p = None
        _lib.check(lib.sq_conv2d_nhwc_fwd_f32(x.data_ptr(), w.data_ptr(), bp, y.t.data_ptr(), N, H, W, C, C, 3, float(wscale),
                                              ops.ACT[act], st), "sq_conv2d_nhwc_fwd_f32")
    torch.cuda.synchronize()
    assert y.bands_intact(), "a store outside y"
    assert p is None or p.bands_intact(), "a store outside pooled"
    assert not bool((y.t == SENTINEL).any()) and (p is None or not bool((p.t == SENTINEL).any())), "an output element never stored"
    return y.t, (p.t if p is not None else None)


_shared = {}


def _case(c):
    """inputs on the device and the generic kernel's outputs of a case, computed once and left unchanged"""
    if c not in _shared:
        x, w, b = _inputs(c.N, c.H, c.W, c.bias, c.weights, rc.case_id(c))
        d = [x.cuda(), w.cuda(), None if b is None else b.cuda()]
        with generic():
            assert rc.takes(c.N, c.H, c.W, pooled=c.pooled) == 0
            ref = _run(d[0], d[1], d[2], c.pooled)
        _shared[c] = (x, w, b, d, ref)
    return _shared[c]


@pytest.mark.parametrize("c", rc.CASES, ids=rc.case_id)
def test_bit_identical_to_the_generic_kernel(c):
    _, _, _, (x, w, b), (ry, rp) = _case(c)
    assert rc.takes(c.N, c.H, c.W, pooled=c.pooled) == 1
    assert ops.conv_r32_takes((c.N, c.H, c.W, C), (3, 3, C, C), pooled=c.pooled)
    y, p = _run(x, w, b, c.pooled)
    assert torch.equal(y, ry)
    if c.pooled:
        assert torch.equal(p, rp)
        assert torch.equal(p, torch.nn.functional.max_pool2d(y.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1))
    if c.weights == "denormal":
        yn = y.cpu().numpy()                                     # the denormal products did reach the outputs
        assert np.count_nonzero(yn.view(np.uint32) & 0x7FFFFFFF) > 0 and float(yn.max()) < 1e-37
    # ... and the wrappers take the same route
    if c.pooled:
        oy, op = ops.conv3x3_pool(x, w, b)
        assert torch.equal(oy, ry) and torch.equal(op, rp)
    else:
        assert torch.equal(ops.conv2d(x, w, b, act="relu"), ry)


def test_equals_the_c_oracle():
    c = rc.Case(2, 256, 256, False, "rand", "normal")
    xh, wh, bh, (x, w, b), _ = _case(c)
    assert rc.takes(c.N, c.H, c.W) == 1
    y, _ = _run(x, w, b, False)
    ref = co.conv2d(xh.numpy(), wh.numpy(), bh.numpy(), act="relu")
    assert np.array_equal(y.cpu().numpy().view(np.uint32), ref.view(np.uint32))


def test_ten_runs_are_equal():
    """the 16-byte store hazard of the level-0 kernel's history showed as 1 pixel in ~3000, different on every run"""
    c = rc.Case(5, 256, 272, True, "rand", "normal")
    _, _, _, (x, w, b), (ry, rp) = _case(c)
    assert rc.takes(c.N, c.H, c.W, pooled=True) == 1
    for i in range(10):
        y, p = _run(x, w, b, True)
        assert torch.equal(y, ry) and torch.equal(p, rp), "run %d" % i


@pytest.mark.parametrize("H,act,wscale", rc.FALLBACKS)
def test_fallbacks_run_the_generic_kernel(H, act, wscale):
    N, W = 2, 256
    x, w, b = (t.cuda() for t in _inputs(N, H, W, "rand", "normal", ("fallback", H, act, wscale)))
    assert rc.takes(N, H, W, act=act) == 0 or wscale != 1.0
    y, _ = _run(x, w, b, False, act=act, wscale=wscale)
    with generic():
        ry, _ = _run(x, w, b, False, act=act, wscale=wscale)
    assert torch.equal(y, ry)
    if wscale == 1.0 and H % 2 == 0:
        y, p = _run(x, w, b, True, act=act)
        with generic():
            ry, rp = _run(x, w, b, True, act=act)
        assert torch.equal(y, ry) and torch.equal(p, rp)


# ---- the walk sweep: every case of rc.R32_WALKS against the C oracle -----------------------------------------------------------
def _walk_inputs(N, H, W, bias, key):
    x, w, b = _inputs(N, H, W, bias, "normal", key)
    x[:, ::7, ::5, ::3] = -0.0                                   # negative zeros in the activations
    return x, w, b


_walks = {}


def _walk_case(c):
    """inputs on the host and on the device and the oracle's output of a case, computed once and left unchanged"""
    if c not in _walks:
        x, w, b = _walk_inputs(c.N, c.H, c.W, c.bias, rc.walk_case_id(c))
        ref = co.conv2d(x.numpy(), w.numpy(), None if b is None else b.numpy(), act="relu")
        _walks[c] = ((x.cuda(), w.cuda(), None if b is None else b.cuda()), ref)
    return _walks[c]


def _run_twice(x, w, b, pooled):
    """(y, pooled or None) of two calls in a row into the same guarded outputs, the second with the first one's bits"""
    N, H, W, _ = x.shape
    bufs = (Guarded(N, H, W), Guarded(N, H // 2, W // 2) if pooled else None)
    y, p = _run(x, w, b, pooled, into=bufs)
    first = (y.clone(), p.clone() if pooled else None)
    y, p = _run(x, w, b, pooled, into=bufs)
    assert torch.equal(y, first[0]) and (not pooled or torch.equal(p, first[1])), "the second run differs from the first"
    return y, p


def _max_pool(y):
    return torch.nn.functional.max_pool2d(y.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)


@pytest.mark.parametrize("c", rc.R32_WALKS, ids=rc.walk_case_id)
def test_walks_equal_the_c_oracle(c):
    """Bit for bit against oracle/sq_oracle.c and against the generic kernel, at the walks the table declares (checked on the CPU
    by tests/test_conv_r32_plan.py): blocks of one tile beside blocks of two, walks of three, four and five tiles -- the stores of
    a tile ride in the next tile's MFMA phase, only the last has an epilogue of its own -- every carry of the stride, tile grids
    one and two tiles wide and one tile high.  The call runs twice into the same guarded buffers."""
    (x, w, b), ref = _walk_case(c)
    assert rc.takes(c.N, c.H, c.W, pooled=c.pooled) == 1
    p = rc.walk(c.N, c.H, c.W, c.pooled)
    y, pl = _run_twice(x, w, b, c.pooled)
    msg = mismatch(y.cpu().numpy(), ref, p, c.H, c.W, bn=C)
    assert msg is None, "conv_r32_kernel against the oracle [%s]\n%s" % (rc.walk_case_id(c), msg)
    with generic():
        assert rc.takes(c.N, c.H, c.W, pooled=c.pooled) == 0
        ry, rp = _run(x, w, b, c.pooled)
    assert torch.equal(y, ry)
    if c.pooled:
        assert torch.equal(pl, _max_pool(y))
        assert torch.equal(pl, rp)


@pytest.mark.parametrize("pooled", [False, True], ids=["plain", "pool"])
def test_non_finite_activations(pooled):
    """NaN, +inf and -inf in x (nonfinite_plants: a tile's first and last pixel, halo pixels of border tiles, image corners, the
    first and the last channel) at 3 x 304 x 144 with a bias: 257 blocks, all but one of two tiles, so deferred stores and a last
    tile's epilogue both see them.  The kernel and the generic one agree: NaN at the same outputs, the same bits everywhere else.
    Both store a NaN pre-activation as +0 (fmaxf(v, 0)), so no NaN is left and every output whose neighbourhood holds a NaN is +0.
    Wherever the whole 3x3 x 32 neighbourhood is finite the output equals the oracle bit for bit.
    The oracle itself applies ReLU as v > 0.0f ? v : 0.0f: a NaN or -inf pre-activation gives +0, +inf stays +inf
    (tests/test_conv_packed_cpu.py pins that); its outputs beside non-finite inputs are not relied on here."""
    N, H, W = rc.NONFINITE_SHAPE
    assert rc.takes(N, H, W, pooled=pooled) == 1
    p = rc.walk(N, H, W, pooled)
    assert p["tmax"] >= 2
    xh, wh, bh = _walk_inputs(N, H, W, "rand", ("non-finite", N, H, W))
    for (n, yy, xx, ch, v) in nonfinite_plants(N, H, W, C):
        xh[n, yy, xx, ch] = v
    finite, has_nan = neighbourhoods(xh)
    assert 0 < int(has_nan.sum()) < int((~finite).sum()) < 200
    x, w, b = xh.cuda(), wh.cuda(), bh.cuda()
    y, pl = _run_twice(x, w, b, pooled)
    with generic():
        ry, rp = _run(x, w, b, pooled)
    nan = torch.isnan(y)
    assert torch.equal(nan, torch.isnan(ry))
    assert torch.equal(y.view(torch.int32)[~nan], ry.view(torch.int32)[~nan])
    assert not bool(nan.any())
    yh = y.cpu()
    assert bool((yh[has_nan].view(torch.int32) == 0).all()), "a NaN pre-activation not stored as +0"
    assert bool(torch.isinf(yh[~finite]).any())                   # the infinities did reach outputs
    ref = co.conv2d(xh.numpy(), wh.numpy(), bh.numpy(), act="relu")
    got = np.where(finite.numpy()[..., None], yh.numpy(), ref)
    msg = mismatch(got, ref, p, H, W, bn=C)
    assert msg is None, "outputs with a finite neighbourhood against the oracle\n%s" % msg
    if pooled:
        assert torch.equal(pl, _max_pool(y)) and torch.equal(pl, rp)


def _logits_and_mask(net, x):
    mask = net.predict(x)
    return net.logits().clone(), mask.clone()


def test_whole_net_bit_equal_with_the_switch_on_and_off():
    """The benchmark's filters on 8 tiles of 256 x 256: level 1 is 8 x 128 x 128 = 512 tiles, the smallest batch at which
    down1/conv2 + pool, up1/conv1 and up1/conv2 take the kernel.  A replayed graph equals the eager pass."""
    params = {"shape": (256, 256), "num_inputs": 1, "num_outputs": 2, "filters": (16, 32, 64, 128, 256), "bridge": "eltwise_mul",
              "device": "cuda:0", "seed": 0}
    net = UNet2D(params, "infer")
    net.load_state_dict(init_unet_weights(params, seed=0))
    assert ops.conv_r32_takes((8, 128, 128, 32), (3, 3, 32, 32)) and ops.conv_r32_takes((8, 128, 128, 32), (3, 3, 32, 32), pooled=True)
    assert not ops.conv_r32_takes((7, 128, 128, 32), (3, 3, 32, 32))
    x = torch.randn((8, 256, 256, 1), generator=torch.Generator(device="cpu").manual_seed(5)).cuda()
    lg, mk = _logits_and_mask(net, x)
    with generic():
        rl, rm = _logits_and_mask(net, x)
    assert torch.equal(lg, rl) and torch.equal(mk, rm)
    graphed = GraphedPredict(net, tuple(x.shape))
    gm, gl = graphed(x)
    assert torch.equal(gl, lg) and torch.equal(gm, mk)
