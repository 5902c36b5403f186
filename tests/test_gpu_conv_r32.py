"""GPU: the 32 -> 32 f32 3x3 conv with the filter held in registers (conv_r32_kernel) against the generic kernel on the same
tensors -- the same call with SQ_CONV_R32=0 (read per call), which the existing sweeps pin to the C oracle.  Every comparison is
torch.equal: the kernel keeps every output's fmaf chain.  Each case first asserts through sq_conv_r32_takes_f32 that the kernel
takes the call, so that a silent fall-back cannot make the comparison vacuous.  Outputs are written between sentinel-filled guard
bands one image row wide, and the bands are checked afterwards: a wrong store bound must not be repaired by a neighbour."""
import os
import zlib

import numpy as np
import pytest
import torch

from oracle import c_oracle as co
from sequitr_amd import _lib, ops
from sequitr_amd.networks.unet import GraphedPredict, UNet2D, init_unet_weights
from tests import conv_r32_cases as rc

pytestmark = pytest.mark.gpu

C = 32
SENTINEL = -12345.678


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


class Guarded(object):
    """an (N, H, W, C) tensor inside sentinel bands of one image row (W * C floats) each"""

    def __init__(self, N, H, W):
        self.band = W * C
        self.buf = torch.full((N * H * W * C + 2 * self.band,), SENTINEL, dtype=torch.float32, device="cuda")
        self.t = self.buf[self.band:self.band + N * H * W * C].view(N, H, W, C)

    def bands_intact(self):
        s = torch.tensor(SENTINEL, dtype=torch.float32, device="cuda")
        return bool((self.buf[:self.band] == s).all()) and bool((self.buf[-self.band:] == s).all())


def _run(x, w, b, pooled, act="relu", wscale=1.0):
    """(y, pooled or None) through the C entry points on guarded outputs; asserts the bands afterwards"""
    N, H, W, _ = x.shape
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    y = Guarded(N, H, W)
    bp = b.data_ptr() if b is not None else None
    if pooled:
        assert wscale == 1.0
        p = Guarded(N, H // 2, W // 2)
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
