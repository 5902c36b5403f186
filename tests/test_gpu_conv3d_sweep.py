"""GPU: the 3-D ops against their stacked-oracle definitions (tests/conv3d_cases.py), bit for bit, on every plan form of
sq_conv3d_plan; outputs are written inside NaN-filled buffers whose guard bands must survive."""
import numpy as np
import pytest
import torch

from sequitr_amd import ops
from tests import conv3d_cases as cc
from tests.util import assert_bit_exact

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 64                                                   # floats of NaN on each side (16-B multiple)


def _guarded(shape):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float('nan'), dtype=torch.float32, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_intact(buf):
    b = buf.cpu().numpy()
    assert np.isnan(b[:GUARD]).all() and np.isnan(b[-GUARD:]).all(), "a kernel wrote outside its output"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("case", cc.SWEEP, ids=[str(c) for c in cc.SWEEP])
def test_conv3d_bit_exact(case):
    N, D, H, W, Cin, Cout, act = case
    rng = np.random.default_rng(sum(case[:6]))
    x = rng.standard_normal((N, D, H, W, Cin)).astype(np.float32)
    w = (rng.standard_normal((3, 3, 3, Cin, Cout)) / np.sqrt(27 * Cin)).astype(np.float32)
    b = (0.1 * rng.standard_normal(Cout)).astype(np.float32)
    buf, y = _guarded((N, D, H, W, Cout))
    ops.conv3d(_dev(x), _dev(w), _dev(b), act=act, out=y)
    torch.cuda.synchronize()
    assert_bit_exact(y.cpu().numpy(), cc.conv3d_ref(x, w, b, act=act), "conv3d %s" % (case,))
    _guards_intact(buf)
    # no bias: the chain alone
    y2 = ops.conv3d(_dev(x), _dev(w), None, act=None)
    assert_bit_exact(y2.cpu().numpy(), cc.conv3d_ref(x, w, None, act=None), "conv3d no bias %s" % (case,))


def test_conv3d_run_to_run_identical():
    rng = np.random.default_rng(3)
    x = _dev(rng.standard_normal((2, 8, 64, 64, 32)).astype(np.float32))
    w = _dev((rng.standard_normal((3, 3, 3, 32, 40)) / 30).astype(np.float32))
    a = ops.conv3d(x, w, None, act='relu').cpu().numpy()
    b = ops.conv3d(x, w, None, act='relu').cpu().numpy()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_conv3d_above_2gib_is_local_in_depth():
    """(1,130,512,512,16): input and output are above 2^31 bytes (the per-slice window addressing).  conv3d is local in
    depth: slices 126..129 of the whole volume equal slices 1..4 of the same op on x[:, 125:130], and slices 0..3 those
    of x[:, 0:5] (both sub-volumes take the flat form)."""
    assert ops.conv3d_plan(1, 130, 512, 512, 16, 16)['addressing'] == 'window'
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.randn((1, 130, 512, 512, 16), generator=g, device=DEV)
    w = torch.randn((3, 3, 3, 16, 16), generator=g, device=DEV) / 20
    b = torch.randn((16,), generator=g, device=DEV) / 10
    y = ops.conv3d(x, w, b, act='relu')
    tail = ops.conv3d(x[:, 125:130].contiguous(), w, b, act='relu')
    head = ops.conv3d(x[:, 0:5].contiguous(), w, b, act='relu')
    torch.cuda.synchronize()
    assert torch.equal(y[:, 126:130], tail[:, 1:5]) and torch.equal(y[:, 0:4], head[:, 0:4])
    del x, y, tail, head
    torch.cuda.empty_cache()


@pytest.mark.parametrize("shape", [(1, 2, 2, 2, 4), (2, 8, 18, 34, 16), (1, 4, 64, 64, 64)])
def test_maxpool2x2x2_bit_exact(shape):
    x = np.random.default_rng(len(shape) + shape[-1]).standard_normal(shape).astype(np.float32)
    N, D, H, W, C = shape
    buf, y = _guarded((N, D // 2, H // 2, W // 2, C))
    ops.maxpool2x2x2(_dev(x), out=y)
    assert_bit_exact(y.cpu().numpy(), cc.maxpool3d_ref(x), "maxpool2x2x2 %s" % (shape,))
    _guards_intact(buf)


@pytest.mark.parametrize("bridge", [None, 'eltwise_add', 'eltwise_mul', 'eltwise_sub'])
@pytest.mark.parametrize("N,D,H,W,Cin,Cout", [(2, 3, 5, 7, 16, 4), (1, 4, 16, 16, 32, 16), (1, 1, 8, 8, 64, 32)])
def test_convT2x2x2s2_bit_exact(N, D, H, W, Cin, Cout, bridge):
    rng = np.random.default_rng(Cin + Cout + D)
    x = rng.standard_normal((N, D, H, W, Cin)).astype(np.float32)
    w = (rng.standard_normal((2, 2, 2, Cout, Cin)) / np.sqrt(Cin)).astype(np.float32)
    b = (0.1 * rng.standard_normal(Cout)).astype(np.float32)
    skip = rng.standard_normal((N, 2 * D, 2 * H, 2 * W, Cout)).astype(np.float32) if bridge else None
    buf, y = _guarded((N, 2 * D, 2 * H, 2 * W, Cout))
    ops.convT2x2x2s2(_dev(x), _dev(w), _dev(b), skip=_dev(skip) if bridge else None, bridge=bridge, out=y)
    assert_bit_exact(y.cpu().numpy(), cc.convT3d_ref(x, w, b, skip, bridge), "convT3d %s" % bridge)
    _guards_intact(buf)


def test_unsupported_shapes_raise():
    from sequitr_amd._lib import SequitrHipError
    x = torch.zeros((1, 2, 8, 8, 24), device=DEV)
    with pytest.raises(SequitrHipError):
        ops.conv3d(x, torch.zeros((3, 3, 3, 24, 16), device=DEV))
    with pytest.raises(SequitrHipError):
        ops.maxpool2x2x2(torch.zeros((1, 3, 8, 8, 16), device=DEV))
    with pytest.raises(SequitrHipError):
        ops.convT2x2x2s2(torch.zeros((1, 2, 4, 4, 8), device=DEV), torch.zeros((2, 2, 2, 16, 8), device=DEV))
    with pytest.raises(ValueError, match='bias'):              # a short bias would be read past its end
        ops.convT2x2x2s2(torch.zeros((1, 2, 4, 4, 16), device=DEV), torch.zeros((2, 2, 2, 8, 16), device=DEV),
                         torch.zeros((4,), device=DEV))
