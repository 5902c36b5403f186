"""CPU: the stacked-oracle definitions of the 3-D ops (include/sequitr_hip.h, "Volumes"; tests/conv3d_cases.py) agree with
torch's fp64 conv3d / conv_transpose3d within f32 rounding (a small multiple of the ~1.5e-7 * sum|a*b| chain error per output), which pins the TF filter
layouts, SAME padding and the zero slices beyond the depth ends independently of the stacking trick.  And the new C entries
refuse bad calls on the host, before any launch, so this needs no GPU."""
import numpy as np
import pytest
import torch

from sequitr_amd import _lib
from tests import conv3d_cases as cc

# ~1.5e-7 * sum|a*b| is the typical error of an f32 fmaf chain; the worst of a few thousand
# outputs reaches ~1.4x that, so the bound is 3e-7 -- a layout, padding or border mistake is off by O(1) relative
U = 3e-7


def _rand(rng, shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def _t(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def _conv3d64(x, w, b=None):
    """fp64 conv3d in NDHWC / (kd,kh,kw,in,out): (value, sum |a*b| + |bias|)"""
    xt, wt = _t(x).permute(0, 4, 1, 2, 3), _t(w).permute(4, 3, 0, 1, 2)
    y = torch.nn.functional.conv3d(xt, wt, padding=1)
    s = torch.nn.functional.conv3d(xt.abs(), wt.abs(), padding=1)
    if b is not None:
        y = y + _t(b).view(1, -1, 1, 1, 1)
        s = s + _t(b).abs().view(1, -1, 1, 1, 1)
    return y.permute(0, 2, 3, 4, 1).numpy(), s.permute(0, 2, 3, 4, 1).numpy()


@pytest.mark.parametrize("N,D,H,W,Cin,Cout", [(1, 1, 5, 7, 1, 4), (2, 3, 6, 5, 2, 8), (1, 4, 9, 6, 16, 12),
                                              (2, 2, 5, 5, 32, 4)])
def test_conv3d_definition_is_torch_conv3d(N, D, H, W, Cin, Cout):
    rng = np.random.default_rng(N * 1000 + D * 100 + Cin)
    x, w, b = _rand(rng, (N, D, H, W, Cin)), _rand(rng, (3, 3, 3, Cin, Cout), 0.2), _rand(rng, (Cout,))
    got = cc.conv3d_ref(x, w, b, act=None)
    ref, s = _conv3d64(x, w, b)
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= U * s + 1e-30).all(), "max err / bound %g" % float((err / (U * s + 1e-30)).max())
    # ReLU after the bias, as in 2-D
    assert np.array_equal(cc.conv3d_ref(x, w, b, act='relu'), np.maximum(got, 0))


def test_conv3d_depth_border_is_zero_slices():
    """slices beyond the depth ends are zeros: a volume of D slices equals the middle of the same volume padded with
    zero slices on both sides"""
    rng = np.random.default_rng(5)
    x, w = _rand(rng, (1, 3, 6, 6, 16)), _rand(rng, (3, 3, 3, 16, 8), 0.2)
    xp = np.concatenate([np.zeros_like(x[:, :2]), x, np.zeros_like(x[:, :2])], axis=1)
    assert np.array_equal(cc.conv3d_ref(x, w), cc.conv3d_ref(xp, w)[:, 2:5])


@pytest.mark.parametrize("bridge", [None, 'eltwise_add', 'eltwise_mul', 'eltwise_sub'])
def test_convT3d_definition_is_torch_conv_transpose3d(bridge):
    rng = np.random.default_rng(11)
    N, D, H, W, Cin, Cout = 2, 3, 4, 5, 16, 8
    x, w, b = _rand(rng, (N, D, H, W, Cin)), _rand(rng, (2, 2, 2, Cout, Cin), 0.3), _rand(rng, (Cout,))
    skip = _rand(rng, (N, 2 * D, 2 * H, 2 * W, Cout)) if bridge else None
    got = cc.convT3d_ref(x, w, b, skip, bridge)
    xt, wt = _t(x).permute(0, 4, 1, 2, 3), _t(w).permute(4, 3, 0, 1, 2)
    up = torch.nn.functional.conv_transpose3d(xt, wt, stride=2) + _t(b).view(1, -1, 1, 1, 1)
    s = torch.nn.functional.conv_transpose3d(xt.abs(), wt.abs(), stride=2) + _t(b).abs().view(1, -1, 1, 1, 1)
    up, s = up.permute(0, 2, 3, 4, 1).numpy(), s.permute(0, 2, 3, 4, 1).numpy()
    # the bridge is one more f32 operation on the rounded upscale: compare before it where it is not the identity
    if bridge is None:
        ref, bound = up, U * s
    else:
        sk = skip.astype(np.float64)
        ref = {'eltwise_add': up + sk, 'eltwise_mul': up * sk, 'eltwise_sub': up - sk}[bridge]
        mag = {'eltwise_add': s + np.abs(sk), 'eltwise_mul': s * np.abs(sk), 'eltwise_sub': s + np.abs(sk)}[bridge]
        bound = 2 * U * mag
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= bound + 1e-30).all(), "max err / bound %g" % float((err / (bound + 1e-30)).max())


def test_maxpool3d_definition():
    rng = np.random.default_rng(2)
    x = _rand(rng, (2, 4, 6, 8, 4))
    ref = torch.nn.functional.max_pool3d(torch.from_numpy(x).permute(0, 4, 1, 2, 3), 2).permute(0, 2, 3, 4, 1).numpy()
    assert np.array_equal(cc.maxpool3d_ref(x), ref)


def test_host_side_validation_needs_no_gpu():
    lib = _lib.load()
    rc = lib.sq_conv3d_ndhwc_fwd_f32(None, None, None, None, 1, 4, 16, 16, 16, 16, 1, None)
    assert rc == -1 and b"null" in lib.sq_last_error()
    rc = lib.sq_conv3d_ndhwc_fwd_f32(16, 16, None, 16, 1, 4, 16, 16, 24, 16, 1, None)
    assert rc == -1 and b"Cin=24" in lib.sq_last_error()
    rc = lib.sq_conv3d_ndhwc_fwd_f32(16, 16, None, 16, 1, 4, 16, 16, 16, 6, 1, None)
    assert rc == -1 and b"multiple of 4" in lib.sq_last_error()
    rc = lib.sq_conv3d_ndhwc_fwd_f32(16, 16, None, 16, 1, 4, 16, 16, 16, 16, 7, None)
    assert rc == -1 and b"activation" in lib.sq_last_error()
    rc = lib.sq_maxpool2x2x2_fwd_f32(None, None, 1, 4, 16, 16, 16, None)
    assert rc == -1 and b"null" in lib.sq_last_error()
    rc = lib.sq_maxpool2x2x2_fwd_f32(16, 32, 1, 3, 16, 16, 16, None)
    assert rc == -1 and b"even" in lib.sq_last_error()
    rc = lib.sq_convT2x2x2s2_ndhwc_fwd_f32(None, None, None, None, None, 1, 2, 4, 4, 16, 16, 0, None)
    assert rc == -1 and b"null" in lib.sq_last_error()
    rc = lib.sq_convT2x2x2s2_ndhwc_fwd_f32(16, 16, None, None, 16, 1, 2, 4, 4, 12, 16, 0, None)
    assert rc == -1 and b"multiple of 16" in lib.sq_last_error()
    rc = lib.sq_convT2x2x2s2_ndhwc_fwd_f32(16, 16, None, None, 16, 1, 2, 4, 4, 16, 6, 0, None)
    assert rc == -1 and b"multiple of 4" in lib.sq_last_error()
    rc = lib.sq_convT2x2x2s2_ndhwc_fwd_f32(16, 16, None, None, 16, 1, 2, 4, 4, 16, 16, 1, None)
    assert rc == -1 and b"skip" in lib.sq_last_error()
