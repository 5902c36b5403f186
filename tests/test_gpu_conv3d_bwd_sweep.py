"""GPU: the volumetric gradient kernels against their fp64 DEFINITIONS (tests/conv3d_bwd_cases.py: sums over shifted views
in numpy, never another kernel), on every plan form sq_conv3d_wgrad_plan returns (tests/test_conv3d_bwd_plan.py checks on
the CPU that the table reaches them).

Weight gradient, exact oracle: X and dY are integers in -3..3, so every product and partial sum is an integer below 2^24
(asserted in test_conv3d_bwd_plan.py) and f32 in any summation order is exact: the kernel must equal fp64 bit for bit.  dW,
db and the workspace start as NaN sentinels and sit between guard bands that must come back untouched (the workspace: past
what its query returned).

Weight gradient, rounding oracle: normal operands, |got - ref| <= 2^p * sum |x * dy| per element, p derived per case from
its plan (conv3d_bwd_cases.chain_roundings): an element's sum passes through 1 rounding of each product, then in its wave 4
pixels per MFMA step x 16 steps per tile x tpb tiles, 3 cross-wave adds in the block, ceil(gx / G) serial adds in a finish
lane and log2(G) butterfly adds; every one of those roundings is at most 2^-24 of a partial ABSOLUTE sum, and the partial
sums of disjoint waves / blocks add up to the element's absolute sum, so the error is at most count * 2^-24 * sum |x dy|.
The planar sweep's 2^-20 would need count <= 16, which the 64 accumulations of a single tile already exceed: the count is 69
to 76 for the cases whose blocks walk one tile (p = -17) and 156 / 201 for the two whose blocks walk 2 / 3 tiles (p = -16).
A truncating conversion or a bf16 operand (2^-8 relative per operand) is far outside either.  Each case runs twice:
bit-identical.

Input gradient: ops.conv3d_dgrad(dy, w) is DEFINED as the forward conv3d of dY with the transformed filter, so it equals
the stacked C oracle cc.conv3d_ref(dy, transform(w)) bit for bit.  Pool backward and space-to-depth move values: exact.
Transpose-conv backward: within 1e-5 of max |ref| (the per-kernel tolerance of test_gpu_train.py)."""
import numpy as np
import pytest
import torch

from sequitr_amd import _lib, ops
from sequitr_amd import functional as F
from sequitr_amd.ops import _ptr, _stream
from tests import conv3d_bwd_cases as bc
from tests import conv3d_cases as cc
from tests.test_gpu_wgrad_sweep import Guarded, Workspace, assert_bits, _rng, _operand
from tests.util import assert_bit_exact

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np64(t):
    return t.double().cpu().numpy()


def _run_wgrad(c, x, dy, want_bias=True):
    """one call of the C entry into guarded, NaN-filled destinations"""
    N, D, H, W, Cin, Cout = c
    lib = _lib.load()
    nbytes = lib.sq_conv3d_ndhwc_wgrad_workspace_f32(N, D, H, W, Cin, Cout)
    assert nbytes == 4 * ops.conv3d_wgrad_plan(*c)['workspace_floats']
    dw, db, wsp = Guarded(27 * Cin * Cout), (Guarded(Cout) if want_bias else None), Workspace(nbytes)
    _lib.check(lib.sq_conv3d_ndhwc_wgrad_f32(_ptr(x), _ptr(dy), dw.ptr(), db.ptr() if db is not None else None, wsp.ptr(),
                                            N, D, H, W, Cin, Cout, _stream()), "sq_conv3d_ndhwc_wgrad_f32")
    torch.cuda.synchronize()
    dw.check("dW"), wsp.check("workspace")
    if db is not None:
        db.check("db")
    return dw, db


def _operands(c, exact):
    N, D, H, W, Cin, Cout = c
    rng = _rng("conv3d_wgrad", c, exact)
    return _operand(rng, (N, D, H, W, Cin), exact), _operand(rng, (N, D, H, W, Cout), exact)


@pytest.mark.parametrize("c", bc.WGRAD_SWEEP, ids=str)
def test_wgrad_exact(c):
    x, dy = _operands(c, True)
    S, Sb = bc.wgrad64(_np64(x), _np64(dy))
    dw, db = _run_wgrad(c, x, dy)
    assert_bits(dw.t, _dev(S.astype(np.float32)), "dW %s" % (c,))
    assert_bits(db.t, _dev(Sb.astype(np.float32)), "db %s" % (c,))
    if c[1] == 1:                                               # one slice: both outer depth taps see only the border
        g = dw.t.view(3, -1)
        assert not bool(g[0].any()) and not bool(g[2].any())
    dw2, none = _run_wgrad(c, x, dy, want_bias=False)           # db = NULL
    assert none is None
    assert_bits(dw2.t, dw.t, "dW without db %s" % (c,))


@pytest.mark.parametrize("c", bc.WGRAD_SWEEP, ids=str)
def test_wgrad_rounding_and_run_to_run(c):
    x, dy = _operands(c, False)
    xn, yn = _np64(x), _np64(dy)
    S, Sb = bc.wgrad64(xn, yn)
    A, Ab = bc.wgrad64(np.abs(xn), np.abs(yn))
    p = bc.rounding_bound_log2(ops.conv3d_wgrad_plan(*c))
    assert -17 <= p <= -16
    got = [_run_wgrad(c, x, dy) for _ in range(2)]
    dw, db = got[0]
    err = np.abs(_np64(dw.t).reshape(S.shape) - S)
    tol = 2.0 ** p * A
    print("%s: bound 2^%d, worst dW error %.3g of the bound, worst db error %.3g of the bound" % (
        c, p, float((err / np.maximum(tol, 1e-300)).max()), float((np.abs(_np64(db.t) - Sb) / (2.0 ** p * Ab)).max())))
    assert (err <= tol).all(), "dW: %d elements off, worst %g of the bound" % (
        int((err > tol).sum()), float((err / np.maximum(tol, 1e-300)).max()))
    assert (np.abs(_np64(db.t) - Sb) <= 2.0 ** p * Ab).all()
    assert_bits(got[1][0].t, dw.t, "dW run to run")
    assert_bits(got[1][1].t, db.t, "db run to run")


def test_wgrad_through_ops_writes_caller_destinations():
    c = (2, 3, 17, 33, 32, 32)
    x, dy = _operands(c, True)
    S, Sb = bc.wgrad64(_np64(x), _np64(dy))
    dw, db = ops.conv3d_wgrad(x, dy)
    assert tuple(dw.shape) == (3, 3, 3, 32, 32) and tuple(db.shape) == (32,)
    assert_bits(dw, _dev(S.astype(np.float32)), "ops.conv3d_wgrad dW")
    assert_bits(db, _dev(Sb.astype(np.float32)), "ops.conv3d_wgrad db")
    flat = torch.full((27 * 32 * 32 + 32,), float('nan'), device=DEV)
    dw2, db2 = ops.conv3d_wgrad(x, dy, dw_out=flat[:27 * 32 * 32], db_out=flat[27 * 32 * 32:])
    assert dw2.data_ptr() == flat.data_ptr()
    assert_bits(flat[:27 * 32 * 32], dw, "dw_out")
    assert_bits(flat[27 * 32 * 32:], db, "db_out")
    dw3, none = ops.conv3d_wgrad(x, dy, want_bias=False)
    assert none is None
    assert_bits(dw3, dw, "want_bias=False")
    with pytest.raises(_lib.SequitrHipError):
        ops.conv3d_wgrad(torch.zeros((1, 2, 8, 8, 24), device=DEV), torch.zeros((1, 2, 8, 8, 16), device=DEV))
    with pytest.raises(_lib.SequitrHipError):
        ops.conv3d_wgrad(torch.zeros((1, 2, 8, 8, 16), device=DEV), torch.zeros((1, 2, 8, 8, 6), device=DEV))


# ---- input gradient --------------------------------------------------------------------------------------------------------
# dY channels -> dX channels (16 -> 16), (32 -> 48), (64 -> 20), then partial tiles and a 4-channel input
@pytest.mark.parametrize("N,D,H,W,Cin,Cout", [(1, 2, 16, 16, 16, 16), (2, 3, 32, 32, 48, 32), (1, 4, 24, 40, 20, 64),
                                              (2, 3, 17, 33, 16, 32), (1, 1, 20, 18, 4, 16)])
def test_dgrad_is_the_forward_conv_of_the_transformed_filter(N, D, H, W, Cin, Cout):
    rng = np.random.default_rng(N + D + H + W + Cin + Cout)
    dy = rng.standard_normal((N, D, H, W, Cout)).astype(np.float32)
    w = (rng.standard_normal((3, 3, 3, Cin, Cout)) / np.sqrt(27 * Cout)).astype(np.float32)
    wt = ops.conv3d_weight_transform(_dev(w))
    assert_bit_exact(wt.cpu().numpy(), bc.transform(w), "weight transform")
    dx = ops.conv3d_dgrad(_dev(dy), _dev(w))
    assert tuple(dx.shape) == (N, D, H, W, Cin)
    assert_bit_exact(dx.cpu().numpy(), cc.conv3d_ref(dy, bc.transform(w)), "dgrad %s" % ((N, D, H, W, Cin, Cout),))
    ref = bc.dgrad64(dy, w)                                     # and it IS the gradient: close to the fp64 definition
    assert np.abs(dx.cpu().numpy() - ref).max() <= 1e-5 * np.abs(ref).max()


def test_dgrad_refuses_what_the_forward_does_not_take():
    with pytest.raises(_lib.SequitrHipError):                   # Cin % 4 != 0
        ops.conv3d_dgrad(torch.zeros((1, 2, 8, 8, 16), device=DEV), torch.zeros((3, 3, 3, 2, 16), device=DEV))
    with pytest.raises(_lib.SequitrHipError):                   # Cout 24: not a forward input channel count
        ops.conv3d_dgrad(torch.zeros((1, 2, 8, 8, 24), device=DEV), torch.zeros((3, 3, 3, 16, 24), device=DEV))
    with pytest.raises(ValueError):
        ops.conv3d_dgrad(torch.zeros((1, 2, 8, 8, 16), device=DEV), torch.zeros((3, 3, 3, 16, 32), device=DEV))


# ---- pool backward, space-to-depth ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 2, 2, 2, 4), (2, 8, 18, 34, 16)])
def test_maxpool_backward_exact_with_ties(shape):
    rng = np.random.default_rng(shape[1] + shape[-1])
    x = rng.integers(-2, 3, shape).astype(np.float32)           # five values over eight voxels: every window has ties
    x[0, :2, :2, :2, 0] = 0.0                                   # an all-zero window
    N, D, H, W, C = shape
    dy = rng.standard_normal((N, D // 2, H // 2, W // 2, C)).astype(np.float32)
    dy[dy == 0] = 1.0
    buf, xd, dyd = Guarded(x.size), _dev(x), _dev(dy)
    _lib.check(_lib.load().sq_maxpool2x2x2_bwd_f32(_ptr(xd), _ptr(dyd), buf.ptr(), N, D, H, W, C, _stream()),
               "sq_maxpool2x2x2_bwd_f32")
    torch.cuda.synchronize()
    buf.check("dx")
    ref = bc.maxpool_bwd(x, dy)
    assert ref[0, 0, 0, 0, 0] == dy[0, 0, 0, 0, 0] and not ref[0, :2, :2, :2, 0].reshape(-1)[1:].any()
    assert_bit_exact(buf.t.view(shape).cpu().numpy(), ref, "maxpool2x2x2_bwd %s" % (shape,))
    assert_bit_exact(ops.maxpool2x2x2_bwd(_dev(x), _dev(dy)).cpu().numpy(), ref, "ops.maxpool2x2x2_bwd")
    with pytest.raises(_lib.SequitrHipError):
        ops.maxpool2x2x2_bwd(torch.zeros((1, 2, 2, 2, 6), device=DEV), torch.zeros((1, 1, 1, 1, 6), device=DEV))


@pytest.mark.parametrize("shape", [(2, 4, 6, 10, 4), (1, 2, 16, 16, 32)])
def test_space_to_depth_exact(shape):
    N, D, H, W, C = shape                                       # the SMALL side
    dy = np.random.default_rng(sum(shape)).standard_normal((N, 2 * D, 2 * H, 2 * W, C)).astype(np.float32)
    buf, dyd = Guarded(dy.size), _dev(dy)
    _lib.check(_lib.load().sq_space_to_depth2x2x2_f32(_ptr(dyd), buf.ptr(), N, D, H, W, C, _stream()),
               "sq_space_to_depth2x2x2_f32")
    torch.cuda.synchronize()
    buf.check("g")
    assert_bit_exact(buf.t.view(N, D, H, W, 8 * C).cpu().numpy(), bc.space_to_depth(dy), "space_to_depth2x2x2")
    assert_bit_exact(ops.space_to_depth2x2x2(_dev(dy)).cpu().numpy(), bc.space_to_depth(dy), "ops.space_to_depth2x2x2")


# ---- transpose-conv backward ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,H,W,Cin,Cout", [(2, 3, 5, 7, 16, 4), (1, 2, 8, 8, 64, 32)])
def test_convT_backward_vs_fp64(N, D, H, W, Cin, Cout):
    rng = np.random.default_rng(Cin + Cout + D)
    x = rng.standard_normal((N, D, H, W, Cin)).astype(np.float32)
    w = (rng.standard_normal((2, 2, 2, Cout, Cin)) / np.sqrt(Cin)).astype(np.float32)
    b = (0.1 * rng.standard_normal(Cout)).astype(np.float32)
    G = rng.standard_normal((N, 2 * D, 2 * H, 2 * W, Cout)).astype(np.float32)
    xt, wt, bt = (_dev(a).requires_grad_(True) for a in (x, w, b))
    y = F.convT2x2x2s2(xt, wt, bt)
    assert_bit_exact(y.detach().cpu().numpy(), cc.convT3d_ref(x, w, b), "convT forward on the tape")
    y.backward(_dev(G))
    dx, dw, db = bc.convT_bwd64(x, w, G)
    for name, got, ref in (("dx", xt.grad, dx), ("dw", wt.grad, dw), ("db", bt.grad, db)):
        err = np.abs(got.double().cpu().numpy() - ref).max()
        print("convT backward %s: max error %.3g of max |ref|" % (name, err / np.abs(ref).max()))
        assert tuple(got.shape) == ref.shape and err <= 1e-5 * np.abs(ref).max(), (name, err, np.abs(ref).max())
