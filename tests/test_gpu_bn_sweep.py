"""GPU: the batch-normalisation kernels of sequitr_amd/csrc/sq_batchnorm.hip, f32 through sequitr_amd.ops and bf16 through
sequitr_amd.ops_bf16, at every launch regime of tests/f32_ops_cases.py's BN_CASES: fewer pixels than a block has rows, channel
group counts that leave threads idle (C = 12, 48), one pixel row per block (C = 1024), the 1024-block cap of the reduction
with a ragged last trip, five trips, the 4096-block cap of the streaming kernels, and a single pixel.

Statistics: two-pass fp64, mean rtol 2e-7 / atol 1e-8, variance rtol 1e-6 / atol 1e-9 (tests/test_gpu_batchnorm.py); the
planted constant channel's variance is exactly 0 and its mean exact; channel 1 (mean 100, std 0.5) is the cancellation case.
Fold and apply: bit for bit against oracle.c_oracle.  Backward: fp64 closed form of the batch-statistics layer (checked
against autograd on the CPU), the activation gated by the SAME output y the kernel reads; 2e-5 max|ref| + 1e-6.
bf16 operands: the comparisons of test_bn_bf16_* (statistics as above on the rounded values, apply / dx within one bf16 ulp
of fp64 with 97 % / 95 % bit-identical)."""
import numpy as np
import pytest
import torch

from oracle import c_oracle as co
from sequitr_amd import ops
from sequitr_amd import ops_bf16 as ob
from tests import f32_ops_cases as fc
from tests.test_gpu_bf16_ops_sweep import dev, same

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
BN_IDS = [str(s) for s, _ in fc.BN_CASES]
BN_SHAPES = [s for s, _ in fc.BN_CASES]
ACTS = (None, "relu", "leaky")


def _stats_close(mean, var, x, what):
    mu, v64 = fc.bn_stats64(x)
    m, v = mean.double().cpu(), var.double().cpu()
    merr = ((m - mu).abs() / (2e-7 * mu.abs() + 1e-8)).max()
    verr = ((v - v64).abs() / (1e-6 * v64.abs() + 1e-9)).max()
    print("%s: worst mean error %.3f, worst variance error %.3f of the tolerance" % (what, float(merr), float(verr)))
    assert float(merr) <= 1.0, "%s: mean" % what
    assert float(verr) <= 1.0, "%s: variance" % what
    assert bool((var >= 0).all()), "%s: a negative variance" % what


def _cpu_forward(x, gamma, beta, act):
    """(mean, var, scale, shift, y) of the layer from oracle.c_oracle, which the GPU forward equals bit for bit"""
    mean, var = co.bn_stats(x.numpy())
    scale, shift = co.bn_fold(gamma.numpy(), beta.numpy(), mean, var, fc.BN_EPS)
    return tuple(torch.from_numpy(t) for t in (mean, var, scale, shift, co.bn_apply(x.numpy(), scale, shift, act)))


@pytest.mark.parametrize("shape", BN_SHAPES, ids=BN_IDS)
def test_bn_statistics_fold_apply(shape):
    i = fc.bn_inputs(shape)
    x = i["x"]
    mean, var = ops.bn_stats(dev(x))
    _stats_close(mean, var, x, "bn_stats %s" % (shape,))
    assert float(var[0]) == 0.0 and float(mean[0]) == fc.BN_CONST, "the constant channel: variance exactly 0, mean exact"
    rmean, rvar = co.bn_stats(x.numpy())
    rscale, rshift = co.bn_fold(i["gamma"].numpy(), i["beta"].numpy(), rmean, rvar, fc.BN_EPS)
    scale, shift = ops.bn_fold(dev(i["gamma"]), dev(i["beta"]), dev(torch.from_numpy(rmean)), dev(torch.from_numpy(rvar)), fc.BN_EPS)
    same(scale, torch.from_numpy(rscale), "bn_fold scale %s" % (shape,))
    same(shift, torch.from_numpy(rshift), "bn_fold shift %s" % (shape,))
    for act in ACTS:
        y = ops.bn_apply(dev(x), scale, shift, act)
        same(y, torch.from_numpy(co.bn_apply(x.numpy(), rscale, rshift, act)), "bn_apply %s %s" % (act, shape))


@pytest.mark.parametrize("shape", BN_SHAPES, ids=BN_IDS)
def test_bn_backward(shape):
    i = fc.bn_inputs(shape)
    x, dy, gamma = i["x"], i["dy"], i["gamma"]
    xd, dyd, gd = dev(x), dev(dy), dev(gamma)
    for act in ACTS:
        mean, var, scale, shift, y = _cpu_forward(x, gamma, i["beta"], act)
        dx64, dg64, db64 = fc.bn_bwd64(x, fc.bn_dact(dy, y, act), gamma)
        dx, dgamma, dbeta = ops.bn_bwd(xd, dyd, dev(y), act, dev(mean), dev(var), gd, fc.BN_EPS)
        fr = [fc.grad_close(got.cpu(), ref, "bn_bwd %s %s: %s" % (shape, act, name))
              for got, ref, name in ((dx, dx64, "dx"), (dgamma, dg64, "dgamma"), (dbeta, db64, "dbeta"))]
        print("bn_bwd %s %s: dx %.3f, dgamma %.3f, dbeta %.3f of the tolerance" % (shape, act, fr[0], fr[1], fr[2]))
        if act is None:                                         # y is not read then
            again = ops.bn_bwd(xd, dyd, None, None, dev(mean), dev(var), gd, fc.BN_EPS)
            for a, b in zip(again, (dx, dgamma, dbeta)):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "bn_bwd without y, a second call"


@pytest.mark.parametrize("npix", fc.BN_MOVING_NPIX)
def test_bn_moving_update(npix):
    g = fc._gen(19, npix)
    mm, mv = fc._randn(g, (48,)), 1 + torch.rand((48,), generator=g)
    m, v = fc._randn(g, (48,)), torch.rand((48,), generator=g)
    dm, dv = dev(mm), dev(mv)
    ops.bn_update_moving_(dm, dv, dev(m), dev(v), npix=npix, momentum=0.99)
    rm, rv = fc.bn_moving_ref(mm, mv, m, v, npix, 0.99)
    assert np.allclose(dm.cpu().numpy(), rm.numpy(), rtol=1e-6, atol=1e-7)
    assert np.allclose(dv.cpu().numpy(), rv.numpy(), rtol=1e-6, atol=1e-7)
    biased = (mv.double() - (mv.double() - v.double()) * (1.0 - float(np.float32(0.99)))).numpy()
    assert np.allclose(rv.numpy(), biased, rtol=1e-6, atol=1e-7) == (npix == 1)     # the unbias factor is 1 at npix = 1 only


# ---- the same kernels on bf16 operands -------------------------------------------------------------------------------------
def _within_one_bf16_ulp(got, ref64, what, min_same):
    g = got.float().cpu().double()
    r = ref64.to(BF16).double()
    bad = (g - ref64).abs() > torch.clamp(r.abs(), min=1e-30) * 2.0 ** -7 + 1e-6
    assert not bool(bad.any()), "%s: %d values off by more than one bf16 ulp, first at flat index %d" % (
        what, int(bad.sum()), int(bad.reshape(-1).nonzero()[0]))
    share = float((g == r).double().mean())
    assert share > min_same, "%s: only %.4f bit-identical" % (what, share)
    return share


@pytest.mark.parametrize("shape", BN_SHAPES, ids=BN_IDS)
def test_bn_bf16_statistics_and_apply(shape):
    i = fc.bn_inputs(shape)
    xb = i["x"].to(BF16)
    mean, var = ob.bn_stats(dev(xb))
    _stats_close(mean, var, xb.float(), "bn_stats bf16 %s" % (shape,))
    assert float(var[0]) == 0.0 and float(mean[0]) == fc.BN_CONST
    scale, shift = i["gamma"], i["beta"]                        # any per-channel pair, as in test_bn_bf16_stats_and_apply
    for act in ACTS:
        y = ob.bn_apply(dev(xb), dev(scale), dev(shift), act)
        assert y.dtype == BF16 and y.shape == xb.shape
        r = xb.double() * scale.double() + shift.double()
        r = torch.relu(r) if act == "relu" else (torch.where(r > 0, r, 0.2 * r) if act == "leaky" else r)
        share = _within_one_bf16_ulp(y, r, "bn_apply bf16 %s %s" % (act, shape), 0.97)
        print("bn_apply bf16 %s %s: %.4f bit-identical" % (shape, act, share))


@pytest.mark.parametrize("shape", BN_SHAPES, ids=BN_IDS)
def test_bn_bf16_backward(shape):
    i = fc.bn_inputs(shape)
    xb, dyb, gamma = i["x"].to(BF16), i["dy"].to(BF16), i["gamma"]
    for act in ACTS:
        mean, var, scale, shift, y = _cpu_forward(xb.float(), gamma, i["beta"], act)
        yb = y.to(BF16)
        dx64, dg64, db64 = fc.bn_bwd64(xb.float(), fc.bn_dact(dyb, yb, act), gamma)
        dx, dgamma, dbeta = ob.bn_bwd(dev(xb), dev(dyb), dev(yb), act, dev(mean), dev(var), dev(gamma), fc.BN_EPS)
        assert dx.dtype == BF16
        share = _within_one_bf16_ulp(dx, dx64, "bn_bwd bf16 %s %s: dx" % (shape, act), 0.95)
        fg = fc.grad_close(dgamma.cpu(), dg64, "bn_bwd bf16 %s %s: dgamma" % (shape, act))
        fb = fc.grad_close(dbeta.cpu(), db64, "bn_bwd bf16 %s %s: dbeta" % (shape, act))
        print("bn_bwd bf16 %s %s: dx %.4f bit-identical, dgamma %.3f, dbeta %.3f of the tolerance" % (shape, act, share, fg, fb))
