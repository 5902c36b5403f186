"""GPU: the GAN's own operators (sequitr_amd/csrc/sq_gan_ops.hip, sq_gan_bf16.hip, sq_dense.hip and pixelnorm_f32_kernel of
sq_pointwise.hip) through their wrappers in sequitr_amd/ops.py, ops_gan_bf16.py and functional.py, against the references
of tests/gan_ops_cases.py at every launch regime of its tables (tests/test_gan_ops_definitions.py checks on the CPU that the
tables reach the regimes and that the references, bounds and replays are right).

Equal to fp64 (exact inputs: small integers, power-of-two scales, every partial sum below 2^24): the small weight gradients and
asum, dot_per_sample, dense forward and weight gradient, the dy-sum of the mbstd backward.
Against fp64 within k u sum |terms| (k counted from the code, gan_ops_cases): the same on randn inputs, the image-side
convolutions, pixel norm in every order, minibatch stdev in every order, lerp, the WGAN-GP losses and their gradients.
Equal to a replay: resize_nearest, mosaic pack / unpack, head_concat and its adjoint, act_fwd, scale, lerp at alpha 0 and 1.
Each bounded check prints its worst error as a fraction of the bound."""
import numpy as np
import pytest
import torch

from sequitr_amd import _lib, ops
from sequitr_amd import functional as F
from sequitr_amd import ops_gan_bf16 as ob
from tests import gan_ops_cases as gc
from tests.test_gpu_bf16_ops_sweep import DEV, dev, same

pytestmark = pytest.mark.gpu
U = gc.U
BF16 = torch.bfloat16


def _ids(cases):
    return ["-".join(str(v) for v in c) for c, _ in cases]


def within(got, ref, tol, what):
    """|got - ref| <= tol elementwise (ref, tol: CPU fp64 tensors); returns the worst error as a fraction of the bound"""
    err = (got.detach().double().cpu().reshape(ref.shape) - ref).abs()
    assert bool(torch.isfinite(err).all()), "%s: not finite" % what
    worst = float(torch.where(err > 0, err / tol.clamp(min=1e-300), torch.zeros_like(err)).max())
    if not bool((err <= tol).all()):
        i = int((err > tol).reshape(-1).nonzero()[0])
        raise AssertionError("%s: %d of %d elements past the bound, worst %.3f of it; first at flat index %d" % (
            what, int((err > tol).sum()), err.numel(), worst, i))
    print("%s: worst error %.3f of the bound" % (what, worst))
    return worst


def equal64(got, ref, what):
    """equal to the fp64 reference as numbers, no tolerance"""
    g = got.detach().double().cpu().reshape(ref.shape)
    if not bool((g == ref).all()):
        bad = (g != ref).reshape(-1).nonzero().reshape(-1)
        i = int(bad[0])
        raise AssertionError("%s: %d of %d elements differ from fp64; first at flat index %d: %r, expected %r" % (
            what, bad.numel(), ref.numel(), i, float(g.reshape(-1)[i]), float(ref.reshape(-1)[i])))


def bdev(t):
    return dev(t.to(BF16))


# ==== 1. image-side small weight gradients =================================================================================
@pytest.mark.parametrize("c,tags", gc.WG32_CASES, ids=_ids(gc.WG32_CASES))
def test_wgrad1x1_small_f32(c, tags):
    npix, Ca, Cb = c
    L = gc.wg32_launch(c)
    a, b = gc.wg_inputs(npix, Ca, Cb, True, False)
    equal64(ops.wgrad1x1_small(dev(a), dev(b)), gc.wg_ref64(a, b)[0], "wgrad1x1_small f32 %r, exact inputs" % (c,))
    a, b = gc.wg_inputs(npix, Ca, Cb, False, False)
    m64, terms, _, _ = gc.wg_ref64(a, b)
    within(ops.wgrad1x1_small(dev(a), dev(b)), m64, L.k() * U * terms, "wgrad1x1_small f32 %r, k = %d" % (c, L.k()))


@pytest.mark.parametrize("c,tags", gc.WGBF_CASES, ids=_ids(gc.WGBF_CASES))
def test_wgrad1x1_small_bf16(c, tags):
    npix, Ca, C, a_none, want_asum, scale = c
    L = gc.wgbf_launch(c)
    for exact in (True, False):
        a, b = gc.wg_inputs(npix, Ca, C, exact, True, a_none)
        out = ob.wgrad1x1_small(None if a is None else dev(a), bdev(b), scale=scale, want_asum=want_asum)
        m, asum = out if want_asum else (out, None)
        assert tuple(m.shape) == (Ca, C) and m.dtype == torch.float32
        m64, terms, s64, sterms = gc.wg_ref64(a, b, scale)
        what = "wgrad1x1_small bf16 %r (C / 8 = %d, %d lanes)" % (c, L.groups, L.pl)
        if exact:
            equal64(m, m64, what + ", exact inputs")
            if want_asum:
                equal64(asum, s64, what + ", asum, exact inputs")
        else:
            within(m, m64, L.k(scale) * U * terms, what + ", k = %d" % L.k(scale))
            if want_asum:
                within(asum, s64, L.k_asum() * U * sterms, what + ", asum, k = %d" % L.k_asum())
    if scale == 1.0 and not want_asum:                          # the dispatch of ops.wgrad1x1_small on a bf16 operand
        same(ops.wgrad1x1_small(None if a is None else dev(a), bdev(b)), m.cpu(), what + " through ops.wgrad1x1_small")


def _image(t, npix):
    return t.reshape(1, 2, npix // 2, t.shape[-1])


@pytest.mark.parametrize("c,tags", gc.SMALLIN_CASES, ids=_ids(gc.SMALLIN_CASES))
def test_conv1x1_smallin_bf16(c, tags):
    npix, CA, C, bias, act = c
    i = gc.image_conv_inputs(c, False)
    with ops.mixed_precision(True, store_bf16=True):
        y = ops.conv2d(dev(_image(i["x"], npix)), dev(i["w"].reshape(1, 1, CA, C)), dev(i["bias"]) if bias else None, act=act,
                       wscale=gc.IMAGE_WSCALE)
    assert y.dtype == BF16 and tuple(y.shape) == (1, 2, npix // 2, C)
    ref, terms = gc.image_conv_ref64(i, act)
    f32_bound = gc.smallin_k(CA) * U * terms
    within(y.reshape(npix, C), ref, f32_bound + gc.HALF_BF16_ULP * (ref.abs() + f32_bound), "conv1x1 smallin %r" % (c,))


@pytest.mark.parametrize("c,tags", gc.SMALLOUT_CASES, ids=_ids(gc.SMALLOUT_CASES))
def test_conv1x1_smallout_bf16(c, tags):
    npix, CO, C, bias, act = c
    i = gc.image_conv_inputs(c, True)
    y = ops.conv2d(bdev(_image(i["x"], npix)), dev(i["w"].reshape(1, 1, C, CO)), dev(i["bias"]) if bias else None, act=act,
                   wscale=gc.IMAGE_WSCALE)
    assert y.dtype == torch.float32 and tuple(y.shape) == (1, 2, npix // 2, CO)
    ref, terms = gc.image_conv_ref64(i, act)
    within(y.reshape(npix, CO), ref, gc.smallout_k(C) * U * terms, "conv1x1 smallout %r, k = %d" % (c, gc.smallout_k(C)))


# ==== 2. pixel norm ========================================================================================================
@pytest.mark.parametrize("c,tags", gc.PN32_CASES + gc.PNBF_CASES, ids=_ids(gc.PN32_CASES + gc.PNBF_CASES))
def test_pixelnorm_all_orders(c, tags):
    bf, C, npix = c
    i = gc.pn_inputs(c)
    r = gc.pn_ref64(i, bf)
    put = bdev if bf else dev
    x, g, v = put(i["x"]), put(i["g"]), put(i["v"])
    what = "pixelnorm %s C %d npix %d" % ("bf16" if bf else "f32", C, npix)

    def stored(name):
        e, b = r[name]
        return e, (gc.pn_store_bound(e, b) if bf else b)

    y = ops.pixelnorm(x)
    assert y.dtype == x.dtype
    within(y, *stored("fwd"), what=what + " forward")
    for act in gc.ACTS:
        e, b = gc.pn_gate(r["bwd"][0], r["bwd"][1], i["x"], act, bf)
        within(ops.pixelnorm_bwd(x, g, act=act), e, b, what + " backward, act %s" % act)
    dg, dx2 = ops.pixelnorm_bwd2(x, g, v)
    within(dg, *stored("dg"), what=what + " second backward, dg")
    within(dx2, *stored("dx2"), what=what + " second backward, dx2")


# ==== 3. minibatch stdev ===================================================================================================
@pytest.mark.parametrize("c,tags", gc.MB32_CASES + gc.MBBF_CASES, ids=_ids(gc.MB32_CASES + gc.MBBF_CASES))
def test_mbstd_map_all_orders(c, tags):
    bf, groups, n, P, cells = c
    i = gc.mb_inputs(c)
    ref, bnd = gc.mb_ref64(i, groups), gc.mb_bounds(i, groups)
    put = bdev if bf else dev
    x, v = put(i["x"]).requires_grad_(True), put(i["v"])
    dy = dev(i["dy"]).requires_grad_(True)
    what = "mbstd_map %s groups %d n %d P %d cells %d" % ("bf16" if bf else "f32", groups, n, P, cells)
    y = F.mbstd_map(x, groups, cells)
    assert y.dtype == torch.float32 and tuple(y.shape) == (groups * n, cells)
    within(y, ref["y"], bnd["y"], what + " map")
    (dx,) = torch.autograd.grad(y, x, dy, create_graph=True)
    ddy, dx2 = torch.autograd.grad(dx, (dy, x), v)
    assert dx.dtype == x.dtype and dx2.dtype == x.dtype and ddy.dtype == torch.float32

    def stored(name):
        return bnd[name] + gc.HALF_BF16_ULP * (ref[name].abs() + bnd[name]) if bf else bnd[name]

    within(dx, ref["dx"], stored("dx"), what + " backward")
    within(ddy, ref["ddy"], bnd["ddy"], what + " second backward, ddy")
    within(dx2, ref["dx2"], stored("dx2"), what + " second backward, dx2")


@pytest.mark.parametrize("c", gc.MB_EXACT_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_mbstd_backward_dy_sum_is_exact(c):
    groups, n, P, cells = c
    i = gc.mb_exact_inputs(c)
    want = ((i["dy"].double().reshape(groups, -1).sum(1) / (P * n)).reshape(groups, 1, 1)
            * i["x"].double().reshape(groups, n, P)).reshape(-1, P)
    equal64(ops.mbstd_map(dev(i["x"]), groups, cells), torch.ones((groups * n, cells), dtype=torch.float64), "mbstd_map %r" % (c,))
    equal64(ops.mbstd_map_bwd(dev(i["x"]), dev(i["dy"]), groups), want, "mbstd_map_bwd f32 %r" % (c,))
    dxb = ops.mbstd_map_bwd(bdev(i["x"]), dev(i["dy"]), groups)
    assert dxb.dtype == BF16
    equal64(dxb.float(), want.float().to(BF16).double(), "mbstd_map_bwd bf16 %r: the exact value rounded once" % (c,))


@pytest.mark.parametrize("N,P", gc.MBSTD_SCALAR_CASES)
def test_mbstd_scalar(N, P):
    i = gc.mb_inputs((False, 1, N, P, 1))
    blocks = min(256, -(-P // 256))
    s = ops.mbstd(dev(i["x"]))
    within(s.reshape(1), gc.mb_ref64(i, 1)["y"][:1, 0], gc.mb_bounds(i, 1, blocks)["y"][:1, 0], "mbstd N %d P %d" % (N, P))


# ==== 4. per-sample algebra and index maps =================================================================================
@pytest.mark.parametrize("c,tags", gc.ALGEBRA_CASES, ids=_ids(gc.ALGEBRA_CASES))
def test_lerp_scale_act(c, tags):
    n, per = c
    i = gc.algebra_inputs(c)
    a, b, p = dev(i["a"]), dev(i["b"]), dev(i["per"])
    what = "n %d per-sample %d" % (n, per)
    within(ops.lerp(a, b, gc.LERP_ALPHA), *gc.lerp_ref64(i["a"], i["b"], gc.LERP_ALPHA), what="lerp scalar " + what)
    within(ops.lerp(a, b, p), *gc.lerp_ref64(i["a"], i["b"], i["per"]), what="lerp per sample " + what)
    out = torch.full((2,) + tuple(a.shape), float("nan"), device=DEV)
    assert ops.lerp(a, b, p, out=out[1]).data_ptr() == out[1].data_ptr()
    same(out[1], ops.lerp(a, b, p).cpu(), "lerp out= " + what)
    assert bool(torch.isnan(out[0]).all()), "lerp out= wrote outside its destination"
    same(ops.lerp(a, b, 1.0), i["a"], "lerp alpha 1 " + what)
    same(ops.lerp(a, b, 0.0), i["b"], "lerp alpha 0 " + what)
    ones = torch.ones_like(i["per"])
    same(ops.lerp(a, b, dev(ones)), i["a"], "lerp per-sample alpha 1 " + what)
    same(ops.lerp(a, b, dev(0 * ones)), i["b"], "lerp per-sample alpha 0 " + what)
    for one_minus in (False, True):
        same(ops.scale(a, 0.37, one_minus), gc.scale_replay(i["a"], 0.37, one_minus), "scale scalar %s %s" % (one_minus, what))
        same(ops.scale(a, p, one_minus), gc.scale_replay(i["a"], i["per"], one_minus), "scale per sample %s %s" % (one_minus, what))
    x = gc._signed_with_zeros(gc._gen(52, n), (n,))
    for act in ("relu", "leaky"):
        same(ops.act_fwd(dev(x), act), gc.act_replay(x, act), "act_fwd f32 %s %s" % (act, what))
        if n % 8 == 0:
            same(ops.act_fwd(bdev(x), act), gc.act_replay(x.to(BF16), act, True), "act_fwd bf16 %s %s" % (act, what))
    xd = dev(x)
    assert ops.act_fwd(xd, None) is xd


@pytest.mark.parametrize("c,tags", gc.DOT_CASES, ids=_ids(gc.DOT_CASES))
def test_dot_per_sample(c, tags):
    a, b = gc.dot_inputs(c, True)
    equal64(ops.dot_per_sample(dev(a), dev(b)), (a.double() * b.double()).sum(1), "dot_per_sample %r, exact inputs" % (c,))
    a, b = gc.dot_inputs(c, False)
    prod = a.double() * b.double()
    within(ops.dot_per_sample(dev(a), dev(b)), prod.sum(1), gc.dot_k(c[1]) * U * prod.abs().sum(1),
           "dot_per_sample %r, k = %d" % (c, gc.dot_k(c[1])))
    within(ops.dot_per_sample(dev(a), dev(a)), (a.double() ** 2).sum(1), gc.dot_k(c[1]) * U * (a.double() ** 2).sum(1),
           "dot_per_sample %r, squared norm" % (c,))


@pytest.mark.parametrize("c,tags", gc.RESIZE_CASES, ids=_ids(gc.RESIZE_CASES))
def test_resize_nearest(c, tags):
    x = gc.resize_input(c)
    same(ops.resize_nearest(dev(x), (c[3], c[4])), gc.resize_replay(x, c[3], c[4]), "resize_nearest %r" % (c,))


@pytest.mark.parametrize("N", gc.WGAN_N)
def test_wgan_losses_and_gradients(N):
    i = gc.wgan_inputs(N)
    gd, gg = 0.7, -1.3
    for ups in ((gd, gg), (gd, None), (None, gg)):
        Dz, Dx, gn2 = (dev(i[k]).requires_grad_(True) for k in ("Dz", "Dx", "gn2"))
        d, g = F.wgan_losses(Dz, Dx, gn2)
        dref, dbnd, gref, gbnd = gc.wgan_ref64(i)
        within(d.reshape(1), dref.reshape(1), dbnd.reshape(1), "wgan d_loss N %d" % N)
        within(g.reshape(1), gref.reshape(1), gbnd.reshape(1), "wgan g_loss N %d" % N)
        outs = [t for t, u in ((d, ups[0]), (g, ups[1])) if u is not None]
        gos = [torch.tensor(u, dtype=torch.float32, device=DEV) for u in ups if u is not None]
        grads = torch.autograd.grad(outs, (Dz, Dx, gn2), gos, allow_unused=True)
        r = gc.wgan_bwd_ref64(i, ups[0], ups[1])
        for name, got in zip(("dDz", "dDx", "dgn2"), grads):
            if got is None:                                     # an unused input: the same as a zero gradient
                got = torch.zeros((N,), device=DEV)
            within(got, *r[name], what="wgan %s N %d upstream %r" % (name, N, ups))
    Dz = dev(i["Dz"]).requires_grad_(True)                      # the generator's step: Dz alone
    _, g = F.wgan_losses(Dz)
    _, _, gref, gbnd = gc.wgan_ref64(i, True)
    within(g.reshape(1), gref.reshape(1), gbnd.reshape(1), "wgan g_loss alone N %d" % N)
    (dDz,) = torch.autograd.grad(g, Dz, torch.tensor(gg, dtype=torch.float32, device=DEV))
    within(dDz, *gc.wgan_bwd_ref64(i, None, gg, True)["dDz"], what="wgan dDz, generator only, N %d" % N)


@pytest.mark.parametrize("c,tags", gc.MOSAIC_CASES, ids=_ids(gc.MOSAIC_CASES))
def test_mosaic_pack_unpack(c, tags):
    N, H, W, C, R, Cc = c
    x = gc.mosaic_input(c)
    m = ops.mosaic_pack(dev(x), R, Cc)
    same(m, gc.mosaic_replay(x, R, Cc), "mosaic_pack %r" % (c,))
    seam = dev(gc.mosaic_seam_mask(c))
    assert bool((m.view(torch.int32)[seam] == 0).all()), "seam rows / columns and empty cells must be +0.0"
    same(ops.mosaic_unpack(m, N, H, W, R, Cc), x, "mosaic_unpack(mosaic_pack(x)) %r" % (c,))


@pytest.mark.parametrize("c,tags", gc.HEAD_CONCAT_CASES, ids=_ids(gc.HEAD_CONCAT_CASES))
def test_head_concat_and_its_adjoint(c, tags):
    N, P, C = c
    i = gc.head_concat_inputs(c)
    conv, mb = dev(i["conv"]).requires_grad_(True), dev(i["mb"]).requires_grad_(True)
    flat = F.head_concat(conv, mb)
    same(flat.detach(), gc.head_concat_replay(i["conv"], i["mb"]), "head_concat %r" % (c,))
    dconv, dmb = torch.autograd.grad(flat, (conv, mb), dev(i["dflat"]))
    wc, wm = gc.head_split_replay(i["dflat"], N, P, C)
    same(dconv, wc, "head_concat backward, dconv %r" % (c,))
    same(dmb, wm, "head_concat backward, dmb %r" % (c,))


# ==== 5. dense =============================================================================================================
@pytest.mark.parametrize("c,tags", gc.DENSE_CASES, ids=_ids(gc.DENSE_CASES))
def test_dense_forward(c, tags):
    M, K, N, bias, act, wscale = c
    for exact_act in (None, "relu"):                            # 0.2 v is not exact: leaky runs on the bounded inputs only
        i = gc.dense_inputs(c, True)
        y = ops.dense(dev(i["x"]), dev(i["w"]), dev(i["bias"]) if bias else None, act=exact_act, wscale=wscale)
        equal64(y, gc.dense_ref64(i, exact_act, wscale)[0], "dense %r act %s, exact inputs" % (c, exact_act))
    i = gc.dense_inputs(c, False)
    y = ops.dense(dev(i["x"]), dev(i["w"]), dev(i["bias"]) if bias else None, act=act, wscale=gc.DENSE_BOUNDED_WSCALE)
    ref, terms = gc.dense_ref64(i, act, gc.DENSE_BOUNDED_WSCALE)
    within(y, ref, gc.dense_k(K) * U * terms, "dense %r, k = %d" % (c, gc.dense_k(K)))


@pytest.mark.parametrize("c,tags", gc.DENSE_WGRAD_CASES, ids=_ids(gc.DENSE_WGRAD_CASES))
def test_dense_wgrad(c, tags):
    M, K, N, accumulate, scale, want_db = c
    k = gc.dense_wgrad_k(M)
    for exact in (True, False):
        i = gc.dense_wgrad_inputs(c, exact)
        dw_out, db_out = dev(i["dw0"]), dev(i["db0"])
        dw, db = ops.dense_wgrad(dev(i["x"]), dev(i["dy"]), want_bias=want_db, dw_scale=scale, dw_out=dw_out,
                                 db_out=db_out if want_db else None, accumulate=accumulate)
        assert dw.data_ptr() == dw_out.data_ptr() and (db is None) == (not want_db)
        dw64, dwt, db64, dbt = gc.dense_wgrad_ref64(i, accumulate, scale)
        what = "dense_wgrad %r" % (c,)
        if exact:
            equal64(dw, dw64, what + " dW, exact inputs")
            if want_db:
                equal64(db, db64, what + " db, exact inputs")
        else:
            within(dw, dw64, k * U * dwt, what + " dW, k = %d" % k)
            if want_db:
                within(db, db64, k * U * dbt, what + " db, k = %d" % k)
        if not want_db:
            same(db_out, i["db0"], what + ": db_out is left alone without want_bias")


# ==== refusals =============================================================================================================
def _misaligned(n, dtype):
    """a contiguous view of n elements that starts one element into a larger buffer: not 16-byte aligned"""
    t = torch.zeros((n + 8,), dtype=dtype, device=DEV)[1:n + 1]
    assert t.data_ptr() % 16 != 0 and t.is_contiguous()
    return t


def test_refusals_are_loud():
    """every case is rejected on the host before any launch (gan_ops_cases.REFUSALS: the wrong operand is never the smaller)"""
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=DEV)        # noqa: E731
    bf = lambda *s: torch.zeros(s, dtype=BF16, device=DEV)                  # noqa: E731
    errs = (_lib.SequitrHipError, ValueError)
    calls = {
        "pixelnorm f32: C = 6": lambda: ops.pixelnorm(f32(5, 6)),
        "pixelnorm bf16: C = 12": lambda: ops.pixelnorm(bf(5, 12)),
        "pixelnorm_bwd f32: C = 6": lambda: ops.pixelnorm_bwd(f32(5, 6), f32(5, 6)),
        "wgrad1x1_small f32: Cb = 6": lambda: ops.wgrad1x1_small(f32(10, 2), f32(10, 6)),
        "wgrad1x1_small bf16: C = 12": lambda: ops.wgrad1x1_small(f32(10, 2), bf(10, 12)),
        "wgrad1x1_small f32: b covers more pixels": lambda: ops.wgrad1x1_small(f32(10, 2), f32(12, 8)),
        "wgrad1x1_small bf16: a covers more pixels": lambda: ops.wgrad1x1_small(f32(12, 2), bf(10, 8)),
        "pixelnorm f32: misaligned view": lambda: ops.pixelnorm(_misaligned(40, torch.float32).view(5, 8)),
        "pixelnorm bf16: misaligned view": lambda: ops.pixelnorm(_misaligned(40, BF16).view(5, 8)),
        "lerp: misaligned view": lambda: ops.lerp(_misaligned(64, torch.float32).view(16, 4), f32(16, 4), 0.5),
        "mbstd_map bf16: odd P": lambda: ops.mbstd_map(bf(4, 7), 1, 16),
        "mbstd_map_bwd bf16: odd P": lambda: ops.mbstd_map_bwd(bf(4, 7), f32(4, 16), 1),
        "dense_wgrad: M = 129": lambda: ops.dense_wgrad(f32(129, 8), f32(129, 4)),
        "dense: K = 6": lambda: ops.dense(f32(2, 6), f32(6, 4)),
    }
    assert set(calls) == {r[0] for r in gc.REFUSALS}
    for name, _, _, _ in gc.REFUSALS:
        with pytest.raises(errs):
            calls[name]()
    torch.cuda.synchronize()                                    # nothing was launched, nothing is pending
    y = ops.pixelnorm(f32(5, 8) + 1.0)                          # and the library still serves a good call
    assert bool(torch.isfinite(y).all())
