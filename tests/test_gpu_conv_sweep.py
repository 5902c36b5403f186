"""GPU: the implicit-GEMM convolutions at every channel-block width, input-channel chunk and epilogue form their dispatchers
pick (tests/conv_sweep_cases.py; tests/test_conv_plan.py checks on the CPU that the tables reach every plan), each against a
DEFINITION rather than another HIP kernel:
  bf16 / mixed: a plain fp64 conv of the same bf16-rounded operands (the products of bf16 numbers are exact in f32, so only
                the summation order and the final rounding may differ), then the epilogue written out on the CPU;
  f32         : the C oracle, bit for bit.
Wide images keep the 32 / 64-channel blocks and give every persistent block several tiles to walk; Cout that the block width
does not divide leaves the last channel block partial."""
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from oracle import c_oracle as co
from sequitr_amd import _lib, ops
from sequitr_amd import ops_bf16 as ob
from sequitr_amd.ops import _ptr, _stream
from tests import conv_sweep_cases as cs
from tests.util import assert_bit_exact, bf16_round, check_bf16

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
ACT = {None: 0, "relu": 1, "leaky": 2}


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _x(rng, shape):
    return torch.as_tensor(rng.standard_normal(shape), dtype=torch.float32)


def _w(rng, K, Cin, Cout):
    return torch.as_tensor(rng.standard_normal((K, K, Cin, Cout)) / np.sqrt(K * K * Cin), dtype=torch.float32)


def conv64(x64, w64, bias=None, act=None):
    """fp64 SAME conv, NHWC x HWIO, + bias, activation"""
    K = w64.shape[0]
    y = TF.conv2d(x64.permute(0, 3, 1, 2), w64.permute(3, 2, 0, 1), None, padding=K // 2).permute(0, 2, 3, 1)
    if bias is not None:
        y = y + bias.double()
    if act == "relu":
        y = TF.relu(y)
    elif act == "leaky":
        y = torch.where(y > 0, y, 0.2 * y)
    return y


def dgrad64(dy64, wf):
    """fp64 input gradient of the conv with forward filter wf (K,K,Cout_dgrad,Cin_dgrad), on the bf16-rounded filter -- what
    the transformed pack (transform=True) multiplies"""
    wt = torch.flip(bf16_round(wf), (0, 1)).permute(0, 1, 3, 2).contiguous()
    return conv64(dy64, wt)


def close(got, want, tol, what):
    want = want.double()
    err = float((got.double().cpu() - want).abs().max()) / max(float(want.abs().max()), 1e-30)
    assert err <= tol, "%s: rel err %.3g > %.3g" % (what, err, tol)


def check_chain(got, t64, fn, what):
    """a documented rounding chain after the conv: `fn` maps the bf16 conv value to the stored one (gates, bridges).  Against
    fn of the once-rounded fp64 conv nearly all values are identical; against fn of the fp64 value itself every one is within
    two bf16 ulps (one rounding of the conv, one of the chain)."""
    g = got.float().cpu().double()
    exact = fn(t64.to(BF)).float().double()
    same = (g == exact).double().mean().item()
    assert same > 0.97, "%s: only %.4f bit-identical" % (what, same)
    ideal = fn(t64).double()
    bad = (g - ideal).abs() > torch.clamp(ideal.abs(), min=1e-30) * 2.0 ** -6 + 1e-6
    assert not bad.any(), "%s: %d values off by more than two bf16 ulps" % (what, int(bad.sum()))


def _plain_case(case):
    N, H, W, Cin, Cout, K, act, with_bias = case
    rng = _rng("plain", case)
    x, w = _x(rng, (N, H, W, Cin)), _w(rng, K, Cin, Cout)
    b = torch.as_tensor(rng.standard_normal(Cout) * 0.1, dtype=torch.float32) if with_bias else None
    ref = conv64(bf16_round(x), bf16_round(w), b, act)
    bc = b.cuda() if b is not None else None
    got = ob.conv2d(x.cuda().to(BF), ob.pack_weights(w.cuda()), bc, K, Cout, act=act)
    check_bf16(got, ref, "bf16 conv %s" % (case,))
    if case in cs.MIXED_PLAIN:
        with ops.mixed_precision():
            y = ops.conv2d(x.cuda(), w.cuda(), bc, act=act)
        assert y.dtype == torch.float32
        close(y, ref, 2e-5, "mixed conv %s" % (case,))


@pytest.mark.parametrize("case", cs.BF16_PLAIN, ids=str)
def test_plain_bf16_and_mixed(case):
    _plain_case(case)


@pytest.mark.parametrize("case", cs.BF16_WIDE, ids=str)
def test_wide_grid_every_block_walks_several_tiles(case):
    _plain_case(case)


def _unpack_mask(m, shape):
    bits = np.unpackbits(m.cpu().numpy().reshape(-1), bitorder="little")
    return torch.from_numpy(bits.reshape(shape).astype(bool))


def _slope_gate(gate64, slope):
    return lambda t: torch.where(gate64 > 0, t, (t.float() * np.float32(slope)).to(BF).double() if t.dtype == BF else t * slope)


@pytest.mark.parametrize("case", cs.FORM_CASES, ids=str)
def test_epilogue_form_against_its_definition(case):
    form, N, H, W, Cin, Cout = case
    rng = _rng("form", case)
    x, w = _x(rng, (N, H, W, Cin)), _w(rng, 3, Cin, Cout)
    b = torch.as_tensor(rng.standard_normal(Cout) * 0.1, dtype=torch.float32)
    xg, wg, bg = x.cuda().to(BF), w.cuda(), b.cuda()
    x64, what = bf16_round(x), "form %s" % (case,)
    if form == cs.POOL:
        y, yp = ob.conv2d_dropout_pool(xg, ob.pack_weights(wg), bg, 3, Cout, "relu", 0.0)
        check_bf16(y, conv64(x64, bf16_round(w), b, "relu"), what + " y")
        want = TF.max_pool2d(y.float().cpu().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
        assert torch.equal(yp.float().cpu(), want), what + ": pooled copy is not the max pool of y"
    elif form == "avgpool":
        ws = float(np.sqrt(np.float32(2.0 / (9 * Cout))))
        y, yp = ops.conv2d_avgpool(xg, wg, bg, act="leaky", wscale=ws)
        check_bf16(y, conv64(x64, bf16_round(w * np.float32(ws)), b, "leaky"), what + " y")
        v = y.float().cpu()
        want = ((v[:, 0::2, 0::2] + v[:, 0::2, 1::2]) + (v[:, 1::2, 0::2] + v[:, 1::2, 1::2])) * 0.25
        assert torch.equal(yp.cpu(), want.to(BF)), what + ": pooled copy is not the f32 mean of y"
    elif form == cs.MASK:
        y, m = ob.conv2d_mask(xg, ob.pack_weights(wg), bg, 3, Cout, "relu")
        check_bf16(y, conv64(x64, bf16_round(w), b, "relu"), what + " y")
        assert torch.equal(_unpack_mask(m, (N, H, W, Cout)), y.float().cpu() > 0), what + ": mask bits != (y > 0)"
    elif form == "dropout":
        wp = ob.pack_weights(wg)
        plain = ob.conv2d(xg, wp, bg, 3, Cout, act="relu")
        check_bf16(plain, conv64(x64, bf16_round(w), b, "relu"), what + " plain part")
        y = ob.conv2d_dropout(xg, wp, bg, 3, Cout, "relu", 0.4, seed=1234)
        want, _ = ob.dropout_fwd(plain, 0.4, seed=1234)
        assert torch.equal(y, want), what + ": y != dropout_fwd(plain y)"
        assert 0.3 < (y == 0).double().mean().item() < 0.8
    elif form == cs.PIXELNORM:
        ws = float(np.sqrt(np.float32(2.0 / (9 * Cout))))
        y, yn = ops.conv2d_pixelnorm(xg, wg, bg, act="leaky", wscale=ws, eps=1e-8)
        check_bf16(y, conv64(x64, bf16_round(w * np.float32(ws)), b, "leaky"), what + " y")
        v = y.double().cpu()
        check_bf16(yn, v * torch.rsqrt((v * v).mean(-1, keepdim=True) + 1e-8), what + " ynorm")
    elif form == cs.FIRSTBLOCK:
        img = _x(rng, (N, H, W, 1))
        w1 = _w(rng, 3, 1, 16)
        b1 = torch.as_tensor(rng.standard_normal(16) * 0.1, dtype=torch.float32)
        y1, m1, y, yp = ob.conv_first_block_dropout_pool(img.cuda(), w1.cuda(), b1.cuda(), ob.pack_weights(wg), bg, 0.0)
        check_bf16(y1, conv64(img.double(), w1.double(), b1, "relu"), what + " y1")
        assert torch.equal(_unpack_mask(m1, (N, H, W, 16)), y1.float().cpu() > 0), what + ": mask bits != (y1 > 0)"
        check_bf16(y, conv64(y1.double().cpu(), bf16_round(w), b, "relu"), what + " y")
        want = TF.max_pool2d(y.float().cpu().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
        assert torch.equal(yp.float().cpu(), want), what + ": pooled copy is not the max pool of y"
    else:                                                       # the dgrad forms: dy (Cin channels) -> dx (Cout channels)
        K = 1 if form == "actgate1" else 3
        dy = _x(rng, (N, H, W, Cin)).to(BF)
        wf = _w(rng, K, Cout, Cin)                              # the forward conv Cout -> Cin whose input gradient this is
        t64 = dgrad64(dy.double(), wf)
        dyg, wp_t = dy.cuda(), ob.pack_weights(wf.cuda(), transform=True)
        if form == cs.MASKGATE:
            bits = torch.from_numpy(rng.random((N, H, W, Cout)) < 0.5)
            m = torch.from_numpy(np.packbits(bits.numpy().reshape(-1), bitorder="little")).cuda()
            for scale in (1.0, 1.0 / 0.6):
                dx = ob.conv2d_dgrad_mask(dyg, wp_t, m, 3, Cout, scale)
                s32 = np.float32(scale)
                check_chain(dx, t64, lambda t: torch.where(bits, (t.float() * s32).to(BF).double() if t.dtype == BF else t * scale,
                                                           0.0), what + " scale %g" % scale)
        elif form in ("relugate", "dropgate"):
            gate = _x(rng, (N, H, W, Cout)).to(BF)
            g64 = gate.double()
            scale = 1.0 if form == "relugate" else 1.0 / 0.6
            dx = ob.conv2d_dgrad_relu(dyg, wp_t, gate.cuda(), 3, scale)
            s32 = np.float32(scale)
            check_chain(dx, t64, lambda t: torch.where(g64 > 0, (t.float() * s32).to(BF).double() if t.dtype == BF else t * scale,
                                                       0.0), what)
        elif form in (cs.ACTGATE, "actgate1"):
            gate = _x(rng, (N, H, W, Cout)).to(BF)
            g64, gg = gate.double(), gate.cuda()
            for act, slope in (("leaky", 0.2), ("relu", 0.0)):
                dx = torch.empty((N, H, W, Cout), dtype=BF, device="cuda")
                _lib.check(_lib.load().sq_conv2d_nhwc_dgrad_actgate_bf16(_ptr(dyg), _ptr(wp_t), _ptr(gg), ACT[act],
                                                                        _ptr(dx), N, H, W, Cin, Cout, K, _stream()),
                           "sq_conv2d_nhwc_dgrad_actgate_bf16")
                check_chain(dx, t64, _slope_gate(g64, slope), what + " " + act)
        elif form == cs.JUNCTION:
            up, skip = _x(rng, (N, H, W, Cout)).to(BF), _x(rng, (N, H, W, Cout)).to(BF)
            for kind in cs.JUNCTION_KINDS:
                g, dskip = ob.conv2d_dgrad_junction(dyg, wp_t, up.cuda(), skip.cuda(), kind, 3, Cout)
                # d_up lands in the space-to-depth layout (N,H/2,W/2,4*Cout): channel block (y & 1) * 2 + (x & 1)
                g = g.cpu().view(N, H // 2, W // 2, 2, 2, Cout).permute(0, 1, 3, 2, 4, 5).reshape(N, H, W, Cout)
                rnd = lambda t, v: (t.float() * v.float()).to(BF).double() if t.dtype == BF else t * v   # noqa: E731
                if kind == "eltwise_mul":
                    fup, fskip = (lambda t: rnd(t, skip)), (lambda t: rnd(t, up))
                elif kind == "eltwise_add":
                    fup = fskip = (lambda t: t.double())
                else:
                    fup, fskip = (lambda t: t.double()), (lambda t: -t.double())
                check_chain(g, t64, fup, what + " %s d_up" % kind)
                check_chain(dskip, t64, fskip, what + " %s d_skip" % kind)
        else:
            raise AssertionError("no check for form %r" % (form,))


@pytest.mark.parametrize("case", cs.MIXED_DGRAD, ids=str)
def test_mixed_dgrad_raw_and_actgate(case):
    N, H, W, Cin, Cout, K = case                                # the dgrad conv: dy (Cin) -> dx (Cout)
    rng = _rng("mixed dgrad", case)
    dy, wf = _x(rng, (N, H, W, Cin)), _w(rng, K, Cout, Cin)
    gate = _x(rng, (N, H, W, Cout))
    ws = 0.7
    t64 = dgrad64(bf16_round(dy), wf * np.float32(ws))
    with ops.mixed_precision():
        dx = ops.conv_dgrad_raw(dy.cuda(), wf.cuda(), ws)
        close(dx, t64, 2e-5, "mixed dgrad %s" % (case,))
        for act, slope in (("leaky", 0.2), ("relu", 0.0)):
            fused = ops.conv_dgrad_actgate(dy.cuda(), wf.cuda(), ws, gate.cuda(), act)
            assert fused is not None, "mixed act-gated dgrad declined %s" % (case,)
            close(fused, torch.where(gate.double() > 0, t64, t64 * slope), 2e-5, "mixed act-gated dgrad %s %s" % (case, act))


@pytest.mark.parametrize("case", cs.MOSAIC, ids=str)
def test_mosaic_and_split_k(case):
    n, h, w_, Cin, Cout, gated = case
    rng = _rng("mosaic", case)
    R, Cc = cs.mosaic_grid(n, h, w_)
    nbytes = cs.splitk_room(n, h, w_, Cout)
    S = cs.plan(cs.BF16, cs.ACTGATE if gated else cs.PLAIN, n, h, w_, Cin, Cout, 3, "leaky", mosaic=(R, Cc),
                workspace_bytes=nbytes)["s"]
    x, w = _x(rng, (n, h, w_, Cin)).to(BF), _w(rng, 3, Cin, Cout)
    b = torch.as_tensor(rng.standard_normal(Cout) * 0.1, dtype=torch.float32)
    gate = _x(rng, (n, h, w_, Cout)).to(BF) if gated else None
    ws = torch.zeros(nbytes // 4, dtype=torch.float32, device="cuda")
    y = torch.empty((n, h, w_, Cout), dtype=BF, device="cuda")
    xg, gg, wp, bg = x.cuda(), gate.cuda() if gated else None, ob.pack_weights(w.cuda()), b.cuda()   # alive until the launch ran
    _lib.check(_lib.load().sq_conv2d_nhwc_mosaic_bf16(_ptr(xg), _ptr(wp), _ptr(bg), _ptr(gg), _ptr(y),
                                                     n, h, w_, Cin, Cout, ACT["leaky"], R, Cc, _ptr(ws), nbytes, _stream()),
               "sq_conv2d_nhwc_mosaic_bf16")
    what = "mosaic %s S=%d" % (case, S)
    for i in range(n):                                          # per image: the SAME padding of each cell is its own
        if gated:
            t64 = conv64(x[i:i + 1].double(), bf16_round(w))
            check_chain(y[i:i + 1], t64, _slope_gate(gate[i:i + 1].double(), 0.2), what + " image %d" % i)
        else:
            check_bf16(y[i:i + 1], conv64(x[i:i + 1].double(), bf16_round(w), b, "leaky"), what + " image %d" % i)


@pytest.mark.parametrize("case", cs.MIXED_MOSAIC, ids=str)
def test_mixed_mosaic(case):
    n, h, w_, Cin, Cout, gated = case
    rng = _rng("mixed mosaic", case)
    R, Cc = cs.mosaic_grid(n, h, w_)
    x, w = _x(rng, (n, h, w_, Cin)), _w(rng, 3, Cin, Cout)
    b = torch.as_tensor(rng.standard_normal(Cout) * 0.1, dtype=torch.float32)
    gate = _x(rng, (n, h, w_, Cout)) if gated else None
    y = torch.empty((n, h, w_, Cout), dtype=torch.float32, device="cuda")
    xg, gg, wp, bg = x.cuda(), gate.cuda() if gated else None, ob.pack_weights(w.cuda()), b.cuda()   # alive until the launch ran
    _lib.check(_lib.load().sq_conv2d_nhwc_mixed_mosaic_f32(_ptr(xg), _ptr(wp), _ptr(bg), _ptr(gg),
                                                          _ptr(y), n, h, w_, Cin, Cout, ACT["leaky"], R, Cc, _stream()),
               "sq_conv2d_nhwc_mixed_mosaic_f32")
    for i in range(n):
        xi = bf16_round(x[i:i + 1])
        if gated:
            t64 = conv64(xi, bf16_round(w))
            want = torch.where(gate[i:i + 1].double() > 0, t64, 0.2 * t64)
        else:
            want = conv64(xi, bf16_round(w), b, "leaky")
        close(y[i:i + 1], want, 2e-5, "mixed mosaic %s image %d" % (case, i))


@pytest.mark.parametrize("case", cs.F32_CASES, ids=str)
def test_f32_v2_bit_exact_against_the_oracle(case):
    form, N, H, W, Cin, Cout, K, act = case
    rng = _rng("f32", case)
    x, w = _x(rng, (N, H, W, Cin)), _w(rng, K, Cin, Cout)
    b = torch.as_tensor(rng.standard_normal(Cout) * 0.1, dtype=torch.float32)
    what = "f32 %s" % (case,)
    if form == cs.CONCAT:
        xb = _x(rng, (N, H, W, Cin))
        w = _w(rng, K, 2 * Cin, Cout)
        got = ops.conv2d_concat(x.cuda(), xb.cuda(), w.cuda(), b.cuda(), act=act)
        want = co.conv2d(torch.cat([x, xb], -1).numpy(), w.numpy(), b.numpy(), act=act)
        assert_bit_exact(got.cpu().numpy(), want, what)
        return
    if form == cs.POOL:
        y, p = ops.conv3x3_pool(x.cuda(), w.cuda(), b.cuda(), act=act)
        want = co.conv2d(x.numpy(), w.numpy(), b.numpy(), act=act)
        assert_bit_exact(y.cpu().numpy(), want, what + " y")
        assert_bit_exact(p.cpu().numpy(), co.maxpool2x2(want), what + " pooled")
        return
    got = ops.conv2d(x.cuda(), w.cuda(), b.cuda(), act=act)
    assert_bit_exact(got.cpu().numpy(), co.conv2d(x.numpy(), w.numpy(), b.numpy(), act=act), what)
