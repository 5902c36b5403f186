"""GPU: every kernel of sequitr_amd/csrc/sq_ops_bf16.hip, through its sequitr_amd.ops_bf16 wrapper, against the CPU references
of tests/bf16_ops_cases.py at every launch regime of that table (tests/test_bf16_ops_definitions.py checks on the CPU that
the table reaches them and that the references are right).

Bit-exact, compared as numbers (+0.0 == -0.0), every element: the streaming ops (pool, bridge, dropout, activation passes,
casts) against their f32-step emulations, the dropout mask against its numpy restatement, the head's logits / argmax / dx
against the fmaf chains of oracle.c_oracle.
Against fp64, with the tolerances the existing tests use: the transpose conv (tests/test_gpu_bf16.py::test_convT_bf16: one
bf16 ulp plain, two bridged, more than 97 % bit-identical), the loss (1e-6 relative) and dz (2e-6 max|w| / npix) of
tests/test_gpu_ops.py::test_wsoftmax_ce_loss_and_grad.
dW / db of the head: |got - fp64| <= k * 2^-24 * sum |terms| per element, k counted from the code beside
bf16_ops_cases.HEAD_K; asserted there to be no looser than rtol 1e-5 / atol 1e-4."""
import numpy as np
import pytest
import torch

from sequitr_amd import _lib, ops
from sequitr_amd import ops_bf16 as ob
from tests import bf16_ops_cases as bc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16 = torch.bfloat16
ULP = 2.0 ** -7


def dev(t):
    return t.contiguous().to(DEV)


def same(got, want, what):
    """equal as numbers at every element (want: a CPU tensor)"""
    assert tuple(got.shape) == tuple(want.shape) and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    w = dev(want)
    eq = got.float() == w.float() if got.dtype == BF16 else got == w
    if not bool(eq.all()):
        bad = (~eq).reshape(-1).nonzero().reshape(-1)
        i = int(bad[0])
        raise AssertionError("%s: %d of %d elements differ; first at flat index %d: %r, expected %r" % (
            what, bad.numel(), eq.numel(), i, float(got.reshape(-1)[i]), float(w.reshape(-1)[i])))


def bits(t):
    return t.view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def same_bits(a, b, what):
    assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and torch.equal(bits(a), bits(b)), what


# ---- streaming ops -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,regime", bc.FLAT_CASES)
def test_flat_ops_equal_their_emulations(n, regime):
    i = bc.flat_inputs(n)
    e = bc.flat_expected(i)
    dy, y, a, b, mask = (dev(i[k]) for k in ("dy", "y", "a", "b", "mask"))
    for act in bc.ACTS:
        same(ob.act_bwd(dy, y, act), e["act_bwd/" + act], "act_bwd %s %s" % (act, regime))
        same(ob.act_dropout_bwd(dy, mask, y, bc.RATE, act), e["act_dropout_bwd/" + act], "act_dropout_bwd %s %s" % (act, regime))
    for kind in bc.KINDS:
        same(ob.bridge(a, b, kind), e["bridge/" + kind], "bridge %s %s" % (kind, regime))
        da, db = ob.bridge_bwd(dy, a, b, kind)
        same(da, e["bridge_bwd/" + kind][0], "bridge_bwd %s da %s" % (kind, regime))
        same(db, e["bridge_bwd/" + kind][1], "bridge_bwd %s db %s" % (kind, regime))
    yd, m = ob.dropout_fwd(a, bc.RATE, mask=mask)                # a given mask is used as it is
    assert m.data_ptr() == mask.data_ptr()
    same(mask, i["mask"], "the given mask is left alone")
    same(yd, e["dropout_fwd"], "dropout_fwd, given mask, %s" % regime)
    same(ob.dropout_bwd(dy, mask, bc.RATE), e["dropout_bwd"], "dropout_bwd %s" % regime)
    same(ob.relu_scale_bwd(dy, y, bc.GATE), e["relu_scale_bwd"], "relu_scale_bwd %s" % regime)


@pytest.mark.parametrize("rate,seed,step", bc.MASK_CASES)
@pytest.mark.parametrize("n", [n for n, _ in bc.FLAT_CASES])
def test_dropout_mask_is_the_restated_hash(n, rate, seed, step):
    x = torch.randn(n, generator=bc._gen(6, n)).to(BF16)
    want = bc.dropout_mask(n, rate, seed, step)
    step_dev = None if step is None else torch.tensor([step], dtype=torch.int32, device=DEV)
    y, m = ob.dropout_fwd(dev(x), rate, seed=seed, step_dev=step_dev)
    assert m.dtype == torch.uint8 and tuple(m.shape) == (n,)
    same(m, torch.from_numpy(want), "bf16 dropout mask n=%d rate=%g seed=%d step=%s" % (n, rate, seed, step))
    same(y, bc.dropout_fwd(x, torch.from_numpy(want), rate), "dropout_fwd with its own mask")
    _, m32 = ops.dropout_fwd(dev(x.float()), rate, seed=seed, step_dev=step_dev)
    same(m32, torch.from_numpy(want), "f32 dropout mask n=%d rate=%g seed=%d step=%s" % (n, rate, seed, step))


@pytest.mark.parametrize("shape,tags", bc.POOL_CASES, ids=lambda v: str(v) if isinstance(v, tuple) else "")
def test_pool_ops_equal_their_emulations(shape, tags):
    i = bc.pool_inputs(shape)
    e = bc.pool_expected(i)
    x, dy, add = dev(i["x"]), dev(i["dy"]), dev(i["add"])
    same(ob.maxpool2x2(x), e["maxpool"], "maxpool %s" % (shape,))
    same(ob.maxpool2x2_bwd(x, dy), e["maxpool_bwd"], "maxpool_bwd %s" % (shape,))
    same(ob.maxpool2x2_bwd_add(x, dy, add), e["maxpool_bwd_add"], "maxpool_bwd_add %s" % (shape,))
    same(ob.maxpool2x2_bwd_add(x, dy, add, gate_scale=bc.GATE), e["maxpool_bwd_add/gate"], "maxpool_bwd_add gated %s" % (shape,))


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_pool_ties_go_to_the_first_maximum(k):
    x, win = bc.tie_case(k)
    dy = torch.arange(1, 9, dtype=torch.float32).reshape(1, 1, 1, 8).to(BF16)
    add = (0.5 * torch.arange(32, dtype=torch.float32)).reshape(1, 2, 2, 8).to(BF16)
    same(ob.maxpool2x2(dev(x)), bc.maxpool(x), "maxpool, tie at %d" % k)
    dx = ob.maxpool2x2_bwd(dev(x), dev(dy))
    same(dx, bc.maxpool_bwd(x, dy), "maxpool_bwd, tie at %d" % k)
    dxw = bc._windows(dx.float().cpu())[0, 0, 0]
    for c in range(8):
        assert int(dxw[c].argmax()) == win[c] and int((dxw[c] != 0).sum()) == 1, (k, c, dxw[c])
    same(ob.maxpool2x2_bwd_add(dev(x), dev(dy), dev(add)), bc.maxpool_bwd_add(x, dy, add), "maxpool_bwd_add, tie at %d" % k)
    same(ob.maxpool2x2_bwd_add(dev(x), dev(dy), dev(add), gate_scale=bc.GATE), bc.maxpool_bwd_add(x, dy, add, bc.GATE),
         "maxpool_bwd_add gated, tie at %d" % k)


@pytest.mark.parametrize("shape,tags", bc.S2D_CASES, ids=lambda v: str(v) if isinstance(v, tuple) else "")
def test_bridge_backward_in_space_to_depth_layout(shape, tags):
    i = bc.s2d_inputs(shape)
    dy, up, skip = dev(i["dy"]), dev(i["up"]), dev(i["skip"])
    for kind in bc.KINDS:
        g_ref, ds_ref = bc.bridge_bwd_s2d(i["dy"], i["up"], i["skip"], kind)
        keep = kind == "eltwise_mul"                            # the other bridges do not read the forward operands
        g, ds = ob.bridge_bwd_s2d(dy, up if keep else None, skip if keep else None, kind)
        same(g, g_ref, "bridge_bwd_s2d %s g %s" % (kind, shape,))
        same(ds, ds_ref, "bridge_bwd_s2d %s dskip %s" % (kind, shape,))
        da, db = ob.bridge_bwd(dy, up, skip, kind)
        same_bits(g, ob.space_to_depth2(da), "bridge_bwd_s2d %s: g = space_to_depth2(bridge_bwd)" % kind)
        same_bits(ds, db, "bridge_bwd_s2d %s: dskip = bridge_bwd's" % kind)


# ---- casts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,regime", bc.CAST_CASES)
def test_casts_equal_round_to_nearest_even(n, regime):
    f = 100.0 * torch.randn(n, generator=bc._gen(8, n))
    b = ob.to_bf16(dev(f))
    same(b, bc.to_bf16(f), "to_bf16 %s" % regime)
    back = ob.to_f32(b)
    same(back, bc.to_f32(bc.to_bf16(f)), "to_f32 %s" % regime)
    assert torch.equal(back.view(torch.int32), b.view(torch.int16).to(torch.int32) << 16)       # exact: the bf16 bits, widened


def test_cast_ties_go_to_even_and_specials_survive():
    lo = np.array([0x3F80, 0x3F81, 0x0080, 0x0081, 0x7F7E, 0x4000, 0x4001, 0xBF80, 0xBF81, 0xC2FE, 0xC2FF, 0x0100],
                  dtype=np.uint32)                              # bf16 patterns of the lower (in magnitude) neighbour, both parities
    half = torch.from_numpy(((lo << 16) | 0x8000).astype(np.uint32).view(np.int32)).view(torch.float32)     # exactly halfway up
    got = ob.to_bf16(dev(half)).view(torch.int16).cpu().numpy().view(np.uint16)
    want = np.where(lo % 2 == 0, lo, lo + 1).astype(np.uint16)                                  # the even one of the two
    assert np.array_equal(got, want), (got, want)
    assert np.array_equal(half.to(BF16).view(torch.int16).numpy().view(np.uint16), want)       # and the CPU emulation agrees
    big = np.finfo(np.float32).max
    spec = torch.tensor([0.0, -0.0, float("inf"), -float("inf"), big, -big, float("nan"), 1.0])
    got = ob.to_bf16(dev(spec)).cpu()
    assert got.view(torch.int16).numpy().view(np.uint16)[:6].tolist() == [0x0000, 0x8000, 0x7F80, 0xFF80, 0x7F80, 0xFF80]
    assert bool(torch.isnan(got[6])) and float(got[7]) == 1.0
    back = ob.to_f32(dev(got)).cpu()
    assert back.view(torch.int32)[:6].tolist() == [0, -2 ** 31, 0x7F800000, 0xFF800000 - 2 ** 32, 0x7F800000, 0xFF800000 - 2 ** 32]
    assert bool(torch.isnan(back[6]))


# ---- transpose conv ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,tags", bc.CONVT_CASES, ids=lambda v: str(v) if isinstance(v, tuple) else "")
def test_transpose_conv_against_fp64_and_the_dual_output_form(c, tags):
    i = bc.convT_inputs(c)
    e = bc.convT_expected(i)
    x, w, bias, skip = dev(i["x"]), dev(i["w"]), dev(i["bias"]), dev(i["skip"])
    wb = ob.to_bf16(w)
    same(wb, i["w"].to(BF16), "the bf16 kernel copy")
    ups = {}
    for kind in (None,) + bc.KINDS:
        got = ob.convT2x2s2(x, wb, bias, skip=skip if kind else None, bridge_kind=kind)
        ups[kind] = got
        g, ref = got.float().cpu().double(), e[kind]
        ulps = 2 if kind else 1                                 # a 1-ulp difference in the stored up-scaled value moves the bridge by one more
        err = (g - ref).abs()
        tol = ulps * ref.abs().clamp(min=1e-30) * ULP + 1e-6
        identical = float((g == ref.to(BF16).double()).double().mean())
        print("convT %s %s: worst error %.3f of %d ulp, %.4f bit-identical" % (c, kind, float((err / tol).max()), ulps, identical))
        assert bool((err <= tol).all()), "convT %s %s: %d values off by more than %d bf16 ulp" % (c, kind, int((err > tol).sum()), ulps)
        assert identical > 0.97, "convT %s %s: only %.4f bit-identical" % (c, kind, identical)
    nb = ob.convT2x2s2(x, wb, None)                             # no bias
    err = (nb.float().cpu().double() - bc.convT64(i["x"], i["w"].to(BF16), None)).abs()
    assert bool((err <= bc.convT64(i["x"], i["w"].to(BF16), None).abs().clamp(min=1e-30) * ULP + 1e-6).all()), "convT without bias"
    for kind in bc.KINDS:
        up, merged = ob.convT2x2s2_bridge_both(x, wb, bias, skip, kind)
        same_bits(up, ups[None], "bridge_both %s %s: up" % (c, kind))
        same_bits(merged, ups[kind], "bridge_both %s %s: merged = the bridged transpose conv" % (c, kind))
        same_bits(merged, ob.bridge(ups[None], skip, kind), "bridge_both %s %s: merged = convT then bridge" % (c, kind))
        same(merged, bc.bridge(ups[None].cpu(), i["skip"], kind), "bridge_both %s %s: merged = the bridge emulation on up" % (c, kind))


# ---- head ----------------------------------------------------------------------------------------------------------------
_HEAD = {}


def _head(c):
    """inputs, references and device copies of one head case, built once for the tests that share them"""
    if c not in _HEAD:
        i = bc.head_inputs(c)
        _HEAD[c] = (i, bc.head_expected(i), {k: dev(v) for k, v in i.items()})
    return _HEAD[c]


HEAD_IDS = [str(c) for c, _ in bc.HEAD_CASES]


@pytest.mark.parametrize("c", [c for c, _ in bc.HEAD_CASES], ids=HEAD_IDS)
def test_head_forward_is_the_oracle_chain(c):
    i, e, d = _head(c)
    Cout = c[4]
    for name, b in (("bias", d["bias"]), ("nobias", None)):
        logits, mask = ob.head_fwd(d["x"], d["w"], b)
        same(logits, e["logits/" + name], "head logits %s %s" % (c, name))
        same(mask, e["mask/" + name], "head mask %s %s" % (c, name))
        z = logits[0, 0, 0].cpu()
        assert float(z[0]) == float(z[-1]) == float(z.max()) and int(mask[0, 0, 0]) == 0, "the planted tie: lowest index wins"
        assert int(mask.max()) <= Cout - 1
        only, none = ob.head_fwd(d["x"], d["w"], b, want_mask=False)
        assert none is None
        same_bits(only, logits, "head logits without the mask")


@pytest.mark.parametrize("c", [c for c, _ in bc.HEAD_CASES], ids=HEAD_IDS)
def test_head_backward_given_dz(c):
    i, e, d = _head(c)
    N, H, W, Cin, Cout = c
    k = bc.head_chain_adds(N * H * W)
    dx, dw, db = ob.head_bwd(d["x"], d["w"], d["dz"])
    same(dx, e["dx"], "head dx %s" % (c,))
    dxg, dwg, dbg = ob.head_bwd(d["x"], d["w"], d["dz"], gate_scale=bc.GATE)
    same(dxg, e["dx/gate"], "head dx gated %s" % (c,))
    assert bool((dxg[d["x"] == 0] == 0).all()) and int((d["x"] == 0).sum()) > 0
    none, dwn, dbn = ob.head_bwd(d["x"], d["w"], d["dz"], want_dx=False)
    assert none is None
    errw = (dw.double().cpu().reshape(Cin, Cout) - e["dw64"]).abs()
    errb = (db.double().cpu() - e["db64"]).abs()
    tolw, tolb = k * 2.0 ** -24 * e["dw_abs"], k * 2.0 ** -24 * e["db_abs"]
    print("head_bwd %s: k = %d, worst dW error %.3f of the bound, worst db error %.3f of the bound" % (
        c, k, float((errw / tolw.clamp(min=1e-300)).max()), float((errb / tolb.clamp(min=1e-300)).max())))
    assert bool((tolw <= 1e-4 + 1e-5 * e["dw64"].abs()).all()) and bool((tolb <= 1e-4 + 1e-5 * e["db64"].abs()).all())
    assert bool((errw <= tolw).all()), "dW: %d elements past %d * 2^-24 * sum |terms|" % (int((errw > tolw).sum()), k)
    assert bool((errb <= tolb).all()), "db: %d elements past %d * 2^-24 * sum |terms|" % (int((errb > tolb).sum()), k)
    for name, other in (("gated", (dwg, dbg)), ("want_dx=False", (dwn, dbn)), ("second call", ob.head_bwd(d["x"], d["w"], d["dz"])[1:])):
        same_bits(other[0], dw, "head dW, %s" % name)
        same_bits(other[1], db, "head db, %s" % name)
    same_bits(ob.head_bwd(d["x"], d["w"], d["dz"])[0], dx, "head dx, second call")


@pytest.mark.parametrize("c", [c for c, _ in bc.HEAD_CASES], ids=HEAD_IDS)
def test_head_with_the_loss(c):
    i, e, d = _head(c)
    N, H, W, Cin, Cout = c
    npix = N * H * W
    k = bc.head_chain_adds(npix)
    dloss = float(i["dloss"])
    wmax = float(i["wgt"].max())
    for name, b in (("bias", d["bias"]), ("nobias", None)):
        loss = ob.head_wce_fwd(d["x"], d["w"], b, d["onehot"], d["wgt"])
        l64 = float(e["loss64/" + name])
        print("head_wce %s %s: loss %.9g, fp64 %.9g, relative error %.3g" % (c, name, float(loss), l64, abs(float(loss) - l64) / max(abs(l64), 1e-300)))
        assert abs(float(loss) - l64) <= 1e-6 * abs(l64)
        # the unfused tape: head -> weighted softmax-CE -> its dz times the incoming gradient -> head backward
        logits, _ = ob.head_fwd(d["x"], d["w"], b)
        loss_ref, dz = ops.wsoftmax_ce(logits, d["onehot"], d["wgt"])
        assert float(loss_ref.to(torch.float32)) == float(loss)
        dz = dz * d["dloss"]
        for gate in (0.0, bc.GATE):
            ref = ob.head_bwd(d["x"], d["w"], dz, gate_scale=gate)
            got = ob.head_wce_bwd(d["x"], d["w"], b, d["onehot"], d["wgt"], d["dloss"], gate_scale=gate)
            loss_out = torch.full((), float("nan"), dtype=torch.float32, device=DEV)
            got2 = ob.head_wce_bwd(d["x"], d["w"], b, d["onehot"], d["wgt"], d["dloss"], gate_scale=gate, loss_out=loss_out)
            same_bits(loss_out, loss, "loss_out %s %s gate %g" % (c, name, gate))
            for what, r, g, g2 in zip(("dx", "dW", "db"), ref, got, got2):
                same_bits(g, r, "head_wce_bwd %s = head_bwd on wsoftmax_ce's dz, %s %s gate %g" % (what, c, name, gate))
                same_bits(g2, r, "head_wce_bwd with loss_out %s, %s %s gate %g" % (what, c, name, gate))
        nodx = ob.head_wce_bwd(d["x"], d["w"], b, d["onehot"], d["wgt"], d["dloss"], want_dx=False)
        assert nodx[0] is None
        dx, dw, db = ob.head_wce_bwd(d["x"], d["w"], b, d["onehot"], d["wgt"], d["dloss"])
        same_bits(nodx[1], dw, "head_wce_bwd dW, want_dx=False")
        same_bits(nodx[2], db, "head_wce_bwd db, want_dx=False")
        # against fp64: each dz within 2e-6 max|w| / npix (times the incoming gradient) of its definition
        dz64 = e["dz64/" + name] * dloss
        dztol = 2e-6 * wmax / npix * abs(dloss)
        w64 = i["w"].double().reshape(Cin, Cout)
        dx64 = (dz64.reshape(-1, Cout) @ w64.t()).reshape(N, H, W, Cin)
        err = (dx.float().cpu().double() - dx64).abs()
        tol = dztol * w64.abs().sum(1) + dx64.abs() * ULP      # the dz tolerance through sum_o |w|, plus one bf16 ulp
        print("head_wce %s %s: worst dx error %.3f of the bound" % (c, name, float((err / tol).max())))
        assert bool((err <= tol).all()), "head_wce dx: %d elements past the bound" % int((err > tol).sum())
        dw64, db64, aw, ab = bc.head_wgrad64(i["x"], dz64)
        xabs = i["x"].double().reshape(-1, Cin).abs().sum(0)
        tolw = dztol * xabs.unsqueeze(1) + k * 2.0 ** -24 * aw    # the dz tolerance through sum_p |x|, plus the summation bound
        tolb = dztol * npix + k * 2.0 ** -24 * ab
        errw, errb = (dw.double().cpu().reshape(Cin, Cout) - dw64).abs(), (db.double().cpu() - db64).abs()
        print("head_wce %s %s: worst dW error %.3f, worst db error %.3f of the bound" % (c, name, float((errw / tolw).max()), float((errb / tolb).max())))
        assert bool((errw <= tolw).all()) and bool((errb <= tolb).all())


# ---- refusals ------------------------------------------------------------------------------------------------------------
def _z(*shape, **kw):
    return torch.zeros(shape, dtype=kw.get("dtype", BF16), device=DEV)


def test_refusals_are_loud():
    bad = (_lib.SequitrHipError, ValueError)
    for shape in ((1, 3, 4, 8), (1, 4, 6 + 1, 8), (1, 4, 4, 12)):          # odd H, odd W, C = 12
        N, H, W, C = shape
        with pytest.raises(bad):
            ob.maxpool2x2(_z(*shape))
        with pytest.raises(bad):
            ob.maxpool2x2_bwd(_z(*shape), _z(N, H // 2, W // 2, C))
        with pytest.raises(bad):
            ob.maxpool2x2_bwd_add(_z(*shape), _z(N, H // 2, W // 2, C), _z(*shape))
    with pytest.raises(bad):
        ob.bridge_bwd_s2d(_z(1, 4, 4, 12), None, None, "eltwise_add")
    a = _z(12)                                                  # numel % 8 != 0
    m = torch.ones(12, dtype=torch.uint8, device=DEV)
    for call in (lambda: ob.act_bwd(a, a, "relu"), lambda: ob.bridge(a, a, "eltwise_add"),
                 lambda: ob.bridge_bwd(a, a, a, "eltwise_mul"), lambda: ob.dropout_fwd(a, 0.4), lambda: ob.dropout_bwd(a, m, 0.4),
                 lambda: ob.relu_scale_bwd(a, a, 1.5), lambda: ob.act_dropout_bwd(a, m, a, 0.4, "relu"),
                 lambda: ob.to_f32(_z(6)), lambda: ob.to_bf16(_z(6, dtype=torch.float32))):
        with pytest.raises(bad):
            call()
    with pytest.raises(bad):                                    # Cin = 16
        ob.convT2x2s2(_z(1, 4, 4, 16), _z(2, 2, 16, 16), None)
    with pytest.raises(bad):                                    # Cout = 8
        ob.convT2x2s2(_z(1, 4, 4, 32), _z(2, 2, 8, 32), None)
    with pytest.raises(bad):                                    # a bridge without its skip
        ob.convT2x2s2(_z(1, 4, 4, 32), _z(2, 2, 16, 32), None, skip=None, bridge_kind="eltwise_add")
    with pytest.raises(bad):
        ob.convT2x2s2_bridge_both(_z(1, 4, 4, 16), _z(2, 2, 16, 16), None, _z(1, 8, 8, 16), "eltwise_add")
    f32 = torch.float32
    with pytest.raises(bad):                                    # Cout = 6
        ob.head_fwd(_z(1, 4, 4, 16), _z(1, 1, 16, 6, dtype=f32), None)
    with pytest.raises(bad):
        ob.head_bwd(_z(1, 4, 4, 16), _z(1, 1, 16, 6, dtype=f32), _z(1, 4, 4, 6, dtype=f32))
    with pytest.raises(bad):                                    # Cin = 24
        ob.head_bwd(_z(1, 4, 4, 24), _z(1, 1, 24, 2, dtype=f32), _z(1, 4, 4, 2, dtype=f32))
    torch.cuda.synchronize()
