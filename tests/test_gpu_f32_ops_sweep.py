"""GPU: the f32 training operators of sequitr_amd/csrc/sq_backward_misc.hip and sq_pointwise.hip and the loss of
sq_convt_loss.hip, through their sequitr_amd.ops wrappers, against the CPU references of tests/f32_ops_cases.py at every
launch regime of its tables (tests/test_f32_ops_definitions.py checks on the CPU that the tables reach them and that the
references are right).

Equal as numbers (+0.0 == -0.0) at every element: activation / bridge / dropout passes, the pools and their gradients, the
2x2 broadcasts and sums, the index maps, the weight transform, argmax, axpy_ with an exactly representable product, the
head's dx (the fmaf chain of oracle.c_oracle).
Against fp64 with bounds counted from the code (f32_ops_cases: ADAM_K, head_chain_adds, wce_k): axpy_ with a general alpha,
the five Adam forms, the head's dW / db, the loss and its gradient.  Each prints its worst error as a fraction of the bound.
Outputs the caller provides (out=, dw_out=, db_out=) are also written into a view of a larger sentinel-filled buffer whose
4 KiB on either side must stay untouched.

The extreme-logit loss case is what pins the softmax of sq_wce_pixel to exp((z - m) - log s): as exp(z - lse) its dz was at
1.68 of 2e-6 max|w| / npix, because lse is rounded at |lse| up to 80."""
import numpy as np
import pytest
import torch

from sequitr_amd import _lib, ops
from tests import f32_ops_cases as fc
from tests.bf16_ops_cases import ACTS, KINDS, RATE, _windows, tie_case
from tests.test_gpu_bf16_ops_sweep import DEV, dev, same, same_bits

pytestmark = pytest.mark.gpu
U = fc.U
SENTINEL = 0x7FC0DEAD                                           # a NaN pattern no kernel here produces
PAD = 1024                                                      # 4 KiB of int32 on either side


class Guarded(object):
    """an f32 tensor of `shape` that is a 16-byte-aligned view inside a larger buffer filled with SENTINEL"""

    def __init__(self, shape):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.int32, device=DEV)
        self.n = n
        self.out = self.buf[PAD:PAD + n].view(torch.float32).view(shape)
        assert self.out.data_ptr() % 16 == 0 and self.out.is_contiguous()

    def check(self, what):
        lo, hi = self.buf[:PAD], self.buf[PAD + self.n:]
        assert bool((lo == SENTINEL).all()), "%s wrote in front of its output" % what
        assert bool((hi == SENTINEL).all()), "%s wrote past its output (first at +%d floats)" % (
            what, int((hi != SENTINEL).nonzero()[0]) if bool((hi != SENTINEL).any()) else -1)
        return self.out


def within(got, ref, tol, what):
    """|got - ref| <= tol elementwise (CPU fp64 tensors); returns the worst error as a fraction of the bound"""
    err = (got.double().cpu() - ref).abs()
    worst = float((err / tol.clamp(min=1e-300)).max())
    if not bool((err <= tol).all()):
        i = int((err > tol).reshape(-1).nonzero()[0])
        raise AssertionError("%s: %d of %d elements past the bound, worst %.3f of it; first at flat index %d" % (
            what, int((err > tol).sum()), err.numel(), worst, i))
    return worst


# ---- flat ops ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,regime", fc.FLAT_CASES)
def test_flat_ops_equal_their_replays(n, regime):
    i = fc.flat_inputs(n)
    e = fc.flat_expected(i)
    dy, y, a, b, mask = (dev(i[k]) for k in ("dy", "y", "a", "b", "mask"))
    for act in ACTS:
        got = ops.act_bwd(dy, y, act)
        same(got, e["act_bwd/" + act], "act_bwd %s %s" % (act, regime))
        assert (got is dy) == (act == "none")
    for kind in KINDS:
        same(ops.bridge(a, b, kind), e["bridge/" + kind], "bridge %s %s" % (kind, regime))
        if regime != "below_256":
            g = Guarded((n,))
            assert ops.bridge(a, b, kind, out=g.out) is g.out
            same(g.check("bridge %s out= %s" % (kind, regime)), e["bridge/" + kind], "bridge %s out= %s" % (kind, regime))
        da, db = ops.bridge_bwd(dy, a, b, kind)
        same(da, e["bridge_bwd/" + kind][0], "bridge_bwd %s da %s" % (kind, regime))
        same(db, e["bridge_bwd/" + kind][1], "bridge_bwd %s db %s" % (kind, regime))
        if kind != "eltwise_mul":                               # the forward operands are not read
            da2, db2 = ops.bridge_bwd(dy, None, None, kind)
            same_bits(da2, da, "bridge_bwd %s without a, b: da" % kind)
            same_bits(db2, db, "bridge_bwd %s without a, b: db" % kind)
    yd, m = ops.dropout_fwd(a, RATE, mask=mask)                 # a given mask is used as it is
    assert m.data_ptr() == mask.data_ptr()
    same(mask, i["mask"], "the given mask is left alone")
    same(yd, e["dropout_fwd"], "dropout_fwd, given mask, %s" % regime)
    same(ops.dropout_bwd(dy, mask, RATE), e["dropout_bwd"], "dropout_bwd %s" % regime)


@pytest.mark.parametrize("n,offset,tags", fc.AXPY_CASES, ids=lambda v: "" if isinstance(v, set) else str(v))
def test_axpy(n, offset, tags):
    ybuf, xbuf = fc.axpy_inputs(n, offset)
    y0, x0 = ybuf[offset:], xbuf[offset:]
    xd = dev(xbuf)[offset:]
    assert (xd.data_ptr() % 16 != 0) == bool(offset)
    for alpha in fc.AXPY_ALPHAS:
        yd = dev(ybuf)
        assert ops.axpy_(yd[offset:], xd, alpha).data_ptr() == yd[offset:].data_ptr()
        same(yd[offset:], fc.axpy(y0, x0, alpha), "axpy_ alpha %g n %d offset %d" % (alpha, n, offset))
        same(yd[:offset], ybuf[:offset], "axpy_ leaves what is in front of its view alone")
    yd = dev(ybuf)
    ops.axpy_(yd[offset:], xd, fc.AXPY_GENERAL_ALPHA)
    exact = fc.axpy64(y0, x0, fc.AXPY_GENERAL_ALPHA)
    worst = within(yd[offset:], exact, U * exact.abs(), "axpy_ alpha %g n %d offset %d" % (fc.AXPY_GENERAL_ALPHA, n, offset))
    print("axpy_ n %d offset %d alpha %g: worst error %.3f of one correctly rounded fmaf" % (n, offset, fc.AXPY_GENERAL_ALPHA, worst))


# ---- Adam ----------------------------------------------------------------------------------------------------------------
def _adam_dev(i):
    return [dev(i[k]) for k in ("p", "g", "m", "v")]


def _adam_got(t):
    return t[0].cpu(), t[2].cpu(), t[3].cpu()


def _state(step):
    return torch.tensor([step, 0], dtype=torch.int32, device=DEV)


def _lr_of(state, step, warmup, what):
    """state[0] counts exactly; state[1] holds lr_t within one f32 ulp of the formula in doubles"""
    s = state.cpu()
    assert int(s[0]) == step, "%s: state[0] = %d after step %d" % (what, int(s[0]), step)
    want = np.array([fc.adam_lr_t(step, warmup)], dtype=np.float64).astype(np.float32)
    assert abs(int(s[1]) - int(want.view(np.int32)[0])) <= 1, "%s: lr_t %r, expected %r" % (what, float(s[1:].view(torch.float32)), float(want[0]))
    return float(s[1:].view(torch.float32)[0])


@pytest.mark.parametrize("n,regime", fc.ADAM_CASES)
def test_adam_forms_against_fp64(n, regime):
    i = fc.adam_inputs(n)
    step = 3
    t = _adam_dev(i)
    ops.adam_step(t[0], t[1], t[2], t[3], fc.LR, fc.B1, fc.B2, fc.EPS, step, fc.GSCALE)
    lr_host = float(np.array([fc.adam_lr_t(step)]).astype(np.float32)[0])
    w1 = fc.adam_check("adam_step n=%d" % n, _adam_got(t), i, lr_host, host_lr=True)
    same(t[1], i["g"], "adam_step leaves g alone")
    t2, s2 = _adam_dev(i), _state(step - 1)
    ops.adam_step_dev(t2[0], t2[1], t2[2], t2[3], fc.LR, fc.B1, fc.B2, fc.EPS, s2, fc.GSCALE)
    lr_t = _lr_of(s2, step, 0, "adam_step_dev")
    w2 = fc.adam_check("adam_step_dev n=%d" % n, _adam_got(t2), i, lr_t)
    t3, s3 = _adam_dev(i), _state(step - 1)
    ops.adam_advance_dev(s3, fc.LR, fc.B1, fc.B2)
    ops.adam_apply_dev(t3[0], t3[1], t3[2], t3[3], fc.B1, fc.B2, fc.EPS, s3, fc.GSCALE)
    same_bits(s3, s2, "adam_advance_dev: the state of adam_step_dev")
    for name, a, b in zip("pgmv", t3, t2):
        same_bits(a, b, "adam_advance_dev + adam_apply_dev = adam_step_dev: %s" % name)
    print("adam n=%d: adam_step worst m %.3f v %.3f p %.3f, adam_step_dev m %.3f v %.3f p %.3f of the bound" % (
        n, w1["m"], w1["v"], w1["p"], w2["m"], w2["v"], w2["p"]))


@pytest.mark.parametrize("warmup", fc.ADAM_WARMUPS)
def test_adam_warmup_walks_the_schedule_on_the_device(warmup):
    i = fc.adam_inputs(1000, key=warmup + 1)
    t, state = _adam_dev(i), _state(0)
    worst = {"m": 0.0, "v": 0.0, "p": 0.0}
    for step in fc.ADAM_STEPS:
        before = {k: v.cpu() for k, v in zip(("p", "g", "m", "v"), t)}
        ops.adam_advance_warmup_dev(state, fc.LR, fc.B1, fc.B2, warmup)
        lr_t = _lr_of(state, step, warmup, "adam_advance_warmup_dev(warmup=%d)" % warmup)
        if warmup == 0:
            plain = _state(step - 1)
            ops.adam_advance_dev(plain, fc.LR, fc.B1, fc.B2)
            same_bits(state, plain, "warmup 0 is adam_advance_dev")
        ops.adam_apply_dev(t[0], t[1], t[2], t[3], fc.B1, fc.B2, fc.EPS, state, fc.GSCALE)
        w = fc.adam_check("warmup %d step %d" % (warmup, step), _adam_got(t), before, lr_t)
        worst = {k: max(worst[k], w[k]) for k in worst}
    print("adam warmup %d, steps 1-5: worst m %.3f v %.3f p %.3f of the bound" % (warmup, worst["m"], worst["v"], worst["p"]))


def test_adam_tensor_list_equals_one_apply_per_tensor():
    ins = [fc.adam_inputs(n, key=7) for n in fc.ADAM_MULTI_COUNTS]
    multi = [_adam_dev(i) for i in ins]
    single = [_adam_dev(i) for i in ins]
    state = _state(4)
    ops.adam_advance_dev(state, fc.LR, fc.B1, fc.B2)
    lr_t = _lr_of(state, 5, 0, "adam_advance_dev")
    table = ops.adam_table(*[[t[k] for t in multi] for k in range(4)])
    assert tuple(table.shape) == (len(ins), 6) and table._sq_chunks == sum(-(-n // 2048) for n in fc.ADAM_MULTI_COUNTS)
    ops.adam_apply_multi_dev(table, fc.B1, fc.B2, fc.EPS, state, fc.GSCALE)
    for n, i, tm, ts in zip(fc.ADAM_MULTI_COUNTS, ins, multi, single):
        ops.adam_apply_dev(ts[0], ts[1], ts[2], ts[3], fc.B1, fc.B2, fc.EPS, state, fc.GSCALE)
        for name, a, b in zip("pgmv", tm, ts):
            same_bits(a, b, "adam_apply_multi_dev, tensor of %d: %s" % (n, name))
        w = fc.adam_check("adam_apply_multi_dev, tensor of %d" % n, _adam_got(tm), i, lr_t)
        print("adam_apply_multi_dev n=%d: worst m %.3f v %.3f p %.3f of the bound" % (n, w["m"], w["v"], w["p"]))


# ---- 2x2 spatial ops -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,tags", fc.SPATIAL_CASES, ids=lambda v: str(v) if isinstance(v, tuple) else "")
def test_pools_and_their_gradients(shape, tags):
    i = fc.spatial_inputs(shape)
    x, dy = dev(i["x"]), dev(i["dy"])
    guard = "below_256" not in tags
    for name, op, ref in (("maxpool2x2", ops.maxpool2x2, fc.maxpool), ("avgpool2x2", ops.avgpool2x2, fc.avgpool)):
        want = ref(i["x"])
        same(op(x), want, "%s %s" % (name, shape))
        if guard:
            g = Guarded(want.shape)
            assert op(x, out=g.out) is g.out
            same(g.check("%s out= %s" % (name, shape)), want, "%s out= %s" % (name, shape))
    dx = ops.maxpool2x2_bwd(x, dy)
    same(dx, fc.maxpool_bwd(i["x"], i["dy"]), "maxpool2x2_bwd %s" % (shape,))
    dxw = _windows(dx)                                          # (N,Ho,Wo,C,4) on the device
    assert bool((dxw.sum(-1) == dy).all()), "maxpool2x2_bwd %s: a window's gradients do not sum to dy" % (shape,)
    assert int((dxw != 0).sum(-1).max()) <= 1, "maxpool2x2_bwd %s: more than one position of a window took the gradient" % (shape,)
    for scale in fc.SUMPOOL_SCALES:
        same(ops.sumpool2x2(x, scale), fc.sumpool(i["x"], scale), "sumpool2x2 scale %g %s" % (scale, shape))


@pytest.mark.parametrize("shape,tags", fc.SPATIAL_CASES, ids=lambda v: str(v) if isinstance(v, tuple) else "")
def test_broadcasts_with_the_shape_as_the_large_side(shape, tags):
    i = fc.spatial_inputs(shape)
    src, gate = dev(i["dy"]), dev(i["gate"])
    for scale in fc.SUMPOOL_SCALES:
        same(ops.broadcast2x2(src, scale), fc.broadcast2x2(i["dy"], scale), "broadcast2x2 scale %g %s" % (scale, shape))
    for act in ACTS:
        same(ops.broadcast2x2_act_bwd(src, gate, 0.25, act), fc.broadcast2x2_act_bwd(i["dy"], i["gate"], 0.25, act),
             "broadcast2x2_act_bwd %s %s" % (act, shape))


@pytest.mark.parametrize("shape,tags", fc.SPATIAL_CASES, ids=lambda v: str(v) if isinstance(v, tuple) else "")
def test_index_maps(shape, tags):
    i = fc.spatial_inputs(shape)
    x, small, large = dev(i["x"]), dev(i["small"]), dev(i["large"])
    want = fc.upsample_nn2x(i["small"])
    same(ops.upsample_nn2x(small), want, "upsample_nn2x %s" % (shape,))
    g = Guarded(want.shape)
    assert ops.upsample_nn2x(small, out=g.out) is g.out
    same(g.check("upsample_nn2x out= %s" % (shape,)), want, "upsample_nn2x out= %s" % (shape,))
    same(ops.zero_insert2x(small), fc.zero_insert2x(i["small"]), "zero_insert2x %s" % (shape,))
    same(ops.gather_odd2x(large), fc.gather_odd2x(i["large"]), "gather_odd2x %s" % (shape,))
    same(ops.space_to_depth2(x), fc.space_to_depth2(i["x"]), "space_to_depth2 %s" % (shape,))


@pytest.mark.parametrize("C", fc.SCALAR_PATH_C + (fc.MISALIGNED_C,))
def test_scalar_path_of_broadcast_and_sumpool(C):
    """C % 4 != 0 takes the one-float-per-thread kernels; so does C = 8 on a view that starts one float into a buffer, and
    there the result must be the vector path's, bit for bit"""
    shape = fc.SCALAR_PATH_SHAPE + (C,)
    g = fc._gen(18, C)
    x, src = fc._randn(g, (2,) + shape[1:]), fc._randn(g, (2, shape[1] // 2, shape[2] // 2, C))
    xd, sd = dev(x), dev(src)
    if C == fc.MISALIGNED_C:
        xv = torch.empty(x.numel() + 1, dtype=torch.float32, device=DEV)[1:].view(x.shape)
        sv = torch.empty(src.numel() + 1, dtype=torch.float32, device=DEV)[1:].view(src.shape)
        xv.copy_(xd), sv.copy_(sd)
        assert xv.data_ptr() % 16 == 4 and sv.data_ptr() % 16 == 4 and xv.is_contiguous()
    for scale in fc.SUMPOOL_SCALES:
        same(ops.sumpool2x2(xd, scale), fc.sumpool(x, scale), "sumpool2x2 C=%d scale %g" % (C, scale))
        same(ops.broadcast2x2(sd, scale), fc.broadcast2x2(src, scale), "broadcast2x2 C=%d scale %g" % (C, scale))
        if C == fc.MISALIGNED_C:
            same_bits(ops.sumpool2x2(xv, scale), ops.sumpool2x2(xd, scale), "sumpool2x2 on a misaligned view, scale %g" % scale)
            same_bits(ops.broadcast2x2(sv, scale), ops.broadcast2x2(sd, scale), "broadcast2x2 on a misaligned view, scale %g" % scale)


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_pool_ties_go_to_the_first_maximum(k):
    x, win = tie_case(k)
    x = x.float()
    dy = torch.arange(1, 9, dtype=torch.float32).reshape(1, 1, 1, 8)
    same(ops.maxpool2x2(dev(x)), fc.maxpool(x), "maxpool2x2, tie at %d" % k)
    dx = ops.maxpool2x2_bwd(dev(x), dev(dy))
    same(dx, fc.maxpool_bwd(x, dy), "maxpool2x2_bwd, tie at %d" % k)
    dxw = _windows(dx.cpu())[0, 0, 0]
    for c in range(8):
        assert int(dxw[c].argmax()) == win[c] and int((dxw[c] != 0).sum()) == 1, (k, c, dxw[c])


@pytest.mark.parametrize("kind", ["signed_zeros", "equal_negative"])
def test_pool_window_edge_cases(kind):
    x, win = fc.pool_window_case(kind)
    dy = torch.tensor([1.0, 2.0, 3.0, 4.0]).reshape(1, 1, 1, 4)
    same(ops.maxpool2x2(dev(x)), fc.maxpool(x), "maxpool2x2 %s" % kind)
    dx = ops.maxpool2x2_bwd(dev(x), dev(dy))
    same(dx, fc.maxpool_bwd(x, dy), "maxpool2x2_bwd %s" % kind)
    dxw = _windows(dx.cpu())[0, 0, 0]
    for c in range(4):
        assert int(dxw[c].argmax()) == win[c] and int((dxw[c] != 0).sum()) == 1, (kind, c, dxw[c])


@pytest.mark.parametrize("c,tags", fc.WT_CASES, ids=lambda v: str(v) if isinstance(v, tuple) else "")
def test_conv_weight_transform(c, tags):
    w = fc.wt_input(c)
    same(ops.conv_weight_transform(dev(w)), fc.conv_weight_transform(w), "conv_weight_transform %s" % (c,))


# ---- head backward -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c, _ in fc.HEAD_CASES], ids=str)
def test_head_backward(c):
    N, H, W, Cin, Cout = c
    i = fc.head_inputs(c)
    e = fc.head_expected(i)
    x, w, dz = dev(i["x"]), dev(i["w"]), dev(i["dz"])
    k = fc.head_chain_adds(N * H * W)
    dx, dw, db = ops.conv1x1_small_bwd(x, w, dz)
    same(dx, e["dx"], "head dx %s" % (c,))
    assert tuple(dw.shape) == (1, 1, Cin, Cout) and tuple(db.shape) == (Cout,)
    ww = within(dw.reshape(Cin, Cout), e["dw64"], k * U * e["dw_abs"], "head dW %s, k = %d" % (c, k))
    wb = within(db, e["db64"], k * U * e["db_abs"], "head db %s, k = %d" % (c, k))
    print("conv1x1_small_bwd %s: k = %d, worst dW error %.3f, worst db error %.3f of the bound" % (c, k, ww, wb))
    none, dwn, dbn = ops.conv1x1_small_bwd(x, w, dz, want_dx=False)
    assert none is None
    gw, gb = Guarded((Cin * Cout,)), Guarded((Cout,))
    dx2, dws, dbs = ops.conv1x1_small_bwd(x, w, dz, dw_out=gw.out, db_out=gb.out)
    assert dws is gw.out and dbs is gb.out
    gw.check("conv1x1_small_bwd dw_out %s" % (c,)), gb.check("conv1x1_small_bwd db_out %s" % (c,))
    for name, other in (("want_dx=False", (dwn, dbn)), ("the sinks", (dws.view(dw.shape), dbs)),
                        ("a second call", ops.conv1x1_small_bwd(x, w, dz)[1:])):
        same_bits(other[0], dw, "head dW, %s" % name)
        same_bits(other[1], db, "head db, %s" % name)
    same_bits(dx2, dx, "head dx, a second call")


# ---- loss ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c, _ in fc.LOSS_CASES], ids=str)
def test_loss_against_fp64(c):
    """loss within 1e-6 relative (plus the derived term in the extreme case), dz within 2e-6 max|w| / npix |grad_scale|"""
    C, npix, kind = c
    i = fc.loss_inputs(c)
    z, y, w = dev(i["z"]), dev(i["onehot"]), dev(i["wgt"])
    results = []
    for gs in fc.LOSS_GRAD_SCALES:
        l64, ltol, dz64, dztol = fc.loss_bounds(c, i, gs)
        loss, dz = ops.wsoftmax_ce(z, y, w, grad_scale=gs)
        assert loss.dtype == torch.float64 and dz.dtype == torch.float32 and tuple(dz.shape) == (npix, C)
        lerr = abs(float(loss) - l64)
        print("wsoftmax_ce %s grad_scale %g: loss %.9g, fp64 %.9g, error %.3f of the bound" % (c, gs, float(loss), l64, lerr / max(ltol, 1e-300)))
        assert lerr <= ltol, "loss %s: error %.3g past %.3g" % (c, lerr, ltol)
        loss2, none = ops.wsoftmax_ce(z, y, w, want_grad=False, grad_scale=gs)
        assert none is None
        assert torch.equal(loss2.view(torch.int64), loss.view(torch.int64)), "loss without the gradient: other bits"
        loss3, dz3 = ops.wsoftmax_ce(z, y, w, grad_scale=gs)
        assert torch.equal(loss3.view(torch.int64), loss.view(torch.int64)), "loss, a second call: other bits"
        same_bits(dz3, dz, "dz, a second call")
        results.append((gs, dz, dz64, dztol))
    zero_rows = (i["onehot"].sum(-1) == 0)
    assert bool((results[0][1].cpu()[zero_rows] == 0).all()) and int(zero_rows.sum()) > 0, "an all-zero label row has no gradient"
    for gs, dz, dz64, dztol in results:
        worst = float((dz.double().cpu() - dz64).abs().max()) / dztol
        print("wsoftmax_ce %s grad_scale %g: worst dz error %.3f of the bound" % (c, gs, worst))
    for gs, dz, dz64, dztol in results:
        within(dz, dz64, torch.full_like(dz64, dztol), "dz %s grad_scale %g" % (c, gs))


@pytest.mark.parametrize("c", [c for c, _ in fc.LOSS_CASES], ids=str)
def test_argmax_lowest_index_wins(c):
    C, npix, kind = c
    z = fc.loss_inputs(c)["z"].clone()
    z[5] = 1.0                                                  # every class tied
    z[6, C // 2:] = 99.0                                        # the upper classes tied
    m = ops.argmax_u8(dev(z))
    same(m, fc.argmax_u8(z), "argmax_u8 %s" % (c,))
    assert int(m[5]) == 0 and int(m[6]) == C // 2


# ---- refusals ------------------------------------------------------------------------------------------------------------
def _z(*shape, **kw):
    return torch.zeros(shape, dtype=kw.get("dtype", torch.float32), device=DEV)


def _misaligned(n, dtype=torch.float32):
    """n elements that start one element into a buffer of n + 4: inside the buffer, off the alignment"""
    return torch.zeros(n + 4, dtype=dtype, device=DEV)[1:1 + n]


def test_refusals_are_loud():
    bad = (_lib.SequitrHipError, ValueError)
    n, shape = fc.REFUSAL_N, fc.REFUSAL_SHAPE
    N, H, W, C = shape
    u8 = torch.uint8
    st = lambda: _state(0)                                      # noqa: E731
    holes = {
        "bridge_bwd: a longer": lambda: ops.bridge_bwd(_z(n), _z(n + 4), _z(n), "eltwise_mul"),
        "bridge_bwd: b float64": lambda: ops.bridge_bwd(_z(n), _z(n), _z(n, dtype=torch.float64), "eltwise_mul"),
        "maxpool2x2_bwd: dy oversize": lambda: ops.maxpool2x2_bwd(_z(2, 4, 4, 8), _z(2, 3, 2, 8)),
        "dropout_fwd: mask longer": lambda: ops.dropout_fwd(_z(n), 0.4, mask=_z(n + 4, dtype=u8)),
        "dropout_bwd: mask longer": lambda: ops.dropout_bwd(_z(n), _z(n + 4, dtype=u8), 0.4),
        "space_to_depth2: odd H": lambda: ops.space_to_depth2(_z(2, 5, 4, 8)),
        "space_to_depth2: odd W": lambda: ops.space_to_depth2(_z(2, 4, 5, 8)),
        "gather_odd2x: odd H": lambda: ops.gather_odd2x(_z(2, 5, 4, 8)),
        "gather_odd2x: odd W": lambda: ops.gather_odd2x(_z(2, 4, 5, 8)),
        "conv1x1_small_bwd: w (1,1,16,2) for Cin 8": lambda: ops.conv1x1_small_bwd(_z(2, 4, 4, 8), _z(1, 1, 16, 2), _z(2, 4, 4, 2)),
        "conv1x1_small_bwd: dz with 4 channels for Cout 2": lambda: ops.conv1x1_small_bwd(_z(2, 4, 4, 8), _z(1, 1, 8, 2), _z(2, 4, 4, 4)),
        "adam_step_dev: g longer": lambda: ops.adam_step_dev(_z(n), _z(n + 4), _z(n), _z(n), 1e-3, 0.9, 0.999, 1e-8, st()),
        "adam_step_dev: m longer": lambda: ops.adam_step_dev(_z(n), _z(n), _z(n + 4), _z(n), 1e-3, 0.9, 0.999, 1e-8, st()),
        "adam_apply_dev: v longer": lambda: ops.adam_apply_dev(_z(n), _z(n), _z(n), _z(n + 4), 0.9, 0.999, 1e-8, st()),
        "bn_apply: scale longer": lambda: ops.bn_apply(_z(*shape), _z(12), _z(8)),
        "bn_apply: shift longer": lambda: ops.bn_apply(_z(*shape), _z(8), _z(12)),
        "bn_bwd: mean longer": lambda: ops.bn_bwd(_z(*shape), _z(*shape), None, None, _z(12), _z(8), _z(8)),
        "bn_bwd: var longer": lambda: ops.bn_bwd(_z(*shape), _z(*shape), None, None, _z(8), _z(12), _z(8)),
        "bn_bwd: gamma longer": lambda: ops.bn_bwd(_z(*shape), _z(*shape), None, None, _z(8), _z(8), _z(12)),
        "bn_bwd: dy oversize": lambda: ops.bn_bwd(_z(*shape), _z(2, 5, 4, 8), None, None, _z(8), _z(8), _z(8)),
        "bn_bwd: y oversize": lambda: ops.bn_bwd(_z(*shape), _z(*shape), _z(2, 5, 4, 8), "relu", _z(8), _z(8), _z(8)),
    }
    assert set(holes) == {name for name, _, _, _ in fc.HOLES}
    already = {
        "maxpool2x2: odd H": lambda: ops.maxpool2x2(_z(1, 3, 4, 8)),
        "maxpool2x2: odd W": lambda: ops.maxpool2x2(_z(1, 4, 7, 8)),
        "avgpool2x2: odd H": lambda: ops.avgpool2x2(_z(1, 3, 4, 8)),
        "maxpool2x2_bwd: odd H": lambda: ops.maxpool2x2_bwd(_z(1, 3, 4, 8), _z(1, 1, 2, 8)),
        "maxpool2x2_bwd: odd W": lambda: ops.maxpool2x2_bwd(_z(1, 4, 7, 8), _z(1, 2, 3, 8)),
        "sumpool2x2: odd H": lambda: ops.sumpool2x2(_z(1, 3, 4, 8)),
        "maxpool2x2: C = 6": lambda: ops.maxpool2x2(_z(1, 4, 4, 6)),
        "avgpool2x2: C = 6": lambda: ops.avgpool2x2(_z(1, 4, 4, 6)),
        "maxpool2x2_bwd: C = 6": lambda: ops.maxpool2x2_bwd(_z(1, 4, 4, 6), _z(1, 2, 2, 6)),
        "upsample_nn2x: C = 6": lambda: ops.upsample_nn2x(_z(1, 2, 2, 6)),
        "zero_insert2x: C = 6": lambda: ops.zero_insert2x(_z(1, 2, 2, 6)),
        "gather_odd2x: C = 6": lambda: ops.gather_odd2x(_z(1, 4, 4, 6)),
        "space_to_depth2: C = 6": lambda: ops.space_to_depth2(_z(1, 4, 4, 6)),
        "broadcast2x2_act_bwd: C = 6": lambda: ops.broadcast2x2_act_bwd(_z(1, 2, 2, 6), _z(1, 4, 4, 6), 0.25, "leaky"),
        "act_bwd: n = 6": lambda: ops.act_bwd(_z(6), _z(6), "relu"),
        "bridge: n = 6": lambda: ops.bridge(_z(6), _z(6), "eltwise_add"),
        "bridge_bwd: n = 6": lambda: ops.bridge_bwd(_z(6), _z(6), _z(6), "eltwise_mul"),
        "dropout_fwd: n = 6": lambda: ops.dropout_fwd(_z(6), 0.4),
        "dropout_bwd: n = 6": lambda: ops.dropout_bwd(_z(6), _z(6, dtype=u8), 0.4),
        "conv1x1_small_bwd: Cin = 24": lambda: ops.conv1x1_small_bwd(_z(1, 4, 4, 24), _z(1, 1, 24, 2), _z(1, 4, 4, 2)),
        "conv1x1_small_bwd: Cout = 5": lambda: ops.conv1x1_small_bwd(_z(1, 4, 4, 8), _z(1, 1, 8, 5), _z(1, 4, 4, 5)),
        "wsoftmax_ce: C = 9": lambda: ops.wsoftmax_ce(_z(16, 9), _z(16, 9, dtype=u8), _z(16, 1)),
        "bn_stats: C = 1028": lambda: ops.bn_stats(_z(1, 1, 2, 1028)),
        "bn_stats: C = 6": lambda: ops.bn_stats(_z(1, 1, 2, 6)),
        "dropout_fwd: rate = 1": lambda: ops.dropout_fwd(_z(n), 1.0),
        "dropout_bwd: rate = 1": lambda: ops.dropout_bwd(_z(n), _z(n, dtype=u8), 1.0),
        # alignment: only where the check stands in the source in front of the launch (sq_act_bwd_f32; the two added ones)
        "act_bwd: dy misaligned": lambda: ops.act_bwd(_misaligned(n), _z(n), "relu"),
        "bridge_bwd: a misaligned (eltwise_mul)": lambda: ops.bridge_bwd(_z(n), _misaligned(n), _z(n), "eltwise_mul"),
        "bridge_bwd: b misaligned (eltwise_mul)": lambda: ops.bridge_bwd(_z(n), _z(n), _misaligned(n), "eltwise_mul"),
        "dropout_fwd: mask misaligned": lambda: ops.dropout_fwd(_z(n), 0.4, mask=_misaligned(n, u8)),
        "dropout_bwd: mask misaligned": lambda: ops.dropout_bwd(_z(n), _misaligned(n, u8), 0.4),
    }
    for name, call in list(holes.items()) + list(already.items()):
        try:
            call()
        except bad + ((TypeError,) if "float64" in name else ()):
            continue
        raise AssertionError("%s was not refused" % name)
    torch.cuda.synchronize()
