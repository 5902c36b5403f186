"""CPU only: what tests/test_gpu_f32_ops_sweep.py and tests/test_gpu_bn_sweep.py trust is checked here first.

* Every case table of tests/f32_ops_cases.py reaches every tag of its *_NEEDED set, and every entry's declared tags EQUAL the
  ones recomputed from the launch arithmetic (removing a case makes a needed tag go missing).
* The replays against independent definitions: torch's max_pool2d / avg_pool2d and their autograd in fp64 (where ties are
  absent; torch's own tie rule is first-wins too and is checked on the tied inputs), conv_transpose2d for the zero-insert +
  convolution identity, naive loops for the index maps, fp64 autograd of gamma (x - mu) / sqrt(var + eps) + beta for BN.
* A numpy restatement of bn_reduce_kernel + bn_stats_finish_kernel stays inside the variance tolerance, with a factor of
  BN_VAR_SPARE to spare, against the two-pass value on every BN case, the mean-100 channel included; the constant channel's
  variance is exactly 0 there.
* Each derived bound (k u sum |terms|) holds for a float32 numpy restatement of the kernel's own order on the table's inputs:
  Adam, the head's dW / db, the loss; and the BN gradient tolerance for the restated bn_bwd, f32 and bf16 operands.
* No refusal case could read or write out of range if its check were missing: the wrong operand is always the larger one."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from tests import f32_ops_cases as fc
from tests.bf16_ops_cases import ACTS, CAP, KINDS, RATE, STREAM_NEEDED, _windows, stream_regime, tie_case

U = fc.U


def _tables_ok(cases, tags_of, needed, what):
    reached = set()
    for c, declared in cases:
        got = tags_of(c)
        assert declared == got, "%s %s: declared %s, its shape gives %s" % (what, c, sorted(declared), sorted(got))
        reached |= declared
    assert not needed - reached, "%s: no case reaches %s" % (what, sorted(needed - reached))


# ---- the tables ----------------------------------------------------------------------------------------------------------
def test_every_table_reaches_every_regime():
    flat = {r for n, r in fc.FLAT_CASES if fc.flat_regime(n) == r and n % 4 == 0}
    assert len(flat) == len(fc.FLAT_CASES) and not STREAM_NEEDED - flat
    adam = {r for n, r in fc.ADAM_CASES if stream_regime(n) == r}
    assert len(adam) == len(fc.ADAM_CASES) and not STREAM_NEEDED - adam
    reached = set()
    for n, off, declared in fc.AXPY_CASES:
        assert declared == fc.axpy_tags(n, off), (n, off)
        reached |= declared
    assert not fc.AXPY_NEEDED - reached, sorted(fc.AXPY_NEEDED - reached)
    assert {n for n, off, _ in fc.AXPY_CASES if off} == {n - 1 for n, _ in fc.FLAT_CASES}
    multi = set().union(*(fc.adam_multi_tags(n) for n in fc.ADAM_MULTI_COUNTS))
    assert not fc.ADAM_MULTI_NEEDED - multi and set(fc.ADAM_MULTI_COUNTS) == {1, 2047, 2048, 2049, 3 * 2048 + 5, 300}
    _tables_ok(fc.SPATIAL_CASES, fc.spatial_tags, fc.SPATIAL_NEEDED, "spatial")
    _tables_ok(fc.WT_CASES, fc.wt_tags, fc.WT_NEEDED, "weight transform")
    _tables_ok(fc.HEAD_CASES, fc.head_tags, fc.HEAD_NEEDED, "head")
    _tables_ok(fc.LOSS_CASES, fc.loss_tags, fc.LOSS_NEEDED, "loss")
    _tables_ok(fc.BN_CASES, fc.bn_tags, fc.BN_NEEDED, "bn")


def test_every_spatial_operator_meets_the_stream_regimes_on_the_side_it_counts():
    """the operators that count items on the full side, or on other operands, still reach the three regimes"""
    for side, shapes in (("pooled", [s for s, _ in fc.SPATIAL_CASES]),                       # pools, sumpool, maxpool_bwd
                         ("full", [s for s, _ in fc.SPATIAL_CASES]),                         # broadcast2x2 (+ act_bwd), space_to_depth2
                         ("full", [fc.large_side(s) for s, _ in fc.SPATIAL_CASES]),          # upsample_nn2x, zero_insert2x
                         ("pooled", [fc.large_side(s) for s, _ in fc.SPATIAL_CASES])):       # gather_odd2x
        got = {stream_regime(fc.spatial_items(s, side)) for s in shapes}
        assert not STREAM_NEEDED - got, (side, sorted(STREAM_NEEDED - got))
    assert fc.spatial_items(fc.BIG_SPATIAL, "pooled") == 529968 > CAP
    for s, _ in fc.SPATIAL_CASES:
        assert s[1] % 2 == 0 and s[2] % 2 == 0 and s[3] % 4 == 0
    biggest = max(int(np.prod(fc.large_side(s))) * 4 for s, _ in fc.SPATIAL_CASES)
    assert biggest == 2 * 362 * 366 * 32 * 4 < 34 << 20


def test_head_k_is_the_recomputed_chain_length():
    for c, _ in fc.HEAD_CASES:
        npix = c[0] * c[1] * c[2]
        assert fc.HEAD_K[fc.head_blocks(npix)] == fc.head_chain_adds(npix), c
    assert fc.head_blocks(131684) == 512 and 131684 - 512 * 256 == 612 and fc.head_blocks(127900) == 500


# ---- replays against independent definitions -----------------------------------------------------------------------------
def _nchw(t):
    return t.double().permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


SMALL_SPATIAL = [s for s, _ in fc.SPATIAL_CASES if s != fc.BIG_SPATIAL] + [(2, 36, 38, 32)]


@pytest.mark.parametrize("shape", SMALL_SPATIAL, ids=str)
def test_pool_replays_against_torch_and_fp64_autograd(shape):
    i = fc.spatial_inputs(shape)
    x, dy = i["x"], i["dy"]
    xw = _windows(x)
    assert int(((xw == xw.max(-1, keepdim=True).values).sum(-1) > 1).sum()) == 0, "random f32 windows hold no ties"
    xt = _nchw(x).clone().requires_grad_(True)
    y = TF.max_pool2d(xt, 2, 2)
    y.backward(_nchw(dy))
    assert torch.equal(fc.maxpool(x).double(), _nhwc(y.detach()))
    assert torch.equal(fc.maxpool_bwd(x, dy).double(), _nhwc(xt.grad))
    a64 = _nhwc(TF.avg_pool2d(_nchw(x), 2, 2))
    err = (fc.avgpool(x).double() - a64).abs()                  # three f32 additions; the product by 0.25 is exact
    assert bool((err <= 2 * U * _windows(x).double().abs().sum(-1) * 0.25).all())
    for scale in fc.SUMPOOL_SCALES:
        err = (fc.sumpool(x, scale).double() - 4 * scale * a64).abs()
        assert bool((err <= 3 * U * _windows(x).double().abs().sum(-1) * scale).all())
    assert torch.equal(fc.avgpool(x), fc.sumpool(x, 0.25))
    # broadcast2x2 is the adjoint of sumpool2x2: fp64 autograd of scale * sum of the window
    for scale in fc.SUMPOOL_SCALES:
        lt = _nchw(i["gate"]).clone().requires_grad_(True)
        (TF.avg_pool2d(lt, 2, 2) * 4 * scale).backward(_nchw(dy))
        err = (fc.broadcast2x2(dy, scale).double() - _nhwc(lt.grad)).abs()
        assert bool((err <= U * _nhwc(lt.grad).abs()).all())
    assert torch.equal(fc.broadcast2x2(dy, 1.0), fc.upsample_nn2x(dy))
    for act in ACTS:
        g = fc.broadcast2x2(dy, 0.25)
        want = torch.where(i["gate"] > 0, g, g * torch.tensor(fc.SLOPE[act]))
        assert torch.equal(fc.broadcast2x2_act_bwd(dy, i["gate"], 0.25, act), want)
    assert int((i["gate"] == 0).sum()) >= i["gate"].numel() // 7 and bool(torch.signbit(i["gate"].view(-1)[7]))


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_pool_ties_go_to_the_first_maximum(k):
    x, win = tie_case(k)
    x = x.float()
    dy = torch.arange(1, 9, dtype=torch.float32).reshape(1, 1, 1, 8)
    dxw = _windows(fc.maxpool_bwd(x, dy))[0, 0, 0]
    for c in range(8):
        want = torch.zeros(4)
        want[win[c]] = float(dy[0, 0, 0, c])
        assert torch.equal(dxw[c], want), (k, c, dxw[c])
    xt = _nchw(x).clone().requires_grad_(True)
    TF.max_pool2d(xt, 2, 2).backward(_nchw(dy))
    assert torch.equal(fc.maxpool_bwd(x, dy).double(), _nhwc(xt.grad))


@pytest.mark.parametrize("kind", ["signed_zeros", "equal_negative"])
def test_pool_window_edge_cases(kind):
    x, win = fc.pool_window_case(kind)
    dy = torch.tensor([1.0, 2.0, 3.0, 4.0]).reshape(1, 1, 1, 4)
    dxw = _windows(fc.maxpool_bwd(x, dy))[0, 0, 0]
    for c in range(4):
        assert int(dxw[c].argmax()) == win[c] and int((dxw[c] != 0).sum()) == 1
    assert torch.equal(fc.maxpool(x), _windows(x)[..., 0])      # equal as numbers to position 0's value


@pytest.mark.parametrize("shape", SMALL_SPATIAL[:4], ids=str)
def test_index_maps_equal_their_naive_loops(shape):
    i = fc.spatial_inputs(shape)
    assert torch.equal(fc.upsample_nn2x(i["small"]), fc.upsample_loop(i["small"]))
    assert torch.equal(fc.space_to_depth2(i["x"]), fc.space_to_depth_loop(i["x"]))
    assert torch.equal(fc.zero_insert2x(i["small"]), fc.zero_insert_loop(i["small"]))
    assert torch.equal(fc.gather_odd2x(i["large"]), fc.gather_odd_loop(i["large"]))
    assert torch.equal(fc.gather_odd2x(fc.zero_insert2x(i["small"])), i["small"])            # the adjoint pair
    assert tuple(fc.space_to_depth2(i["x"]).shape) == (shape[0], shape[1] // 2, shape[2] // 2, 4 * shape[3])


@pytest.mark.parametrize("c", [c for c, _ in fc.WT_CASES[:9]], ids=str)
def test_weight_transform_equals_its_naive_loop(c):
    w = fc.wt_input(c)
    assert int(w.unique().numel()) == w.numel()                 # distinct values: a wrong index cannot hide
    assert torch.equal(fc.conv_weight_transform(w), fc.weight_transform_loop(w))


def test_zero_insert_then_conv_is_the_transpose_conv():
    """conv2d(zero_insert2x(x), conv_weight_transform(w)) with SAME padding = conv_transpose2d(k 3, s 2, SAME), w (3,3,Cout,Cin)"""
    g = fc._gen(21)
    x, w = fc._randn(g, (2, 5, 4, 8)), fc._randn(g, (3, 3, 4, 8))
    u = fc.zero_insert2x(x)
    wt = fc.conv_weight_transform(w)                            # (3,3,Cin,Cout) as an HWIO filter from Cin to Cout
    y = TF.conv2d(_nchw(u), wt.double().permute(3, 2, 0, 1), padding=1)
    # TF's SAME transpose conv at stride 2 and kernel 3: output 2H x 2W, i.e. padding 1 on the low side, output_padding 1
    ref = TF.conv_transpose2d(_nchw(x), w.double().permute(3, 2, 0, 1), stride=2, padding=1, output_padding=1)
    # zero insertion puts x at the ODD positions, so the two agree after the one-pixel shift that SAME's padding split implies
    full = TF.conv_transpose2d(_nchw(x), w.double().permute(3, 2, 0, 1), stride=2)       # (2H+1, 2W+1), no cropping
    assert float((y - full[:, :, :-1, :-1]).abs().max()) <= 1e-12
    assert ref.shape == y.shape


def test_flat_replays_against_fp64_autograd():
    i = fc.flat_inputs(4 * 1000)
    dy, y, a, b, mask = i["dy"], i["y"], i["a"], i["b"], i["mask"]
    assert int((y == 0).sum()) >= y.numel() // 7 and bool(torch.signbit(y[7])) and not bool(torch.signbit(y[0]))
    fwd = {"relu": TF.relu, "leaky": lambda t: TF.leaky_relu(t, 0.2), "none": lambda t: t * 1.0}
    for act in ACTS:
        yt = y.double().clone().requires_grad_(True)
        fwd[act](yt).backward(dy.double())
        # two roundings: the slope 0.2f itself and the product
        assert bool(((fc.act_bwd(dy, y, act).double() - yt.grad).abs() <= 2 * U * yt.grad.abs()).all()), act
    assert fc.act_bwd(dy, y, "none") is dy
    op = {"eltwise_add": lambda p, q: p + q, "eltwise_mul": lambda p, q: p * q, "eltwise_sub": lambda p, q: p - q}
    for kind in KINDS:
        at, bt = a.double().clone().requires_grad_(True), b.double().clone().requires_grad_(True)
        out = op[kind](at, bt)
        out.backward(dy.double())
        assert bool(((fc.bridge(a, b, kind).double() - out.detach()).abs() <= U * out.detach().abs()).all())
        da, db = fc.bridge_bwd(dy, a, b, kind)
        assert bool(((da.double() - at.grad).abs() <= U * at.grad.abs()).all())
        assert bool(((db.double() - bt.grad).abs() <= U * bt.grad.abs()).all())
    keep = mask.double() / (1.0 - float(np.float32(RATE)))
    for got, ref in ((fc.dropout_fwd(a, mask, RATE), a.double() * keep), (fc.dropout_bwd(dy, mask, RATE), dy.double() * keep)):
        assert bool(((got.double() - ref).abs() <= 3 * U * ref.abs()).all())     # 1 - rate, its reciprocal, the product
    for alpha in fc.AXPY_ALPHAS:
        assert torch.equal(fc.axpy(a, b, alpha).double(), fc.axpy64(a, b, alpha).float().double())
    z = fc.loss_inputs((3, 1000, "plain"))["z"]
    z[5] = 1.0                                                  # a three-way tie and a two-way tie: the lowest index
    z[6, 1:] = 9.0
    m = fc.argmax_u8(z)
    assert int(m[5]) == 0 and int(m[6]) == 1 and torch.equal(m.long(), z.max(-1).indices) and m.dtype == torch.uint8


# ---- derived bounds on float32 restatements --------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [n for n, _ in fc.ADAM_CASES] + list(fc.ADAM_MULTI_COUNTS))
def test_adam_bound_holds_for_the_restated_update(n):
    i = fc.adam_inputs(n)
    for warmup in fc.ADAM_WARMUPS:
        for step in fc.ADAM_STEPS:
            lr_t = np.float32(fc.adam_lr_t(step, warmup))
            worst = fc.adam_check("restated adam n=%d" % n, fc.adam_f32(i, lr_t), i, lr_t)
    print("adam n=%d: worst m %.3f, v %.3f, p %.3f of the bound" % (n, worst["m"], worst["v"], worst["p"]))
    assert abs(fc.adam_lr_t(1, 3) * 3 / fc.adam_lr_t(1) - 1) < 1e-15 and abs(fc.adam_lr_t(2, 3) * 1.5 / fc.adam_lr_t(2) - 1) < 1e-15
    assert fc.adam_lr_t(3, 3) == fc.adam_lr_t(3)                # the ramp is crossed at t = 3
    assert float(np.float32(1.0) - np.float32(fc.B1)) == 1.0 - float(np.float32(fc.B1))               # Sterbenz: exact


@pytest.mark.parametrize("c", [c for c, _ in fc.HEAD_CASES], ids=str)
def test_head_bound_holds_for_the_restated_reduction(c):
    i = fc.head_inputs(c)
    dw64, db64, aw, ab = fc.head_wgrad64(i["x"], i["dz"])
    k = fc.head_chain_adds(c[0] * c[1] * c[2])
    dw, db = fc.head_wgrad_f32(i)
    errw, errb = (dw.double() - dw64).abs(), (db.double() - db64).abs()
    tolw, tolb = k * U * aw, k * U * ab
    print("head %s: k = %d, restated dW %.3f, db %.3f of the bound" % (
        c, k, float((errw / tolw.clamp(min=1e-300)).max()), float((errb / tolb.clamp(min=1e-300)).max())))
    assert bool((errw <= tolw).all()) and bool((errb <= tolb).all())
    assert float((i["x"] == 0).float().mean()) > 0.5            # relu, then dropout: most of a block output is zero


@pytest.mark.parametrize("c", [c for c, _ in fc.LOSS_CASES], ids=str)
def test_loss_tolerances_hold_for_the_restated_pixel(c):
    """The loss bound (the extreme case's derived term included) and the dz tolerance on every case: sq_wce_pixel forms the
    softmax as exp((z - m) - log s), whose error does not grow with the logits (exp(z - lse) would be at 1.6 of the dz
    tolerance in the extreme case: lse is rounded at |lse| up to 80)."""
    i = fc.loss_inputs(c)
    for gs in fc.LOSS_GRAD_SCALES:
        l64, ltol, dz64, dztol = fc.loss_bounds(c, i, gs)
        loss, dz = fc.wce_f32(i, gs)
        print("loss %s gs %g: restated loss error %.3f, dz error %.3f of the bound" % (
            c, gs, abs(loss - l64) / max(ltol, 1e-300), float((dz.double() - dz64).abs().max()) / dztol))
        assert abs(loss - l64) <= ltol
        assert float((dz.double() - dz64).abs().max()) <= dztol


def test_loss_definition_against_torch_cross_entropy():
    i = fc.loss_inputs((3, 1000, "plain"))
    z = i["z"].double().requires_grad_(True)
    yt = i["onehot"].double().sum(-1)
    lab = i["onehot"].argmax(-1)
    (TF.cross_entropy(z, lab, reduction="none") * i["wgt"].double().reshape(-1) * yt).mean().backward()
    l64, _, dz64, _ = fc.loss_bounds((3, 1000, "plain"), i)
    assert float((dz64 - z.grad).abs().max()) <= 1e-15 and l64 > 0


# ---- batch normalisation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [s for s, _ in fc.BN_CASES], ids=str)
def test_bn_restated_statistics_keep_the_tolerance_with_room(shape):
    x = fc.bn_inputs(shape)["x"]
    mu, var = fc.bn_stats64(x)
    m, v, raw = fc.bn_stats_restated(x)
    merr = np.abs(m.astype(np.float64) - mu.numpy()) / (2e-7 * np.abs(mu.numpy()) + 1e-8)
    verr = np.abs(v.astype(np.float64) - var.numpy()) / (1e-6 * np.abs(var.numpy()) + 1e-9)
    print("bn %s: restated mean %.3f, variance %.3f of the tolerance (channel 1: %.3f)" % (shape, merr.max(), verr.max(), verr[1]))
    assert merr.max() <= 1.0 and verr.max() * fc.BN_VAR_SPARE <= 1.0
    assert v[0] == 0.0 and raw[0] == 0.0 and m[0] == np.float32(fc.BN_CONST)       # exactly 0 before the clamp, never negative
    assert float(var[0]) == 0.0 and (v >= 0).all()
    if shape[0] * shape[1] * shape[2] >= 100:
        assert abs(float(mu[1]) - fc.BN_MEAN) < 0.3 and 0.1 < float(var[1]) < 0.5


@pytest.mark.parametrize("shape", [s for s, _ in fc.BN_CASES], ids=str)
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_bn_backward_closed_form_autograd_and_restatement(shape, bf16):
    from oracle import c_oracle as co
    i = fc.bn_inputs(shape)
    x, dy, gamma, beta = i["x"], i["dy"], i["gamma"], i["beta"]
    if bf16:
        x, dy = x.to(torch.bfloat16).float(), dy.to(torch.bfloat16).float()
    mean, var = (torch.from_numpy(t) for t in co.bn_stats(x.numpy()))
    scale, shift = co.bn_fold(gamma.numpy(), beta.numpy(), mean.numpy(), var.numpy(), fc.BN_EPS)
    small = x.numel() <= 1 << 21
    for act in (None, "relu", "leaky"):
        y = torch.from_numpy(co.bn_apply(x.numpy(), scale, shift, act))
        if bf16:
            y = y.to(torch.bfloat16).float()
        d64 = fc.bn_dact(dy, y, act)
        dx64, dg64, db64 = fc.bn_bwd64(x, d64, gamma)
        if small and act is None:                               # the closed form against autograd of the definition
            xt, gt = x.double().clone().requires_grad_(True), gamma.double().clone().requires_grad_(True)
            bt = beta.double().clone().requires_grad_(True)
            mu = xt.reshape(-1, shape[3]).mean(0)
            vr = ((xt - mu) ** 2).reshape(-1, shape[3]).mean(0)
            (gt * (xt - mu) / torch.sqrt(vr + fc.BN_EPS) + bt).backward(d64)
            for a, b in ((dx64, xt.grad), (dg64, gt.grad), (db64, bt.grad)):
                assert float((a - b).abs().max()) <= 1e-9 * max(1.0, float(b.abs().max()))
        dx, dg, db = fc.bn_bwd_f32(x, fc.bn_dact(dy, y, act, torch.float32), mean, var, gamma)
        fr = [fc.grad_close(dg, dg64, "dgamma"), fc.grad_close(db, db64, "dbeta")]
        if bf16:
            g, r = dx.to(torch.bfloat16).double(), dx64.to(torch.bfloat16).double()
            bad = (g - dx64).abs() > r.abs().clamp(min=1e-30) * 2.0 ** -7 + 1e-6
            assert not bool(bad.any()), "restated bf16 dx: %d values off by more than one bf16 ulp" % int(bad.sum())
            assert float((g == r).double().mean()) > 0.95
        else:
            fr.append(fc.grad_close(dx, dx64, "dx"))
        print("bn_bwd %s %s %s: restated errors %s of the tolerance" % (shape, "bf16" if bf16 else "f32", act, ["%.3f" % f for f in fr]))


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_every_refusal_case_has_the_larger_operand_wrong():
    names = " ".join(n for n, _, _, _ in fc.HOLES)
    for op in ("bridge_bwd", "maxpool2x2_bwd", "dropout_fwd", "dropout_bwd", "space_to_depth2", "gather_odd2x",
               "conv1x1_small_bwd", "adam_step_dev", "adam_apply_dev", "bn_apply", "bn_bwd"):
        assert op + ":" in names, "no refusal case for %s" % op
    for name, operand, given, covered in fc.HOLES:
        assert given > covered > 0, "%s: the wrong %s must be LARGER than what an unchecked launch would touch" % (name, operand)
