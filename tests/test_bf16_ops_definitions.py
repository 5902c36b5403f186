"""CPU only: what tests/test_gpu_bf16_ops_sweep.py trusts is checked here first.

* Every emulation of tests/bf16_ops_cases.py against fp64: the fp64 side is torch autograd of the forward expression (or
  torch's max_pool2d, whose tie rule is also first-wins), never the emulation's own code.  A one-rounding op must be within
  |ref| * 2^-7 of fp64, a two-rounding op within 2 * |ref| * 2^-7 (each RNE rounding to bf16 is at most 2^-8 relative, the
  f32 operation under it 2^-24), on every element of inputs that hold ties, zero windows and exact zeros.
* The numpy restatement of the dropout mask: deterministic, seed- and step-dependent, all-kept at rate 0, kept share within
  four standard deviations of p over 2^20 elements, one byte per element and quad q = elements 4q .. 4q+3.
* The case tables reach every regime the sweep is there for, recomputed from the shapes.
* Building every reference of the GPU file is affordable (asserted: under a minute).  Measured on 8 CPU threads: 3.4 s in
  all -- flat 0.3 s, pool and space-to-depth 1.5 s, transpose conv and head 1.5 s."""
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from tests import bf16_ops_cases as bc

BF16 = torch.bfloat16
ULP = 2.0 ** -7


def _within(emu, ref64, roundings, what):
    err = (emu.double() - ref64).abs()
    tol = roundings * ref64.abs() * ULP
    worst = float((err / tol.clamp(min=1e-300)).max()) if err.numel() else 0.0
    print("%s: worst error %.3f of the bound (%d rounding%s)" % (what, worst, roundings, "s" if roundings > 1 else ""))
    assert bool((err <= tol).all()), "%s: %d elements past %d bf16 roundings, worst %.3f of the bound" % (
        what, int((err > tol).sum()), roundings, worst)


def _pool_shapes():
    return [s for s, _ in bc.POOL_CASES if s != bc.BIG_POOL] + [(2, 36, 38, 64)]


def _pool_grad64(x, dy):
    """torch autograd of max_pool2d in fp64 (first maximum wins, as in the kernels)"""
    xt = x.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = TF.max_pool2d(xt, 2, 2)
    y.backward(dy.double().permute(0, 3, 1, 2))
    return y.detach().permute(0, 2, 3, 1), xt.grad.permute(0, 2, 3, 1)


def _tied(shape):
    """pool inputs with many ties: five values over four positions, and the workload-like input of the sweep"""
    i = bc.pool_inputs(shape)
    g = bc._gen(9, *shape)
    i["x_ties"] = torch.randint(-1, 4, shape, generator=g).to(BF16)
    return i


@pytest.mark.parametrize("shape", _pool_shapes(), ids=str)
def test_pool_emulations_against_fp64_autograd(shape):
    i = _tied(shape)
    for name in ("x", "x_ties"):
        x = i[name]
        y64, dx64 = _pool_grad64(x, i["dy"])
        assert torch.equal(bc.maxpool(x).double(), y64), name
        assert torch.equal(bc.maxpool_bwd(x, i["dy"]).double(), dx64), name        # values move, nothing rounds
        _within(bc.maxpool_bwd_add(x, i["dy"], i["add"]), dx64 + i["add"].double(), 1, "pool bwd + add (%s)" % name)
        gated = (dx64 + i["add"].double()) * (x.double() > 0) * bc.GATE
        _within(bc.maxpool_bwd_add(x, i["dy"], i["add"], bc.GATE), gated, 2, "pool bwd + add, gated (%s)" % name)


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_hand_made_ties_go_to_the_first_maximum(k):
    x, win = bc.tie_case(k)
    dy = torch.arange(1, 9, dtype=torch.float32).reshape(1, 1, 1, 8).to(BF16)
    dxw = bc._windows(bc.maxpool_bwd(x, dy).float())[0, 0, 0]                       # (8, 4)
    for c in range(8):
        want = torch.zeros(4)
        want[win[c]] = float(dy[0, 0, 0, c])
        assert torch.equal(dxw[c], want), (k, c, dxw[c])
    assert win[:6] == [min(k, j) for j in bc.TIE_PARTNER[k]]                        # a last-wins rule would pick max(k, j)
    _, dx64 = _pool_grad64(x, dy)
    assert torch.equal(bc.maxpool_bwd(x, dy).double(), dx64)
    assert torch.equal(bc.maxpool(x).float().reshape(-1), torch.tensor([2.0] * 6 + [3.0, 0.0]))


def _autograd(f, *ops):
    """gradients of sum(f(*ops) * dy) in fp64; f's last argument is dy"""
    leaves = [o.double().clone().requires_grad_(True) for o in ops[:-1]]
    f(*leaves).backward(ops[-1].double())
    return [t.grad for t in leaves]


@pytest.mark.parametrize("n", [8 * 37, 8 * 1000, 8 * 8191])
def test_flat_emulations_against_fp64_autograd(n):
    i = bc.flat_inputs(n)
    dy, y, a, b, mask = i["dy"], i["y"], i["a"], i["b"], i["mask"]
    keep = mask.double() / (1.0 - bc.RATE)
    assert int((y == 0).sum()) >= n // 7 and 0.5 < float(mask.float().mean()) < 0.7
    fwd = {"relu": TF.relu, "leaky": lambda t: TF.leaky_relu(t, 0.2), "none": lambda t: t * 1.0}
    for act in bc.ACTS:
        (g64,) = _autograd(fwd[act], y, dy)
        _within(bc.act_bwd(dy, y, act), g64, 1, "act_bwd %s" % act)
        (g64,) = _autograd(lambda t: fwd[act](t) * keep, y, dy)
        _within(bc.act_dropout_bwd(dy, mask, y, bc.RATE, act), g64, 1 if act != "leaky" else 2, "act_dropout_bwd %s" % act)
    op = {"eltwise_add": lambda p, q: p + q, "eltwise_mul": lambda p, q: p * q, "eltwise_sub": lambda p, q: p - q}
    for kind in bc.KINDS:
        _within(bc.bridge(a, b, kind), op[kind](a.double(), b.double()), 1, "bridge %s" % kind)
        da64, db64 = _autograd(op[kind], a, b, dy)
        da, db = bc.bridge_bwd(dy, a, b, kind)
        _within(da, da64, 1, "bridge_bwd %s da" % kind)
        _within(db, db64, 1, "bridge_bwd %s db" % kind)
    _within(bc.dropout_fwd(a, mask, bc.RATE), a.double() * keep, 1, "dropout_fwd")
    (g64,) = _autograd(lambda t: t * keep, a, dy)
    _within(bc.dropout_bwd(dy, mask, bc.RATE), g64, 1, "dropout_bwd")
    (g64,) = _autograd(lambda t: TF.relu(t) * bc.GATE, y, dy)
    _within(bc.relu_scale_bwd(dy, y, bc.GATE), g64, 1, "relu_scale_bwd")
    f = torch.randn(n, generator=bc._gen(8, n))
    _within(bc.to_bf16(f), f.double(), 1, "to_bf16")
    assert torch.equal(bc.to_f32(bc.to_bf16(f)).double(), bc.to_bf16(f).double())


@pytest.mark.parametrize("shape", [s for s, _ in bc.S2D_CASES[:4]], ids=str)
def test_space_to_depth_bridge_backward_against_its_index_definition(shape):
    i = bc.s2d_inputs(shape)
    N, H2, W2, C = shape
    for kind in bc.KINDS:
        g, dskip = bc.bridge_bwd_s2d(i["dy"], i["up"], i["skip"], kind)
        da, db = bc.bridge_bwd(i["dy"], i["up"], i["skip"], kind)
        assert torch.equal(dskip.float(), db.float()) and tuple(g.shape) == (N, H2 // 2, W2 // 2, 4 * C)
        for a in range(2):
            for b in range(2):                                  # g[n,i,j,(2a+b)C + c] = d_up[n,2i+a,2j+b,c]
                assert torch.equal(g[..., (2 * a + b) * C:(2 * a + b + 1) * C].float(), da[:, a::2, b::2, :].float())


# ---- the mask ------------------------------------------------------------------------------------------------------------
def test_mask_restatement_is_deterministic_and_keyed_by_seed_and_step():
    n = 1 << 12
    m = bc.dropout_mask(n, 0.4, 3, 7)
    assert m.dtype == np.uint8 and m.shape == (n,) and set(np.unique(m)) == {0, 1}
    assert np.array_equal(m, bc.dropout_mask(n, 0.4, 3, 7))
    for other in ((0.4, 4, 7), (0.4, 3, 8), (0.4, 3, None)):
        d = float((bc.dropout_mask(n, *other) != m).mean())
        assert 0.3 < d < 0.7, (other, d)                       # independent masks differ at 2 p (1 - p) = 0.48
    assert np.array_equal(bc.dropout_mask(n, 0.4, 3, 0), bc.dropout_mask(n, 0.4, 3, None))   # step 0 adds nothing to the seed
    assert bc.dropout_mask(n, 0.0, 1).all()


@pytest.mark.parametrize("rate,seed,step", bc.MASK_SHARE_CASES)
def test_mask_restatement_keeps_the_share_it_should(rate, seed, step):
    n = 1 << 20
    p = 1.0 - np.floor(np.float32(rate) * 65536.0) / 65536.0
    assert p == bc.keep_probability(rate)
    share = float(bc.dropout_mask(n, rate, seed, step).mean())
    print("rate %g seed %d step %s: kept %.6f, p %.6f, 4 sigma %.6f" % (rate, seed, step, share, p, 4 * np.sqrt(p * (1 - p) / n)))
    assert abs(share - p) <= 4 * np.sqrt(p * (1 - p) / n)


def test_mask_layout_is_one_byte_per_element_and_one_hash_per_quad():
    key, thr = bc.dropout_key(3, 7), bc.dropout_thr16(0.4)
    m = bc.dropout_mask(4096, 0.4, 3, 7)
    for q in (0, 1, 2, 511, 1023):
        assert np.array_equal(m[4 * q:4 * q + 4], bc.dropout_keep4(key, [q], thr)[0].astype(np.uint8))
    assert np.array_equal(bc.dropout_mask(64, 0.4, 3, 7), m[:64])                   # a prefix: element i depends on i alone
    # the hash by hand for quad 0, seed 0, no step: s1 = 0x7F4A7C15, s2 = mix(0x68E31DA4 * 0x85EBCA6B)
    M = 0xFFFFFFFF
    s2 = (0x68E31DA4 * 0x85EBCA6B) & M
    s2 ^= s2 >> 13
    h = 0x7F4A7C15
    h ^= h >> 16
    h = (h * 0x7FEB352D) & M
    h = h ^ (h >> 15) ^ s2
    h = (h * 0x846CA68B) & M
    h ^= h >> 16
    g = ((h ^ 0x5BD1E995) * 0x2C1B3C6D) & M
    g ^= g >> 15
    thr = int(0.4 * 65536)
    want = [(h & 0xFFFF) >= thr, (h >> 16) >= thr, (g & 0xFFFF) >= thr, (g >> 16) >= thr]
    assert list(bc.dropout_mask(4, 0.4, 0)) == [int(v) for v in want]


# ---- fp64 definitions ------------------------------------------------------------------------------------------------------
def test_transpose_conv_definition_against_its_index_form():
    i = bc.convT_inputs((2, 3, 5, 32, 16))
    x, w, b = i["x"].double(), i["w"].to(BF16).double(), i["bias"].double()
    y = bc.convT64(i["x"], i["w"].to(BF16), i["bias"])
    for a in range(2):
        for c in range(2):                                      # y[n,2i+a,2j+c,o] = sum_k x[n,i,j,k] w[a,c,o,k] + bias[o]
            ref = torch.einsum("nijk,ok->nijo", x, w[a, c]) + b
            assert float((y[:, a::2, c::2] - ref).abs().max()) <= 1e-12
    e = bc.convT_expected(i)
    assert torch.equal(e["eltwise_sub"], e[None].to(BF16).double() - i["skip"].double())


def test_loss_definition_against_torch_cross_entropy():
    i = bc.head_inputs((2, 23, 25, 16, 3))
    z = bc.head_logits64(i["x"], i["w"], i["bias"]).requires_grad_(True)
    w = i["wgt"].double().reshape(-1)
    lab = i["onehot"].reshape(-1, 3).argmax(-1)
    loss = (TF.cross_entropy(z.reshape(-1, 3), lab, reduction="none") * w).mean()
    loss.backward()
    l64, dz64 = bc.wce64(z.detach(), i["onehot"], i["wgt"])
    assert abs(float(l64) - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    assert float((dz64 - z.grad).abs().max()) <= 1e-15
    dw, db, aw, ab = bc.head_wgrad64(i["x"], i["dz"])
    assert tuple(dw.shape) == (16, 3) and bool((dw.abs() <= aw).all()) and bool((db.abs() <= ab).all())


# ---- the tables ------------------------------------------------------------------------------------------------------------
def _missing(cases, tags_of, needed):
    reached = set()
    for shape, declared in cases:
        got = tags_of(shape)
        assert declared <= got, "%s is in the table for %s but its shape gives %s" % (shape, sorted(declared - got), sorted(got))
        reached |= declared
    return sorted(needed - reached)


def test_the_sweep_reaches_every_regime():
    missing = {}
    flat = {r for n, r in bc.FLAT_CASES if bc.flat_regime(n, 8) == r and n % 8 == 0}
    cast = {r for n, r in bc.CAST_CASES if bc.flat_regime(n, 4) == r and n % 4 == 0}
    assert len(flat) == len(bc.FLAT_CASES) and len(cast) == len(bc.CAST_CASES), "a flat case is not in the regime it names"
    missing["flat"] = sorted(bc.STREAM_NEEDED - flat)
    missing["cast"] = sorted(bc.STREAM_NEEDED - cast)
    missing["pool"] = _missing(bc.POOL_CASES, bc.spatial_tags, bc.SPATIAL_NEEDED)
    missing["s2d"] = _missing(bc.S2D_CASES, bc.s2d_tags, bc.SPATIAL_NEEDED)
    missing["convT"] = _missing(bc.CONVT_CASES, bc.convT_tags, bc.CONVT_NEEDED)
    missing["head"] = _missing(bc.HEAD_CASES, bc.head_tags, bc.HEAD_NEEDED)
    missing = {k: v for k, v in missing.items() if v}
    assert not missing, "no case reaches: %s" % missing
    assert bc.stream_regime(2 * 181 * 183 * 8) == "above_cap_ragged" and 2 * 181 * 183 * 8 == 529968
    for shape, _ in bc.POOL_CASES + bc.S2D_CASES:               # what the wrappers take
        assert shape[1] % 2 == 0 and shape[2] % 2 == 0 and shape[3] % 8 == 0
    for c, _ in bc.HEAD_CASES:
        npix = c[0] * c[1] * c[2]
        assert bc.HEAD_K[bc.head_blocks(npix)] == bc.head_chain_adds(npix), c
    biggest = max([int(np.prod(s)) * 2 for s, _ in bc.POOL_CASES + bc.S2D_CASES] + [n * 4 for n, _ in bc.CAST_CASES] +
                  [c[0] * c[1] * c[2] * max(2 * c[3], 4 * c[4]) for c, _ in bc.HEAD_CASES])
    assert biggest < 64 << 20, "a tensor of %d bytes" % biggest


def test_pool_inputs_look_like_the_workload():
    """about a quarter of the windows all zero (relu, then a 0.4-rate dropout) and a few tied positive maxima"""
    zero, tied = bc.pool_input_statistics(bc.pool_inputs(bc.BIG_POOL)["x"])
    print("all-zero windows %.4f, tied positive maxima %d" % (zero, tied))
    assert zero >= 0.10 and tied >= 1


def test_the_head_bound_is_no_looser_than_the_existing_tolerance():
    """k * 2^-24 * sum |terms| <= atol 1e-4 + rtol 1e-5 |ref| (test_head_and_first_wgrad_bf16) at every head case"""
    for c, _ in bc.HEAD_CASES:
        i = bc.head_inputs(c)
        dw, db, aw, ab = bc.head_wgrad64(i["x"], i["dz"])
        k = bc.head_chain_adds(c[0] * c[1] * c[2])
        assert bool((k * 2.0 ** -24 * aw <= 1e-4 + 1e-5 * dw.abs()).all()), c
        assert bool((k * 2.0 ** -24 * ab <= 1e-4 + 1e-5 * db.abs()).all()), c


def test_the_references_are_affordable():
    t0 = time.perf_counter()
    for n, _ in bc.FLAT_CASES:
        bc.flat_expected(bc.flat_inputs(n))
    for n, _ in bc.CAST_CASES:
        bc.to_f32(bc.to_bf16(torch.randn(n, generator=bc._gen(8, n))))
    t1 = time.perf_counter()
    for shape, _ in bc.POOL_CASES:
        bc.pool_expected(bc.pool_inputs(shape))
    for shape, _ in bc.S2D_CASES:
        i = bc.s2d_inputs(shape)
        for kind in bc.KINDS:
            bc.bridge_bwd_s2d(i["dy"], i["up"], i["skip"], kind)
    t2 = time.perf_counter()
    for c, _ in bc.CONVT_CASES:
        bc.convT_expected(bc.convT_inputs(c))
    for c, _ in bc.HEAD_CASES:
        bc.head_expected(bc.head_inputs(c))
    t3 = time.perf_counter()
    print("references: flat %.1f s, spatial %.1f s, transpose conv and head %.1f s, total %.1f s" % (
        t1 - t0, t2 - t1, t3 - t2, t3 - t0))
    assert t3 - t0 < 60.0
