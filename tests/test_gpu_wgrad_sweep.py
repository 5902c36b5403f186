"""GPU: the weight gradients at every block shape, kind, prefetch phase and group path their plans reach
(tests/wgrad_sweep_cases.py; tests/test_wgrad_plan.py checks on the CPU that the tables reach every plan), each against a
DEFINITION -- sums over shifted views in fp64 (for the transpose conv, its 2x2 / stride-2 definition), never another kernel.

Exact oracle (indexing): X and dY are integers in -3..3.  Every product and partial sum is an integer below 2^24 (asserted in
test_wgrad_plan.py), so f32, bf16 MFMA and any summation order are exact: the kernel must equal fp64 bit for bit, whatever the
plan.  dW * dw_scale is f32(f32(S) * scale), an accumulated destination f32(prior + that).  First-write destinations start as
NaN, and dW, db and the workspace sit between guard bands that must come back untouched (the workspace: past what its query
returned as well).

Rounding oracle (precision): real operands, one case per (family, shape, kind).  Reference: fp64 on the operands the kernel
multiplies (bf16 RNE-rounded for bf16 / mixed).  Per element |got - ref| <= 2^-20 * sum_p |x_p dy_p|.  A block's chain of f32
additions is at most ~2 x 7 MFMA steps of its tile run + 4 waves + the finish's <= 2^7 / 16 + 4 partials, about 30 roundings of
partial sums each below the absolute sum: <= 30 * 2^-24 < 2^-19 in the worst case, and in practice far less, so 2^-20 holds
with margin while a truncating conversion (2^-8 per operand) is far outside.  Every rounding case runs twice: bit-identical."""
import zlib

import numpy as np
import pytest
import torch

from sequitr_amd import _lib, ops
from sequitr_amd import ops_bf16 as ob
from sequitr_amd import ops_gan_bf16 as og
from sequitr_amd.ops import _ptr, _stream
from tests import wgrad_sweep_cases as ws

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
GUARD = 4096                                                    # floats on either side of every destination
SENTINEL = 0x7FA5A5A5                                           # a NaN payload no kernel writes
DEV = "cuda:0"


def _rng(*key):
    g = torch.Generator(device=DEV)
    g.manual_seed(zlib.crc32(repr(key).encode()))
    return g


def _operand(rng, shape, exact):
    if exact:
        return torch.randint(-3, 4, shape, generator=rng, device=DEV).float()
    return torch.randn(shape, generator=rng, device=DEV)


class Guarded(object):
    """n floats inside an allocation with SENTINEL guard bands; fill: NaN (first write) or given values"""

    def __init__(self, n, fill=None):
        self.n = n
        self.buf = torch.empty(n + 2 * GUARD, dtype=torch.float32, device=DEV)
        self.buf.view(torch.int32).fill_(SENTINEL)
        self.t = self.buf[GUARD:GUARD + n]
        if fill is None:
            self.t.fill_(float("nan"))
        else:
            self.t.copy_(fill.reshape(-1))

    def ptr(self):
        return self.t.data_ptr()

    def check(self, what):
        g = self.buf.view(torch.int32)
        assert bool((g[:GUARD] == SENTINEL).all()) and bool((g[GUARD + self.n:] == SENTINEL).all()), \
            "%s: a guard band was written" % what


class Workspace(Guarded):
    def __init__(self, nbytes):
        assert nbytes >= 0 and nbytes % 4 == 0
        Guarded.__init__(self, nbytes // 4, torch.zeros(nbytes // 4, device=DEV))
        self.t.view(torch.int32).fill_(SENTINEL)               # not even the reserved room is assumed clean


def wgrad64(x, dy, K):
    """dW[ky, kx, ci, co] = sum_p X[p + (ky - K//2, kx - K//2)][ci] * dY[p][co] (zero outside each image), db = sum_p dY[p]"""
    x, dy = x.double(), dy.double()
    N, H, W, Cin = x.shape
    pad = K // 2
    xp = torch.nn.functional.pad(x, (0, 0, pad, pad, pad, pad))
    d = dy.reshape(-1, dy.shape[3])
    dw = torch.stack([torch.stack([xp[:, ky:ky + H, kx:kx + W, :].reshape(-1, Cin).t() @ d for kx in range(K)])
                      for ky in range(K)])
    return dw, d.sum(0)


def convT_wgrad64(x, G):
    """the 2x2 / stride-2 transpose conv y[n, 2i+a, 2j+b, c] = sum_ci x[n, i, j, ci] W[a, b, c, ci] + bias[c], from its full
    output gradient G: dW[a, b, c, ci] = sum x[n, i, j, ci] G[n, 2i+a, 2j+b, c], db[c] = sum G[..., c]"""
    x, G = x.double(), G.double()
    xf = x.reshape(-1, x.shape[3])
    dw = torch.stack([torch.stack([(xf.t() @ G[:, a::2, b::2, :].reshape(-1, G.shape[3])).t() for b in range(2)])
                      for a in range(2)])
    return dw, G.reshape(-1, G.shape[3]).sum(0)


def space_to_depth(G):
    """g[n, i, j, (2a+b) C + c] = G[n, 2i+a, 2j+b, c]: the layout sq_convT2x2s2_wgrad_bf16 reads"""
    N, H2, W2, C = G.shape
    return G.reshape(N, H2 // 2, 2, W2 // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, H2 // 2, W2 // 2, 4 * C).contiguous()


def operands(c, exact, seed=0):
    """(x, dy as the kernel takes them, the fp64 values it multiplies, the full-res G of a transpose conv)"""
    rng = _rng(c["fam"], c["N"], c["H"], c["W"], c["Cin"], c["Cout"], c["K"], c.get("convT", 0), exact, seed)
    x = _operand(rng, (c["N"], c["H"], c["W"], c["Cin"]), exact)
    G = None
    if c.get("convT"):
        G = _operand(rng, (c["N"], 2 * c["H"], 2 * c["W"], c["convT"]), exact)
        dy = space_to_depth(G)
    else:
        dy = _operand(rng, (c["N"], c["H"], c["W"], c["Cout"]), exact)
    if c["fam"] == "bf16":
        x, dy = x.to(BF), dy.to(BF)
        xm, ym = x.double(), dy.double()
    elif c["fam"] == "mixed":
        xm, ym = x.to(BF).double(), dy.to(BF).double()       # the loader rounds to bf16, to nearest even
    elif c["fam"] == "first":
        dy = dy.to(BF)
        xm, ym = x.double(), dy.double()
    else:
        xm, ym = x.double(), dy.double()
    if G is not None:
        G = G.to(BF).double() if c["fam"] == "bf16" else G.double()
    return x, dy, xm, ym, G


def reference(c, xm, ym, G, absolute=False):
    if absolute:
        xm, ym, G = xm.abs(), ym.abs(), (G.abs() if G is not None else None)
    if c.get("convT"):
        return convT_wgrad64(xm, G)
    return wgrad64(xm, ym, c["K"])


def run(c, x, dy, dw, db, ws_):
    """one call of the entry the case names"""
    lib = _lib.load()
    N, H, W, Cin, Cout, K, s = c["N"], c["H"], c["W"], c["Cin"], c["Cout"], c["K"], float(c.get("scale", 1.0))
    dbp = db.ptr() if db is not None else None
    a = (_ptr(x), _ptr(dy), dw.ptr(), dbp, ws_.ptr())
    if c.get("convT"):
        rc, who = lib.sq_convT2x2s2_wgrad_bf16(*a, N, H, W, Cin, c["convT"], _stream()), "convT"
    elif c.get("mosaic"):
        R, Cc = c["mosaic"]
        fn = lib.sq_conv2d_nhwc_wgrad_mosaic_bf16 if c["fam"] == "bf16" else lib.sq_conv2d_nhwc_wgrad_mixed_mosaic_f32
        rc, who = fn(*a, N, H, W, Cin, Cout, R, Cc, s, _stream()), "mosaic"
    elif c["fam"] == "first":
        rc, who = lib.sq_conv3x3_first_wgrad_bf16(*a, N, H, W, Cin, Cout, _stream()), "first"
    else:
        fn = {"bf16": lib.sq_conv2d_nhwc_wgrad_scaled_bf16, "mixed": lib.sq_conv2d_nhwc_wgrad_scaled_mixed_f32,
              "f32": lib.sq_conv2d_nhwc_wgrad_scaled_f32}[c["fam"]]
        rc, who = fn(*a, N, H, W, Cin, Cout, K, s, _stream()), c["fam"]
    _lib.check(rc, who)


def ws_bytes(c):
    p = ws.case_plan(c)
    return int(p["ws"]) * 4


def dw_shape(c):
    return (2, 2, c["convT"], c["Cin"]) if c.get("convT") else (c["K"], c["K"], c["Cin"], c["Cout"])


def db_len(c):
    return c["convT"] if c.get("convT") else c["Cout"]


def _id(c):
    return "%s-%dx%dx%dx%d-%d-%d-K%d%s%s" % (c["fam"], c["N"], c["H"], c["W"], c["Cin"], c["Cout"], c.get("convT", 0), c["K"],
                                           "-mos%dx%d" % tuple(c["mosaic"]) if c.get("mosaic") else "",
                                           "" if c.get("bias", True) else "-nob")


def f32_scaled(S, scale):
    return (S.float() * torch.tensor(scale, dtype=torch.float32, device=S.device)).float()


def assert_bits(got, want, what):
    g, w = got.reshape(-1).float(), want.reshape(-1).float()
    bad = g.view(torch.int32) != w.view(torch.int32)
    bad &= ~((g == 0) & (w == 0))
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        raise AssertionError("%s: %d of %d elements differ, first at %d: %r vs %r" % (
            what, int(bad.sum()), g.numel(), i, float(g[i]), float(w[i])))


@pytest.mark.parametrize("c", ws.CASES, ids=_id)
def test_exact(c):
    x, dy, xm, ym, G = operands(c, True)
    S, Sb = reference(c, xm, ym, G)
    dw = Guarded(int(np.prod(dw_shape(c))))
    db = Guarded(db_len(c)) if c.get("bias", True) else None
    wsp = Workspace(ws_bytes(c))
    run(c, x, dy, dw, db, wsp)
    torch.cuda.synchronize()
    dw.check("dW"), wsp.check("workspace")
    assert_bits(dw.t, f32_scaled(S, c.get("scale", 1.0)), "dW")
    if db is not None:
        db.check("db")
        assert_bits(db.t, Sb.float(), "db")


def _rounding_cases():
    seen, out = set(), []
    for c in ws.CASES:
        p = ws.case_plan(c)
        key = (c["fam"], p["ks"], p["ni"], p["no"], p["kind"])
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


@pytest.mark.parametrize("c", _rounding_cases(), ids=_id)
def test_rounding_and_run_to_run(c):
    x, dy, xm, ym, G = operands(c, False)
    S, Sb = reference(c, xm, ym, G)
    A, Ab = reference(c, xm, ym, G, absolute=True)
    scale = float(c.get("scale", 1.0))
    got = []
    for _ in range(2):
        dw = Guarded(int(np.prod(dw_shape(c))))
        db = Guarded(db_len(c)) if c.get("bias", True) else None
        run(c, x, dy, dw, db, Workspace(ws_bytes(c)))
        torch.cuda.synchronize()
        got.append((dw.t.clone(), db.t.clone() if db is not None else None))
    dw, db = got[0]
    err = (dw.double().reshape(S.shape) - S * scale).abs()
    tol = 2.0 ** -20 * A * abs(scale)
    assert bool((err <= tol).all()), "dW: %d elements off, worst %g of the bound" % (int((err > tol).sum()), float((err / tol.clamp(min=1e-300)).max()))
    if db is not None:
        errb = (db.double() - Sb).abs()
        assert bool((errb <= 2.0 ** -20 * Ab).all()), "db off by %g" % float(errb.max())
        assert_bits(got[1][1], db, "db run to run")
    assert_bits(got[1][0], dw, "dW run to run")


# ---- the grouped launch --------------------------------------------------------------------------------------------------
def _run_group(items, exact, seed=0):
    lib = _lib.load()
    rng = _rng("group", len(items), exact, seed)
    xs, dys, defs, ptrs = [], [], {}, {}
    for i, it in enumerate(items):
        x = _operand(rng, (it["N"], it["H"], it["W"], it["Cin"]), exact).to(BF)
        if it.get("convT"):
            G = _operand(rng, (it["N"], 2 * it["H"], 2 * it["W"], it["convT"]), exact).to(BF)
            dy = space_to_depth(G)
            S, Sb = convT_wgrad64(x, G)
            A, Ab = convT_wgrad64(x.double().abs(), G.double().abs())
        else:
            dy = _operand(rng, (it["N"], it["H"], it["W"], it["Cout"]), exact).to(BF)
            S, Sb = wgrad64(x, dy, it["K"])
            A, Ab = wgrad64(x.double().abs(), dy.double().abs(), it["K"])
        xs.append(x), dys.append(dy)
        ptrs[("x", i)], ptrs[("dy", i)] = _ptr(x), _ptr(dy)
        defs[i] = (S, Sb, A, Ab)
    dests = {}                                                  # every destination starts as NaN: its first item writes it
    for it in items:
        for name, shape in ((it["dw"], (2, 2, it["convT"], it["Cin"]) if it.get("convT") else (it["K"], it["K"], it["Cin"], it["Cout"])),
                            (it.get("db"), (it["convT"] if it.get("convT") else it["Cout"],))):
            if name and name not in dests:
                dests[name] = Guarded(int(np.prod(shape)))
                ptrs[name] = dests[name].ptr()
    arr = ws.items_array(items, ptrs)
    nbytes = lib.sq_conv2d_nhwc_wgrad_group_workspace_bf16(arr, len(items))
    wsp = Workspace(nbytes)
    _lib.check(lib.sq_conv2d_nhwc_wgrad_group_bf16(arr, len(items), wsp.ptr(), _stream()), "sq_conv2d_nhwc_wgrad_group_bf16")
    torch.cuda.synchronize()
    wsp.check("group workspace")
    for d in dests.values():
        d.check("group destination")
    return dests, defs


@pytest.mark.parametrize("name", sorted(ws.GROUPS))
def test_group_exact(name):
    items = ws.GROUPS[name]
    dests, defs = _run_group(items, True)
    # expected contents, item by item in order: write, or add to what the destination holds
    want = {}
    for i, it in enumerate(items):
        S, Sb, _, _ = defs[i]
        v = f32_scaled(S, it.get("scale", 1.0))
        want[it["dw"]] = (want[it["dw"]] + v) if (it.get("acc", 0) & 1) else v
        if it.get("db"):
            vb = Sb.float()
            want[it["db"]] = (want[it["db"]] + vb) if (it.get("acc", 0) & 2) else vb
    for k, d in dests.items():
        assert_bits(d.t, want[k], "%s: %s" % (name, k))


@pytest.mark.parametrize("name", sorted(ws.GROUPS))
def test_group_rounding_and_run_to_run(name):
    items = [dict(it, acc=0) for it in ws.GROUPS[name]]
    seen, uniq = set(), []                                      # one item per destination: no accumulation chains here
    for it in items:
        if it["dw"] not in seen and (not it.get("db") or it["db"] not in seen):
            seen |= {it["dw"], it.get("db")}
            uniq.append(it)
    runs = [_run_group(uniq, False, seed=1) for _ in range(2)]
    dests, defs = runs[0]
    for i, it in enumerate(uniq):
        S, Sb, A, Ab = defs[i]
        s = float(it.get("scale", 1.0))
        err = (dests[it["dw"]].t.double().reshape(S.shape) - S * s).abs()
        assert bool((err <= 2.0 ** -20 * A * abs(s)).all()), (name, i, float(err.max()))
        if it.get("db"):
            assert bool(((dests[it["db"]].t.double() - Sb).abs() <= 2.0 ** -20 * Ab).all()), (name, i)
    for k in dests:
        assert_bits(runs[1][0][k].t, dests[k].t, "%s run to run: %s" % (name, k))


# ---- the Python entries, once through each branch ---------------------------------------------------------------------------
def _ints(shape, dtype=torch.float32, seed=0):
    return _operand(_rng("route", shape, seed), shape, True).to(dtype)


def _check(dw, db, x, dy, K, scale=1.0):
    S, Sb = wgrad64(x, dy, K)
    assert_bits(dw, f32_scaled(S, scale), "dW")
    if db is not None:
        assert_bits(db, Sb.float(), "db")


def test_routing_f32_entries(monkeypatch):
    # dense (K = 1, <= 128 pixels, Cin * Cout >= 2^16), the 1x1 reshape of narrow images, small Cin
    for shape, cin, cout, K in [((2, 4, 8), 256, 256, 1), ((4, 4, 4), 32, 48, 1), ((2, 20, 20), 3, 16, 3)]:
        x, dy = _ints(shape + (cin,)), _ints(shape + (cout,), seed=1)
        dw, db = ops.conv2d_wgrad(x, dy, K)
        _check(dw.reshape(K, K, cin, cout), db, x, dy, K)
    # small images: the mixed kernel addressing the mosaic in-kernel, and the mosaic_pack path of the f32 kernel
    x, dy = _ints((6, 4, 4, 32)), _ints((6, 4, 4, 48), seed=1)
    for mixed in (True, False):
        monkeypatch.setattr(ops, "MIXED", mixed)
        dw, db = ops.conv2d_wgrad(x, dy, 3, dw_scale=0.5)
        _check(dw, db, x, dy, 3, 0.5)
    monkeypatch.setattr(ops, "MIXED", False)
    # image-side 1x1 convs: wgrad1x1_small with the image as the input, and as the output
    for cin, cout in ((3, 16), (32, 2)):
        x, dy = _ints((2, 8, 8, cin)), _ints((2, 8, 8, cout), seed=1)
        dw, db = ops.conv_wgrad_raw(x, dy, 1, want_bias=True)
        _check(dw, db, x, dy, 1)


def test_routing_bf16_entries():
    x, dy = _ints((2, 21, 19, 48), BF), _ints((2, 21, 19, 80), BF, seed=1)
    dw, db = ob.conv2d_wgrad(x, dy, 3)
    _check(dw, db, x, dy, 3)
    xt, G = _ints((2, 7, 9, 64), BF), _ints((2, 14, 18, 24), BF, seed=1)
    dw, db = ob.convT_wgrad(xt, space_to_depth(G), 24)
    S, Sb = convT_wgrad64(xt, G)
    assert_bits(dw, S.float(), "convT dW"), assert_bits(db, Sb.float(), "convT db")
    # the queue takes a layer with gradient sinks and 16-channel multiples, defers it, and the flush writes it
    dws = torch.full((3, 3, 48, 80), float("nan"), device=DEV)
    dbs = torch.full((80,), float("nan"), device=DEV)
    with ob.deferred_wgrads() as q:
        assert q.takes(x, 48, 80, dws) and not q.takes(x, 48, 80, None) and not q.takes(x, 40, 80, dws)
        ob.conv2d_wgrad(x, dy, 3, dw_out=dws, db_out=dbs)
        assert len(q.items) == 1
    _check(dws, dbs, x, dy, 3)
    # bf16 storage (GAN): small-image mosaic, and the image-side 1x1 forms on wgrad1x1_small_bf16 (a == NULL: the column sums)
    xm, dym = _ints((6, 4, 4, 32), BF), _ints((6, 4, 4, 48), BF, seed=1)
    dw, db = og.conv_wgrad(xm, dym, 3, want_bias=True, dw_scale=0.25)
    _check(dw, db, xm, dym, 3, 0.25)
    for cin, cout, xd, yd in ((3, 32, torch.float32, BF), (32, 3, BF, torch.float32)):
        x1, y1 = _ints((2, 8, 8, cin), xd), _ints((2, 8, 8, cout), yd, seed=1)
        dw, db = og.conv_wgrad(x1, y1, 1, want_bias=True, dw_scale=0.5)
        _check(dw, db, x1, y1, 1, 0.5)


def test_other_parameter_gradient_kernels():
    # sq_dense_wgrad_f32: accumulate bits 0..3 and the scale
    x, dy = _ints((96, 64)), _ints((96, 40), seed=1)
    S, Sb = x.double().t() @ dy.double(), dy.double().sum(0)
    for acc in range(4):
        dw0, db0 = _ints((64, 40), seed=2), _ints((40,), seed=3)
        dw, db = dw0.clone(), db0.clone()
        ops.dense_wgrad(x, dy, True, 0.5, dw_out=dw, db_out=db, accumulate=acc)
        v = f32_scaled(S, 0.5)
        assert_bits(dw, dw0 + v if acc & 1 else v, "dense dW acc %d" % acc)
        assert_bits(db, db0 + Sb.float() if acc & 2 else Sb.float(), "dense db acc %d" % acc)
    # sq_wgrad1x1_small_f32 / _bf16 (a == NULL: sums of b)
    a, b = _ints((300, 4)), _ints((300, 16), seed=1)
    assert_bits(ops.wgrad1x1_small(a, b), (a.double().t() @ b.double()).float(), "wgrad1x1_small_f32")
    m = og.wgrad1x1_small(None, b.to(BF))
    assert_bits(m.reshape(-1), b.double().sum(0).float(), "wgrad1x1_small_bf16(NULL)")
    m = og.wgrad1x1_small(a, b.to(BF), 0.5)
    assert_bits(m, f32_scaled(a.double().t() @ b.double(), 0.5), "wgrad1x1_small_bf16")
    # dw / db of the to_image head backward, plain and gated
    lib = _lib.load()
    for cin, cout in ((16, 2), (32, 1)):
        xh, dz, w = _ints((700, cin), BF), _ints((700, cout), seed=1), _ints((cin, cout), seed=2)
        wsb = torch.empty(max(4, lib.sq_conv1x1_head_bwd_workspace_bf16(700, cin, cout)) // 4 + 4, device=DEV)
        for gate in (0.0, 1.25):
            dw, db = Guarded(cin * cout), Guarded(cout)
            if gate:
                rc = lib.sq_conv1x1_head_bwd_gate_bf16(_ptr(xh), _ptr(w), _ptr(dz), None, dw.ptr(), db.ptr(), _ptr(wsb), 700,
                                                       cin, cout, gate, _stream())
            else:
                rc = lib.sq_conv1x1_head_bwd_bf16(_ptr(xh), _ptr(w), _ptr(dz), None, dw.ptr(), db.ptr(), _ptr(wsb), 700, cin,
                                                  cout, _stream())
            _lib.check(rc, "head bwd")
            torch.cuda.synchronize()
            dw.check("head dW"), db.check("head db")
            assert_bits(dw.t, (xh.double().t() @ dz.double()).float(), "head dW gate %g" % gate)
            assert_bits(db.t, dz.double().sum(0).float(), "head db gate %g" % gate)
