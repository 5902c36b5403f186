"""GPU: the persistent f32 inference kernels where blocks walk tiles -- conv_l0_kernel in every instantiation, the generic
conv_mfma_f32_v2_kernel in its plain / FIRST / UP / head forms and on wide channel blocks, convT2x2_v2_kernel at every row-tile
count -- against the C oracle, bit for bit.  The tables (tests/f32_walk_cases.py) are checked on the CPU to reach their regimes
(tests/test_f32_walk_plan.py): blocks of three or more tiles, uneven walks, every carry of the tile stride, ragged last tiles.
A mismatch is reported with the tile it lies in and that tile's position in its block's walk, from the same walk plan."""
import collections
import zlib

import numpy as np
import pytest
import torch

from oracle import c_oracle as co
from sequitr_amd import ops
from tests import f32_walk_cases as wc
from tests.util import assert_bit_exact

pytestmark = pytest.mark.gpu


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _f32(rng, shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def _bias(rng, kind, n):
    b = _f32(rng, (n,), 0.1)                                # drawn in every case: the other inputs do not depend on `kind`
    return None if kind is None else (np.zeros(n, np.float32) if kind == "zero" else b)


def inputs_of(c):
    """every input of a case, from a generator keyed on the case"""
    rng = _rng(wc.case_id(c))
    N, H, W = c.N, c.H, c.W
    t = {}
    if c.form == wc.CONVT:
        t["x"] = _f32(rng, (N, H, W, c.Cin))
        t["w"] = _f32(rng, (2, 2, c.Cout, c.Cin), 0.2)
        t["b"] = _bias(rng, c.bias, c.Cout)
        t["skip"] = _f32(rng, (N, 2 * H, 2 * W, c.Cout)) if c.opt else None
        return t
    t["w"] = _f32(rng, (3, 3, 16 if c.form == wc.FIRST else c.Cin, c.Cout), 1.0 / np.sqrt(9 * max(c.Cin, 16)))
    t["b"] = _bias(rng, c.bias, c.Cout)
    if c.form == wc.FIRST:
        t["x"] = _f32(rng, (N, H, W, 1))
        t["w1"], t["b1"] = _f32(rng, (3, 3, 1, 16), 0.5), _f32(rng, (16,), 0.1)
    elif c.form == wc.UP:
        t["x"] = _f32(rng, (N, H, W, 16))                   # the skip tensor
        t["xl"] = _f32(rng, (N, H // 2, W // 2, 32))
        t["wt"], t["bt"] = _f32(rng, (2, 2, 16, 32), 0.2), _f32(rng, (16,), 0.1)
    elif c.form == wc.CONCAT:
        t["x"], t["xb"] = _f32(rng, (N, H, W, c.Cin // 2)), _f32(rng, (N, H, W, c.Cin // 2))
    else:
        t["x"] = _f32(rng, (N, H, W, c.Cin))
    if c.form == wc.HEAD:
        t["hw"], t["hb"] = _f32(rng, (1, 1, 16, c.opt), 0.25), _f32(rng, (c.opt,), 0.1)
    return t


def reference(c, t):
    """{output: array} from the C oracle, composed of its plain operators"""
    if c.form == wc.CONVT:
        return {"y": co.convT2x2s2(t["x"], t["w"], t["b"], skip=t["skip"], bridge=c.opt)}
    if c.form == wc.FIRST:
        y = co.conv2d(co.conv2d(t["x"], t["w1"], t["b1"], act="relu"), t["w"], t["b"], act="relu")
        return {"y": y, "pooled": co.maxpool2x2(y)} if c.opt else {"y": y}
    if c.form == wc.UP:
        merged = co.convT2x2s2(t["xl"], t["wt"], t["bt"], skip=t["x"] if c.opt else None, bridge=c.opt)
        return {"y": co.conv2d(merged, t["w"], t["b"], act=c.act)}
    x = np.concatenate([t["x"], t["xb"]], -1) if c.form == wc.CONCAT else t["x"]
    y = co.conv2d(x, t["w"], t["b"], act=c.act)
    if c.form == wc.POOL:
        return {"y": y, "pooled": co.maxpool2x2(y)}
    if c.form == wc.HEAD:
        logits = co.conv2d(y, t["hw"], t["hb"], act=None)
        return {"logits": logits, "mask": co.argmax_u8(logits)}
    return {"y": y}


def run(c, d):
    """{output: device tensor} from the library, `d` the inputs on the device"""
    if c.form == wc.CONVT:
        return {"y": ops.convT2x2s2(d["x"], d["w"], d["b"], skip=d["skip"], bridge=c.opt)}
    if c.form == wc.FIRST:
        y, p = ops.conv3x3_first_block(d["x"], d["w1"], d["b1"], d["w"], d["b"], want_pool=bool(c.opt))
        return {"y": y, "pooled": p} if c.opt else {"y": y}
    if c.form == wc.UP:
        return {"y": ops.convT_conv3x3(d["xl"], d["wt"], d["bt"], d["x"], c.opt, d["w"], d["b"], act=c.act)}
    if c.form == wc.CONCAT:
        return {"y": ops.conv2d_concat(d["x"], d["xb"], d["w"], d["b"], act=c.act)}
    if c.form == wc.POOL:
        y, p = ops.conv3x3_pool(d["x"], d["w"], d["b"], act=c.act)
        return {"y": y, "pooled": p}
    if c.form == wc.HEAD:
        logits, mask = ops.conv3x3_head(d["x"], d["w"], d["b"], d["hw"], d["hb"], act=c.act)
        return {"logits": logits, "mask": mask}
    return {"y": ops.conv2d(d["x"], d["w"], d["b"], act=c.act)}


def where(got, ref, c, p, name):
    """the first differing elements by tile and by the tile's position in its block's walk, and how the differing tiles
    spread over walk positions: a seam bug shows as mismatches at positions >= 1 only (or at the last one only)"""
    bits = lambda a: a.view(np.uint32) if a.dtype == np.float32 else a
    bad = np.argwhere(bits(got) != bits(ref))[:20000]
    sub = 2 if name == "pooled" else 1                      # a pooled pixel lies in the tile of the pixels it pools
    tx, ty = wc.tiles_xy(c)
    lines, spread = [], collections.Counter()
    for k, idx in enumerate(bad):
        n, y, x = (int(v) for v in idx[:3])
        ch = int(idx[3]) if len(idx) > 3 else 0
        if c.form == wc.CONVT:
            rt, pt, b, pos, cnt = wc.convT_position(p, c, n, y, x, ch)
            tile = "row tile %d, pixel tile %d" % (rt, pt)
        else:
            tyi, txi = y * sub // 16, x * sub // 16
            b, pos, cnt = wc.tile_position(p, tx, ty, n, tyi, txi)
            tile = "tile (n %d, ty %d, tx %d)" % (n, tyi, txi)
        spread[(pos, cnt)] += 1
        if k < 5:
            lines.append("  %s %s: %r vs %r -- %s, item %d of %d of block %d (of %d blocks)" % (
                name, tuple(int(v) for v in idx), got[tuple(idx)], ref[tuple(idx)], tile, pos, cnt, b, p["G"]))
    lines.append("  differing elements by (position in the walk, items of the walk): %s" % sorted(spread.items()))
    return "\n".join(lines)


def check(out, ref, c, p, what):
    assert set(out) == set(ref)
    for name in sorted(ref):
        got = out[name].cpu().numpy()
        try:
            assert_bit_exact(got, ref[name], "%s %s [%s]" % (what, name, wc.case_id(c)))
        except AssertionError as e:
            if got.shape != ref[name].shape or got.dtype != ref[name].dtype:
                raise
            raise AssertionError("%s\n%s" % (e, where(got, ref[name], c, p, name))) from None


def sweep(c, kernel):
    p = wc.walk_of(c)
    assert p["kernel"] == kernel and p["tmax"] >= 3 and p["tmin"] < p["tmax"], (c, p)   # tests/test_f32_walk_plan.py has the rest
    t = inputs_of(c)
    out = run(c, {k: _dev(v) for k, v in t.items()})
    check(out, reference(c, t), c, p, {wc.L0: "level-0", wc.V2: "generic", wc.CT: "convT v2"}[kernel])


@pytest.mark.parametrize("c", wc.L0_CASES, ids=wc.case_id)
def test_level0_family_walk_bit_exact(c, monkeypatch):
    """every level-0 instantiation over walks of 3 (G = 1024) or 5 (G = 512) tiles with every carry of advance(), and the generic
    kernel on the same inputs (SQ_CONV_L0=0, read per call): both bit-exact against the oracle, and identical to each other"""
    monkeypatch.delenv("SQ_CONV_L0", raising=False)
    p0 = wc.walk_of(c)
    assert p0["kernel"] == wc.L0 and p0["tmax"] >= 3 and p0["tmin"] < p0["tmax"], (c, p0)
    t = inputs_of(c)
    d = {k: _dev(v) for k, v in t.items()}
    ref = reference(c, t)
    out0 = run(c, d)
    monkeypatch.setenv("SQ_CONV_L0", "0")
    p1 = wc.walk_of(c)
    assert p1["kernel"] == wc.V2 and p1["tmax"] >= 3 and p1["tmin"] < p1["tmax"], (c, p1)
    out1 = run(c, d)
    monkeypatch.delenv("SQ_CONV_L0")
    check(out0, ref, c, p0, "level-0")
    check(out1, ref, c, p1, "generic")
    for name in ref:
        assert torch.equal(out0[name], out1[name]), "level-0 and generic kernels differ in %s [%s]" % (name, wc.case_id(c))


@pytest.mark.parametrize("c", wc.RAGGED_CASES, ids=wc.case_id)
def test_generic_forms_walk_ragged_bit_exact(c, monkeypatch):
    """UP (no other test launches the generic form), FIRST, head and the plain 16-channel-block form over walks of three tiles
    with a partial last row and column of tiles"""
    monkeypatch.delenv("SQ_CONV_L0", raising=False)
    sweep(c, wc.V2)


@pytest.mark.parametrize("c", [w[0] for w in wc.WIDE_CASES], ids=wc.case_id)
def test_generic_wide_blocks_walk_bit_exact(c, monkeypatch):
    """64- and 32-channel blocks, stage-32, concat and pooled forms over uneven walks of three or more tiles"""
    monkeypatch.delenv("SQ_CONV_L0", raising=False)
    sweep(c, wc.V2)


@pytest.mark.parametrize("c", wc.CONVT_CASES, ids=wc.case_id)
def test_convT_walk_bit_exact(c):
    """one to five row tiles per pixel tile at the default 32-pixel tiles, more than two work items per block, a ragged last tile"""
    sweep(c, wc.CT)
