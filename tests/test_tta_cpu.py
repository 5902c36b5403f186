"""CPU: the numpy restatement of "Tile views and probability stitch" (tests/tta_cases.py) against pure-Python loops, numpy's
own flips and turns, the header's inverse table, and the float32 softmax against the float64 one inside the bound the GPU
tests hold the kernel to."""
import itertools
import os
import re

import numpy as np
import pytest

from tests import tta_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def asym(N, T, E, seed=0):
    """tiles whose every element is different: no symmetry survives"""
    return (np.arange(N * T * T * E, dtype=np.float32).reshape(N, T, T, E) * 1.5 + seed).astype(np.float32)


def view_loops(x, op):
    N, T, _, E = x.shape
    out = np.empty_like(x)
    for n, i, j, e in itertools.product(range(N), range(T), range(T), range(E)):
        p, q = (j, i) if op & 4 else (i, j)
        a = T - 1 - p if op & 1 else p
        b = T - 1 - q if op & 2 else q
        out[n, i, j, e] = x[n, a, b, e]
    return out


@pytest.mark.parametrize("T,E", [(1, 1), (2, 3), (3, 2), (4, 1), (5, 3)])
def test_restated_views_equal_the_loops(T, E):
    x = asym(2, T, E)
    for op in tc.OPS:
        v = tc.view(x, op)
        assert np.array_equal(v, view_loops(x, op)), op
        assert np.array_equal(tc.unview(v, op), x), op
        assert np.array_equal(tc.unview(x, op), view_loops(x, tc.INVERSE[op])), op


def test_views_are_numpy_flips_and_turns():
    x = asym(2, 5, 3)
    per_tile = lambda f: np.stack([f(t) for t in x])
    assert np.array_equal(tc.view(x, 0), x)
    assert np.array_equal(tc.view(x, 1), np.flip(x, 1))
    assert np.array_equal(tc.view(x, 2), np.flip(x, 2))
    assert np.array_equal(tc.view(x, 3), per_tile(lambda t: np.rot90(t, 2)))          # the half turn
    assert np.array_equal(tc.view(x, 4), np.transpose(x, (0, 2, 1, 3)))
    assert np.array_equal(tc.view(x, 5), per_tile(lambda t: np.rot90(t, -1)))         # the clockwise quarter turn
    assert np.array_equal(tc.view(x, 6), per_tile(lambda t: np.rot90(t, 1)))          # the counter-clockwise one
    assert np.array_equal(tc.view(x, 7), np.flip(np.flip(np.transpose(x, (0, 2, 1, 3)), 1), 2))   # the other diagonal
    assert tc.SETS["flips"] == (0, 1, 2, 3) and tc.SETS["dihedral"] == tuple(range(8)) and tc.SETS[None] == (0,)


def test_the_eight_views_differ_and_invert():
    x = asym(1, 4, 2)
    views = [tc.view(x, op) for op in tc.OPS]
    for a, b in itertools.combinations(tc.OPS, 2):
        assert not np.array_equal(views[a], views[b]), (a, b)
    for op in tc.OPS:
        assert np.array_equal(tc.unview(views[op], op), x)
        assert np.array_equal(tc.view(views[op], tc.INVERSE[op]), x)          # unview_op == view_op'
        assert np.array_equal(tc.unview(x, op), tc.view(x, tc.INVERSE[op]))


def test_inverse_table_is_the_headers():
    text = open(os.path.join(ROOT, "include", "sequitr_hip.h")).read()
    at = text.index("Tile views and probability stitch")
    section = text[at:at + 6000]
    m = re.search(r"op' = op\s+for op in \{([0-9, ]+)\}", section)
    assert m, "the header must state which ops are their own inverse"
    own = {int(v) for v in m.group(1).split(",")}
    assert re.search(r"5' = 6\s+and\s+6' = 5", section)
    table = {op: op for op in own}
    table.update({5: 6, 6: 5})
    assert table == tc.INVERSE
    in_lib = re.search(r"inverse_op\[8\] = \{([0-9, ]+)\}", open(os.path.join(ROOT, "sequitr_amd", "csrc", "sq_tta.hip")).read())
    assert [int(v) for v in in_lib.group(1).split(",")] == [tc.INVERSE[op] for op in tc.OPS]


@pytest.mark.parametrize("name", ["flips", "dihedral"])
def test_merging_identical_logits_returns_them(name):
    ops = tc.SETS[name]
    rng = np.random.default_rng(3)
    L = (rng.standard_normal((2, 5, 5, 3)) * 7).astype(np.float32)
    # 21 significant bits: then 3x, 5x, 6x and 7x fit float32's 24 and every partial sum of the sequential merge is exact
    # (with all 24 bits x + x + x already rounds, so "n copies return x" holds for such logits only)
    L = (L.view(np.uint32) & np.uint32(0xfffffff8)).view(np.float32)
    acc = tc.merge({op: tc.view(L, op) for op in ops}, ops)                   # a perfectly equivariant network
    mean = acc * np.float32(1.0 / len(ops))
    assert np.array_equal(mean, L)                                            # n copies sum and scale back exactly
    assert np.array_equal(tc.argmax_rows(acc), tc.argmax_rows(L))


def test_merge_adds_in_op_order():
    ops = tc.SETS["dihedral"]
    rng = np.random.default_rng(4)
    by_op = {op: (rng.standard_normal((1, 3, 3, 2)) * 10.0 ** rng.integers(-3, 4)).astype(np.float32) for op in ops}
    acc = tc.merge(by_op, ops)
    want = np.zeros((1, 3, 3, 2), np.float32)
    for n, a, b, e in itertools.product(range(1), range(3), range(3), range(2)):
        s = None
        for op in ops:
            v = view_loops(by_op[op], tc.INVERSE[op])[n, a, b, e]
            s = v if s is None else np.float32(s + v)
        want[n, a, b, e] = s
    assert np.array_equal(acc, want)


def test_argmax_rule():
    nan, inf = np.nan, np.inf
    rows = np.array([[1, 1, 0], [0, 2, 2], [nan, 5, 6], [1, nan, 0], [0, nan, 3], [-0.0, 0.0, 0.0], [0.0, -0.0, 1e-45],
                     [-inf, -inf, -inf], [inf, inf, 1], [nan, nan, nan]], np.float32)
    assert tc.argmax_rows(rows).tolist() == [0, 1, 0, 0, 2, 0, 2, 0, 0, 0]


def test_softmax_rules():
    nan, inf = np.nan, np.inf
    p = tc.softmax64(np.array([[0, 0], [nan, 1], [1, nan], [inf, 0], [-inf, -inf], [-inf, 0], [0, 800]], np.float32))
    assert np.array_equal(p[0], [0.5, 0.5])
    assert np.isnan(p[1:5]).all()
    assert np.array_equal(p[5], [0.0, 1.0]) and np.array_equal(p[6], [0.0, 1.0])
    one = tc.softmax64(np.array([[3.0], [nan], [inf], [-inf], [-0.0]], np.float32))       # K == 1
    assert np.array_equal(np.isnan(one[:, 0]), [False, True, True, True, False]) and one[0, 0] == 1.0 and one[4, 0] == 1.0
    assert tc.to_u8(np.array([0.0, 0.5, 1.0, nan, 0.00196, 0.00197])).tolist() == [0, 128, 255, 0, 0, 1]


@pytest.mark.parametrize("K", range(1, 17))
def test_float32_softmax_stays_inside_the_bound(K):
    rng = np.random.default_rng(K)
    worst = 0.0
    for inv_n in (1.0, 0.25, 0.125):
        rows = [tc.special_rows(K, rng)]
        for spread in (0.0, 1e-3, 20.0, 88.0, 104.0):
            rows.append((rng.random((4000, K)) * spread).astype(np.float32) / np.float32(inv_n))
        rows.append((rng.standard_normal((4000, K)) * 6).astype(np.float32))
        acc = np.concatenate(rows)
        p64, p32 = tc.softmax64(acc, inv_n), tc.softmax32(acc, inv_n)
        nan = np.isnan(p64)
        assert np.array_equal(np.isnan(p32), nan)
        worst = max(worst, float(np.abs(p32.astype(np.float64) - p64)[~nan].max()))
        s = p64.sum(-1)
        assert np.allclose(s[~np.isnan(s)], 1.0, atol=1e-12)
    assert worst <= tc.prob_bound(K), (K, worst, tc.prob_bound(K))


def test_uint8_boundary_share_of_the_gpu_case():
    """the GPU test asserts that fewer than 1 % of its uint8 values lie within 255 * bound of a rounding boundary: with
    logits of spread 20 the restatement leaves out far fewer"""
    rng = np.random.default_rng(0)
    for K in (1, 2, 3, 4, 7, 8, 16):
        p = tc.softmax64((rng.random((20000, K)) * 20).astype(np.float32))
        v = 255.0 * p
        share = float((np.abs(v - np.floor(v) - 0.5) <= 255.0 * tc.prob_bound(K)).mean())
        assert share < 0.001, (K, share)


def test_stitch_takes_every_pixel_from_its_owner():
    H, W, T, m = 37, 53, 16, 2
    ymap, xmap, TR, TC = tc.owner_maps(H, W, T, m)
    tiles = np.arange(2 * TR * TC * T * T, dtype=np.int64).reshape(2 * TR * TC, T, T)
    got = tc.stitch(tiles, H, W, T, m)
    assert got.shape == (2, H, W)
    for f, y, x in [(0, 0, 0), (1, 36, 52), (0, 15, 13), (1, 14, 14), (0, 20, 40)]:
        t = (f * TR + (ymap[y] >> 16)) * TC + (xmap[x] >> 16)
        assert got[f, y, x] == tiles[t, ymap[y] & 0xffff, xmap[x] & 0xffff]
