"""CPU: the numpy restatement of "Brick views and probability scatter" (tests/volume_tta_cases.py) against the volume
sampler's numpy text, the header's inverse table, the group the 16 ops form, the exact merge of identical logits and the
partition the owner boxes make of a volume."""
import itertools
import os
import re

import numpy as np
import pytest

from sequitr_amd import frontend
from tests import volume_tta_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def asym(shape, seed=0):
    """bricks whose every element is different: no symmetry survives"""
    return (np.arange(int(np.prod(shape)), dtype=np.float32).reshape(shape) * 1.5 + seed).astype(np.float32)


def test_unview_inverts_view():
    x = asym((2, 3, 5, 5, 3))
    for op in vc.OPS:
        assert np.array_equal(vc.unview(vc.view(x, op), op), x), op
        assert np.array_equal(vc.view(vc.unview(x, op), op), x), op
    r = asym((2, 3, 4, 7, 2))                                   # rectangular slices: the mirrors only
    for op in range(8):
        assert vc.view(r, op).shape == r.shape
        assert np.array_equal(vc.unview(vc.view(r, op), op), r), op
    with pytest.raises(AssertionError):
        vc.view(r, 8)


def test_inverse_table_is_the_headers():
    text = open(os.path.join(ROOT, "include", "sequitr_hip.h")).read()
    at = text.index("Brick views and probability scatter")
    section = text[at:at + 8000]
    m = re.search(r"\*\s+op\s+((?:\d+\s+){16})\*\s+op'\s+((?:\d+\s*){16})", section)
    assert m, "the header must state the inverse table"
    ops, inv = [int(v) for v in m.group(1).split()], [int(v) for v in m.group(2).split()]
    assert ops == list(vc.OPS) and dict(zip(ops, inv)) == vc.INVERSE
    assert {op for op in vc.OPS if vc.INVERSE[op] == op} == set(range(10)) | {14, 15}
    assert (vc.INVERSE[10], vc.INVERSE[12], vc.INVERSE[11], vc.INVERSE[13]) == (12, 10, 13, 11)
    src = open(os.path.join(ROOT, "sequitr_amd", "csrc", "sq_tta.hip")).read()
    in_lib = re.search(r"inverse_op\[16\] = \{([0-9, ]+)\}", src)
    assert [int(v) for v in in_lib.group(1).split(",")] == [vc.INVERSE[op] for op in vc.OPS]
    x = asym((2, 3, 5, 5, 3))
    for op in vc.OPS:                                           # the proof: unview_op == view_op'
        assert np.array_equal(vc.unview(x, op), vc.view(x, vc.INVERSE[op])), op
        assert np.array_equal(vc.view(vc.view(x, op), vc.INVERSE[op]), x), op


def test_view_is_the_volume_samplers_text():
    x = asym((2, 3, 5, 5, 3))
    for op in vc.OPS:
        assert np.array_equal(vc.view(x, op), vc.view_sampler_text(x, op)), op
    r = asym((2, 3, 4, 7, 2))
    for op in range(8):
        assert np.array_equal(vc.view(r, op), vc.view_sampler_text(r, op)), op
    assert (frontend.OP_FLIP_Z, frontend.OP_FLIP_X, frontend.OP_FLIP_Y, frontend.OP_TRANSPOSE) == (1, 2, 4, 8)
    assert np.array_equal(vc.view(x, 1), np.flip(x, 1)) and np.array_equal(vc.view(x, 2), np.flip(x, 2))
    assert np.array_equal(vc.view(x, 4), np.flip(x, 3)) and np.array_equal(vc.view(x, 8), x.transpose(0, 1, 3, 2, 4))


def test_the_sixteen_ops_are_a_group():
    x = asym((1, 2, 4, 4, 2))
    views = [vc.view(x, op) for op in vc.OPS]
    for a, b in itertools.combinations(vc.OPS, 2):
        assert not np.array_equal(views[a], views[b]), (a, b)
    for a, b in itertools.product(vc.OPS, vc.OPS):              # closed under composition
        both = vc.view(views[a], b)
        assert sum(np.array_equal(both, v) for v in views) == 1, (a, b)


def test_sets_are_ascending_prefixes():
    assert vc.SETS[None] == (0,) and vc.SETS["flips"] == tuple(range(8)) and vc.SETS["dihedral"] == tuple(range(16))
    assert {k: tuple(v) for k, v in frontend.VOLUME_TTA_OPS.items()} == vc.SETS
    for name in (None, "flips", "dihedral"):
        assert tuple(frontend.check_volume_tta(name)) == vc.SETS[name]
    assert tuple(frontend.check_volume_tta("dihedral", (4, 8, 8))) == vc.OPS
    assert tuple(frontend.check_volume_tta("flips", (4, 8, 16))) == vc.SETS["flips"]
    for bad in (("dihedral", (4, 8, 16)), ("rot90", None), (8, None), (True, None), (("flips",), None)):
        with pytest.raises(ValueError):
            frontend.check_volume_tta(*bad)


@pytest.mark.parametrize("name", ["flips", "dihedral"])
def test_merging_identical_logits_returns_them(name):
    ops = vc.SETS[name]
    rng = np.random.default_rng(3)
    L = (rng.standard_normal((2, 3, 5, 5, 3)) * 7).astype(np.float32)
    # 21 significant bits (the planar test's narrowing) carry the 8 mirrors: every partial sum k * x, k <= 8, needs at most
    # 21 + 3 = 24 bits.  The 16-fold sum passes k = 9 .. 15, four bits wide, so there x keeps 20: 20 + 4 = 24.
    L = (L.view(np.uint32) & np.uint32(0xfffffff8 if len(ops) == 8 else 0xfffffff0)).view(np.float32)
    acc = vc.merge({op: vc.view(L, op) for op in ops}, ops)     # a perfectly equivariant network
    assert np.array_equal(acc, L * np.float32(len(ops)))        # n copies sum exactly
    assert np.array_equal(acc * np.float32(1.0 / len(ops)), L)
    assert np.array_equal(vc.argmax_rows(acc), vc.argmax_rows(L))


def test_merge_adds_in_op_order():
    ops = vc.SETS["dihedral"]
    rng = np.random.default_rng(4)
    by_op = {op: (rng.standard_normal((1, 2, 3, 3, 2)) * 10.0 ** rng.integers(-3, 4)).astype(np.float32) for op in ops}
    acc = vc.merge(by_op, ops)
    want = None
    for op in ops:
        back = vc.view_sampler_text(by_op[op], vc.INVERSE[op])
        want = back if want is None else (want + back).astype(np.float32)
    assert np.array_equal(acc, want)


@pytest.mark.parametrize("shape,brick,margin", [((9, 21, 37), (4, 8, 16), (1, 2, 3)), ((3, 5, 40), (4, 8, 16), (1, 2, 3))])
def test_owner_boxes_partition_the_volume(shape, brick, margin):
    boxes = vc.owner_boxes(shape, brick, margin)
    assert len(boxes) == frontend.volume_bricks(shape, brick, margin).per_volume
    count = np.zeros(shape, np.int32)
    for o, lo, hi in boxes:
        assert all(o[d] <= lo[d] < hi[d] <= min(o[d] + brick[d], shape[d]) for d in range(3)), (o, lo, hi)
        count[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] += 1
    assert (count == 1).all()
    ids = np.full((1,) + shape, -1, np.int64)                   # scatter writes exactly the owned boxes
    vals = np.stack([np.full(brick, k, np.int64) for k in range(len(boxes))])
    vc.scatter(vals, ids, shape, brick, margin)
    assert (ids >= 0).all() and len(np.unique(ids)) == len(boxes)


def test_scatter_probs_restated():
    shape, brick, margin, K = (9, 21, 37), (4, 8, 16), (1, 2, 3), 3
    nb = len(vc.owner_boxes(shape, brick, margin))
    rng = np.random.default_rng(2)
    acc = (rng.standard_normal((2 * nb,) + brick + (K,)) * 4).astype(np.float32)
    mask = np.full((2,) + shape, 99, np.uint8)
    prob = np.full((2, K) + shape, -1.0)
    vc.scatter_probs(acc, 0.125, shape, brick, margin, mask, prob)
    assert mask.max() < K and np.allclose(prob.sum(1), 1.0) and prob.min() >= 0
    logits = vc.scatter(acc, np.zeros((2,) + shape + (K,), np.float32), shape, brick, margin)
    assert np.array_equal(mask, vc.argmax_rows(logits))
    assert np.array_equal(prob, np.moveaxis(vc.softmax64(logits, 0.125), -1, 1))


@pytest.mark.parametrize("K", vc.SCATTER_K)
def test_uint8_boundary_share_of_the_gpu_cases(K):
    """check_probs_u8's cap (fewer than 1 % of the values at a rounding boundary) is a condition on the inputs: the float64
    restatement of every case the GPU test scatters stays far under it with the seeds the GPU test uses"""
    for which, (shape, brick, margin) in enumerate(vc.SCATTER_VOLUMES):
        for n in vc.SCATTER_N:
            acc = vc.scatter_case(shape, brick, margin, 2, K, 1.0 / n, vc.scatter_seed(K, n, which), specials=which == 0)
            prob = np.full((2, K) + shape, np.nan)
            vc.scatter_probs(acc, 1.0 / n, shape, brick, margin, None, prob)
            assert not np.isnan(prob).all() and vc.boundary_share(prob, K) < 0.01, (K, n, which)
