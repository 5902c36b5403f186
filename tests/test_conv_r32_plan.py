"""CPU: which calls the 32 -> 32 filter-in-registers conv takes (sq_conv_r32_takes_f32, the rule the dispatch itself applies),
and that the launch plans the other tests pin are untouched by it: the kernel walks the generic kernel's grid."""
import pytest

from tests import conv_r32_cases as rc
from tests import f32_walk_cases as wc


@pytest.fixture(autouse=True)
def _switch_unset(monkeypatch):
    monkeypatch.delenv("SQ_CONV_R32", raising=False)
    monkeypatch.delenv("SQ_CONV_STAGE32", raising=False)


@pytest.mark.parametrize("pooled", [False, True])
def test_takes_the_benchmark_layers(pooled):
    assert rc.takes(2, 256, 256, pooled=pooled) == 1              # 512 tiles: the smallest call on the plan
    assert rc.takes(32, 256, 256, pooled=pooled) == 1             # level 1 of 32 tiles of 512 x 512


@pytest.mark.parametrize("pooled", [False, True])
@pytest.mark.parametrize("departure", [dict(N=1), dict(H=250), dict(W=250), dict(Cin=16), dict(Cout=48), dict(Cin=64), dict(K=1),
                                       dict(act=None), dict(act="leaky")],
                         ids=lambda d: "-".join("%s_%s" % kv for kv in d.items()))
def test_declines_every_single_departure(departure, pooled):
    shape = dict(N=2, H=256, W=256, Cin=32, Cout=32, K=3, act="relu")
    assert rc.takes(pooled=pooled, **shape) == 1
    shape.update(departure)
    assert rc.takes(pooled=pooled, **shape) == 0


def test_declines_a_tensor_of_2gib():
    # 32 channels x 4 bytes: 2^24 pixels are exactly 2 GiB
    assert 64 * 512 * 512 * 32 * 4 == 2 ** 31
    assert rc.takes(64, 512, 512) == 0 and rc.takes(64, 512, 512, pooled=True) == 0
    assert rc.takes(63, 512, 512) == 1 and rc.takes(64, 512, 496) == 1


def test_the_switch_is_read_per_call(monkeypatch):
    assert rc.takes(2, 256, 256) == 1
    monkeypatch.setenv("SQ_CONV_R32", "0")
    assert rc.takes(2, 256, 256) == 0 and rc.takes(2, 256, 256, pooled=True) == 0
    monkeypatch.setenv("SQ_CONV_R32", "1")
    assert rc.takes(2, 256, 256) == 1 and rc.takes(2, 256, 256, pooled=True) == 1


@pytest.mark.parametrize("c", rc.CASES, ids=rc.case_id)
def test_plans_are_the_generic_kernels_with_the_switch_on_and_off(c, monkeypatch):
    assert rc.takes(c.N, c.H, c.W, pooled=c.pooled) == 1
    on = (rc.walk(c.N, c.H, c.W, c.pooled), rc.plan(c.N, c.H, c.W, c.pooled))
    monkeypatch.setenv("SQ_CONV_R32", "0")
    assert rc.takes(c.N, c.H, c.W, pooled=c.pooled) == 0
    off = (rc.walk(c.N, c.H, c.W, c.pooled), rc.plan(c.N, c.H, c.W, c.pooled))
    assert on == off
    w, p = on
    assert w["kernel"] == wc.V2 and w["cblocks"] == 1 and p == dict(bn=32, kc=32, gy=1, s=1, l0=0)
    assert w["items"] == c.N * (c.H // 16) * (c.W // 16) and w["items"] >= 512


@pytest.mark.parametrize("c", rc.R32_WALKS, ids=rc.walk_case_id)
def test_walk_cases_reach_the_regimes_they_declare(c, monkeypatch):
    """every case of the walk sweep (tests/test_gpu_conv_r32.py): the tags it declares are the ones the walk plan and the shape
    give, the kernel takes it, and plan and walk are the generic kernel's with the switch on and off"""
    assert set(c.tags) == rc.r32_tags(c)
    assert rc.takes(c.N, c.H, c.W, pooled=c.pooled) == 1
    assert c.N * c.H * c.W * 32 * 4 <= 140e6                           # no tensor much over 130 MB
    on = (rc.walk(c.N, c.H, c.W, c.pooled), rc.plan(c.N, c.H, c.W, c.pooled))
    monkeypatch.setenv("SQ_CONV_R32", "0")
    assert rc.takes(c.N, c.H, c.W, pooled=c.pooled) == 0
    off = (rc.walk(c.N, c.H, c.W, c.pooled), rc.plan(c.N, c.H, c.W, c.pooled))
    assert on == off
    w, p = on
    assert w["kernel"] == wc.V2 and w["cblocks"] == 1 and p == dict(bn=32, kc=32, gy=1, s=1, l0=0)
    tiles_x, tiles_y = c.W // 16, c.H // 16
    assert w["items"] == c.N * tiles_x * tiles_y and w["items"] >= 512
    counts = [wc.block_count(w, b) for b in range(w["G"])]
    assert (min(counts), max(counts), sum(counts)) == (w["tmin"], w["tmax"], w["items"])
    assert w["G"] == (w["gn"] * tiles_y + w["gy"]) * tiles_x + w["gx"]
    for b in range(w["G"]):
        wc.carries_of_block(w, tiles_x, tiles_y, b)                    # asserts every step lands on tile b + k G
    if "tmin=1<tmax/%s" % ("pooled" if c.pooled else "plain") in c.tags:
        assert sorted(set(counts)) == [1, 2]
    if tiles_x == 2:                                                   # an odd stride: the column carries at every other step
        assert w["gx"] == 1


def test_walk_table_reaches_every_needed_regime():
    """a regime that loses its last case fails here; walks of 1, 2, 3 and 4 or more tiles all occur"""
    carried = {}
    for c in rc.R32_WALKS:
        for t in c.tags:
            carried.setdefault(t, []).append(rc.walk_case_id(c))
    assert set(carried) == rc.R32_NEEDED, (rc.R32_NEEDED - set(carried), set(carried) - rc.R32_NEEDED)
    assert len({rc.walk_case_id(c) for c in rc.R32_WALKS}) == len(rc.R32_WALKS)
    for pooled in (False, True):
        lengths = set()
        for c in rc.R32_WALKS:
            if c.pooled == pooled:
                w = rc.walk(c.N, c.H, c.W, pooled)
                lengths |= {wc.block_count(w, b) for b in range(w["G"])}
        assert {1, 2, 3} <= lengths and max(lengths) >= 4, lengths
    N, H, W = rc.NONFINITE_SHAPE
    assert {c.bias for c in rc.R32_WALKS if (c.N, c.H, c.W) == (N, H, W)} == {"rand"} and rc.walk(N, H, W, False)["tmax"] >= 2


def test_the_tables_reach_their_regimes():
    """(2, 256, 256): one tile per block; (5, 256, 272): 454 blocks of 2 or 3 tiles, a non-square tile grid, and walks with a step
    that carries nothing, one that carries the column into the row and one that carries the row into the image"""
    w = rc.walk(2, 256, 256, False)
    assert (w["G"], w["tmin"], w["tmax"]) == (512, 1, 1)
    w = rc.walk(5, 256, 272, True)
    assert (w["G"], w["items"], w["tmin"], w["tmax"]) == (454, 1360, 2, 3)
    tiles_x, tiles_y = 272 // 16, 256 // 16
    assert tiles_x != tiles_y and w["G"] % (tiles_x * tiles_y) != 0
    steps = [s for b in range(w["G"]) for s in wc.carries_of_block(w, tiles_x, tiles_y, b)]
    assert any(not cx and not cy for cx, cy in steps) and any(cx for cx, _ in steps) and any(cy for _, cy in steps)
    assert rc.walk(32, 256, 256, False)["G"] == 512              # the benchmark's level 1: 16 tiles per block
