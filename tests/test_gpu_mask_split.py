"""GPU: sq_mask_split_u8 (maskops.split) and the ``split`` step of MaskCleanup against the scipy restatement of
include/sequitr_hip.h, "Mask clean-up: splitting" (tests/mask_split_cases.py).  Every case runs with both regrowth forms
(SQ_SPLIT_LDS, read per launch) and through both entry points; every comparison is exact."""
import numpy as np
import pytest
import torch

from sequitr_amd import maskops
from tests import mask_cleanup_cases as mc
from tests import mask_split_cases as sc
from tests import objects_cases as oc

pytestmark = pytest.mark.gpu
TILE = maskops.SPLIT_TILE
K = maskops.SPLIT_STEPS
REACHES = (1, K - 1, K, K + 1, 2 * K + 3, 64)
_REFS = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def both_forms(monkeypatch, fn):
    """fn(what) with the LDS tiles and with SQ_SPLIT_LDS=0, one step per launch; the switch is read per launch"""
    monkeypatch.delenv("SQ_SPLIT_LDS", raising=False)
    fn("LDS form")
    monkeypatch.setenv("SQ_SPLIT_LDS", "1")
    fn("SQ_SPLIT_LDS=1")
    monkeypatch.setenv("SQ_SPLIT_LDS", "0")
    fn("SQ_SPLIT_LDS=0")
    monkeypatch.delenv("SQ_SPLIT_LDS", raising=False)


def check(monkeypatch, mask, C, r, st, reach, key=None):
    """maskops.split and MaskCleanup.apply, both forms, against the restatement (computed once per key)"""
    mask = np.ascontiguousarray(mask, np.uint8)
    if key is None or key not in _REFS:
        want = sc.split_ref(mask, r, st, reach, C)
        if key is not None:
            _REFS[key] = want
    else:
        want = _REFS[key]
    d = dev(mask)
    step = {"op": "split", "erosions": r, "structure": st, "reach": reach}
    mcl = maskops.MaskCleanup([step])

    def run(what):
        for name, got in (("split", maskops.split(d, r, st, reach, classes=C)), ("MaskCleanup", mcl.apply(d, C))):
            got = got.cpu().numpy()
            assert np.array_equal(got, want), "%s, %s r=%d %s reach=%r C=%d %s: %d pixels differ" % (
                what, name, r, st, reach, C, mask.shape, int((got != want).sum()))

    both_forms(monkeypatch, run)
    assert np.array_equal(d.cpu().numpy(), mask)                # the input is not written
    return want


@pytest.mark.parametrize("shape", sc.split_shapes(TILE), ids=lambda s: "%dx%dx%d" % s)
def test_shapes(monkeypatch, shape):
    N, H, W = shape
    C = (2, 3, 5)[(H + W) % 3]
    density = (0.5, 0.8, 0.95)[(H * 7 + W) % 3]
    mask = mc.random_mask(H * 1000 + W, N, H, W, C, density)
    for r, st in ((1, "cross"), (2, "square")):
        check(monkeypatch, mask, C, r, st, None)
    check(monkeypatch, mask, C, 1, "square", K + 1)


@pytest.mark.parametrize("C", [2, 3, 5])
@pytest.mark.parametrize("density", [0.5, 0.8, 0.95])
def test_random_masks_over_several_tiles(monkeypatch, C, density):
    mask = mc.random_mask(C * 10 + int(density * 10), 3, TILE[0] + 9, 2 * TILE[1] + 13, C, density)   # bytes C, C + 3, 255 inside
    changed = 0
    for r, st, reach in ((1, "cross", None), (2, "cross", None), (1, "square", 2 * K + 3), (2, "square", 64)):
        changed += int((check(monkeypatch, mask, C, r, st, reach) != mask).sum())
    assert changed > 0 or density < 0.8
    assert np.array_equal(check(monkeypatch, mask, C, 1, "cross", 3)[mask >= C], mask[mask >= C])


@pytest.mark.parametrize("case", sc.splitting_cases(TILE), ids=lambda c: c[0])
def test_splitting_cases(monkeypatch, case):
    name, mask, C, r, st, reach = case
    want = check(monkeypatch, mask, C, r, st, reach, key=name)
    assert (want != mask).any() and sc.count_objects(want, C) > sc.count_objects(mask, C)


@pytest.mark.parametrize("case", sc.unchanged_cases(TILE), ids=lambda c: c[0])
def test_unchanged_cases(monkeypatch, case):
    name, mask, C, r, st, reach = case
    assert np.array_equal(check(monkeypatch, mask, C, r, st, reach), mask)


@pytest.mark.parametrize("reach", REACHES)
def test_reach(monkeypatch, reach):
    """the corridors of every length across a tile seam, the elbows around the tile corners (two seams each way, cut only
    at reach 64), and touching disks on every seam with fewer steps than they need"""
    check(monkeypatch, sc.gaps(TILE), 2, 1, "cross", reach)
    check(monkeypatch, sc.elbows(TILE), 2, 1, "square", reach)
    check(monkeypatch, sc.seam_pairs(TILE, 8), 2, 8, "cross", reach)
    check(monkeypatch, np.concatenate([sc.chambers("spiral"), sc.chambers("spiral")[:, ::-1].copy()]), 2, 2, "cross", reach)


def test_largest_erosion_over_two_tiles_each_way(monkeypatch):
    H, W = TILE[0] + 36, TILE[1] + 108
    m = np.concatenate([mc.random_mask(1, 1, H, W, 3, 0.97), oc.disks(3, 1, H, W, 14, classes=2, rmax=40)])
    yy, xx = np.mgrid[0:H, 0:W]
    big = np.zeros((1, H, W), np.uint8)
    for cx in (40, 85, 130):                                    # three disks of radius 25 in a row: cores survive r = 16
        big[0][(yy - 50) ** 2 + (xx - cx) ** 2 <= 25 * 25] = 1
    m = np.concatenate([m, big])
    for st in sc.STRUCTURES:
        want = check(monkeypatch, m, 3, maskops.MORPH_MAX_ITER, st, None)
        if st == "cross":
            assert sc.count_objects(want[2:], 2) == 3


def test_guards_views_and_overlap(monkeypatch):
    mask = np.concatenate([sc.seam_pairs(TILE, 4)[:, :70, :150], mc.random_mask(9, 1, 70, 150, 3, 0.9)])
    d = dev(mask)
    want = sc.split_ref(mask, 4, "cross", None, 3)
    assert (want != mask).any()
    lib = maskops._lib.load()
    k, nws = mask.size, int(lib.sq_mask_split_workspace(*mask.shape))
    assert nws == (k * 9 + 15) // 16 * 16

    def run(what):
        for off in (16, 13):                                    # 13: out is not 4-byte aligned
            buf = torch.full((k + 64,), 0xAB, dtype=torch.uint8, device="cuda")
            wsb = torch.full((nws + 64,), 0xCD, dtype=torch.uint8, device="cuda")
            out = buf[off:off + k].view(mask.shape)
            ws = wsb[32:32 + nws]
            assert ws.data_ptr() % 16 == 0
            got = maskops.split(d, 4, classes=3, out=out, workspace=ws)
            assert got is out and np.array_equal(out.cpu().numpy(), want), what
            guard, wguard = buf.cpu().numpy(), wsb.cpu().numpy()
            assert np.all(guard[:off] == 0xAB) and np.all(guard[off + k:] == 0xAB), what
            assert np.all(wguard[:32] == 0xCD) and np.all(wguard[32 + nws:] == 0xCD), what

    both_forms(monkeypatch, run)
    assert np.array_equal(d.cpu().numpy(), mask)
    with pytest.raises(ValueError, match="contiguous"):
        maskops.split(d[:, :, :50], 2, classes=3)
    with pytest.raises(ValueError, match="volumes are out of scope"):
        maskops.split(d[None], 2, classes=3)
    with pytest.raises(ValueError, match="workspace holds"):
        maskops.split(d, 2, classes=3, workspace=torch.empty(16, dtype=torch.int32, device="cuda"))
    buf = torch.zeros(k + 8, dtype=torch.uint8, device="cuda")
    buf[:k] = d.reshape(-1)
    with pytest.raises(maskops._lib.SequitrHipError, match="overlap"):
        maskops.split(buf[:k].view(mask.shape), 2, classes=3, out=buf[8:8 + k].view(mask.shape))
    zero = torch.zeros((1, 5, 6), dtype=torch.uint8, device="cuda")
    assert not maskops.split(zero, 1).any()                     # classes default to 2 on an all-background mask


def test_twice_is_bit_identical_and_a_captured_graph_replays_the_eager_bits(monkeypatch):
    mask = np.concatenate([sc.seam_pairs(TILE, 4), mc.random_mask(77, 2, 190, 172, 2, 0.9, unknown=False)])
    d = dev(mask)
    mcl = maskops.MaskCleanup([{"op": "split", "erosions": 4}])

    def run(what):
        a, b = maskops.split(d, 4, classes=2), maskops.split(d, 4, classes=2)
        assert torch.equal(a, b), what
        assert torch.equal(mcl.apply(d, 2).clone(), mcl.apply(d, 2)) and torch.equal(mcl.apply(d, 2), a), what

    both_forms(monkeypatch, run)
    eager = maskops.split(d, 4, "square", 2 * K + 3, classes=2)
    out = torch.empty_like(d)
    ws = torch.empty(int(maskops._lib.load().sq_mask_split_workspace(*mask.shape)) // 4, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        maskops.split(d, 4, "square", 2 * K + 3, classes=2, out=out, workspace=ws)      # warm up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    out.zero_()
    with torch.cuda.graph(graph):                               # one linear chain of launches on one stream
        maskops.split(d, 4, "square", 2 * K + 3, classes=2, out=out, workspace=ws)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    assert np.array_equal(eager.cpu().numpy(), sc.split_ref(mask, 4, "square", 2 * K + 3, 2))


def test_mask_cleanup_composition(monkeypatch):
    steps = [{"op": "open", "iterations": 1, "structure": "cross"}, {"op": "fill_holes", "max_area": 40},
             {"op": "split", "erosions": 4, "structure": "cross", "reach": None}, {"op": "clear_border"}]
    mask = np.concatenate([sc.seam_pairs(TILE, 4), sc.seam_pairs(TILE, 4, cls=2),
                           oc.disks(11, 1, 190, 172, 60, classes=2, rmax=12)])
    mask[mc.random_mask(13, 3, 190, 172, 2, 0.02, unknown=False) > 0] = 0           # pepper the objects with holes
    d = dev(mask)
    want = sc.steps_ref(mask, steps, 3)
    before = mc.steps_ref(mask, steps[:2] + steps[3:], 3)
    assert sc.count_objects(want, 3) > sc.count_objects(before, 3)                  # the split step matters in the chain
    mcl = maskops.MaskCleanup(steps)

    def run(what):
        got = mcl.apply(d, 3)
        assert np.array_equal(got.cpu().numpy(), want), what
        buffers = {k: tuple(t.data_ptr() for t in v if t is not None) for k, v in mcl._cache.items()}
        again = mcl.apply(d, 3)
        assert again.data_ptr() == got.data_ptr() and np.array_equal(again.cpu().numpy(), want), what
        assert {k: tuple(t.data_ptr() for t in v if t is not None) for k, v in mcl._cache.items()} == buffers   # nothing new

    both_forms(monkeypatch, run)
    assert np.array_equal(d.cpu().numpy(), mask)
