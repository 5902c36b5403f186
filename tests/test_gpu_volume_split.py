"""GPU: sq_volume_split_u8 (volumeops.split3d) and the ``split3d`` step of VolumeCleanup against the scipy restatement of
include/sequitr_hip.h, "Volume clean-up: splitting" (tests/volume_split_cases.py).  Every case runs with both regrowth
forms (SQ_SPLIT3D_LDS, read per call) and through both entry points; every comparison is exact."""
import numpy as np
import pytest
import torch

from sequitr_amd import maskops, volumeops
from tests import mask_cleanup_cases as mc
from tests import mask_split_cases as ms
from tests import volume_cleanup_cases as vc
from tests import volume_split_cases as sc

pytestmark = pytest.mark.gpu
TILE = volumeops.SPLIT3D_TILE
K = volumeops.SPLIT3D_STEPS
REACHES = tuple(sorted({1, K - 1, K, K + 1, 2 * K + 3, 64}))       # K - 1 is 1 when a launch runs two steps
_REFS = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def both_forms(monkeypatch, fn):
    """fn(what) with the form that runs when nothing is set, with the LDS bricks and with one step per launch; the switch
    is read per call"""
    monkeypatch.delenv("SQ_SPLIT3D_LDS", raising=False)
    fn("default form")
    monkeypatch.setenv("SQ_SPLIT3D_LDS", "1")
    fn("SQ_SPLIT3D_LDS=1")
    monkeypatch.setenv("SQ_SPLIT3D_LDS", "0")
    fn("SQ_SPLIT3D_LDS=0")
    monkeypatch.delenv("SQ_SPLIT3D_LDS", raising=False)


def check(monkeypatch, mask, C, r, st, reach, key=None):
    """volumeops.split3d and VolumeCleanup.apply, both forms, against the restatement (computed once per key)"""
    mask = np.ascontiguousarray(mask, np.uint8)
    if key is None or key not in _REFS:
        want = sc.split3d_ref(mask, r, st, reach, C)
        if key is not None:
            _REFS[key] = want
    else:
        want = _REFS[key]
    d = dev(mask)
    vcl = volumeops.VolumeCleanup([{"op": "split3d", "erosions": r, "structure": st, "reach": reach}])

    def run(what):
        for name, got in (("split3d", volumeops.split3d(d, r, st, reach, classes=C)), ("VolumeCleanup", vcl.apply(d, C))):
            got = got.cpu().numpy()
            assert np.array_equal(got, want), "%s, %s r=%d %s reach=%r C=%d %s: %d voxels differ" % (
                what, name, r, st, reach, C, mask.shape, int((got != want).sum()))

    both_forms(monkeypatch, run)
    assert np.array_equal(d.cpu().numpy(), mask)                # the input is not written
    return want


@pytest.mark.parametrize("shape", sc.split_shapes(TILE), ids=lambda s: "%dx%dx%dx%d" % s)
def test_shapes(monkeypatch, shape):
    N, D, H, W = shape
    C = (2, 3, 5)[(D + H + W) % 3]
    density = (0.8, 0.95)[(D + H * 7 + W) % 2]
    mask = vc.random_volume(D * 100000 + H * 1000 + W, N, D, H, W, C, density)      # bytes C, C + 3, 255 inside
    check(monkeypatch, mask, C, 1, "cross", None)
    check(monkeypatch, mask, C, 1, "plane_cross", K + 1)
    check(monkeypatch, mask, C, 2, "plane_square", None)
    check(monkeypatch, mask, C, 1, "cube", 2 * K + 3)


@pytest.mark.parametrize("C", [2, 3, 5])
@pytest.mark.parametrize("density", [0.8, 0.95])
def test_random_volumes_over_several_bricks(monkeypatch, C, density):
    mask = vc.random_volume(C * 10 + int(density * 10), 2, 2 * TILE[0] + 3, TILE[1] + 9, 2 * TILE[2] + 5, C, density)
    changed = 0
    for r, st, reach in ((1, "cross", None), (1, "cube", None), (1, "plane_cross", 2 * K + 3), (2, "plane_square", 64)):
        changed += int((check(monkeypatch, mask, C, r, st, reach) != mask).sum())
    assert changed > 0
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
    """the corridors of every length across a brick seam along each axis, the elbows round the brick edges (cut only at
    reach 64), the junction, and touching balls on every seam with fewer steps than they need: the remainder launch and
    both parities of the ping-pong"""
    for axis in range(3):
        check(monkeypatch, sc.gaps(TILE, axis), 2, 1, "cross", reach)
    check(monkeypatch, sc.elbows(TILE), 2, 1, "cube", reach)
    check(monkeypatch, sc.junction(), 2, 1, "cross", reach)
    check(monkeypatch, sc.seam_pairs(TILE)[3::4], 2, 4, "cross", reach)     # the three corner pairs


@pytest.mark.parametrize("case", sc.erosion_chain_cases(), ids=lambda c: c[0])
def test_erosion_chains(monkeypatch, case):
    """one to four chained 3-D erosion launches, odd and even counts, and the planar launch at r = 1 and 16"""
    name, mask, C, r, st = case
    want = check(monkeypatch, mask, C, r, st, None)
    assert sc.count_objects(want, C) == 2
    # a dense random volume of several bricks through the same chain; where no core survives it comes back unchanged
    check(monkeypatch, vc.random_volume(r, 1, 2 * TILE[0] + 1, TILE[1] + 3, TILE[2] + 2, 3, 0.97), 3, r, st, 5)


@pytest.mark.parametrize("st,plane_st", [("cross", "plane_cross"), ("square", "plane_square")])
def test_a_frame_is_a_volume_of_one_slice(monkeypatch, st, plane_st):
    """sq_mask_split_u8 and sq_volume_split_u8 are one program after the seeds: at D = 1 the plane structures give the
    planar split, under every regrowth form of both switches.  The mask spans 2 x 3 planar tiles and 5 x 5 bricks; the
    reaches are K - 1, K, K + 1 of both geometries and one with a remainder launch.  (The 3-D structures are no part of
    this: at D = 1 their erosion removes everything, by scipy's definition.)"""
    m = np.concatenate([ms.seam_pairs(maskops.SPLIT_TILE, 4)[:, :70, :150], mc.random_mask(9, 1, 70, 150, 3, 0.9)])
    d2, d3 = dev(m), dev(m[:, None])
    for reach in (1, 2, 3, 7, 8, 9, 19):
        want = ms.split_ref(m, 4, st, reach, 3)
        for planar_form in (None, "1", "0"):
            if planar_form is None:
                monkeypatch.delenv("SQ_SPLIT_LDS", raising=False)
            else:
                monkeypatch.setenv("SQ_SPLIT_LDS", planar_form)
            frame = maskops.split(d2, 4, st, reach, classes=3).cpu().numpy()
            assert np.array_equal(frame, want), (st, reach, planar_form)

        def run(what):
            volume = volumeops.split3d(d3, 4, plane_st, reach, classes=3)[:, 0].cpu().numpy()
            assert np.array_equal(volume, want), (plane_st, reach, what)

        both_forms(monkeypatch, run)
    monkeypatch.delenv("SQ_SPLIT_LDS", raising=False)
    assert (want != m).any()


def test_guards_views_and_overlap(monkeypatch):
    mask = np.concatenate([sc.seam_pairs(TILE)[3:4, :, :, :50], vc.random_volume(9, 1, 36, 40, 50, 3, 0.9)])
    d = dev(mask)
    want = {r: sc.split3d_ref(mask, r, "cross", None, 3) for r in (4, 5)}
    assert (want[4] != mask).any() and (want[5] != mask).any()
    lib = volumeops._lib.load()
    k, nws = mask.size, int(lib.sq_volume_split_workspace(*mask.shape))
    assert nws == (k * 9 + 15) // 16 * 16

    def run(what):
        for off in (16, 13):                                    # 13: out is not 4-byte aligned
            for r in (4, 5):                                    # one erosion launch, and two that ping-pong through `out`
                buf = torch.full((k + 64,), 0xAB, dtype=torch.uint8, device="cuda")
                wsb = torch.full((nws + 64,), 0xCD, dtype=torch.uint8, device="cuda")
                out = buf[off:off + k].view(mask.shape)
                ws = wsb[32:32 + nws]
                assert ws.data_ptr() % 16 == 0
                got = volumeops.split3d(d, r, "cross", classes=3, out=out, workspace=ws)
                assert got is out and np.array_equal(out.cpu().numpy(), want[r]), (what, r)
                guard, wguard = buf.cpu().numpy(), wsb.cpu().numpy()
                assert np.all(guard[:off] == 0xAB) and np.all(guard[off + k:] == 0xAB), (what, r)
                assert np.all(wguard[:32] == 0xCD) and np.all(wguard[32 + nws:] == 0xCD), (what, r)

    both_forms(monkeypatch, run)
    assert np.array_equal(d.cpu().numpy(), mask)
    with pytest.raises(ValueError, match="contiguous"):
        volumeops.split3d(d[:, :, :, :30], 2, classes=3)
    with pytest.raises(ValueError, match="use sequitr_amd.maskops"):
        volumeops.split3d(d[0], 2, classes=3)
    with pytest.raises(ValueError, match="workspace holds"):
        volumeops.split3d(d, 2, classes=3, workspace=torch.empty(16, dtype=torch.int32, device="cuda"))
    buf = torch.zeros(k + 8, dtype=torch.uint8, device="cuda")
    buf[:k] = d.reshape(-1)
    with pytest.raises(volumeops._lib.SequitrHipError, match="overlap"):
        volumeops.split3d(buf[:k].view(mask.shape), 2, classes=3, out=buf[8:8 + k].view(mask.shape))
    zero = torch.zeros((1, 3, 5, 6), dtype=torch.uint8, device="cuda")
    assert not volumeops.split3d(zero, 1).any()                 # classes default to 2 on an all-background mask


def test_twice_is_bit_identical_and_a_captured_graph_replays_the_eager_bits(monkeypatch):
    mask = np.concatenate([sc.seam_pairs(TILE)[9:11], vc.random_volume(77, 2, 36, 40, 56, 2, 0.9, unknown=False)])
    d = dev(mask)
    vcl = volumeops.VolumeCleanup([{"op": "split3d", "erosions": 4}])

    def run(what):
        a, b = volumeops.split3d(d, 4, classes=2), volumeops.split3d(d, 4, classes=2)
        assert torch.equal(a, b), what
        assert torch.equal(vcl.apply(d, 2).clone(), vcl.apply(d, 2)) and torch.equal(vcl.apply(d, 2), a), what

    both_forms(monkeypatch, run)
    args = (d, 5, "cross", 2 * K + 3)                           # two erosion launches through `out`, an odd count of regrowths
    eager = volumeops.split3d(*args, classes=2)
    out = torch.empty_like(d)
    ws = torch.empty(int(volumeops._lib.load().sq_volume_split_workspace(*mask.shape)) // 4, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        volumeops.split3d(*args, classes=2, out=out, workspace=ws)      # warm up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    out.zero_()
    with torch.cuda.graph(graph):                               # one linear chain of launches on one stream
        volumeops.split3d(*args, classes=2, out=out, workspace=ws)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    assert np.array_equal(eager.cpu().numpy(), sc.split3d_ref(mask, 5, "cross", 2 * K + 3, 2))


def test_volume_cleanup_composition(monkeypatch):
    steps = [{"op": "open", "iterations": 1, "structure": "cross"}, {"op": "fill_holes", "max_voxels": 40},
             {"op": "split3d", "erosions": 4, "structure": "cross", "reach": None}, {"op": "clear_border", "faces": "all"}]
    mask = np.concatenate([sc.seam_pairs(TILE)[::5], sc.seam_pairs(TILE, cls=2)[1::5]])
    mask[vc.random_volume(13, mask.shape[0], 36, 40, 56, 2, 0.02, unknown=False) > 0] = 0       # pepper the objects with cavities
    d = dev(mask)
    want = sc.steps_ref(mask, steps, 3)
    before = vc.steps_ref(mask, steps[:2] + steps[3:], 3)
    assert sc.count_objects(want, 3) > sc.count_objects(before, 3)                  # the split step matters in the chain
    vcl = volumeops.VolumeCleanup(steps)

    def run(what):
        got = vcl.apply(d, 3)
        assert np.array_equal(got.cpu().numpy(), want), what
        buffers = {k: tuple(t.data_ptr() for t in v if t is not None) for k, v in vcl._cache.items()}
        again = vcl.apply(d, 3)
        assert again.data_ptr() == got.data_ptr() and np.array_equal(again.cpu().numpy(), want), what
        assert {k: tuple(t.data_ptr() for t in v if t is not None) for k, v in vcl._cache.items()} == buffers   # nothing new

    both_forms(monkeypatch, run)
    assert np.array_equal(d.cpu().numpy(), mask)
