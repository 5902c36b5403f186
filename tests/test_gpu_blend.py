"""GPU: sq_stitch_blend against the numpy restatement of the header's "Seam blending" (tests/blend_cases.py), and
segment_frames(blend=) against that restatement around the network's own net.build.  Masks are byte-equal (the blended
logits are restated bit for bit), float32 probabilities within (K + 4) * 2^-23 of the float64 softmax of the restated l_k,
uint8 ones equal away from a rounding boundary.  Every case hands the kernel NaN at the tile positions whose weight is
zero everywhere, and the restatement the clean logits: a NaN that does not contribute must not show."""
import numpy as np
import pytest
import torch

from sequitr_amd import _lib
from sequitr_amd.frontend import FrameTiler, PIX, segment_frames
from tests import blend_cases as bc
from tests import tta_cases as tc
from tests.test_gpu_tta import FRAME, MARGIN, TILE, make_frames, make_net

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("K", bc.KS)
@pytest.mark.parametrize("H,W,T,margin,B", bc.geometry_cases())
def test_stitch_blend_matches_the_restatement(H, W, T, margin, B, K):
    tl = FrameTiler((H, W), tile=T, margin=margin, device=DEV)
    worst = 0.0
    for F in (1, 3):
        for n in (1, 4, 8):
            clean, poisoned = bc.blend_case(H, W, T, margin, B, F, K, 1.0 / n, seed=1000 * B + 100 * K + 10 * F + n)
            acc = torch.from_numpy(poisoned).to(DEV)
            want_mask, want_p = bc.stitch_blend(clean, 1.0 / n, H, W, T, margin, B)
            assert np.isnan(want_p).any() and np.isfinite(want_p).any()
            mask, p32 = tl.stitch_blend(acc, B, n=n, probabilities="float32")
            mask_b, p8 = tl.stitch_blend(acc, B, n=n, probabilities="uint8")
            what = "%dx%d T=%d B=%d F=%d n=%d" % (H, W, T, B, F, n)
            assert mask.dtype == torch.uint8 and np.array_equal(mask.cpu().numpy(), want_mask), what
            assert torch.equal(mask, mask_b)
            assert tuple(p32.shape) == (F, K, H, W) and p32.dtype == torch.float32
            worst = max(worst, tc.check_probs(p32.cpu().numpy(), want_p, K, what))
            assert bc.u8_boundary_share(want_p, K) < 0.01, what                    # at least 99 % of the values are compared
            tc.check_probs_u8(p8.cpu().numpy(), want_p, K, what)
            only_mask, none = tl.stitch_blend(acc, B, n=n)                          # each output alone
            assert none is None and torch.equal(only_mask, mask)
            none, only_p = tl.stitch_blend(acc, B, n=n, mask=False, probabilities="float32")
            assert none is None and torch.equal(only_p.view(torch.int32), p32.view(torch.int32))
    print("K=%d %dx%d B=%d: worst |p - p64| = %.3g of %.3g allowed" % (K, H, W, B, worst, tc.prob_bound(K)))


@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("H,W,T,margin", bc.GEOMETRIES + [bc.BIG_GEOMETRY])
def test_no_blend_is_stitch_probs_bit_for_bit(H, W, T, margin, K):
    tl = FrameTiler((H, W), tile=T, margin=margin, device=DEV)
    _, poisoned = bc.blend_case(H, W, T, margin, 0, 2, K, 0.25, seed=K)
    acc = torch.from_numpy(poisoned).to(DEV)
    for kind in ("float32", "uint8"):
        mask, p = tl.stitch_blend(acc, 0, n=4, probabilities=kind)
        want_mask, want_p = tl.stitch_probs(acc, n=4, probabilities=kind)
        assert torch.equal(mask, want_mask)
        assert torch.equal(p.view(torch.int32) if kind == "float32" else p, want_p.view(torch.int32) if kind == "float32" else want_p)


def raw_blend(tl, B, acc, inv_n, mask, prob, F, K):
    yslots, xslots = tl._blend_slots[B]                         # made by the first FrameTiler.stitch_blend of this blend
    dtype = PIX[prob.dtype] if prob is not None else 0
    return _lib.load().sq_stitch_blend(acc.data_ptr(), yslots.data_ptr(), xslots.data_ptr(),
                                       mask.data_ptr() if mask is not None else None,
                                       prob.data_ptr() if prob is not None else None, dtype, inv_n, F, tl.H, tl.W, tl.TR, tl.TC,
                                       tl.T, K, stream())


@pytest.mark.parametrize("K", [2, 3, 16])
def test_stitch_blend_guards_twice_and_graph(K):
    H, W, T, margin, B, F = 37, 53, 16, 4, 4, 3
    tl = FrameTiler((H, W), tile=T, margin=margin, device=DEV)
    acc = torch.from_numpy(bc.blend_case(H, W, T, margin, B, F, K, 0.25, seed=K)[1]).to(DEV)
    npix = F * H * W
    mask = torch.full((npix + GUARD,), 201, dtype=torch.uint8, device=DEV)
    p32 = torch.full((npix * K + GUARD,), -5.0, dtype=torch.float32, device=DEV)
    p8 = torch.full((npix * K + GUARD,), 202, dtype=torch.uint8, device=DEV)
    want_mask, want_p = tl.stitch_blend(acc, B, n=4, probabilities="float32")
    assert raw_blend(tl, B, acc, 0.25, mask, p32, F, K) == 0 and raw_blend(tl, B, acc, 0.25, None, p8, F, K) == 0
    want_p8 = tl.stitch_blend(acc, B, n=4, mask=False, probabilities="uint8")[1]
    torch.cuda.synchronize()
    assert (mask[npix:] == 201).all() and (p32[npix * K:] == -5.0).all() and (p8[npix * K:] == 202).all()
    assert torch.equal(mask[:npix], want_mask.view(-1))
    assert torch.equal(p32[:npix * K].view(torch.int32), want_p.view(-1).view(torch.int32))       # run to run the same bits
    assert torch.equal(p8[:npix * K], want_p8.view(-1))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        raw_blend(tl, B, acc, 0.25, mask, p32, F, K)
    for _ in range(2):
        mask.fill_(0), p32.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(mask[:npix], want_mask.view(-1))
        assert torch.equal(p32[:npix * K].view(torch.int32), want_p.view(-1).view(torch.int32))
    # refusals: nothing is written
    before = (mask.clone(), p32.clone())
    lib = _lib.load()
    yslots, xslots = tl._blend_slots[B]
    assert raw_blend(tl, B, acc, 0.25, None, None, F, K) != 0 and b"mask_out, prob_out" in lib.sq_last_error()
    assert raw_blend(tl, B, acc, 0.0, mask, p32, F, K) != 0 and raw_blend(tl, B, acc, 0.25, mask, p32, F, 17) != 0
    assert raw_blend(tl, B, acc, 0.25, mask, p32, F, 0) != 0 and raw_blend(tl, B, acc, 2.0, mask, p32, F, K) != 0
    call = lambda a=acc.data_ptr(), ys=yslots.data_ptr(), xs=xslots.data_ptr(), m=mask.data_ptr(), p=p32.data_ptr(), dt=2, f=F: \
        lib.sq_stitch_blend(a, ys, xs, m, p, dt, 0.25, f, H, W, tl.TR, tl.TC, T, K, stream())
    cases = {"u16 probabilities": call(dt=1), "null logits": call(a=None), "null yslots": call(ys=None),
             "null xslots": call(xs=None), "no frames": call(f=0), "logits misaligned": call(a=acc.data_ptr() + 4),
             "slots misaligned": call(ys=yslots.data_ptr() + 4), "probabilities misaligned": call(p=p32.data_ptr() + 2)}
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in cases.values()), cases
    assert cases["logits misaligned"] == -3                                                # SQ_EALIGN
    assert torch.equal(mask, before[0]) and torch.equal(p32.view(torch.int32), before[1].view(torch.int32))
    for bad in (lambda: tl.stitch_blend(acc, B, n=2), lambda: tl.stitch_blend(acc, B, mask=False),
                lambda: tl.stitch_blend(acc, B, probabilities="float16"), lambda: tl.stitch_blend(acc[1:], B),
                lambda: tl.stitch_blend(acc[:, :8], B), lambda: tl.stitch_blend(acc, 5), lambda: tl.stitch_blend(acc, -1),
                lambda: tl.stitch_blend(acc, True), lambda: tl.stitch_blend(acc, 1.0)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(_lib.SequitrHipError):
        tl.stitch_blend(acc.cpu(), B)
    assert sorted(tl._blend_slots) == [4]                       # one pair of tables per blend, made once
    tables = tl._blend_slots[4]
    tl.stitch_blend(acc, 4), tl.stitch_blend(acc, 2)
    assert tl._blend_slots[4] is tables and sorted(tl._blend_slots) == [2, 4]


def test_stitch_blend_past_the_grid_cap():
    """2100 x 2100 pixels are more than 16384 chunks of 256"""
    H = W = 2100
    T, margin, B, K = 300, 10, 7, 2
    tl = FrameTiler((H, W), tile=T, margin=margin, device=DEV)
    rng = np.random.default_rng(9)
    acc_h = (rng.standard_normal((tl.tiles_per_frame, T, T, K)) * 5).astype(np.float32)
    mask, p = tl.stitch_blend(torch.from_numpy(acc_h).to(DEV), B, probabilities="float32")
    want_mask, want_p = bc.stitch_blend(acc_h, 1.0, H, W, T, margin, B)
    assert np.array_equal(mask.cpu().numpy(), want_mask)
    tc.check_probs(p.cpu().numpy(), want_p, K, "2100x2100")


# ---- segment_frames ----------------------------------------------------------------------------------------------------
def restate(net, frames, tta, fpb, blend):
    """(masks, float64 probabilities) of the header's text around net.build, batched as segment_frames batches"""
    stacks = frames if isinstance(frames, list) else [frames]
    C, F = len(stacks), stacks[0].shape[0]
    tl = FrameTiler(FRAME, tile=TILE, margin=MARGIN, device=DEV, channels=C)
    ops_, masks, probs = tc.SETS[tta], [], []
    for first in range(0, F, fpb):
        raw = torch.from_numpy(np.stack([s[first:first + fpb] for s in stacks])).to(DEV)
        tiles = tl.tiles(raw[0] if C == 1 else raw).cpu().numpy()
        by_op = {op: net.build(torch.from_numpy(tc.view(tiles, op)).to(DEV)).cpu().numpy().copy() for op in ops_}
        m, p = bc.stitch_blend(tc.merge(by_op, ops_), 1.0 / len(ops_), FRAME[0], FRAME[1], TILE, MARGIN, blend)
        masks.append(m), probs.append(p)
    return np.concatenate(masks), np.concatenate(probs)


@pytest.fixture(scope="module")
def net2():
    return make_net()


@pytest.fixture(scope="module")
def plain(net2):
    """today's arrays: no blend"""
    return segment_frames(net2, make_frames(), tile=TILE, margin=MARGIN, frames_per_batch=2)


def seam_pixels(blend):
    (_, ys), (_, xs) = bc.axis_blend(FRAME[0], TILE, MARGIN, blend), bc.axis_blend(FRAME[1], TILE, MARGIN, blend)
    return ((ys[:, :, 1] > 0).sum(1) > 1)[:, None] | ((xs[:, :, 1] > 0).sum(1) > 1)[None, :]


@pytest.mark.parametrize("fpb", [3, 1, 2])
@pytest.mark.parametrize("tta", [None, "flips"])
@pytest.mark.parametrize("blend", [2, 4])
def test_segment_frames_blend_matches_the_restatement(net2, plain, blend, tta, fpb):
    frames = make_frames()
    want_mask, want_p = restate(net2, frames, tta, fpb, blend)
    masks = segment_frames(net2, frames, tile=TILE, margin=MARGIN, frames_per_batch=fpb, tta=tta, blend=blend)
    assert isinstance(masks, np.ndarray) and masks.dtype == np.uint8 and np.array_equal(masks, want_mask)
    assert 0 < masks.mean() < 1
    if tta is None:                                             # the blend changes the mask, and only where tiles are mixed
        changed = masks != plain
        print("blend=%d changes %d of %d pixels" % (blend, int(changed.sum()), masks.size))
        assert changed.any() and not changed[:, ~seam_pixels(blend)].any()
    for kind, check in (("float32", tc.check_probs), ("uint8", tc.check_probs_u8)):
        m, p = segment_frames(net2, frames, tile=TILE, margin=MARGIN, frames_per_batch=fpb, tta=tta, probabilities=kind,
                              blend=blend)
        assert np.array_equal(m, want_mask) and p.shape == (3, 2) + FRAME and p.dtype == np.dtype(kind)
        check(p, want_p, 2, "blend=%d %s %s fpb=%d" % (blend, tta, kind, fpb))


def test_no_blend_is_exactly_today(net2, plain):
    frames = make_frames()
    for blend in (None, 0):
        assert np.array_equal(segment_frames(net2, frames, tile=TILE, margin=MARGIN, frames_per_batch=2, blend=blend), plain)
        m, p = segment_frames(net2, frames, tile=TILE, margin=MARGIN, frames_per_batch=2, tta="flips", probabilities="float32",
                              blend=blend)
        m0, p0 = segment_frames(net2, frames, tile=TILE, margin=MARGIN, frames_per_batch=2, tta="flips", probabilities="float32")
        assert np.array_equal(m, m0) and np.array_equal(p.view(np.uint32), p0.view(np.uint32))


def test_two_channels_three_classes_blended():
    net = make_net(C=2, K=3, seed=5)
    frames = make_frames(C=2)
    want_mask, want_p = restate(net, frames, "flips", 2, 4)
    m, p = segment_frames(net, frames, tile=TILE, margin=MARGIN, frames_per_batch=2, tta="flips", probabilities="float32", blend=4)
    assert np.array_equal(m, want_mask) and p.shape == (3, 3) + FRAME
    tc.check_probs(p, want_p, 3, "C=2 K=3 blend=4")


def test_sinks_and_postprocess_see_the_blended_mask(net2):
    frames = make_frames()
    want_mask, want_p = restate(net2, frames, None, 2, 4)
    for sink in ("on_masks", "on_batch"):
        seen = []
        on_probs = lambda first, p: seen.append(("probs", first, p.cpu().numpy()))
        on_masks = lambda first, m: seen.append(("masks", first, m.cpu().numpy()))
        on_batch = lambda first, raw, m: seen.append(("masks", first, m.cpu().numpy(), tuple(raw.shape)))
        kw = {"on_masks": on_masks} if sink == "on_masks" else {"on_batch": on_batch}
        assert segment_frames(net2, frames, tile=TILE, margin=MARGIN, frames_per_batch=2, probabilities="float32",
                              on_probs=on_probs, blend=4, **kw) is None
        assert [(s[0], s[1]) for s in seen] == [("probs", 0), ("masks", 0), ("probs", 2), ("masks", 2)]
        assert np.array_equal(np.concatenate([s[2] for s in seen if s[0] == "masks"]), want_mask)
        tc.check_probs(np.concatenate([s[2] for s in seen if s[0] == "probs"]), want_p, 2, sink)
    steps = [{"op": "open", "iterations": 1, "structure": "cross"}, {"op": "clear_border"}]
    m = segment_frames(net2, frames, tile=TILE, margin=MARGIN, frames_per_batch=2, postprocess=steps, blend=4)
    from sequitr_amd.maskops import MaskCleanup
    cleaned = MaskCleanup(steps).apply(torch.from_numpy(want_mask).to(DEV), 2).cpu().numpy()
    assert np.array_equal(m, cleaned) and not np.array_equal(m, want_mask)


def test_bad_blends_raise_before_a_frame_is_read(net2):
    class Untouchable(object):
        shape, dtype = (3,) + FRAME, np.dtype("uint16")

        def __getitem__(self, key):
            raise AssertionError("a frame was read")

    fr = Untouchable()
    for kw in ({"blend": 5}, {"blend": -1}, {"blend": True}, {"blend": 2.0}, {"blend": "2"}, {"blend": 1, "margin": 0},
               {"blend": 5, "margin": 12}):
        with pytest.raises(ValueError, match="blend"):
            segment_frames(net2, fr, **dict(dict(tile=TILE, margin=MARGIN), **kw))
    with pytest.raises(AssertionError, match="a frame was read"):      # a good value does get as far as the frames
        segment_frames(net2, fr, tile=TILE, margin=MARGIN, blend=4)
