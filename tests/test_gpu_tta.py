"""GPU: sq_tiles_view_f32 and sq_stitch_probs against the numpy restatement of the header (tests/tta_cases.py), and
segment_frames(tta=, probabilities=) against that restatement around the network's own net.build.  Views are bit-exact
(copies by bit pattern, accumulations against numpy float32 adds), masks byte-equal, probabilities within
(K + 4) * 2^-23 of the float64 softmax."""
import numpy as np
import pytest
import torch

from sequitr_amd import _lib, ops
from sequitr_amd.frontend import FrameTiler, PIX, segment_frames
from sequitr_amd.networks.unet import UNet2D, init_unet_weights
from tests import tta_cases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
BLOCKS = (32, 16)                                               # sq_tiles_view_block: E <= 4, E > 4
T_SIZES = (1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130)    # both blocks - 1 / exact / + 1 / two blocks + 1
E_SIZES = (1, 2, 3, 4, 5, 8, 16)


def tiler_for(T=16):
    return FrameTiler((T, T), tile=T, margin=0, device=DEV)


def stream():
    return torch.cuda.current_stream().cuda_stream


def test_block_sizes_are_the_ones_the_cases_cover():
    lib = _lib.load()
    assert [lib.sq_tiles_view_block(E) for E in range(1, 17)] == [32] * 4 + [16] * 12
    assert lib.sq_tiles_view_block(0) == -1 and lib.sq_tiles_view_block(17) == -1
    for B in BLOCKS:
        assert {B - 1, B, B + 1, 2 * B + 1} <= set(T_SIZES)


def run_all_views(x, pre, monkeypatch, N, T, E):
    """every (lds form, op, direction, plain / accumulating) into its own guarded slot of one buffer: (slots, keys)"""
    tl = tiler_for()
    n = x.numel()
    pitch = n + GUARD + (-n) % 4                                # every slot starts 16-byte aligned
    keys = [(lds, op, inv, acc) for lds in ("1", "0") for op in tc.OPS for inv in (False, True) for acc in (False, True)]
    slots = torch.empty((len(keys), pitch), dtype=torch.float32, device=DEV)
    slots[:, :n] = pre.reshape(-1)
    slots[:, n:] = -77.0
    for s, (lds, op, inv, acc) in enumerate(keys):
        monkeypatch.setenv("SQ_TTA_LDS", lds)
        tl.view(x, op, inverse=inv, out=slots[s, :n].view(N, T, T, E), accumulate=acc)
    torch.cuda.synchronize()
    return slots.cpu().numpy(), keys, n


@pytest.mark.parametrize("E", E_SIZES)
@pytest.mark.parametrize("N,T", [(3, T) for T in T_SIZES] + [(1, 1), (1, 3), (1, 33)])
def test_views_are_bit_exact(monkeypatch, N, T, E):
    rng = np.random.default_rng(1000 * T + 10 * E + N)
    x_h, pre_h = tc.special_values((N, T, T, E), rng), tc.special_values((N, T, T, E), rng)
    x, pre = torch.from_numpy(x_h).to(DEV), torch.from_numpy(pre_h).to(DEV)
    got, keys, n = run_all_views(x, pre, monkeypatch, N, T, E)
    want = {(op, inv): (tc.unview if inv else tc.view)(x_h, op) for op in tc.OPS for inv in (False, True)}
    by_key = {}
    for s, (lds, op, inv, acc) in enumerate(keys):
        out = got[s, :n].reshape(N, T, T, E)
        assert (got[s, n:] == -77.0).all(), ("guard", lds, op, inv, acc)
        ref = want[(op, inv)]
        if acc:
            with np.errstate(invalid="ignore"):
                assert tc.same_bits_nan_aware(out, pre_h + ref), ("accumulate", lds, op, inv)
        else:
            assert np.array_equal(tc.bits(out), tc.bits(ref)), ("copy", lds, op, inv)       # NaN payloads included
        by_key[(lds, op, inv, acc)] = out
    for (lds, op, inv, acc), out in by_key.items():             # the two forms give the same bits
        if lds == "1":
            assert np.array_equal(tc.bits(out), tc.bits(by_key[("0", op, inv, acc)])), (op, inv, acc)


def test_views_past_the_grid_cap(monkeypatch):
    """N * blocks > 16384 items of the LDS form and more than 16384 * 256 floats of the row form: the block-stride loops"""
    N, T, E = 4100, 33, 1
    rng = np.random.default_rng(5)
    x_h = rng.standard_normal((N, T, T, E)).astype(np.float32)
    pre_h = rng.standard_normal((N, T, T, E)).astype(np.float32)
    x, tl = torch.from_numpy(x_h).to(DEV), tiler_for()
    for lds, op, acc in (("1", 5, False), ("1", 6, True), ("0", 5, True), ("1", 2, False), ("1", 3, True)):
        monkeypatch.setenv("SQ_TTA_LDS", lds)
        out = torch.from_numpy(pre_h).to(DEV)
        tl.view(x, op, out=out, accumulate=acc)
        ref = tc.view(x_h, op)
        assert np.array_equal(tc.bits(out.cpu().numpy()), tc.bits(pre_h + ref if acc else ref)), (lds, op, acc)
    x4 = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(x_h[:1100], (1100, T, T, 4)))).to(DEV)   # 16-byte units
    out = tl.view(x4, 3)
    assert np.array_equal(tc.bits(out.cpu().numpy()), tc.bits(tc.view(x4.cpu().numpy(), 3)))


@pytest.mark.parametrize("E", [3, 8])
def test_views_twice_and_graph_replay(monkeypatch, E):
    N, T = 3, 65
    rng = np.random.default_rng(E)
    x = torch.from_numpy(tc.special_values((N, T, T, E), rng)).to(DEV)
    pre = torch.from_numpy(rng.standard_normal((N, T, T, E)).astype(np.float32)).to(DEV)
    tl = tiler_for()
    for lds in ("1", "0"):
        monkeypatch.setenv("SQ_TTA_LDS", lds)

        def chain(buf):                                         # the merge of the dihedral set, as segment_frames runs it
            for op in tc.OPS:
                tl.view(x, op, inverse=True, out=buf, accumulate=op != 0)

        a, b, c = pre.clone(), pre.clone(), pre.clone()
        chain(a)
        chain(b)
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            chain(c)
        for _ in range(2):
            c.copy_(pre)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(a.view(torch.int32), c.view(torch.int32)), lds


def test_view_refusals_leave_dst_untouched():
    lib = _lib.load()
    N, T, E = 2, 8, 4
    n = N * T * T * E
    buf = torch.arange(3 * n + 8, dtype=torch.float32, device=DEV)
    before = buf.clone()
    src, dst = buf[:n], buf[2 * n:3 * n]
    call = lambda s, d, N=N, T=T, E=E, op=1: lib.sq_tiles_view_f32(s, d, N, T, E, op, 0, 0, stream())
    cases = {
        "same": call(src.data_ptr(), src.data_ptr()),
        "overlap ahead": call(src.data_ptr(), buf[n // 2:].data_ptr()),
        "overlap behind": call(buf[n // 2:].data_ptr(), src.data_ptr()),
        "op 8": call(src.data_ptr(), dst.data_ptr(), op=8),
        "op -1": call(src.data_ptr(), dst.data_ptr(), op=-1),
        "E 0": call(src.data_ptr(), dst.data_ptr(), E=0),
        "E 17": call(src.data_ptr(), dst.data_ptr(), E=17),
        "T 0": call(src.data_ptr(), dst.data_ptr(), T=0),
        "T 65536": call(src.data_ptr(), dst.data_ptr(), T=65536),
        "N 0": call(src.data_ptr(), dst.data_ptr(), N=0),
        "null": call(None, dst.data_ptr()),
        "src misaligned": call(buf[1:].data_ptr(), dst.data_ptr()),
        "dst misaligned": call(src.data_ptr(), buf[2 * n + 1:].data_ptr()),
    }
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in cases.values()), cases
    assert cases["src misaligned"] == cases["dst misaligned"] == -3          # SQ_EALIGN
    assert torch.equal(buf, before)
    assert call(src.data_ptr(), buf[n:2 * n].data_ptr()) == 0                # adjacent ranges do not overlap
    tl = tiler_for()
    x = src.view(N, T, T, E)
    for bad in (lambda: tl.view(x, 8), lambda: tl.view(x, True), lambda: tl.view(x, 1, accumulate=True),
                lambda: tl.view(x, 1, out=torch.empty(n, device=DEV)), lambda: tl.view(x[:, :, :4], 1),
                lambda: tl.view(x.double(), 1)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(_lib.SequitrHipError):
        tl.view(x, 1, out=x)
    with pytest.raises(_lib.SequitrHipError):
        tl.view(x.cpu(), 1)


# ---- stitch ------------------------------------------------------------------------------------------------------------
def stitch_case(H, W, T, margin, F, K, inv_n, seed):
    """tile sums whose mean has a spread of 20, with every special row written once at a frame pixel through its owner"""
    rng = np.random.default_rng(seed)
    ymap, xmap, TR, TC = tc.owner_maps(H, W, T, margin)
    acc = ((rng.random((F * TR * TC, T, T, K)) * 20.0).astype(np.float32) / np.float32(inv_n)).astype(np.float32)
    rows = tc.special_rows(K, rng)
    where = rng.permutation(F * H * W)[:len(rows)]
    for r, flat in zip(rows, where):
        f, y, x = flat // (H * W), (flat // W) % H, flat % W
        acc[(f * TR + (ymap[y] >> 16)) * TC + (xmap[x] >> 16), ymap[y] & 0xffff, xmap[x] & 0xffff] = r / np.float32(inv_n)
    return acc


@pytest.mark.parametrize("K", [1, 2, 3, 4, 7, 8, 16])
@pytest.mark.parametrize("H,W", [(37, 53), (64, 64), (16, 80)])
def test_stitch_probs_matches_the_restatement(H, W, K):
    T, margin = 16, 2
    tl = FrameTiler((H, W), tile=T, margin=margin, device=DEV)
    worst = 0.0
    for F in (1, 3):
        for n in (1, 4, 8):
            acc_h = stitch_case(H, W, T, margin, F, K, 1.0 / n, seed=100 * K + 10 * F + n)
            acc = torch.from_numpy(acc_h).to(DEV)
            want_mask, want_p = tc.stitch_probs(acc_h, 1.0 / n, H, W, T, margin)
            mask, p32 = tl.stitch_probs(acc, n=n, probabilities="float32")
            mask_b, p8 = tl.stitch_probs(acc, n=n, probabilities="uint8")
            what = "%dx%d F=%d n=%d" % (H, W, F, n)
            assert mask.dtype == torch.uint8 and np.array_equal(mask.cpu().numpy(), want_mask), what
            assert torch.equal(mask, mask_b)
            if n == 1:                                          # today's path on the same logits, byte for byte
                assert torch.equal(mask, tl.stitch(ops.argmax_u8(acc))), what
            assert tuple(p32.shape) == (F, K, H, W) and p32.dtype == torch.float32
            worst = max(worst, tc.check_probs(p32.cpu().numpy(), want_p, K, what))
            tc.check_probs_u8(p8.cpu().numpy(), want_p, K, what)
            only_mask, none = tl.stitch_probs(acc, n=n)         # each output alone
            assert none is None and torch.equal(only_mask, mask)
            none, only_p = tl.stitch_probs(acc, n=n, mask=False, probabilities="float32")
            assert none is None and torch.equal(only_p.view(torch.int32), p32.view(torch.int32))
    print("K=%d %dx%d: worst |p - p64| = %.3g of %.3g allowed" % (K, H, W, worst, tc.prob_bound(K)))


def raw_stitch(tl, acc, inv_n, mask, prob, F, K):
    dtype = PIX[prob.dtype] if prob is not None else 0
    return _lib.load().sq_stitch_probs(acc.data_ptr(), tl._ymap.data_ptr(), tl._xmap.data_ptr(),
                                       mask.data_ptr() if mask is not None else None,
                                       prob.data_ptr() if prob is not None else None, dtype, inv_n, F, tl.H, tl.W, tl.TR, tl.TC,
                                       tl.T, K, stream())


@pytest.mark.parametrize("K", [2, 3, 16])
def test_stitch_probs_guards_twice_and_graph(K):
    H, W, T, margin, F = 37, 53, 16, 2, 3
    tl = FrameTiler((H, W), tile=T, margin=margin, device=DEV)
    acc = torch.from_numpy(stitch_case(H, W, T, margin, F, K, 0.25, seed=K)).to(DEV)
    npix = F * H * W
    mask = torch.full((npix + GUARD,), 201, dtype=torch.uint8, device=DEV)
    p32 = torch.full((npix * K + GUARD,), -5.0, dtype=torch.float32, device=DEV)
    p8 = torch.full((npix * K + GUARD,), 202, dtype=torch.uint8, device=DEV)
    assert raw_stitch(tl, acc, 0.25, mask, p32, F, K) == 0 and raw_stitch(tl, acc, 0.25, None, p8, F, K) == 0
    want_mask, want_p = tl.stitch_probs(acc, n=4, probabilities="float32")
    want_p8 = tl.stitch_probs(acc, n=4, mask=False, probabilities="uint8")[1]
    torch.cuda.synchronize()
    assert (mask[npix:] == 201).all() and (p32[npix * K:] == -5.0).all() and (p8[npix * K:] == 202).all()
    assert torch.equal(mask[:npix], want_mask.view(-1))
    assert torch.equal(p32[:npix * K].view(torch.int32), want_p.view(-1).view(torch.int32))       # run to run the same bits
    assert torch.equal(p8[:npix * K], want_p8.view(-1))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        raw_stitch(tl, acc, 0.25, mask, p32, F, K)
    for _ in range(2):
        mask.fill_(0), p32.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(mask[:npix], want_mask.view(-1))
        assert torch.equal(p32[:npix * K].view(torch.int32), want_p.view(-1).view(torch.int32))
    # refusals: nothing is written
    before = (mask.clone(), p32.clone())
    lib = _lib.load()
    assert raw_stitch(tl, acc, 0.25, None, None, F, K) != 0 and b"mask_out, prob_out" in lib.sq_last_error()
    assert raw_stitch(tl, acc, 0.0, mask, p32, F, K) != 0 and raw_stitch(tl, acc, 0.25, mask, p32, F, 17) != 0
    assert lib.sq_stitch_probs(acc.data_ptr(), tl._ymap.data_ptr(), tl._xmap.data_ptr(), mask.data_ptr(), p32.data_ptr(), 1,
                               0.25, F, H, W, tl.TR, tl.TC, T, K, stream()) != 0            # SQ_PIX_U16 is no probability type
    torch.cuda.synchronize()
    assert torch.equal(mask, before[0]) and torch.equal(p32.view(torch.int32), before[1].view(torch.int32))
    for bad in (lambda: tl.stitch_probs(acc, n=2), lambda: tl.stitch_probs(acc, mask=False),
                lambda: tl.stitch_probs(acc, probabilities="float16"), lambda: tl.stitch_probs(acc[1:]),
                lambda: tl.stitch_probs(acc[:, :8])):
        with pytest.raises(ValueError):
            bad()


def test_stitch_probs_past_the_grid_cap():
    """2100 x 2100 pixels are more than 16384 chunks of 256"""
    H = W = 2100
    T, margin, K = 300, 10, 2
    tl = FrameTiler((H, W), tile=T, margin=margin, device=DEV)
    rng = np.random.default_rng(9)
    acc_h = (rng.standard_normal((tl.tiles_per_frame, T, T, K)) * 5).astype(np.float32)
    mask, p = tl.stitch_probs(torch.from_numpy(acc_h).to(DEV), probabilities="float32")
    want_mask, want_p = tc.stitch_probs(acc_h, 1.0, H, W, T, margin)
    assert np.array_equal(mask.cpu().numpy(), want_mask)
    tc.check_probs(p.cpu().numpy(), want_p, K, "2100x2100")


# ---- segment_frames ----------------------------------------------------------------------------------------------------
TILE, MARGIN, FRAME = 32, 4, (70, 90)


def make_net(C=1, K=2, seed=11):
    params = {"shape": (TILE, TILE), "filters": (16, 32), "device": DEV, "num_inputs": C, "num_outputs": K}
    net = UNet2D(params, "infer")
    net.load_state_dict(init_unet_weights(params, seed))
    return net


def make_frames(C=1, seed=3):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:FRAME[0], :FRAME[1]]
    stacks = []
    for c in range(C):                                          # blobs on a ramp: nothing a symmetry maps onto itself
        f = 400 + 3 * yy[None] + 2 * xx[None] + rng.integers(0, 300, (3,) + FRAME)
        for k in range(6):
            cy, cx, r = rng.integers(8, 62), rng.integers(8, 82), rng.integers(4, 9)
            f = f + 1500 * ((yy - cy) ** 2 + (xx - cx) ** 2 < r * r)[None] * (np.arange(3)[:, None, None] + 1 + c)
        stacks.append(f.astype(np.uint16))
    return stacks[0] if C == 1 else stacks


def restate(net, frames, tta, fpb):
    """(masks, float64 probabilities, sums) of the header's text around net.build, batched as segment_frames batches"""
    stacks = frames if isinstance(frames, list) else [frames]
    C, F = len(stacks), stacks[0].shape[0]
    tl = FrameTiler(FRAME, tile=TILE, margin=MARGIN, device=DEV, channels=C)
    ops_, masks, probs = tc.SETS[tta], [], []
    for first in range(0, F, fpb):
        raw = torch.from_numpy(np.stack([s[first:first + fpb] for s in stacks])).to(DEV)
        tiles = tl.tiles(raw[0] if C == 1 else raw).cpu().numpy()
        by_op = {}
        for op in ops_:
            viewed = torch.from_numpy(tc.view(tiles, op)).to(DEV)
            by_op[op] = net.build(viewed).cpu().numpy().copy()
        acc = tc.merge(by_op, ops_)
        m, p = tc.stitch_probs(acc, 1.0 / len(ops_), FRAME[0], FRAME[1], TILE, MARGIN)
        masks.append(m), probs.append(p)
    return np.concatenate(masks), np.concatenate(probs)


@pytest.fixture(scope="module")
def net2():
    return make_net()


@pytest.mark.parametrize("fpb", [3, 1, 2])
@pytest.mark.parametrize("tta", ["dihedral", "flips"])
def test_segment_frames_tta_matches_the_restatement(net2, tta, fpb):
    frames = make_frames()
    want_mask, want_p = restate(net2, frames, tta, fpb)
    masks = segment_frames(net2, frames, tile=TILE, margin=MARGIN, frames_per_batch=fpb, tta=tta)
    assert isinstance(masks, np.ndarray) and masks.dtype == np.uint8 and np.array_equal(masks, want_mask)
    plain = segment_frames(net2, frames, tile=TILE, margin=MARGIN, frames_per_batch=fpb)
    print("tta=%s changes %d of %d pixels; foreground %.3f" % (tta, int((masks != plain).sum()), masks.size, masks.mean()))
    assert 0 < masks.mean() < 1
    for kind, check in (("float32", tc.check_probs), ("uint8", tc.check_probs_u8)):
        m, p = segment_frames(net2, frames, tile=TILE, margin=MARGIN, frames_per_batch=fpb, tta=tta, probabilities=kind)
        assert np.array_equal(m, want_mask) and p.shape == (3, 2) + FRAME and p.dtype == np.dtype(kind)
        check(p, want_p, 2, "%s %s fpb=%d" % (tta, kind, fpb))


def test_probabilities_alone_keep_the_plain_masks(net2):
    frames = make_frames()
    plain = segment_frames(net2, frames, tile=TILE, margin=MARGIN, frames_per_batch=2)
    m, p = segment_frames(net2, frames, tile=TILE, margin=MARGIN, frames_per_batch=2, probabilities="float32")
    assert np.array_equal(m, plain)
    want_mask, want_p = restate(net2, frames, None, 2)
    assert np.array_equal(plain, want_mask)
    tc.check_probs(p, want_p, 2, "tta=None")
    assert np.array_equal(p.argmax(1).astype(np.uint8)[p.max(1) > 0.5 + 1e-6], plain[p.max(1) > 0.5 + 1e-6])


def test_two_channels_three_classes():
    net = make_net(C=2, K=3, seed=5)
    frames = make_frames(C=2)
    want_mask, want_p = restate(net, frames, "dihedral", 2)
    m, p = segment_frames(net, frames, tile=TILE, margin=MARGIN, frames_per_batch=2, tta="dihedral", probabilities="float32")
    assert np.array_equal(m, want_mask) and p.shape == (3, 3) + FRAME
    tc.check_probs(p, want_p, 3, "C=2 K=3")
    m8, p8 = segment_frames(net, np.stack(frames, -1), tile=TILE, margin=MARGIN, frames_per_batch=3, tta="dihedral",
                            probabilities="uint8")                      # the interleaved form of the same frames
    assert np.array_equal(m8, restate(net, frames, "dihedral", 3)[0])
    tc.check_probs_u8(p8, restate(net, frames, "dihedral", 3)[1], 3, "C=2 K=3 uint8")


def test_sinks_see_probabilities_first_and_postprocess_only_the_masks(net2):
    frames = make_frames()
    want_mask, want_p = restate(net2, frames, "flips", 2)
    for sink in ("on_masks", "on_batch"):
        seen = []
        on_probs = lambda first, p: seen.append(("probs", first, p.cpu().numpy()))
        on_masks = lambda first, m: seen.append(("masks", first, m.cpu().numpy()))
        on_batch = lambda first, raw, m: seen.append(("masks", first, m.cpu().numpy(), tuple(raw.shape)))
        kw = {"on_masks": on_masks} if sink == "on_masks" else {"on_batch": on_batch}
        assert segment_frames(net2, frames, tile=TILE, margin=MARGIN, frames_per_batch=2, tta="flips", probabilities="float32",
                              on_probs=on_probs, **kw) is None
        assert [(s[0], s[1]) for s in seen] == [("probs", 0), ("masks", 0), ("probs", 2), ("masks", 2)]
        assert np.array_equal(np.concatenate([s[2] for s in seen if s[0] == "masks"]), want_mask)
        tc.check_probs(np.concatenate([s[2] for s in seen if s[0] == "probs"]), want_p, 2, sink)
    steps = [{"op": "open", "iterations": 1, "structure": "cross"}, {"op": "clear_border"}]
    m, p = segment_frames(net2, frames, tile=TILE, margin=MARGIN, frames_per_batch=2, tta="flips", probabilities="float32",
                          postprocess=steps)
    m0, p0 = segment_frames(net2, frames, tile=TILE, margin=MARGIN, frames_per_batch=2, tta="flips", probabilities="float32")
    assert np.array_equal(m0, want_mask) and not np.array_equal(m, m0) and (m <= m0).all()
    assert np.array_equal(p.view(np.uint32), p0.view(np.uint32))        # the probabilities are the network's own


def test_bad_values_raise_before_a_frame_is_read(net2):
    class Untouchable(object):
        shape, dtype = (3,) + FRAME, np.dtype("uint16")

        def __getitem__(self, key):
            raise AssertionError("a frame was read")

    fr = Untouchable()
    kw = dict(tile=TILE, margin=MARGIN)
    for bad in ({"tta": "rot90"}, {"tta": 4}, {"tta": True}, {"tta": ("flips",)}, {"probabilities": "float16"},
                {"probabilities": True}, {"probabilities": np.float32}, {"on_probs": print},
                {"probabilities": "uint8", "on_probs": print}, {"probabilities": "uint8", "on_masks": print},
                {"tta": "flips", "on_probs": print, "on_masks": print}):
        with pytest.raises(ValueError):
            segment_frames(net2, fr, **dict(kw, **bad))
    with pytest.raises(AssertionError, match="a frame was read"):      # good values do get as far as the frames
        segment_frames(net2, fr, tta="flips", **kw)
