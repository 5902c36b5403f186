"""GPU: multi-channel frames (include/sequitr_hip.h, the _mc paragraphs of "Tile front end" and "Tile sampler").

(a) sq_frames_to_tiles_mc: channel c of the interleaved tiles has the bits the single-channel tiler gives on channel c's
    stack, under every mode and a mixed vector; the tiles equal the numpy restatement (tests/multichannel_cases.py); a
    strided [:, :n] view equals its packed copy; nothing is written past the output; C = 1 is sq_frames_to_tiles /
    sq_frames_to_tiles_bg byte for byte.
(b) sq_tile_sample_affine_mc: channel c equals sq_tile_sample_affine on channel c's stack, labels and weights equal the old
    entry's, both forms of SQ_ROTATE_LDS agree, CI = 1 is the old entry, a captured graph replays the eager bits.
(c) segment_frames and the three jobs on two channels, and the single-channel jobs unchanged.
Everything is compared bit for bit: the kernels evaluate the single-channel kernels' expressions."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import frontend_ref
from sequitr_amd import _lib, frontend, jobs
from sequitr_amd.frontend import FrameClean, FrameTiler, TileSampler, segment_frames, tile_sample_plan
from sequitr_amd.networks.unet import UNet2D, init_unet_weights
from tests import multichannel_cases as mc
from tests import tile_sampler_cases as tsc
from tests.util import assert_bit_exact

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BG = FrameClean(bgsubtract=True)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def cut(src, modes, tl, mean32=None, std32=None, coef=None, mean64=None, std64=None, out=None):
    """sq_frames_to_tiles_mc itself on (C, F, H, W) planes `src` (any view FrameTiler takes)"""
    C, F = int(src.shape[0]), int(src.shape[1])
    if out is None:
        out = torch.empty((F * tl.TR * tl.TC, tl.T, tl.T, C), dtype=torch.float32, device=DEV)
    m = np.asarray(modes, np.int32)
    _lib.check(_lib.load().sq_frames_to_tiles_mc(src.data_ptr(), frontend.PIX[src.dtype], src.stride(0), m.ctypes.data,
                                                 ptr(mean32), ptr(std32), ptr(coef), ptr(mean64), ptr(std64),
                                                 tl._oy.data_ptr(), tl._ox.data_ptr(), out.data_ptr(), F, tl.H, tl.W, C,
                                                 tl.TR, tl.TC, tl.T, stream()), 'sq_frames_to_tiles_mc')
    return out


def single(shape):
    """the single-channel tiler the multi-channel results are held to"""
    return FrameTiler(shape, mc.TILE, mc.MARGIN, device=DEV)


# ---- (a) the tile cutter ------------------------------------------------------------------------------------------------

API_MODES = [("cast", False, None, mc.CAST), ("norm", True, None, mc.NORM), ("bg", False, BG, mc.BG),
             ("bg_norm", True, BG, mc.BG_NORM)]


@pytest.mark.parametrize("dtype", mc.DTYPES)
@pytest.mark.parametrize("C", [1, 2, 3, 4, 8])
def test_tiles_channel_c_is_the_single_channel_tiler(C, dtype):
    """C = 1: FrameTiler(channels=1) takes the (F, H, W) stack and returns (F,) statistics and (F, 6) coefficients; it is
    held to the numpy restatement like the others"""
    for shape, F in zip(mc.FRAME_SHAPES, (3, 1)):
        fr = mc.planes(C, F, shape, dtype, seed=10 + C)
        one = single(shape)
        many = FrameTiler(shape, mc.TILE, mc.MARGIN, device=DEV, channels=C)
        x = dev(fr) if C > 1 else dev(fr[0])
        N = F * one.TR * one.TC
        for name, normalise, clean, mode in API_MODES:
            got = many.tiles(x, normalise=normalise, clean=clean)
            assert got.shape == (N, mc.TILE, mc.TILE, C) and got.dtype == torch.float32 and got.is_contiguous()
            again = many.tiles(x, normalise=normalise, clean=clean)
            assert torch.equal(got.view(torch.int32), again.view(torch.int32)), "%s: two runs differ" % name
            g = got.cpu().numpy()
            for c in range(C):
                want = one.tiles(x[c] if C > 1 else x, normalise=normalise, clean=clean).cpu().numpy()
                assert_bit_exact(g[..., c], want[..., 0], "%s %s C=%d channel %d" % (name, shape, C, c))
            # the numpy restatement, from numpy's own float32 statistics or from the device's fit
            if mode in (mc.CAST, mc.NORM):
                st = np.array([[mc.np_frame_stats(fr[c, f]) for f in range(F)] for c in range(C)])
                ref = mc.np_tiles_mc(fr, [mode] * C, one.oy, one.ox, mc.TILE, mean32=st[..., 0], std32=st[..., 1])
            elif shape != mc.FRAME_SHAPES[0] or C > 3:
                # the restated surface rounds every fused multiply-add in exact rational arithmetic, ~10 us a pixel: it runs
                # on the odd frame at C = 2 and 3 here and at C = 4 in the mixed test; the bit-equality with the
                # single-channel tiler above runs for every case
                continue
            else:
                f32 = many.to_f32(x)
                coef = many.background(f32)
                m64, s64 = many.background_stats(f32, coef)
                assert coef.shape == ((C, F, 6) if C > 1 else (F, 6)) and m64.shape == ((C, F) if C > 1 else (F,))
                ref = mc.np_tiles_mc(fr, [mode] * C, one.oy, one.ox, mc.TILE, coef=coef.cpu().numpy().reshape(C, F, 6),
                                     mean64=m64.cpu().numpy().reshape(C, F), std64=s64.cpu().numpy().reshape(C, F))
            assert_bit_exact(g, ref, "%s %s C=%d against numpy" % (name, shape, C))


@pytest.mark.parametrize("dtype", mc.DTYPES)
def test_mixed_modes_and_per_channel_statistics(dtype):
    """[NORM, BG_NORM, BG, CAST] in one launch, the statistics (C, F) taken by the per-frame kernels on each channel's slice"""
    shape, C, F = mc.FRAME_SHAPES[0], 4, 3
    fr = mc.planes(C, F, shape, dtype, seed=21)
    x = dev(fr)
    one = single(shape)
    many = FrameTiler(shape, mc.TILE, mc.MARGIN, device=DEV, channels=C)
    f32 = many.to_f32(x)
    assert f32.shape == (C, F) + shape and f32.dtype == torch.float32
    mean32, std32 = many.stats(f32)
    coef = many.background(f32)
    mean64, std64 = many.background_stats(f32, coef)
    for c in range(C):                                          # (C, F) statistics: row c is the single-channel call's
        m1, s1 = one.stats(x[c])
        assert torch.equal(mean32[c], m1) and torch.equal(std32[c], s1)
        k1 = one.background(f32[c])
        assert torch.equal(coef[c], k1)
        m2, s2 = one.background_stats(f32[c], k1)
        assert torch.equal(mean64[c], m2) and torch.equal(std64[c], s2)
    got = cut(f32, mc.MIXED, many, mean32, std32, coef, mean64, std64).cpu().numpy()
    want = [one.tiles(x[0], normalise=True), one.tiles(x[1], normalise=True, clean=BG),
            one.tiles(x[2], normalise=False, clean=BG), one.tiles(x[3], normalise=False)]
    for c in range(C):
        assert_bit_exact(got[..., c], want[c].cpu().numpy()[..., 0], "mixed: channel %d" % c)
    ref = mc.np_tiles_mc(fr, mc.MIXED, one.oy, one.ox, mc.TILE, mean32.cpu().numpy(), std32.cpu().numpy(), coef.cpu().numpy(),
                         mean64.cpu().numpy(), std64.cpu().numpy())
    assert_bit_exact(got, ref, "mixed against numpy")
    # NULL statistics that no channel's mode reads
    lone = cut(f32, [mc.CAST, mc.NORM, mc.NORM, mc.CAST], many, mean32, std32).cpu().numpy()
    assert_bit_exact(lone[..., 1], one.tiles(x[1]).cpu().numpy()[..., 0], "NORM without the fp64 arrays")
    assert_bit_exact(lone[..., 3], got[..., 3], "CAST")


def test_a_clean_per_channel():
    """tiles(clean=[...]): one FrameClean per channel, None for a channel that is not cleaned"""
    shape, C, F = mc.FRAME_SHAPES[0], 4, 3
    fr = mc.planes(C, F, shape, np.uint16, seed=22)
    fr[2, 1, 9, 11] = fr[3, 0, 20, 30] = 65000                  # hot pixels
    x = dev(fr)
    one = single(shape)
    many = FrameTiler(shape, mc.TILE, mc.MARGIN, device=DEV, channels=C)
    cleans = [None, BG, FrameClean(outliers=(3, 900.)), FrameClean(outliers=(3, 900.), bgsubtract=True)]
    for normalise in (True, False):
        got = many.tiles(x, normalise=normalise, clean=cleans).cpu().numpy()
        for c in range(C):
            want = one.tiles(x[c], normalise=normalise, clean=cleans[c]).cpu().numpy()
            assert_bit_exact(got[..., c], want[..., 0], "normalise=%r channel %d under %r" % (normalise, c, cleans[c]))
    with pytest.raises(ValueError, match='3 entries for 4 channels'):
        many.tiles(x, clean=cleans[:3])
    with pytest.raises(ValueError):
        many.tiles(x[0])                                        # (F, H, W) into a four-channel tiler
    with pytest.raises(ValueError):
        many.tiles(x[:, :, :, :50])


@pytest.mark.parametrize("clean", [None, FrameClean(outliers=(3, 900.), bgsubtract=True)])
def test_a_view_of_a_staging_buffer_equals_its_packed_copy(clean):
    shape, C, B, n = mc.FRAME_SHAPES[0], 3, 3, 2
    buf = dev(mc.planes(C, B, shape, np.uint16, seed=23))
    view = buf[:, :n]
    assert not view.is_contiguous() and view.stride(0) == B * shape[0] * shape[1]
    packed = view.contiguous()
    many = FrameTiler(shape, mc.TILE, mc.MARGIN, device=DEV, channels=C)
    want = many.tiles(packed, clean=clean)
    got = many.tiles(view, clean=clean)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    scratch = many.clean_scratch(B, clean)                      # made for B frames, used for n: the (C, n) statistics are packed
    via = many.tiles(view, clean=clean, scratch=scratch)
    assert torch.equal(via.view(torch.int32), want.view(torch.int32))
    full = many.tiles(buf, clean=clean, scratch=scratch)        # and for all B, from the same scratch
    per = many.tiles_per_frame
    assert torch.equal(full[:n * per].view(torch.int32), want.view(torch.int32))
    m, s = many.stats(view)
    mp, sp = many.stats(packed)
    assert m.shape == (C, n) and torch.equal(m, mp) and torch.equal(s, sp)


@pytest.mark.parametrize("C", [1, 3, 8])
def test_nothing_is_written_past_the_output(C):
    shape, F = mc.FRAME_SHAPES[0], 3
    x = dev(mc.planes(C, F, shape, np.uint8, seed=24))
    one = single(shape)
    n = F * one.TR * one.TC * mc.TILE * mc.TILE * C
    assert n % 4 != 0 or C == 8                                 # odd tiles: the output ends off a 16-byte boundary
    guard = 4096
    raw = torch.full((n + guard,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    out = raw[:n].view(torch.float32).view(F * one.TR * one.TC, mc.TILE, mc.TILE, C)
    cut(x, [mc.CAST] * C, one, out=out)
    torch.cuda.synchronize()
    assert bool((raw[n:] == 0x5A5A5A5A).all()), "the guard behind the tiles was written"
    assert bool((raw[:n] != 0x5A5A5A5A).all()), "a tile element was left unwritten"
    ref = mc.np_tiles_mc(x.cpu().numpy(), [mc.CAST] * C, one.oy, one.ox, mc.TILE)
    assert_bit_exact(out.cpu().numpy(), ref, "cast tiles in front of the guard")


def single_entry(x, tl, mean=None, std=None, coef=None):
    """sq_frames_to_tiles on one (F, H, W) stack, or sq_frames_to_tiles_bg when `coef` is given"""
    F = int(x.shape[0])
    out = torch.empty((F * tl.TR * tl.TC, tl.T, tl.T, 1), dtype=torch.float32, device=DEV)
    tail = (tl._oy.data_ptr(), tl._ox.data_ptr(), out.data_ptr(), F, tl.H, tl.W, tl.TR, tl.TC, tl.T, stream())
    lib = _lib.load()
    if coef is None:
        _lib.check(lib.sq_frames_to_tiles(x.data_ptr(), frontend.PIX[x.dtype], ptr(mean), ptr(std), *tail), 'sq_frames_to_tiles')
    else:
        _lib.check(lib.sq_frames_to_tiles_bg(x.data_ptr(), coef.data_ptr(), ptr(mean), ptr(std), *tail), 'sq_frames_to_tiles_bg')
    return out


@pytest.mark.parametrize("dtype", mc.DTYPES)
def test_one_channel_is_the_single_channel_entries_byte_for_byte(dtype):
    """C = 1 of sq_frames_to_tiles_mc, FrameTiler(channels=1) and the direct single-channel entries are one kernel; the
    direct entries equal the numpy restatement bit for bit in all four modes, the background ones included (statistics and
    coefficients are the device's own)"""
    for shape, F in zip(mc.FRAME_SHAPES, (3, 1)):
        fr = mc.planes(1, F, shape, dtype, seed=25)
        x = dev(fr)
        one = single(shape)
        mean, std = one.stats(x[0])
        for name, got, want in (("cast", cut(x, [mc.CAST], one), one.tiles(x[0], normalise=False)),
                                ("norm", cut(x, [mc.NORM], one, mean.view(1, F), std.view(1, F)), one.tiles(x[0]))):
            assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32)), (name, shape)
        f32 = one.to_f32(x[0])
        coef = one.background(f32)
        m64, s64 = one.background_stats(f32, coef)
        planes32 = f32.view((1,) + tuple(f32.shape))
        got = cut(planes32, [mc.BG], one, coef=coef)
        assert torch.equal(got.view(torch.int32), one.tiles(x[0], normalise=False, clean=BG).view(torch.int32)), ("bg", shape)
        got = cut(planes32, [mc.BG_NORM], one, coef=coef, mean64=m64, std64=s64)
        assert torch.equal(got.view(torch.int32), one.tiles(x[0], clean=BG).view(torch.int32)), ("bg_norm", shape)
        # the direct entries against numpy
        stats = dict(mean32=mean.cpu().numpy()[None], std32=std.cpu().numpy()[None], coef=coef.cpu().numpy()[None],
                     mean64=m64.cpu().numpy()[None], std64=s64.cpu().numpy()[None])
        for name, mode, got in (("cast", mc.CAST, single_entry(x[0], one)),
                                ("norm", mc.NORM, single_entry(x[0], one, mean, std)),
                                ("bg", mc.BG, single_entry(f32, one, coef=coef)),
                                ("bg_norm", mc.BG_NORM, single_entry(f32, one, m64, s64, coef=coef))):
            ref = mc.np_tiles_mc(fr, [mode], one.oy, one.ox, mc.TILE, **stats)
            assert_bit_exact(got.cpu().numpy(), ref, "%s %s: the single-channel entry against numpy" % (name, shape))


# ---- (b) the sampler ------------------------------------------------------------------------------------------------------

def sample_mc(x, stats, labels, weights, plan, coef, C, tile=mc.SAMPLER_TILE, out=None):
    """sq_tile_sample_affine_mc itself on (CI, F, H, W) planes"""
    CI, F, H, W = (int(v) for v in x.shape)
    count = int(plan.shape[0])
    if out is None:
        out = (torch.empty((count,) + tile + (CI,), dtype=torch.float32, device=DEV),
               torch.empty((count,) + tile + (C,), dtype=torch.uint8, device=DEV),
               torch.empty((count,) + tile + (1,), dtype=torch.float32, device=DEV))
    _lib.check(_lib.load().sq_tile_sample_affine_mc(x.data_ptr(), frontend.PIX[x.dtype], x.stride(0), ptr(stats[0]),
                                                    ptr(stats[1]), ptr(labels), ptr(weights), plan.data_ptr(),
                                                    coef.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                                                    out[2].data_ptr(), F, H, W, CI, tile[0], tile[1], C, count, stream()),
               'sq_tile_sample_affine_mc')
    return out


def both_forms(monkeypatch, fn):
    monkeypatch.setenv('SQ_ROTATE_LDS', '1')
    a = fn()
    monkeypatch.setenv('SQ_ROTATE_LDS', '0')
    b = fn()
    monkeypatch.delenv('SQ_ROTATE_LDS', raising=False)
    return a, b


def host(t):
    return tuple(None if v is None else v.cpu().numpy() for v in t)


_sampler_sources = {}


def sampler_sources(dtype):
    """the eight-channel stack, labels and weights, once per pixel type; fewer channels are its first planes"""
    key = np.dtype(dtype).name
    if key not in _sampler_sources:
        H, W = mc.SAMPLER_FRAME
        _sampler_sources[key] = (mc.planes(8, 3, (H, W), dtype, seed=30), tsc.random_labels((3, H, W), 4),
                                 tsc.random_weights((3, H, W), 5))
    return _sampler_sources[key]


@pytest.mark.parametrize("CI", mc.CHANNELS)
def test_sampler_channel_c_is_the_single_channel_sampler(CI, monkeypatch):
    C = 3
    for dtype in ((np.uint16,) if CI != 3 else mc.DTYPES):
        fr8, labels, weights = sampler_sources(dtype)
        fr = fr8[:CI]
        x, lab, wts = dev(fr), dev(labels), dev(weights)
        old = TileSampler(mc.SAMPLER_FRAME, mc.SAMPLER_TILE, DEV)
        for rows, tile in ((mc.sampler_rows(), mc.SAMPLER_TILE), (mc.hostile_rows(), mc.SAMPLER_TILE),
                           (mc.sampler_rows(7), (48, 64))):                   # the last: tiles larger than the frame
            plan, coef = (dev(a) for a in rows)
            old = TileSampler(mc.SAMPLER_FRAME, tile, DEV)
            for normalise in (True, False):
                stats = (None, None)
                if normalise:
                    per = [old.stats(x[c]) for c in range(CI)]
                    stats = (torch.stack([p[0] for p in per]), torch.stack([p[1] for p in per]))
                lds, direct = both_forms(monkeypatch, lambda: host(sample_mc(x, stats, lab, wts, plan, coef, C, tile)))
                for a, b in zip(lds, direct):
                    assert_bit_exact(a, b, "SQ_ROTATE_LDS=1 against 0, CI=%d" % CI)
                for c in range(CI):
                    want = host(old.sample(x[c], lab, wts, plan, coef, C, normalise=normalise))
                    assert_bit_exact(direct[0][..., c], want[0][..., 0], "CI=%d %s channel %d, tile %r" % (CI, dtype, c, tile))
                assert np.array_equal(direct[1], want[1])
                assert_bit_exact(direct[2], want[2], "weights")
                if CI > 1:                                      # the class on top of the entry
                    sm = TileSampler(mc.SAMPLER_FRAME, tile, DEV, channels=CI)
                    if normalise:
                        m, s = sm.stats(x)
                        assert m.shape == (CI, 3) and torch.equal(m, stats[0]) and torch.equal(s, stats[1])
                    api = host(sm.sample(x, lab, wts, plan, coef, C, normalise=normalise))
                    for a, b in zip(api, direct):
                        assert_bit_exact(a, b, "TileSampler(channels=%d)" % CI)
        # the numpy restatement
        plan, coef = mc.sampler_rows()
        normed = np.stack([tsc.np_normalised(fr[c]) for c in range(CI)])
        per = [TileSampler(mc.SAMPLER_FRAME, mc.SAMPLER_TILE, DEV).stats(x[c]) for c in range(CI)]
        stats = (torch.stack([p[0] for p in per]), torch.stack([p[1] for p in per]))
        got = host(sample_mc(x, stats, lab, wts, dev(plan), dev(coef), C))
        ref = mc.np_sample_mc(normed, labels, weights, plan, coef, mc.SAMPLER_TILE, C)
        for g, r, name in zip(got, ref, ('image', 'onehot', 'weights')):
            assert_bit_exact(g, r.astype(g.dtype), "%s against numpy, CI=%d" % (name, CI))


def test_sampler_image_alone_and_a_strided_stack():
    """frames without labels and weights, out of a [:, :n] view of a larger stack"""
    fr8, _, _ = sampler_sources(np.uint16)
    buf = dev(fr8[:3])                                          # (3, 3, H, W)
    view = buf[:, :2]
    plan, coef = mc.sampler_rows()
    plan[:, 0] = np.clip(plan[:, 0], -1, 2)
    plan, coef = dev(plan), dev(coef)
    sm = TileSampler(mc.SAMPLER_FRAME, mc.SAMPLER_TILE, DEV, channels=3)
    a = sm.sample(view, None, None, plan, coef, 2)
    b = sm.sample(view.contiguous(), None, None, plan, coef, 2)
    assert a[1] is None and a[2] is None and a[0].shape == (5,) + mc.SAMPLER_TILE + (3,)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    with pytest.raises(ValueError):
        sm.sample(buf[0], None, None, plan, coef, 2)            # (F, H, W) into a three-channel sampler


@pytest.mark.parametrize("CI", [2, 3])
def test_sampler_graph_replay_equals_eager(CI):
    fr8, labels, weights = sampler_sources(np.uint16)
    x, lab, wts = dev(fr8[:CI]), dev(labels), dev(weights)
    plan, coef = (dev(a) for a in mc.sampler_rows())
    sm = TileSampler(mc.SAMPLER_FRAME, mc.SAMPLER_TILE, DEV, channels=CI)
    stats = sm.stats(x)
    eager = host(sm.sample(x, lab, wts, plan, coef, 3, stats=stats))
    bufs = [torch.zeros_like(dev(e)) for e in eager]
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sm.sample(x, lab, wts, plan, coef, 3, stats=stats, out=bufs)          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sm.sample(x, lab, wts, plan, coef, 3, stats=stats, out=bufs)
    for b in bufs:
        b.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for b, e in zip(bufs, eager):
        assert_bit_exact(b.cpu().numpy(), e, "replay against eager")


# ---- (c) end to end -------------------------------------------------------------------------------------------------------

NET = {"shape": (32, 32), "filters": (16, 32), "num_inputs": 2, "num_outputs": 2, "device": DEV}
E2E_SHAPE, E2E_MARGIN = (37, 53), 2


def e2e_planes(F=3):
    fr = mc.planes(2, F, E2E_SHAPE, np.uint16, seed=40)
    yy, xx = np.mgrid[0:E2E_SHAPE[0], 0:E2E_SHAPE[1]]
    for f in range(F):                                          # a bright cell in bright field, a dimmer one in fluorescence
        fr[0, f][(yy - 12 - f) ** 2 + (xx - 20) ** 2 < 40] += 9000
        fr[1, f][(yy - 25) ** 2 + (xx - 35 - f) ** 2 < 30] += 4000
    return fr


def seeded_net():
    net = UNet2D(NET, "infer")
    w = init_unet_weights(NET, 4)
    net.load_state_dict(w)
    return net


def test_segment_frames_on_two_channels():
    fr = e2e_planes()
    net = seeded_net()
    as_list = segment_frames(net, [fr[0], fr[1]], tile=32, margin=E2E_MARGIN, frames_per_batch=3)
    interleaved = np.ascontiguousarray(np.moveaxis(fr, 0, -1))  # (F, H, W, 2)
    as_array = segment_frames(net, interleaved, tile=32, margin=E2E_MARGIN, frames_per_batch=3)
    assert as_list.shape == (3,) + E2E_SHAPE and as_list.dtype == np.uint8
    assert np.array_equal(as_list, as_array)
    assert 0 < as_list.mean() < 1, "the seeded net's masks must not be trivial"
    # the same through numpy: the host pipe per channel, sliced at the tiler's origins, stacked, predicted, stitched
    tl = FrameTiler(E2E_SHAPE, 32, E2E_MARGIN, device=DEV)
    st = np.array([[mc.np_frame_stats(fr[c, f]) for f in range(3)] for c in range(2)])
    tiles = mc.np_tiles_mc(fr, [mc.NORM] * 2, tl.oy, tl.ox, 32, mean32=st[..., 0], std32=st[..., 1])
    tile_masks = net.predict(dev(tiles)).cpu().numpy()
    ref = frontend_ref.stitch(tile_masks, tl.oy, tl.ox, tl.ymap, tl.xmap, *E2E_SHAPE)
    assert np.array_equal(as_list, ref)
    # a partial last batch: the [:, :1] view of the staging buffer
    assert np.array_equal(segment_frames(net, [fr[0], fr[1]], tile=32, margin=E2E_MARGIN, frames_per_batch=2), ref)
    seen = []
    assert segment_frames(net, interleaved, tile=32, margin=E2E_MARGIN, frames_per_batch=2,
                          on_batch=lambda first, raw, m: seen.append((first, raw.cpu().numpy(), m.cpu().numpy()))) is None
    assert [s[0] for s in seen] == [0, 2] and [s[1].shape for s in seen] == [(2, 2) + E2E_SHAPE, (2, 1) + E2E_SHAPE]
    assert np.array_equal(np.concatenate([s[1] for s in seen], 1), fr) and np.array_equal(np.concatenate([s[2] for s in seen]), ref)
    # per-channel cleaning goes through; one FrameClean for both equals the list of two
    a = segment_frames(net, [fr[0], fr[1]], tile=32, margin=E2E_MARGIN, frames_per_batch=2, clean=BG)
    b = segment_frames(net, interleaved, tile=32, margin=E2E_MARGIN, frames_per_batch=3, clean=[BG, BG])
    assert np.array_equal(a, b)
    with pytest.raises(ValueError, match='takes 2 input channels, the frames have 3'):
        segment_frames(net, [fr[0], fr[1], fr[0]], tile=32, margin=E2E_MARGIN)


def job_dir(tmp_path, name):
    out = str(tmp_path / name)
    os.makedirs(out)
    return out


def test_frame_jobs_on_two_channels(tmp_path):
    from sequitr_amd.objects import measure_objects
    fr = e2e_planes()
    np.save(str(tmp_path / "bf.npy"), fr[0])
    np.save(str(tmp_path / "gfp.npy"), fr[1])
    base = {"input": [str(tmp_path / "bf.npy"), str(tmp_path / "gfp.npy")], "shape": (32, 32), "filters": (16, 32),
            "num_outputs": 2, "seed": 2, "margin": E2E_MARGIN, "frames_per_batch": 2}
    out = job_dir(tmp_path, "seg")
    info = jobs.SERVER_segment_frames(dict(base, output=out, measure_channel=1), {"gpu": 0, "measure": True})
    masks = np.load(os.path.join(out, "mask.npy"))
    assert masks.shape == (3,) + E2E_SHAPE and 0 < masks.mean() < 1
    rec = json.load(open(os.path.join(out, "segment.json")))
    assert rec["channels"] == 2 and rec["measure_channel"] == 1 and "pipeline" not in rec and info["channels"] == 2
    want = measure_objects(dev(masks), image=dev(fr[1])).columns()
    z = np.load(os.path.join(out, "objects.npz"))
    assert sorted(z.files) == sorted(want) and len(want['area']) > 0
    for name in want:
        assert np.array_equal(z[name], want[name]), name
    other = measure_objects(dev(masks), image=dev(fr[0])).columns()
    assert not np.array_equal(z['intensity_sum'], other['intensity_sum']), "channel 0 was measured"
    # the interleaved array and an explicit pipeline list give the same masks; the record is per channel
    out2 = job_dir(tmp_path, "seg2")
    from sequitr_amd import pipeline as pl
    norm = pl.ImagePipeline([pl.ImageNorm()])
    jobs.SERVER_segment_frames(dict(base, input=np.ascontiguousarray(np.moveaxis(fr, 0, -1)), output=out2, num_inputs=2,
                                    pipeline=[norm, None]), {"gpu": 0})
    assert np.array_equal(np.load(os.path.join(out2, "mask.npy")), masks)
    rec2 = json.load(open(os.path.join(out2, "segment.json")))
    assert rec2["channels"] == 2 and rec2["pipeline"] == [[{"ImageNorm": {}}], [{"ImageNorm": {}}]]
    # SERVER_evaluate counts the same masks
    labels = (np.random.default_rng(3).random((3,) + E2E_SHAPE) < 0.3).astype(np.uint8)
    labels[0, :4] = 255                                         # unlabelled
    ev = job_dir(tmp_path, "ev")
    einfo = jobs.SERVER_evaluate(dict(base, output=ev, labels=labels), {"gpu": 0, "masks": True})
    assert np.array_equal(np.load(os.path.join(ev, "mask.npy")), masks) and einfo["channels"] == 2
    got = np.load(os.path.join(ev, "confusion.npy"))
    want_c = np.zeros((3, 2, 2), np.int64)
    for f in range(3):
        ok = labels[f] < 2
        np.add.at(want_c[f], (labels[f][ok], masks[f][ok]), 1)
    assert got.dtype == np.int64 and np.array_equal(got, want_c) and einfo["ignored"] == int((labels >= 2).sum())


def test_single_channel_jobs_write_what_they_wrote(tmp_path):
    """one (F, H, W) source: mask.npy, confusion.npy and the records are those of the single-channel functions called
    directly -- no 'channels' key, the same key order"""
    fr = e2e_planes()[0]
    np.save(str(tmp_path / "bf.npy"), fr)
    base = {"input": str(tmp_path / "bf.npy"), "shape": (32, 32), "filters": (16, 32), "num_outputs": 2, "seed": 2,
            "margin": E2E_MARGIN, "frames_per_batch": 2}
    out = job_dir(tmp_path, "seg")
    jobs.SERVER_segment_frames(dict(base, output=out), {"gpu": 0})
    net = UNet2D({"shape": (32, 32), "filters": (16, 32), "num_outputs": 2, "seed": 2, "device": DEV}, "infer")
    net.initialize()
    direct = segment_frames(net, fr, tile=32, margin=E2E_MARGIN, frames_per_batch=2)
    np.save(str(tmp_path / "direct.npy"), direct)
    assert open(os.path.join(out, "mask.npy"), "rb").read() == open(str(tmp_path / "direct.npy"), "rb").read()
    rec = json.load(open(os.path.join(out, "segment.json")))
    assert list(rec) == ["frames", "shape", "tile", "seconds", "mpixels_per_s", "device"]
    assert sorted(os.listdir(out)) == ["mask.npy", "segment.json"]
    from sequitr_amd import pipeline as pl
    out_p = job_dir(tmp_path, "seg_p")
    chain = pl.ImagePipeline([pl.ImageBGSubtract(), pl.ImageNorm()])
    jobs.SERVER_segment_frames(dict(base, output=out_p, pipeline=chain), {"gpu": 0})
    rec = json.load(open(os.path.join(out_p, "segment.json")))
    assert list(rec) == ["frames", "shape", "tile", "seconds", "mpixels_per_s", "device", "pipeline"]
    assert rec["pipeline"] == [{"ImageBGSubtract": {}}, {"ImageNorm": {}}]
    assert np.array_equal(np.load(os.path.join(out_p, "mask.npy")),
                          segment_frames(net, fr, tile=32, margin=E2E_MARGIN, frames_per_batch=2, clean=BG))
    labels = (np.random.default_rng(3).random(fr.shape) < 0.3).astype(np.uint8)
    ev = job_dir(tmp_path, "ev")
    einfo = jobs.SERVER_evaluate(dict(base, output=ev, labels=labels), {"gpu": 0})
    want_c = np.zeros((3, 2, 2), np.int64)
    for f in range(3):
        np.add.at(want_c[f], (labels[f], direct[f]), 1)
    assert np.array_equal(np.load(os.path.join(ev, "confusion.npy")), want_c)
    assert "channels" not in einfo and "pipeline" not in einfo and sorted(os.listdir(ev)) == ["confusion.npy", "evaluate.json"]
    assert list(einfo)[:7] == ["frames", "shape", "tile", "num_classes", "seconds", "mpixels_per_s", "device"]


TRAIN_TILE, TRAIN_STACK = (32, 32), (3, 80, 96)


def train_stack(tmp_path):
    rng = np.random.default_rng(0)
    F, H, W = TRAIN_STACK
    yy, xx = np.mgrid[0:H, 0:W]
    lab = np.zeros(TRAIN_STACK, np.uint8)
    lab[0][(yy - 30) ** 2 + (xx - 34) ** 2 < 180] = 1
    lab[1][(yy - 40) ** 2 + (xx - 50) ** 2 < 250] = 1
    lab[2][(yy - 20) ** 2 + (xx - 75) ** 2 < 120] = 1
    bf = (400 + lab * 900.0 + rng.standard_normal(TRAIN_STACK) * 150).clip(0, 65535).astype(np.uint16)
    gfp = (90 + lab * 300.0 + rng.standard_normal(TRAIN_STACK) * 40 + 0.5 * xx).clip(0, 65535).astype(np.uint16)
    np.save(str(tmp_path / "bf.npy"), bf)
    np.save(str(tmp_path / "gfp.npy"), gfp)
    np.save(str(tmp_path / "im2.npy"), np.stack([bf, gfp], -1))
    np.save(str(tmp_path / "lab.npy"), lab)
    return np.stack([bf, gfp]), lab


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_train_job_on_a_two_channel_stack(dtype, tmp_path, monkeypatch):
    """The job's first loss against a fresh UNetTrainer on the first batch restated in numpy (both channels normalised per
    whole frame and sampled at the same coordinates), bit for bit, as tests/test_gpu_tile_sampler.py holds the
    single-channel job; then the saved model segments the same two sources."""
    from sequitr_amd import core, utils
    from sequitr_amd.train import UNetTrainer
    from sequitr_amd.weightmap import device_weightmaps
    planes, lab = train_stack(tmp_path)
    monkeypatch.setattr(core.TensorflowConfiguration, "MODELDIR", job_dir(tmp_path, "models"))
    sources = [str(tmp_path / "bf.npy"), str(tmp_path / "gfp.npy")]
    images = sources if dtype == "bf16" else str(tmp_path / "im2.npy")       # both forms of the input
    params = {"images": images, "labels": str(tmp_path / "lab.npy"), "tile": TRAIN_TILE, "batch_size": 4, "dropout": 0.0,
              "num_inputs": 2, "num_outputs": 2, "seed": 5, "num_epochs": 2, "dtype": dtype,
              "output": job_dir(tmp_path, "out")}
    info = jobs.SERVER_train(params, {"gpu": 0, "max_steps": 3})
    tj = json.load(open(str(tmp_path / "out" / "train.json")))
    assert info["steps"] == 3 and np.isfinite(tj["losses"]).all() and tj["channels"] == 2 and tj["dtype"] == dtype
    cfg = json.load(open(os.path.join(info["model_dir"], "net.config")))["NetConfiguration"]
    assert tuple(cfg["shape"]) == TRAIN_TILE and cfg["num_inputs"] == 2

    per = frontend.covering_tiles(TRAIN_STACK[1:], TRAIN_TILE)
    plan, coef = tile_sample_plan(TRAIN_STACK[1:], TRAIN_TILE, TRAIN_STACK[0], 3 * per, np.random.default_rng(5), ("rotate",))
    wmap = device_weightmaps(lab, 10., 5., device=DEV).cpu().numpy()
    normed = np.stack([tsc.np_normalised(planes[c]) for c in range(2)])
    batches = [[dev(a) for a in mc.np_sample_mc(normed, lab, wmap[..., 0], plan[i:i + 4], coef[i:i + 4], TRAIN_TILE, 2)]
               for i in (0, 4, 8)]
    batch = batches[0]
    assert batch[0].shape == (4,) + TRAIN_TILE + (2,)
    net_p = {"shape": TRAIN_TILE, "num_inputs": 2, "num_outputs": 2, "dropout": 0.0, "seed": 5, "dtype": dtype, "device": DEV}
    fresh = [float(UNetTrainer(net_p).step(*batch).cpu()) for _ in range(2)]
    print("first loss (%s): job %r, fresh trainers %r" % (dtype, tj["losses"][0], fresh))
    assert np.float32(fresh[0]).tobytes() == np.float32(fresh[1]).tobytes(), fresh
    assert np.float32(tj["losses"][0]).tobytes() == np.float32(fresh[0]).tobytes(), (tj["losses"][0], fresh)
    # the first loss of a fresh network barely sees the image; the next two do, through the updated weights.  The job's
    # captured step replays the eager step's bits (tests/test_gpu_tile_sampler.py holds it to that), so three eager steps of a
    # fresh trainer on the three restated batches give the job's three losses.
    trainer = UNetTrainer(net_p)
    eager = [float(trainer.step(*b).cpu()) for b in batches]
    swapped = UNetTrainer(net_p)
    other = [float(swapped.step(b[0].flip(-1).contiguous(), b[1], b[2]).cpu()) for b in batches]
    print("losses (%s): job %r, eager %r, channels swapped %r" % (dtype, tj["losses"], eager, other))
    assert other[1:] != eager[1:], "the later losses must depend on which channel is which"
    assert [np.float32(v).tobytes() for v in tj["losses"]] == [np.float32(v).tobytes() for v in eager], (tj["losses"], eager)

    seg = {"input": sources, "model": info["model_dir"], "shape": TRAIN_TILE, "margin": 4, "num_outputs": 2,
           "output": job_dir(tmp_path, "seg")}
    sinfo = jobs.SERVER_segment_frames(seg, {"gpu": 0})
    assert sinfo["frames"] == 3 and sinfo["channels"] == 2
    mask = np.load(str(tmp_path / "seg" / "mask.npy"))
    net = UNet2D({"shape": TRAIN_TILE, "num_inputs": 2, "num_outputs": 2, "device": DEV}, "infer")
    net.load_state_dict(utils.load_model_weights(info["model_dir"]), strict=True)
    assert np.array_equal(mask, segment_frames(net, [planes[0], planes[1]], tile=32, margin=4))


def test_single_channel_train_job_is_what_it_was(tmp_path, monkeypatch):
    """SERVER_train with `tile` on one (F, H, W) stack, whose loader and order of construction this path shares with the
    multi-channel one: the losses are those of a fresh UNetTrainer on the batches of the single-channel restatement
    (tests/tile_sampler_cases.py), net.config says num_inputs 1, and train.json has no 'channels' key."""
    from sequitr_amd import core
    from sequitr_amd.train import UNetTrainer
    from sequitr_amd.weightmap import device_weightmaps
    planes, lab = train_stack(tmp_path)
    monkeypatch.setattr(core.TensorflowConfiguration, "MODELDIR", job_dir(tmp_path, "models"))
    params = {"images": str(tmp_path / "bf.npy"), "labels": str(tmp_path / "lab.npy"), "tile": TRAIN_TILE, "batch_size": 4,
              "dropout": 0.0, "num_outputs": 2, "seed": 5, "num_epochs": 2, "output": job_dir(tmp_path, "out")}
    info = jobs.SERVER_train(params, {"gpu": 0, "max_steps": 3})
    tj = json.load(open(str(tmp_path / "out" / "train.json")))
    assert "channels" not in tj and "channels" not in info and info["steps"] == 3
    assert list(tj)[:10] == ["steps", "first_loss", "last_loss", "seconds", "ms_per_step", "steady_steps", "batch_size",
                             "frames", "frame_shape", "tile"]
    cfg = json.load(open(os.path.join(info["model_dir"], "net.config")))["NetConfiguration"]
    assert tuple(cfg["shape"]) == TRAIN_TILE and cfg["num_inputs"] == 1
    per = frontend.covering_tiles(TRAIN_STACK[1:], TRAIN_TILE)
    plan, coef = tile_sample_plan(TRAIN_STACK[1:], TRAIN_TILE, TRAIN_STACK[0], 3 * per, np.random.default_rng(5), ("rotate",))
    wmap = device_weightmaps(lab, 10., 5., device=DEV).cpu().numpy()
    normed = tsc.np_normalised(planes[0])
    batches = [[dev(a) for a in tsc.np_sample(normed, lab, wmap[..., 0], plan[i:i + 4], coef[i:i + 4], TRAIN_TILE, 2)]
               for i in (0, 4, 8)]
    assert batches[0][0].shape == (4,) + TRAIN_TILE + (1,)
    net_p = {"shape": TRAIN_TILE, "num_inputs": 1, "num_outputs": 2, "dropout": 0.0, "seed": 5, "device": DEV}
    trainer = UNetTrainer(net_p)
    eager = [float(trainer.step(*b).cpu()) for b in batches]
    print("single-channel losses: job %r, eager %r" % (tj["losses"], eager))
    assert [np.float32(v).tobytes() for v in tj["losses"]] == [np.float32(v).tobytes() for v in eager], (tj["losses"], eager)


class _Sealed(np.ndarray):
    """an array whose pixels must not be touched"""

    def __getitem__(self, item):
        raise AssertionError('a pixel was read')


def test_bf16_trainer_refuses_eight_channels_before_any_upload(tmp_path, monkeypatch):
    """the bf16 graph takes 1 .. 7 input channels: the job raises the trainer's own message, and has neither read a pixel
    nor built a weight map by then"""
    from sequitr_amd import core, weightmap
    monkeypatch.setattr(core.TensorflowConfiguration, "MODELDIR", job_dir(tmp_path, "models"))
    stacks = {"lab.npy": np.zeros(TRAIN_STACK, np.uint8).view(_Sealed)}
    for c in range(8):
        stacks["c%d.npy" % c] = np.zeros(TRAIN_STACK, np.uint16).view(_Sealed)
    monkeypatch.setattr(jobs.np, "load", lambda path, **kw: stacks[os.path.basename(path)])
    monkeypatch.setattr(weightmap, "device_weightmaps", lambda *a, **kw: pytest.fail("a weight map was built"))
    params = {"images": ["c%d.npy" % c for c in range(8)], "labels": "lab.npy", "tile": TRAIN_TILE, "batch_size": 4,
              "num_inputs": 8, "num_outputs": 2, "seed": 5, "dtype": "bf16", "output": job_dir(tmp_path, "out")}
    with pytest.raises(ValueError, match="bf16 graph takes an f32 image of 1..7 channels"):
        jobs.SERVER_train(params, {"gpu": 0, "max_steps": 1})
    assert os.listdir(str(tmp_path / "out")) == []


def test_frame_stats_take_a_slice_at_any_pixel_aligned_address():
    """a channel's slice of odd-sized uint8 planes starts off every 16-byte boundary: sq_frame_stats gives it the
    statistics of its packed copy (numpy's, bit for bit)"""
    shape, C, F = mc.FRAME_SHAPES[0], 3, 3
    fr = mc.planes(C, F, shape, np.uint8, seed=26)
    x = dev(fr)
    one = single(shape)
    assert x[1].data_ptr() % 2 != 0                             # channel 1 starts at an odd address
    for c in range(C):
        m, s = one.stats(x[c])
        mp, sp = one.stats(x[c].clone())
        assert torch.equal(m, mp) and torch.equal(s, sp)
        want = np.array([mc.np_frame_stats(fr[c, f]) for f in range(F)], np.float32)
        assert_bit_exact(m.cpu().numpy(), want[:, 0], "mean of channel %d" % c)
        assert_bit_exact(s.cpu().numpy(), want[:, 1], "std of channel %d" % c)


def test_one_source_in_a_list_takes_a_list_of_one_clean():
    fr = e2e_planes()[0]
    net = UNet2D(dict(NET, num_inputs=1), "infer")
    net.load_state_dict(init_unet_weights(dict(NET, num_inputs=1), 4))
    want = segment_frames(net, fr, tile=32, margin=E2E_MARGIN, frames_per_batch=2, clean=BG)
    assert np.array_equal(segment_frames(net, [fr], tile=32, margin=E2E_MARGIN, frames_per_batch=2, clean=[BG]), want)
    assert np.array_equal(segment_frames(net, fr[..., None], tile=32, margin=E2E_MARGIN, frames_per_batch=2, clean=[BG]), want)
    many = FrameTiler(E2E_SHAPE, 32, E2E_MARGIN, device=DEV, channels=2)
    x = dev(e2e_planes())
    scratch = many.clean_scratch(3, None)
    m, s = many.stats(x, scratch=scratch)                       # the caller's scratch is used, not dropped
    assert m.data_ptr() == scratch['mean'].data_ptr() and torch.equal(m, many.stats(x)[0])
