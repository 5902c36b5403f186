"""GPU: ImageBlur in the frame-cleaning chain (include/sequitr_hip.h "Frame cleaning", sq_frame_blur_f32) -- the kernel bit
for bit against the numpy restatement of tests/frame_blur_cases.py (itself pinned to scipy and the host pipe on the CPU), the
chains through FrameTiler.tiles against the host ImagePipeline, multi-channel planes, segment_frames and the two frame jobs."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from oracle import frontend_ref
from sequitr_amd import _lib, jobs
from sequitr_amd import pipeline as pl
from sequitr_amd.frontend import BLUR_TILES, PIX, FrameClean, FrameTiler, segment_frames
from sequitr_amd.networks.unet import UNet2D
from tests import frame_blur_cases as fb
from tests import frame_clean_cases as fc
from tests import multichannel_cases as mc
from tests.util import assert_bit_exact

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = fb.GOLDEN
# the largest radius of every radius class of the kernel (8, 16, 32) and the first radius of the next class; 2 and 3 besides
CLASS_SIGMAS = {2: 0.5, 3: 0.7, 8: 2, 9: 2.2, 16: 4, 17: 4.2, 32: 8.124}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def stream():
    return torch.cuda.current_stream().cuda_stream


def tiler(H, W):
    return FrameTiler((H, W), tile=min(H, W, 32), margin=0, device=DEV)


def device_blur(frames, sigma):
    """FrameTiler.blur of (F, H, W) numpy frames, back on the host"""
    return tiler(*frames.shape[1:]).blur(dev(frames), sigma).cpu().numpy()


def check(frames, sigma, what):
    got = device_blur(frames, sigma)
    assert got.shape == frames.shape and got.dtype == np.float32
    for f in range(len(frames)):
        assert fb.equal_bits(got[f], fb.blur_restated(frames[f], sigma)), "%s: frame %d at sigma %g" % (what, f, sigma)
    return got


def test_the_classes_are_what_the_tests_assume():
    assert [c[0] for c in BLUR_TILES] == [8, 16, 32]
    assert {R: fb.radius(s) for R, s in CLASS_SIGMAS.items()} == {R: R for R in CLASS_SIGMAS}
    assert [fb.radius(s) for s in fb.SIGMAS_GPU] == [0, 1, 2, 3, 6, 8, 9, 13, 16, 17, 32]


# ---- the kernel against the restatement ------------------------------------------------------------------------------
SIZES = (1, 2, 3, 5, 63, 64, 65, 127, 128, 129, 130, 200)
SHAPES = [(h, w) for h in SIZES for w in SIZES]                # with 1 x 200, 200 x 1 and 3 x 5: smaller than R = 32 on one axis, on both
KINDS = ("u16", "f32", "u8")


@pytest.mark.parametrize("sigma", fb.SIGMAS_GPU)
def test_kernel_equals_the_restatement_on_small_and_odd_frames(sigma):
    """sizes around the wave, the tile and the block, frames smaller than the radius on one axis and on both"""
    for n, shape in enumerate(SHAPES):
        check(fb.plane((1,) + shape, KINDS[n % 3], 300 + n), sigma, "%s %s" % (shape, KINDS[n % 3]))


@pytest.mark.parametrize("R", sorted(CLASS_SIGMAS))
def test_kernel_equals_the_restatement_around_the_tile_seams(R):
    """the class's tile height and width - 1, exact, + 1 and two tiles + 1, a bright pixel on every seam and in every
    frame corner"""
    th, tw = [(h, w) for rmax, h, w in BLUR_TILES if R <= rmax][0]
    for n, (H, W) in enumerate((h, w) for h in (th - 1, th, th + 1, 2 * th + 1) for w in (tw - 1, tw, tw + 1, 2 * tw + 1)):
        fr = fb.seams((H, W), th, tw, F=1, seed=n, dtype=(np.uint16, np.uint8)[n % 2])
        got = check(fr, CLASS_SIGMAS[R], "%d x %d" % (H, W))
        assert (got[0] != fr[0]).any()


@pytest.mark.parametrize("sigma", [0.1, 0.5, 2, 3.3, 8.124])
def test_every_pixel_type_and_the_special_values(sigma):
    shape = (1, 65, 130)
    for kind in ("u8", "u16", "f32", "big"):
        check(fb.plane(shape, kind, 7), sigma, kind)
    x = fb.special_plane(shape, 8)
    assert np.isnan(x).any() and np.isinf(x).any() and (np.abs(x[x != 0]) < 1e-38).any() and np.signbit(x[x == 0]).any()
    got = check(x, sigma, "special values")
    if sigma == 0.1:                                            # R = 0: every value times 1.0, the zeros keep their sign
        assert np.array_equal(got.view(np.uint32)[~np.isnan(x)], x.view(np.uint32)[~np.isnan(x)])
    zeros = np.zeros(shape, np.float32)
    zeros[0, ::2] = -0.0
    assert np.array_equal(device_blur(zeros, sigma).view(np.uint32), fb.blur_restated(zeros[0], sigma)[None].view(np.uint32))


@pytest.mark.parametrize("sigma", [1.5, 8.124])
def test_frames_do_not_bleed_into_each_other(sigma):
    fr = fb.seams((70, 140), 32, 64, F=3, seed=5)
    assert (fr[0] != fr[1]).any() and (fr[1] != fr[2]).any()
    got = check(fr, sigma, "three frames")
    alone = device_blur(fr[1:2], sigma)
    assert np.array_equal(alone[0].view(np.uint32), got[1].view(np.uint32))


def raw_blur(frames, out, sigma, F, H, W):
    w = fb.weights(sigma)
    rc = _lib.load().sq_frame_blur_f32(frames.data_ptr(), PIX[frames.dtype], out.data_ptr(), w.ctypes.data, len(w) - 1, F, H, W,
                                       stream())
    assert rc == 0, _lib.load().sq_last_error()


@pytest.mark.parametrize("W", [129, 132])
@pytest.mark.parametrize("offset", [0, 1])
def test_both_store_paths_and_the_guard_behind_out(W, offset):
    """W % 4 == 0 with `out` on 16 bytes takes the vector store; an odd W or `out` 4 bytes further the scalar one"""
    F, H, guard = 2, 33, 4096
    fr = fb.plane((F, H, W), "u16", 11)
    n = F * H * W
    for sigma in (0.5, 2, 3.3):
        raw = torch.full((offset + n + guard,), -7.0, dtype=torch.float32, device=DEV)
        out = raw[offset:offset + n]
        assert (out.data_ptr() % 16 == 0) == (offset == 0)
        raw_blur(dev(fr), out, sigma, F, H, W)
        torch.cuda.synchronize()
        assert bool((raw[offset + n:] == -7.0).all()) and bool((raw[:offset] == -7.0).all()), "written outside out"
        got = out.cpu().numpy().reshape(F, H, W)
        for f in range(F):
            assert fb.equal_bits(got[f], fb.blur_restated(fr[f], sigma)), (W, offset, sigma, f)


def test_two_calls_give_the_same_bits_and_a_graph_replays_them():
    fr = dev(fb.plane((2, 70, 150), "u16", 12))
    tl = tiler(70, 150)
    for sigma in (0.5, 2, 8.124):
        eager = tl.blur(fr, sigma)
        assert torch.equal(eager.view(torch.int32), tl.blur(fr, sigma).view(torch.int32))
        buf = torch.zeros_like(eager)
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            tl.blur(fr, sigma, out=buf)                         # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            tl.blur(fr, sigma, out=buf)
        buf.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(buf.view(torch.int32), eager.view(torch.int32)), sigma


def test_reference_vector():
    got = device_blur(G["img_in"][None], 1.5)[0]
    assert_bit_exact(got, np.ascontiguousarray(G["blur_out"][..., 0]), "blur_out")


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_the_entry_refuses_what_it_cannot_blur():
    lib = _lib.load()
    fr = dev(fb.plane((1, 7, 5), "u8", 1))
    out = torch.full((1, 7, 5), -7.0, device=DEV)
    w = np.full(40, 0.01, np.float64)
    nan_w = w.copy()
    nan_w[1] = np.nan
    good = (fr.data_ptr(), 0, out.data_ptr(), w.ctypes.data, 2, 1, 7, 5)
    for change in ({4: 33}, {4: -1}, {0: None}, {2: None}, {3: None}, {1: 3}, {1: -1}, {5: 0}, {5: 65536}, {6: 0}, {7: 0},
                   {3: nan_w.ctypes.data}, {6: 4097, 7: 4097}):
        args = list(good)
        for k, v in change.items():
            args[k] = v
        rc = lib.sq_frame_blur_f32(*(args + [stream()]))
        assert rc == -1 and b"sq_frame_blur_f32" in lib.sq_last_error(), change
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())                            # nothing was launched
    assert lib.sq_frame_blur_f32(*(list(good) + [stream()])) == 0
    tl = tiler(7, 5)
    for sigma in (8.125, 0):
        with pytest.raises(ValueError, match="ImageBlur"):
            tl.blur(fr, sigma)
    with pytest.raises(ValueError, match="ImageBlur"):
        tl.tiles(fr, clean=FrameClean(blur=9))


# ---- chains through tiles() ------------------------------------------------------------------------------------------
CHAIN_CASES = (1, 2, 4)                                         # 48 x 40 float32, 37 x 53 uint16, 150 x 210 uint16


def chain_tiler(case):
    (_, H, W), _ = fc.CASES[case]
    return FrameTiler((H, W), tile=32, margin=4, device=DEV)


def cut(tl, full):
    return np.stack([full[y:y + tl.T, x:x + tl.T] for y in tl.oy for x in tl.ox])


@functools.lru_cache(maxsize=None)
def host_blurred(case, f, outliers, sigma):
    """frame f of the case through the host pipes in front of the fit: (H, W) float32"""
    pipes = ([pl.ImageOutliers(*outliers)] if outliers else []) + [pl.ImageBlur(sigma)]
    out = np.ascontiguousarray(pl.ImagePipeline(pipes)(np.array(fc.frames(case)[f]))[..., 0])
    assert out.dtype == np.float32
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("outliers", [None, (2, 50.)], ids=["blur-norm", "outliers-blur-norm"])
@pytest.mark.parametrize("case", CHAIN_CASES, ids=[fc.CASE_IDS[c] for c in CHAIN_CASES])
def test_blur_norm_chains_are_bit_exact_with_the_host_pipeline(case, outliers):
    fr, tl = fc.frames(case), chain_tiler(case)
    for sigma in (0.5, 1.5):
        clean = FrameClean(outliers=outliers, blur=sigma)
        host = pl.ImagePipeline(([pl.ImageOutliers(*outliers)] if outliers else []) + [pl.ImageBlur(sigma), pl.ImageNorm()])
        ref = np.concatenate([cut(tl, host(np.array(f))[..., 0]) for f in fr])
        got = tl.tiles(dev(fr), clean=clean)
        assert_bit_exact(got.cpu().numpy()[..., 0], ref, "%r" % (clean,))
        scratch = tl.clean_scratch(len(fr) + 1, clean)
        assert ("blurred" in scratch) == (outliers is not None)
        for batch in range(2):                                  # a second batch on the same scratch
            via = tl.tiles(dev(fr), clean=clean, scratch=scratch)
            assert torch.equal(via.view(torch.int32), got.view(torch.int32)), batch
        if outliers is None:
            plain = tl.tiles(dev(fr), normalise=False, clean=FrameClean(blur=sigma)).cpu().numpy()[..., 0]
            assert_bit_exact(plain, np.concatenate([cut(tl, host_blurred(case, f, None, sigma)) for f in range(len(fr))]),
                             "blur alone")


@pytest.mark.parametrize("normalise", [False, True], ids=["blur-bgsubtract", "blur-bgsubtract-norm"])
@pytest.mark.parametrize("case", CHAIN_CASES, ids=[fc.CASE_IDS[c] for c in CHAIN_CASES])
def test_blur_bgsubtract_tiles_within_the_bound(case, normalise):
    """every tile element t against the oracle's z (float64) on the host-blurred frame:
    |t - z| <= ulp32(z) + (1 + |z|) delta / std, the bound of tests/test_gpu_frame_clean.py"""
    (F, H, W), _ = fc.CASES[case]
    fr, tl = fc.frames(case), chain_tiler(case)
    for outliers in (None, (2, 50.)):
        clean = FrameClean(outliers=outliers, bgsubtract=True, blur=1.5)
        got = tl.tiles(dev(fr), normalise=normalise, clean=clean)
        via = tl.tiles(dev(fr), normalise=normalise, clean=clean, scratch=tl.clean_scratch(F, clean, normalise))
        assert torch.equal(via.view(torch.int32), got.view(torch.int32))
        got = got.cpu().numpy()[..., 0].reshape(F, tl.tiles_per_frame, tl.T, tl.T).astype(np.float64)
        for f in range(F):
            z, std, d = fc.oracle_chain(host_blurred(case, f, outliers, 1.5), None, True, normalise)
            z = cut(tl, z)
            err, bound = np.abs(got[f] - z), fc.ulp32(z) + (1 + np.abs(z)) * d / std
            print("case %d frame %d outliers %r: max error / bound %.3g" % (case, f, outliers, (err / bound).max()))
            assert (err <= bound).all(), (f, outliers, float((err / bound).max()))


# ---- channels > 1 ----------------------------------------------------------------------------------------------------
BLUR, OUT_BLUR, BLUR_BG = FrameClean(blur=0.7), FrameClean(outliers=(3, 900.), blur=1.5), FrameClean(bgsubtract=True, blur=2.2)
MC_CLEANS = {2: ([BLUR, None], BLUR, OUT_BLUR), 3: ([OUT_BLUR, BLUR_BG, None], BLUR, BLUR_BG)}


@pytest.mark.parametrize("C", [2, 3])
def test_channel_c_is_the_single_channel_result(C):
    shape, F = mc.FRAME_SHAPES[0], 3
    fr = mc.planes(C, F, shape, np.uint16, seed=60 + C)
    fr[0, 1, 9, 11] = fr[C - 1, 0, 20, 30] = 65000              # hot pixels
    x = dev(fr)
    one = FrameTiler(shape, mc.TILE, mc.MARGIN, device=DEV)
    many = FrameTiler(shape, mc.TILE, mc.MARGIN, device=DEV, channels=C)
    b = many.blur(x, 1.5).cpu().numpy()
    for c in range(C):
        for f in range(F):
            assert fb.equal_bits(b[c, f], fb.blur_restated(fr[c, f], 1.5)), (c, f)
    for cleans in MC_CLEANS[C]:
        per = cleans if isinstance(cleans, list) else [cleans] * C
        for normalise in (True, False):
            got = many.tiles(x, normalise=normalise, clean=cleans)
            for c in range(C):
                want = one.tiles(x[c], normalise=normalise, clean=per[c]).cpu().numpy()
                assert_bit_exact(got.cpu().numpy()[..., c], want[..., 0], "channel %d under %r" % (c, per[c]))
            scratch = many.clean_scratch(F + 1, cleans, normalise)
            assert ("blur_in" in scratch) == any(p is not None and p.outliers is not None and p.blur is not None for p in per)
            for batch in range(2):
                via = many.tiles(x, normalise=normalise, clean=cleans, scratch=scratch)
                assert torch.equal(via.view(torch.int32), got.view(torch.int32))


@pytest.mark.parametrize("C", [2, 3])
def test_a_view_of_a_staging_buffer_equals_its_packed_copy(C):
    shape, B, n = mc.FRAME_SHAPES[0], 3, 2
    buf = dev(mc.planes(C, B, shape, np.uint16, seed=70 + C))
    view = buf[:, :n]
    assert not view.is_contiguous()
    many = FrameTiler(shape, mc.TILE, mc.MARGIN, device=DEV, channels=C)
    for cleans in MC_CLEANS[C]:
        want = many.tiles(view.contiguous(), clean=cleans)
        assert torch.equal(many.tiles(view, clean=cleans).view(torch.int32), want.view(torch.int32))
        scratch = many.clean_scratch(B, cleans)
        assert torch.equal(many.tiles(view, clean=cleans, scratch=scratch).view(torch.int32), want.view(torch.int32))


# ---- segment_frames and the jobs -------------------------------------------------------------------------------------
SEG = {"shape": (64, 64), "filters": (16, 32), "num_outputs": 2, "seed": 6}
SEG_CLEAN = FrameClean(outliers=(2, 50.), blur=0.5)
SEG_PIPES = [{"ImageOutliers": {"sigma": 2, "threshold": 50.0}}, {"ImageBlur": {"sigma": 0.5}}, {"ImageNorm": {}}]


def job_net(**more):
    return UNet2D(dict(SEG, device=DEV, **more), "infer").initialize()


@functools.lru_cache(maxsize=None)
def seg_frames():
    rng = np.random.default_rng(17)
    v, u = np.mgrid[0:150, 0:210]
    fr = 1500 + 3. * u + 2. * v + 600 * (np.hypot(u - 90, v - 70) < 25) + 250 * rng.standard_normal((4, 150, 210))
    fr[:, ::13, ::29] += 9000
    fr = np.rint(fr).astype(np.uint16)
    fr.setflags(write=False)
    return fr


def host_masks(net, fr, pipes):
    """the host pipeline per frame, cut at the tiler's origins, through net.predict and the owner maps"""
    H, W = fr.shape[1:]
    tl = FrameTiler((H, W), 64, 8, device=DEV)
    host = pl.ImagePipeline(pipes)
    tiles = np.concatenate([cut(tl, host(np.array(f))[..., 0]) for f in fr])[..., None]
    return frontend_ref.stitch(net.predict(dev(tiles)).cpu().numpy(), tl.oy, tl.ox, tl.ymap, tl.xmap, H, W)


def test_segment_frames_with_a_blur_equals_the_host_pipeline():
    net, fr = job_net(), seg_frames()
    ref = host_masks(net, fr, [pl.ImageOutliers(2, 50.), pl.ImageBlur(0.5), pl.ImageNorm()])
    for per_batch in (4, 3, 2):                                 # 3: a partial last batch
        got = segment_frames(net, fr, tile=64, margin=8, frames_per_batch=per_batch, clean=SEG_CLEAN)
        assert got.shape == (4, 150, 210) and np.array_equal(got, ref), per_batch
    assert 0 < ref.mean() < 1
    unblurred = segment_frames(net, fr, tile=64, margin=8, frames_per_batch=3, clean=FrameClean(outliers=(2, 50.)))
    assert np.array_equal(unblurred, host_masks(net, fr, [pl.ImageOutliers(2, 50.), pl.ImageNorm()]))
    assert (unblurred != ref).any(), "the blur must change at least one pixel of the masks"


def test_frame_jobs_with_a_blur_in_the_pipeline(tmp_path):
    fr = seg_frames()
    np.save(str(tmp_path / "frames.npy"), fr)
    pl.ImagePipeline([pl.ImageOutliers(2, 50.), pl.ImageBlur(0.5), pl.ImageNorm()]).save(str(tmp_path / "pipe.json"))
    base = dict(SEG, input=str(tmp_path / "frames.npy"), margin=8, frames_per_batch=3, pipeline=str(tmp_path / "pipe.json"))
    out = str(tmp_path / "seg")
    os.makedirs(out)
    jobs.SERVER_segment_frames(dict(base, output=out), {"gpu": 0})
    ref = segment_frames(job_net(), fr, tile=64, margin=8, frames_per_batch=3, clean=SEG_CLEAN)
    masks = np.load(os.path.join(out, "mask.npy"))
    assert np.array_equal(masks, ref)
    rec = json.load(open(os.path.join(out, "segment.json")))
    assert rec["pipeline"] == SEG_PIPES and rec["frames"] == 4
    labels = (np.random.default_rng(3).random(fr.shape) < 0.3).astype(np.uint8)
    ev = str(tmp_path / "ev")
    os.makedirs(ev)
    einfo = jobs.SERVER_evaluate(dict(base, output=ev, labels=labels), {"gpu": 0})
    want = np.zeros((4, 2, 2), np.int64)
    for f in range(4):
        np.add.at(want[f], (labels[f], masks[f]), 1)
    assert np.array_equal(np.load(os.path.join(ev, "confusion.npy")), want) and einfo["pipeline"] == SEG_PIPES


def test_a_list_input_with_a_blur_on_one_channel(tmp_path):
    fr = seg_frames()
    other = np.ascontiguousarray(fr[::-1] // 2)
    np.save(str(tmp_path / "a.npy"), fr)
    np.save(str(tmp_path / "b.npy"), other)
    blur = pl.ImagePipeline([pl.ImageBlur(1.5), pl.ImageNorm()])
    blur.save(str(tmp_path / "blur.json"))
    out = str(tmp_path / "seg")
    os.makedirs(out)
    jobs.SERVER_segment_frames(dict(SEG, input=[str(tmp_path / "a.npy"), str(tmp_path / "b.npy")], margin=8, frames_per_batch=3,
                                    pipeline=[str(tmp_path / "blur.json"), None], output=out), {"gpu": 0})
    ref = segment_frames(job_net(num_inputs=2), [fr, other], tile=64, margin=8, frames_per_batch=3,
                         clean=[FrameClean(blur=1.5), None])
    assert np.array_equal(np.load(os.path.join(out, "mask.npy")), ref)
    rec = json.load(open(os.path.join(out, "segment.json")))
    assert rec["pipeline"] == [[{"ImageBlur": {"sigma": 1.5}}, {"ImageNorm": {}}], [{"ImageNorm": {}}]]
    plain = segment_frames(job_net(num_inputs=2), [fr, other], tile=64, margin=8, frames_per_batch=3)
    assert (plain != ref).any()


def test_a_job_refuses_a_blur_in_front_of_the_outliers(tmp_path):
    pl.ImagePipeline([pl.ImageBlur(0.5), pl.ImageOutliers(2, 50.)]).save(str(tmp_path / "pipe.json"))
    params = dict(SEG, input=str(tmp_path / "never_read.npy"), output=str(tmp_path), pipeline=str(tmp_path / "pipe.json"))
    with pytest.raises(ValueError, match="ImageBlur"):          # before the frames (which do not exist) are opened
        jobs.SERVER_segment_frames(params, {"gpu": 0})
    assert not os.path.exists(str(tmp_path / "mask.npy"))
