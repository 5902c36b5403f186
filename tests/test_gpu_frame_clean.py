"""GPU: frame cleaning in front of ImageNorm (include/sequitr_hip.h "Frame cleaning") -- ImageOutliers bit-exact with the
host pipe, ImageBGSubtract within delta = 2^-32 max|x| of the long-double oracle of tests/frame_clean_cases.py, the chain
through FrameTiler.tiles, segment_frames and the SERVER_segment_frames job."""
import argparse
import functools
import json
import os

import numpy as np
import pytest
import torch

from sequitr_amd import _lib, jobs, worker
from sequitr_amd.frontend import FrameClean, FrameTiler, segment_frames
from sequitr_amd.networks.unet import UNet2D, init_unet_weights
from sequitr_amd.pipeline import ImageBGSubtract, ImageFlip, ImageNorm, ImageOutliers, ImagePipeline
from tests import frame_clean_cases as fc
from tests.test_jobs_config import write_job
from tests.util import assert_bit_exact

pytestmark = pytest.mark.gpu
G = fc.GOLDEN
NCASE = range(len(fc.CASES))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def tiler(case, margin=None):
    """the case's tiler: 32-pixel tiles with a margin of 4 where they fit, else one tile as large as the frame allows"""
    (_, H, W), _ = fc.CASES[case]
    T = min(H, W, 32)
    return FrameTiler((H, W), tile=T, margin=(4 if T == 32 else 0) if margin is None else margin, device="cuda:0")


def cut(tl, full):
    """(TR*TC, T, T) tiles of one full-frame array, in the tiler's order"""
    return np.stack([full[y:y + tl.T, x:x + tl.T] for y in tl.oy for x in tl.ox])


@functools.lru_cache(maxsize=None)
def chain(case, f, outliers, bgsubtract, normalise):
    return fc.oracle_chain(fc.frames(case)[f], outliers, bgsubtract, normalise)


# ---- hot pixels ------------------------------------------------------------------------------------------------------
# every case with every window that fits it (one that does not is refused: test_outliers_refuses_what_it_cannot_filter)
FITS = [(c, size, thr) for c in NCASE for size, thr in ((2, 50.), (3, 50.), (3, 4.), (4, 50.), (5, 50.))
        if min(fc.CASES[c][0][1:]) >= size]


@pytest.mark.parametrize("case,size,threshold", FITS, ids=["%s-size%d-thr%g" % (fc.CASE_IDS[c], s, t) for c, s, t in FITS])
def test_outliers_bit_exact_with_the_host_pipe(case, size, threshold):
    (F, H, W), _ = fc.CASES[case]
    fr = fc.frames(case)
    got = tiler(case).outliers(dev(fr), size, threshold).cpu().numpy()
    assert got.shape == (F, H, W) and got.dtype == np.float32
    for f in range(F):
        assert_bit_exact(got[f], fc.outliers_host(fr[f], size, threshold), "frame %d" % f)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
def test_outliers_every_pixel_type_on_one_frame(dtype):
    """the same counts as uint8, uint16 and float32: 150 x 210, more than one tile row, lanes past the right edge"""
    fr = np.minimum(fc.frames(4) // 32, 255).astype(dtype)
    fr[0, ::17, ::13] = 250
    tl = FrameTiler((150, 210), tile=64, margin=8, device="cuda:0")
    for size in fc.SIZES:
        assert_bit_exact(tl.outliers(dev(fr), size, 20.).cpu().numpy()[0], fc.outliers_host(fr[0], size, 20.), "size %d" % size)


def test_outliers_reference_vector():
    tl = FrameTiler((48, 40), tile=32, margin=4, device="cuda:0")
    got = tl.outliers(dev(G["img_in"][None]), 2, 50.).cpu().numpy()[0]
    assert_bit_exact(got, G["outliers_out"][..., 0], "outliers_out")


def test_outliers_refuses_what_it_cannot_filter():
    lib = _lib.load()
    fr = dev(fc.frames(0))                                      # 7 x 5
    out = torch.full((1, 7, 5), -7.0, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    for size, H, W in ((6, 7, 5), (1, 7, 5), (5, 7, 4), (4, 3, 5)):
        rc = lib.sq_frame_outliers_f32(fr.data_ptr(), 0, out.data_ptr(), 1, H, W, size, 5.0, st)
        assert rc == -1 and b"sq_frame_outliers_f32" in lib.sq_last_error(), (size, H, W)
    torch.cuda.synchronize()
    assert (out == -7.0).all()                                  # nothing was launched
    tl = tiler(0)
    with pytest.raises(ValueError, match="ImageOutliers"):
        tl.outliers(fr, 6, 5.)
    with pytest.raises(ValueError, match="does not fit"):
        FrameTiler((4, 9), tile=4, margin=0, device="cuda:0").outliers(dev(np.zeros((1, 4, 9), np.uint8)), 5, 5.)


# ---- outliers -> norm ------------------------------------------------------------------------------------------------
def test_outliers_norm_reference_chain():
    """chain_out_0 was written by the reference's own ImagePipeline([ImageOutliers(2, 50.), ImageNorm()])"""
    tl = FrameTiler((48, 40), tile=32, margin=4, device="cuda:0")
    tiles = tl.tiles(dev(G["img_in"][None]), clean=FrameClean(outliers=(2, 50.))).cpu().numpy()
    ref = cut(tl, np.ascontiguousarray(G["chain_out_0"][..., 0]))
    assert tiles.shape == (len(ref), 32, 32, 1)
    for k in range(len(ref)):
        assert_bit_exact(tiles[k, ..., 0], ref[k], "tile %d" % k)


@pytest.mark.parametrize("case", [0, 2, 5], ids=[fc.CASE_IDS[c] for c in (0, 2, 5)])
def test_outliers_norm_bit_exact_with_the_host_chain(case):
    fr, tl = fc.frames(case), tiler(case)
    got = tl.tiles(dev(fr), clean=FrameClean(outliers=(2, 50.))).cpu().numpy()[..., 0]
    host = ImagePipeline([ImageOutliers(2, 50.), ImageNorm()])
    ref = np.concatenate([cut(tl, host(np.array(f))[..., 0]) for f in fr])
    assert_bit_exact(got, ref, "outliers -> norm tiles")


# ---- background ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NCASE, ids=fc.CASE_IDS)
def test_background_surface_within_delta_of_the_oracle(case):
    (F, H, W), _ = fc.CASES[case]
    fr, tl = fc.frames(case), tiler(case)
    x = tl.to_f32(dev(fr))
    assert_bit_exact(x.cpu().numpy(), np.stack([fc.as_float32(f) for f in fr]), "float32 frames")
    coef = tl.background(x).cpu().numpy()
    assert coef.shape == (F, 6) and coef.dtype == np.float64
    for f in range(F):
        xf = fc.as_float32(fr[f])
        err = np.abs(fc.basis_surface(coef[f], H, W) - fc.oracle_fit(xf)[0]).max()
        print("case %d frame %d: surface error %.3g, delta %.3g" % (case, f, err, fc.delta(xf)))
        assert err <= fc.delta(xf), (f, err, fc.delta(xf))


VARIANTS = {"bgsubtract": (None, False), "bgsubtract-norm": (None, True), "outliers-bgsubtract-norm": ((2, 50.), True)}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("case", NCASE, ids=fc.CASE_IDS)
def test_background_tiles_within_the_bound(case, variant):
    """every tile element t against the oracle's z (float64): |t - z| <= ulp32(z) + (1 + |z|) delta / std"""
    outliers, normalise = VARIANTS[variant]
    (F, H, W), _ = fc.CASES[case]
    fr, tl = fc.frames(case), tiler(case)
    got = tl.tiles(dev(fr), normalise=normalise, clean=FrameClean(outliers, True)).cpu().numpy()
    assert got.shape == (F * tl.tiles_per_frame, tl.T, tl.T, 1) and got.dtype == np.float32
    got = got[..., 0].reshape(F, tl.tiles_per_frame, tl.T, tl.T).astype(np.float64)
    for f in range(F):
        z, std, d = chain(case, f, outliers, True, normalise)
        z = cut(tl, z)
        err, bound = np.abs(got[f] - z), fc.ulp32(z) + (1 + np.abs(z)) * d / std
        print("case %d frame %d %s: max error / bound %.3g, %d of %d elements differ from float32(z)" % (
            case, f, variant, (err / bound).max(), int((got[f] != z.astype(np.float32)).sum()), z.size))
        assert (err <= bound).all(), (f, float((err / bound).max()))


def test_background_statistics_are_those_of_the_residual():
    fr, tl = fc.frames(2), tiler(2)
    x = tl.to_f32(dev(fr))
    coef = tl.background(x)
    mean, std = (t.cpu().numpy() for t in tl.background_stats(x, coef))
    for f in range(3):
        xf = fc.as_float32(fr[f])
        r = xf.astype(np.float64) - fc.oracle_fit(xf)[0]
        d = fc.delta(xf)
        assert abs(mean[f] - r.mean()) <= d and abs(std[f] - r.std()) <= d, (f, mean[f], r.mean(), std[f], r.std())


def test_background_is_deterministic_and_independent_of_the_batch():
    fr, tl = dev(fc.frames(2)), tiler(2)                        # 3 frames of 37 x 53
    x = tl.to_f32(fr)

    def run(frames):
        coef = tl.background(frames)
        mean, std = tl.background_stats(frames, coef)
        return [t.cpu().numpy().view(np.uint64) for t in (coef, mean, std)]

    a, b, alone = run(x), run(x), run(x[1:2].contiguous())
    for p, q, r in zip(a, b, alone):
        assert np.array_equal(p, q) and np.array_equal(p[1:2], r)
    big, tb = dev(fc.frames(5)), tiler(5)                       # more than one strip of rows per frame
    xb = tb.to_f32(big)
    assert np.array_equal(tb.background(xb).cpu().numpy().view(np.uint64), tb.background(xb).cpu().numpy().view(np.uint64))


def test_background_refuses_frames_it_cannot_fit():
    lib = _lib.load()
    x = torch.zeros((1, 2, 40), device="cuda:0")
    coef = torch.full((1, 6), -7.0, dtype=torch.float64, device="cuda:0")
    ws = torch.zeros(4096, dtype=torch.float64, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    for H, W in ((2, 40), (40, 2)):
        assert lib.sq_frame_bgfit_workspace(1, H, W) == -1
        rc = lib.sq_frame_bgfit_f64(x.data_ptr(), coef.data_ptr(), ws.data_ptr(), 1, H, W, st)
        assert rc == -1 and b"sq_frame_bgfit_f64" in lib.sq_last_error()
        rc = lib.sq_frame_bg_stats_f64(x.data_ptr(), coef.data_ptr(), ws.data_ptr(), ws.data_ptr(), ws.data_ptr(), 1, H, W, st)
        assert rc == -1 and b"sq_frame_bg_stats_f64" in lib.sq_last_error()
    assert lib.sq_frame_bgfit_workspace(1, 4097, 4096) == -1 and lib.sq_frame_bgfit_workspace(1, 4096, 4096) > 0
    torch.cuda.synchronize()
    assert (coef == -7.0).all()
    with pytest.raises(ValueError, match="H, W >= 3"):
        FrameTiler((2, 40), tile=2, margin=0, device="cuda:0").background(x)
    with pytest.raises(ValueError, match="float32"):
        tiler(2).background(dev(fc.frames(2)))                  # uint16: the fit reads cleaned float32 frames


# ---- streamed path ---------------------------------------------------------------------------------------------------
NET = {"shape": (64, 64), "filters": (16, 32), "device": "cuda:0"}
ALL3 = FrameClean(outliers=(2, 50.), bgsubtract=True)


def _net(seed):
    net = UNet2D(NET, "infer")
    net.load_state_dict(init_unet_weights(NET, seed))
    return net


def _stream_frames():
    rng = np.random.default_rng(8)
    v, u = np.mgrid[0:96, 0:160]
    fr = 1500 + 4. * u + 2. * v - 0.01 * u * v + 300 * (np.hypot(u - 70, v - 40) < 12) + 20 * rng.standard_normal((5, 96, 160))
    fr[:, ::11, ::23] += 3000
    return np.rint(fr).astype(np.uint16)


def test_segment_frames_with_the_whole_chain_equals_the_steps_one_at_a_time(monkeypatch):
    net, fr = _net(4), _stream_frames()
    seen, batches = {}, []
    tl = FrameTiler((96, 160), tile=64, margin=8, device="cuda:0")
    plain_tiles = FrameTiler.tiles

    def recording_tiles(self, frames, *args, **kwargs):
        out = plain_tiles(self, frames, *args, **kwargs)
        if kwargs.get("clean"):
            batches.append(out.cpu().numpy())
        return out

    monkeypatch.setattr(FrameTiler, "tiles", recording_tiles)
    got = segment_frames(net, fr, tile=64, margin=8, frames_per_batch=2, clean=ALL3)
    monkeypatch.setattr(FrameTiler, "tiles", plain_tiles)
    assert [len(b) for b in batches] == [2 * tl.tiles_per_frame, 2 * tl.tiles_per_frame, tl.tiles_per_frame]
    ref = []
    for first in (0, 2, 4):                                     # clean -> tiles -> net.predict -> stitch, batch by batch
        x = tl.outliers(dev(fr[first:first + 2]), 2, 50.)
        coef = tl.background(x)
        mean, std = tl.background_stats(x, coef)
        tiles = torch.empty((x.shape[0] * tl.tiles_per_frame, 64, 64, 1), device="cuda:0")
        _lib.check(_lib.load().sq_frames_to_tiles_bg(x.data_ptr(), coef.data_ptr(), mean.data_ptr(), std.data_ptr(),
                                                     tl._oy.data_ptr(), tl._ox.data_ptr(), tiles.data_ptr(), x.shape[0], 96,
                                                     160, tl.TR, tl.TC, 64, torch.cuda.current_stream().cuda_stream), "tiles")
        seen[first] = tiles.cpu().numpy()
        ref.append(tl.stitch(net.predict(tiles)).cpu().numpy())
    ref = np.concatenate(ref)
    assert got.shape == (5, 96, 160) and np.array_equal(got, ref)
    assert_bit_exact(batches[0], seen[0], "tiles of the first batch")
    streamed = []
    assert segment_frames(net, fr, tile=64, margin=8, frames_per_batch=4, clean=ALL3,
                          on_masks=lambda first, m: streamed.append(m.cpu().numpy())) is None
    assert np.array_equal(np.concatenate(streamed), ref)


def test_segment_frames_without_clean_is_unchanged():
    net, fr = _net(4), _stream_frames()
    plain = segment_frames(net, fr, tile=64, margin=8, frames_per_batch=2)
    assert np.array_equal(segment_frames(net, fr, tile=64, margin=8, frames_per_batch=2, clean=None), plain)
    assert np.array_equal(segment_frames(net, fr, tile=64, margin=8, frames_per_batch=2, clean=FrameClean()), plain)


# ---- job -------------------------------------------------------------------------------------------------------------
def test_segment_frames_job_with_a_pipeline(tmp_path):
    fr = _stream_frames()[:3]
    np.save(str(tmp_path / "frames.npy"), fr)
    ImagePipeline([ImageOutliers(2, 50.), ImageBGSubtract(), ImageNorm()]).save(str(tmp_path / "pipe.json"))
    params = {"input": str(tmp_path / "frames.npy"), "shape": (64, 64), "filters": (16, 32), "seed": 2, "margin": 8,
              "frames_per_batch": 2, "pipeline": str(tmp_path / "pipe.json")}
    fn = write_job(tmp_path, func="SERVER_segment_frames", params=repr(params), options="{'gpu': 0}")
    out = str(tmp_path / "out")
    worker.worker(argparse.Namespace(job=fn, out=out))
    logs = open(os.path.join(out, [f for f in os.listdir(out) if f.startswith("LOG_")][0])).read()
    assert "exception" not in logs, logs
    ref = segment_frames(_net(2), fr, tile=64, margin=8, frames_per_batch=2, clean=ALL3)
    assert np.array_equal(np.load(os.path.join(out, "mask.npy")), ref)
    info = json.load(open(os.path.join(out, "segment.json")))
    assert info["frames"] == 3
    assert info["pipeline"] == [{"ImageOutliers": {"sigma": 2, "threshold": 50.0}}, {"ImageBGSubtract": {}}, {"ImageNorm": {}}]


def test_segment_frames_job_refuses_a_pipe_the_device_does_not_run(tmp_path):
    ImagePipeline([ImageFlip(), ImageNorm()]).save(str(tmp_path / "pipe.json"))
    params = {"input": str(tmp_path / "never_read.npy"), "output": str(tmp_path), "shape": (64, 64), "filters": (16, 32),
              "pipeline": str(tmp_path / "pipe.json")}
    with pytest.raises(ValueError, match="ImageFlip"):          # before the frames (which do not exist) are opened
        jobs.SERVER_segment_frames(params, {"gpu": 0})
    assert not os.path.exists(str(tmp_path / "mask.npy"))
