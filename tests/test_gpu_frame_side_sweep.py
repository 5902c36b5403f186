"""GPU: the frame-side kernels at the regimes of tests/frame_side_cases.py (the plan: tests/test_frame_side_plan.py).
Statistics, hot pixels, confusion counts, centroids and the tiles of a blank frame are compared for equality -- bit for
bit with numpy / scipy, NaN for NaN where the host gives NaN; the background surface and the residual statistics keep
their stated bound, frame_clean_cases.delta = 2^-32 max|x|."""
import numpy as np
import pytest
import torch

from oracle import frontend_ref
from sequitr_amd import _lib, centroids, ops
from sequitr_amd.frontend import FrameClean, FrameTiler, VolumeTiler
from tests import confusion_cases as cc
from tests import frame_clean_cases as fc
from tests import frame_side_cases as fsc
from tests import multichannel_cases as mcc
from tests.util import assert_bit_exact

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def whole_tiler(H, W):
    """one tile as large as the frame allows: the statistics and the cleaning kernels do not look at the tiling"""
    return FrameTiler((H, W), tile=min(H, W, 32), margin=0, device=DEV)


# ---- statistics -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(fsc.STATS_CASES)), ids=fsc.STATS_IDS)
def test_frame_stats_bit_exact_at_every_tail(case):
    (F, H, W), dtype, _ = fsc.STATS_CASES[case]
    fr = fsc.stats_frames((F, H, W), dtype, case)
    mean, std = (t.cpu().numpy() for t in whole_tiler(H, W).stats(dev(fr)))
    assert mean.shape == std.shape == (F,) and mean.dtype == std.dtype == np.float32
    for f in range(F):
        a = fsc.as_float32(fr[f])
        assert_bit_exact(mean[f], np.mean(a), "mean of frame %d" % f)
        assert_bit_exact(std[f], np.std(a), "std of frame %d" % f)


@pytest.mark.parametrize("case", range(len(fsc.VOLUME_CASES)), ids=["%dx%dx%dx%d" % s for s, _ in fsc.VOLUME_CASES])
def test_volume_stats_bit_exact_at_whole_groups_of_chunk_sums(case):
    shape, dtype = fsc.VOLUME_CASES[case]
    vols = fsc.stats_frames(shape, dtype, 70 + case)
    mean, std = (t.cpu().numpy() for t in VolumeTiler(shape[1:], shape[1:], 0, device=DEV).stats(dev(vols)))
    assert mean.shape == std.shape == (shape[0],) and mean.dtype == std.dtype == np.float32
    for v in range(shape[0]):
        a = fsc.as_float32(vols[v])
        assert_bit_exact(mean[v], np.mean(a), "mean of volume %d" % v)
        assert_bit_exact(std[v], np.std(a), "std of volume %d" % v)


# ---- hot pixels -------------------------------------------------------------------------------------------------------
GUARD = 64                                                      # floats on either side: whole 16-byte slots


def guarded_outliers(fr, size, threshold, lead):
    """ImageOutliers of the frames written into a NaN-filled buffer `lead` floats behind a guard band: (result, guards)"""
    F, H, W = fr.shape
    n = F * H * W
    buf = torch.full((GUARD + lead + n + GUARD,), float("nan"), device=DEV)
    sentinel = buf[:1].cpu().numpy().view(np.uint32)[0]
    out = buf[GUARD + lead:GUARD + lead + n].view(F, H, W)
    assert out.data_ptr() % 16 == 4 * lead
    got = whole_tiler(H, W).outliers(dev(fr), size, threshold, out=out)
    assert got.data_ptr() == out.data_ptr()
    host = buf.cpu().numpy()
    guards = np.concatenate([host[:GUARD + lead], host[GUARD + lead + n:]]).view(np.uint32)
    assert (guards == sentinel).all(), "%d guard floats were written" % int((guards != sentinel).sum())
    return host[GUARD + lead:GUARD + lead + n].reshape(F, H, W)


def check_outliers(fr, size, threshold):
    W = fr.shape[2]
    want = np.stack([fc.outliers_host(f, size, threshold) for f in fr])
    for lead in (0, 1) if W % 4 == 0 else (0,):                 # lead 1: rows of whole slots, but no store is aligned
        got = guarded_outliers(fr, size, threshold, lead)
        for f in range(fr.shape[0]):
            assert_bit_exact(got[f], want[f], "frame %d, %d floats into the buffer" % (f, lead))


@pytest.mark.parametrize("case", range(len(fsc.HOT_CASES)), ids=fsc.HOT_IDS)
def test_outliers_into_a_guarded_buffer(case):
    H, W, size, dtype, _ = fsc.HOT_CASES[case]
    check_outliers(fsc.hot_frames(H, W, dtype), size, fsc.HOT_THRESHOLD)


def test_outliers_keep_a_pixel_exactly_on_the_threshold():
    H, W, size, dtype, thr = fsc.TIE_CASE
    check_outliers(fsc.hot_frames(H, W, dtype, seed=1), size, thr)


# ---- background -------------------------------------------------------------------------------------------------------
def fitted(case):
    (F, H, W), _ = fsc.BG_CASES[case]
    tl = whole_tiler(H, W)
    x = tl.to_f32(dev(fsc.bg_frames(case)))
    return tl, x, tl.background(x)


@pytest.mark.parametrize("case", range(len(fsc.BG_CASES)), ids=fsc.BG_IDS)
def test_background_surface_of_tall_and_wide_frames(case):
    (F, H, W), _ = fsc.BG_CASES[case]
    fr = fsc.bg_frames(case)
    tl, x, coef_d = fitted(case)
    coef = coef_d.cpu().numpy()
    assert coef.shape == (F, 6) and coef.dtype == np.float64
    assert np.array_equal(coef.view(np.uint64), tl.background(x).cpu().numpy().view(np.uint64))          # two runs, the same bits
    alone = tl.background(x[1:2].contiguous()).cpu().numpy()
    assert np.array_equal(coef[1:2].view(np.uint64), alone.view(np.uint64))    # frame 1 of the batch is the frame alone
    mean, std = (t.cpu().numpy() for t in tl.background_stats(x, coef_d))
    for f in range(F):
        xf = fc.as_float32(fr[f])
        want, d = fc.oracle_fit(xf)[0], fc.delta(xf)
        err = np.abs(fc.basis_surface(coef[f], H, W) - want).max()
        rmean, rstd = fsc.two_pass_stats(xf.astype(np.longdouble) - want.astype(np.longdouble))
        print("%s frame %d: surface error %.3g, residual mean error %.3g, std error %.3g, delta %.3g"
              % (fsc.BG_IDS[case], f, err, abs(mean[f] - rmean), abs(std[f] - rstd), d))
        assert err <= d, (f, err, d)
        assert abs(mean[f] - rmean) <= d and abs(std[f] - rstd) <= d, (f, mean[f], rmean, std[f], rstd, d)


def test_residual_statistics_with_coefficients_that_fit_nothing():
    """zero coefficients on a flat frame at 60000 with noise 1: the one-pass variance cancels nine digits and stays inside
    delta = 2^-32 max|x| all the same"""
    xh = fsc.zero_coef_frame()
    H, W = xh.shape
    tl = whole_tiler(H, W)
    coef = torch.zeros((1, 6), dtype=torch.float64, device=DEV)
    mean, std = (float(t.cpu().numpy()[0]) for t in tl.background_stats(dev(xh[None]), coef))
    want_mean, want_std = fsc.two_pass_stats(xh)
    d = fc.delta(xh)
    print("zero coefficients: mean error %.3g, std error %.3g = %.3g relative (float32 half-ulp %.3g), delta %.3g"
          % (abs(mean - want_mean), abs(std - want_std), abs(std - want_std) / want_std, 2.0 ** -25, d))
    assert abs(mean - want_mean) <= d and abs(std - want_std) <= d, (mean, want_mean, std, want_std, d)


# ---- confusion --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(fsc.CONFUSION_CASES)), ids=fsc.CONFUSION_IDS)
def test_confusion_units_beyond_the_grid(case):
    _, n, C = fsc.CONFUSION_CASES[case]
    p, t = fsc.confusion_inputs(case)
    items = fsc.CONFUSION_ITEMS
    assert ops.confusion_chunk(items, n) == fsc.MIN_CHUNK
    want_c, want_i = cc.confusion_ref(p, t, C)
    counts = torch.zeros((items, C, C), dtype=torch.int64, device=DEV)
    ignored = torch.zeros((items,), dtype=torch.int64, device=DEV)
    ops.confusion_(counts, ignored, dev(p), dev(t), C)
    got_c, got_i = counts.cpu().numpy(), ignored.cpu().numpy()
    bad = np.flatnonzero((got_c != want_c).any((1, 2)) | (got_i != want_i))
    assert not len(bad), "%d items differ, the first is item %d (the grid holds %d)" % (len(bad), bad[0], fsc.MAX_GRID)


# ---- centroids --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["planar", "volumetric"])
def test_centroids_when_the_components_outnumber_the_rows(kind, monkeypatch):
    mask, ref, total = fsc.centroid_case(kind)
    seen = mask if kind == "planar" else np.swapaxes(mask, 1, -1)      # as CentroidWriter.write hands a volume on
    md = dev(seen)
    entry = "sq_mask_centroids_u8" if kind == "planar" else "sq_volume_centroids_u8"
    calls = []
    plain = _lib.check
    monkeypatch.setattr(_lib, "check", lambda rc, name: (calls.append(name), plain(rc, name))[1])
    for max_out, launches in ((fsc.SMALL_MAX_OUT, 2), (total, 1)):       # a retry with room for all; exactly enough room
        del calls[:]
        monkeypatch.setattr(centroids, "_MAX_OUT", max_out)
        got = centroids.mask_centroids(md)
        assert calls == [entry] * launches, (max_out, calls)
        assert len(got) == len(ref)
        for i, (a, b) in enumerate(zip(got, ref)):
            assert a.shape == b.shape, (max_out, i, a.shape, b.shape)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (max_out, i, a[:3], b[:3])


# ---- a blank frame ----------------------------------------------------------------------------------------------------
def test_tiles_of_a_blank_frame():
    fr = fsc.blank_frames()
    F, H, W = fr.shape
    T = fsc.BLANK_TILE
    tl = FrameTiler((H, W), tile=T, margin=fsc.BLANK_MARGIN, device=DEV)
    per = tl.tiles_per_frame
    got = tl.tiles(dev(fr)).cpu().numpy()
    with np.errstate(invalid="ignore"):
        want = frontend_ref.tiles(fr, tl.oy, tl.ox, T)
    assert got.shape == want.shape == (F * per, T, T, 1) and got.dtype == np.float32
    for f in (0, 2):
        assert_bit_exact(got[f * per:(f + 1) * per], want[f * per:(f + 1) * per], "tiles of frame %d" % f)
    assert np.isnan(want[per:2 * per]).all()
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%d tile elements of the blank frame are not NaN" % int(
        (~np.isnan(got[per:2 * per])).sum())
    # ImageBGSubtract in front: fp64 all the way, and 1e-99 + 0 is not 0 there
    x = tl.to_f32(dev(fr))
    coef_d = tl.background(x)
    coef = coef_d.cpu().numpy()
    mean, std = (t.cpu().numpy() for t in tl.background_stats(x, coef_d))
    got = tl.tiles(dev(fr), clean=FrameClean(bgsubtract=True)).cpu().numpy()
    assert np.isfinite(got).all()
    planes = [mcc.np_plane(fr[f], mcc.BG_NORM, coef=coef[f], mean64=mean[f], std64=std[f]) for f in range(F)]
    want = np.stack([p[y:y + T, x0:x0 + T] for p in planes for y in tl.oy for x0 in tl.ox])[..., None]
    assert_bit_exact(got, want, "SQ_CH_BG_NORM tiles against the header's fp64 expression")
