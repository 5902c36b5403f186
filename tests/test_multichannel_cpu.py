"""CPU: multi-channel frames.  The numpy restatements of the _mc entries (tests/multichannel_cases.py) against the host
pipes, which already work per channel of an (H, W, C) image; the host-side refusals of the two entries; what the jobs
refuse before they read a pixel; and the tiling geometry, which does not depend on the number of channels."""
import ctypes

import numpy as np
import pytest

from sequitr_amd import _lib, frontend, jobs, pipeline
from tests import multichannel_cases as mc
from tests import tile_sampler_cases as tsc
from tests.util import assert_bit_exact


def _hwc(planes_cf, f):
    """frame f of (C, F, H, W) planes as the host pipes take it: (H, W, C) float32"""
    return np.ascontiguousarray(np.moveaxis(planes_cf[:, f], 0, -1)).astype(np.float32)


@pytest.mark.parametrize("C", [2, 3])
@pytest.mark.parametrize("dtype", mc.DTYPES)
def test_tile_restatement_is_the_host_image_norm(C, dtype):
    H, W = mc.FRAME_SHAPES[0]
    fr = mc.planes(C, 2, (H, W), dtype, seed=1)
    oy, _ = frontend.axis_tiles(H, mc.TILE, mc.MARGIN)
    ox, _ = frontend.axis_tiles(W, mc.TILE, mc.MARGIN)
    stats = np.array([[mc.np_frame_stats(fr[c, f]) for f in range(2)] for c in range(C)])
    got = mc.np_tiles_mc(fr, [mc.NORM] * C, oy, ox, mc.TILE, mean32=stats[..., 0], std32=stats[..., 1])
    k = 0
    for f in range(2):
        host = pipeline.ImageNorm()(_hwc(fr, f))              # per channel of the (H, W, C) image
        assert host.dtype == np.float32 and host.shape == (H, W, C)
        for y in oy:
            for x in ox:
                assert_bit_exact(got[k], host[y:y + mc.TILE, x:x + mc.TILE], "tile %d" % k)
                k += 1
    assert k == got.shape[0]


def test_tile_restatement_is_outliers_then_norm_on_the_host():
    C, (H, W) = 3, mc.FRAME_SHAPES[0]
    fr = mc.planes(C, 1, (H, W), np.uint16, seed=2)
    fr[1, 0, 5, 7] = 60000                                      # a hot pixel in one channel only
    host = pipeline.ImagePipeline([pipeline.ImageOutliers(3, 500.), pipeline.ImageNorm()])(_hwc(fr, 0))
    cleaned = np.stack([pipeline.ImageOutliers(3, 500.)(np.array(fr[c, 0]))[..., 0] for c in range(C)])[:, None]
    assert cleaned[1, 0, 5, 7] != 60000
    stats = np.array([[mc.np_frame_stats(cleaned[c, 0])] for c in range(C)])
    oy, ox = (frontend.axis_tiles(L, mc.TILE, mc.MARGIN)[0] for L in (H, W))
    got = mc.np_tiles_mc(cleaned, [mc.NORM] * C, oy, ox, mc.TILE, mean32=stats[..., 0], std32=stats[..., 1])
    k = 0
    for y in oy:
        for x in ox:
            assert_bit_exact(got[k], host[y:y + mc.TILE, x:x + mc.TILE], "tile %d" % k)
            k += 1


def test_fused_surface_is_the_polynomial():
    """bg_surface states the order of operations; its value is the header's polynomial to fp64 rounding"""
    from tests import frame_clean_cases as fcc
    coef = np.array([31.5, -4.25, 2.125, 0.75, -1.5, 0.3])
    H, W = mc.FRAME_SHAPES[0]
    np.testing.assert_allclose(mc.bg_surface(coef, H, W), fcc.basis_surface(coef, H, W), rtol=0, atol=2.0 ** -44)
    a, b, c = np.float64(1 + 2.0 ** -30), np.float64(1 - 2.0 ** -30), np.float64(-1.0)
    assert mc._fma(a, b, c)[()] == -2.0 ** -60 and a * b + c == 0.0      # one rounding, not two


@pytest.mark.parametrize("CI", [1, 2, 3])
def test_sampler_restatement_is_the_single_channel_one_per_channel(CI):
    H, W = mc.SAMPLER_FRAME
    fr = mc.planes(CI, 3, (H, W), np.uint16, seed=3)
    normed = np.stack([tsc.np_normalised(fr[c]) for c in range(CI)])
    labels, weights = tsc.random_labels((3, H, W), 4), tsc.random_weights((3, H, W), 5)
    for plan, coef in (mc.sampler_rows(), mc.hostile_rows()):
        img, hot, wts = mc.np_sample_mc(normed, labels, weights, plan, coef, mc.SAMPLER_TILE, 3)
        assert img.shape == (len(plan),) + mc.SAMPLER_TILE + (CI,)
        for c in range(CI):
            one, hot1, wts1 = tsc.np_sample(normed[c], labels, weights, plan, coef, mc.SAMPLER_TILE, 3)
            assert_bit_exact(img[..., c], one[..., 0], "channel %d" % c)
        assert np.array_equal(hot, hot1)
        assert_bit_exact(wts, wts1, "weights")


def _buf(n=4096):
    raw = ctypes.create_string_buffer(n + 64)
    return raw, (ctypes.addressof(raw) + 63) & ~63


def test_tile_cutter_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    keep, p = _buf()
    err = lambda: lib.sq_last_error()

    def call(**kw):
        a = dict(frames=p, dtype=1, chan_stride=2 * 37 * 53, modes=[1, 0], mean32=p, std32=p, coef=None, mean64=None,
                 std64=None, oy=p, ox=p, tiles=p, F=2, H=37, W=53, C=2, TR=3, TC=5, TS=15)
        a.update(kw)
        modes = None if a['modes'] is None else (ctypes.c_int32 * len(a['modes']))(*a['modes'])
        return lib.sq_frames_to_tiles_mc(a['frames'], a['dtype'], a['chan_stride'],
                                         None if modes is None else ctypes.addressof(modes), a['mean32'], a['std32'],
                                         a['coef'], a['mean64'], a['std64'], a['oy'], a['ox'], a['tiles'], a['F'], a['H'],
                                         a['W'], a['C'], a['TR'], a['TC'], a['TS'], None)

    for name in ('frames', 'modes', 'oy', 'ox', 'tiles'):
        assert call(**{name: None}) == -1 and b"null" in err(), name
    for C in (0, -1, 9):
        assert call(C=C, modes=[0] * 9) == -1 and b"channels" in err(), C
    for mode in (-1, 4, 17):
        assert call(modes=[0, mode]) == -1 and b"unknown mode" in err(), mode
    assert call(dtype=3) == -1 and b"pixel type 3" in err()
    assert call(chan_stride=2 * 37 * 53 - 1) == -1 and b"chan_stride" in err()
    assert call(TS=38) == -1 and b"does not fit" in err()
    assert call(TS=0) == -1 and b"does not fit" in err()
    assert call(F=0) == -1
    # a statistics pointer may be missing only if no channel's mode reads it
    assert call(mean32=None) == -1 and b"SQ_CH_NORM" in err()
    assert call(modes=[0, 2], dtype=2) == -1 and b"coef" in err()
    assert call(modes=[0, 3], dtype=2, coef=p) == -1 and b"mean64" in err()
    assert call(modes=[0, 2], dtype=1, coef=p) == -1 and b"float32" in err()          # the background reads float32 frames
    assert call(tiles=p + 4) != 0 and b"aligned" in err()
    assert call(frames=p + 1) == -1 and b"aligned" in err()    # uint16 pixels at an odd address
    assert call(coef=p + 4, modes=[0, 2], dtype=2) == -1 and b"aligned" in err()
    assert call(F=40000, TR=60, TC=60, TS=15, chan_stride=40000 * 37 * 53) == -1 and b"out of range" in err()


def test_single_channel_cutter_refuses_tile_rows_beyond_32_bits_without_a_device():
    """the shared kernel indexes tile rows in 32 bits: F * TR * TC * TS beyond 2^31 - 1 is refused, not looped over"""
    lib = _lib.load()
    keep, p = _buf()
    call = lambda F: lib.sq_frames_to_tiles(p, 1, p, p, p, p, p, F, 37, 53, 60, 60, 15, None)
    assert 39769 * 60 * 60 * 15 > 2 ** 31 - 1 >= 39768 * 60 * 60 * 15
    assert call(39769) == -1 and b"sq_frames_to_tiles: 2147526000 tile rows are out of range" in lib.sq_last_error()
    assert lib.sq_frames_to_tiles_bg(p, p, p, p, p, p, p, 39769, 37, 53, 60, 60, 15, None) == -1
    assert b"sq_frames_to_tiles_bg: 2147526000 tile rows are out of range" in lib.sq_last_error()


def test_sampler_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    keep, p = _buf()
    err = lambda: lib.sq_last_error()

    def call(**kw):
        a = dict(frames=p, dtype=1, chan_stride=2 * 40 * 56, mean=p, std=p, labels=p, weights=p, plan=p, coef=p, oi=p, oh=p,
                 ow=p, F=2, H=40, W=56, CI=2, TH=16, TW=24, C=2, count=5)
        a.update(kw)
        return lib.sq_tile_sample_affine_mc(a['frames'], a['dtype'], a['chan_stride'], a['mean'], a['std'], a['labels'],
                                            a['weights'], a['plan'], a['coef'], a['oi'], a['oh'], a['ow'], a['F'], a['H'],
                                            a['W'], a['CI'], a['TH'], a['TW'], a['C'], a['count'], None)

    assert call(plan=None) == -1 and b"null" in err()
    assert call(oi=None) == -1 and b"go together" in err()
    assert call(labels=None) == -1 and b"go together" in err()
    assert call(frames=None, oi=None, labels=None, oh=None, weights=None, ow=None) == -1 and b"no output" in err()
    assert call(std=None) == -1 and b"both" in err()
    for CI in (0, -2, 9):
        assert call(CI=CI) == -1 and b"image channels" in err(), CI
    assert call(chan_stride=2 * 40 * 56 - 1) == -1 and b"chan_stride" in err()
    for C in (0, 17):
        assert call(C=C) == -1 and b"classes" in err(), C
    for count in (0, 65536):
        assert call(count=count) == -1 and b"count" in err(), count
    assert call(H=4097, W=4096, chan_stride=2 * 4097 * 4096) == -1 and b"2^24" in err()
    assert call(dtype=3) == -1 and b"pixel type 3" in err()
    assert call(frames=p + 1) == -1 and b"aligned" in err()
    assert call(TH=0) == -1 and b"positive" in err()


def test_geometry_does_not_depend_on_the_channels(monkeypatch):
    """the planned tiles and owner maps for channels > 1 are those for 1 (the tables' upload is stubbed: no device here)"""
    from types import SimpleNamespace
    monkeypatch.setattr(frontend.torch, 'from_numpy', lambda a: SimpleNamespace(to=lambda d: a))
    for shape in mc.FRAME_SHAPES:
        one = frontend.FrameTiler(shape, mc.TILE, mc.MARGIN, device='cuda:0')
        for C in (2, 3, 8):
            many = frontend.FrameTiler(shape, mc.TILE, mc.MARGIN, device='cuda:0', channels=C)
            assert (many.TR, many.TC, many.tiles_per_frame) == (one.TR, one.TC, one.tiles_per_frame)
            for name in ('oy', 'ox', 'ymap', 'xmap'):
                assert np.array_equal(getattr(many, name), getattr(one, name)), name
            assert many.channels == C
    with pytest.raises(ValueError, match='channels'):
        frontend.FrameTiler((64, 64), 32, 0, device='cuda:0', channels=9)
    with pytest.raises(ValueError, match='channels'):
        frontend.TileSampler((64, 64), (32, 32), device='cuda:0', channels=0)


def test_open_channels_reads_no_pixel_and_refuses_ragged_sources():
    a = np.zeros((3, 20, 24), np.uint16)
    gets, shape, dtype, C = frontend.open_channels(a)
    assert (shape, dtype, C, len(gets)) == ((3, 20, 24), np.dtype('uint16'), None, 1)
    gets, shape, dtype, C = frontend.open_channels([a, a + 1])
    assert (shape, C, len(gets)) == ((3, 20, 24), 2, 2) and gets[1](1, 2).shape == (2, 20, 24) and gets[1](0, 1).max() == 1
    gets, shape, dtype, C = frontend.open_channels(np.zeros((3, 20, 24, 4), np.float32))
    assert (shape, C, len(gets)) == ((3, 20, 24), 4, 1) and gets[0](0, 2).shape == (2, 20, 24, 4)
    gets, shape, dtype, C = frontend.open_channels(np.zeros((3, 20, 24, 1), np.uint8))
    assert (shape, C) == ((3, 20, 24), 1) and gets[0](0, 2).shape == (2, 20, 24)
    for bad in ([a, a[:2]], [a, a[:, :19]], [a, a.astype(np.uint8)]):
        with pytest.raises(ValueError, match='share one length, shape and pixel type'):
            frontend.open_channels(bad)
    with pytest.raises(ValueError, match='channels'):
        frontend.open_channels([a] * 9)
    with pytest.raises(ValueError, match='channels'):
        frontend.open_channels(np.zeros((1, 8, 8, 9), np.uint8))
    assert frontend.channel_cleans(None, 3) == [None] * 3
    c = frontend.FrameClean(bgsubtract=True)
    assert frontend.channel_cleans(c, 2) == [c, c] and frontend.channel_cleans([c, None], 2) == [c, None]
    assert frontend.channel_cleans([frontend.FrameClean(), c], 2) == [None, c]
    with pytest.raises(ValueError, match='2 entries for 3 channels'):
        frontend.channel_cleans([c, None], 3)


class _Unreadable(np.ndarray):
    """an array whose pixels must not be touched: the jobs under test raise before they read one"""

    def __getitem__(self, item):
        raise AssertionError('a pixel was read')


def _sealed(shape, dtype):
    return np.zeros(shape, dtype).view(_Unreadable)


@pytest.mark.parametrize("job", ["SERVER_segment_frames", "SERVER_evaluate"])
def test_frame_jobs_refuse_before_reading_a_pixel(job, tmp_path):
    run = getattr(jobs, job)
    a, b = _sealed((3, 40, 48), np.uint16), _sealed((3, 40, 48), np.uint16)
    base = {'output': str(tmp_path), 'shape': (32, 32), 'filters': (16, 32), 'num_outputs': 2, 'device': 'cuda:0',
            'labels': np.zeros((3, 40, 48), np.uint8)}
    for ragged in (_sealed((2, 40, 48), np.uint16), _sealed((3, 40, 47), np.uint16), _sealed((3, 40, 48), np.uint8)):
        with pytest.raises(ValueError, match='share one length, shape and pixel type'):
            run(dict(base, input=[a, ragged]), {})
    with pytest.raises(ValueError, match="num_inputs'\\] is 3, the input has 2 channels"):
        run(dict(base, input=[a, b], num_inputs=3), {})
    with pytest.raises(ValueError, match="num_inputs'\\] is 1, the input has 2 channels"):
        run(dict(base, input=_sealed((3, 40, 48, 2), np.uint16), num_inputs=1), {})
    norm = pipeline.ImagePipeline([pipeline.ImageNorm()])
    with pytest.raises(ValueError, match='3 pipelines for 2 channels'):
        run(dict(base, input=[a, b], pipeline=[norm, None, norm]), {})
    with pytest.raises(ValueError, match='agree on ImageNorm'):
        run(dict(base, input=[a, b], pipeline=[pipeline.ImagePipeline([pipeline.ImageOutliers(3, 5.)]), None]), {})
    with pytest.raises(ValueError, match='one channel'):
        run(dict(base, input=a, pipeline=[norm, norm]), {})
    if job == "SERVER_segment_frames":
        for bad in (2, -1):
            with pytest.raises(ValueError, match='measure_channel'):
                run(dict(base, input=[a, b], measure_channel=bad), {'measure': True})
        with pytest.raises(ValueError, match='measure_channel'):
            run(dict(base, input=a, measure_channel=1), {'measure': True})


def test_channel_setup_records_the_pipeline_per_channel():
    out = pipeline.ImagePipeline([pipeline.ImageOutliers(3, 5.), pipeline.ImageNorm()])
    bg = pipeline.ImagePipeline([pipeline.ImageBGSubtract(), pipeline.ImageNorm()])
    clean, normalise, record, n_in = jobs._channel_setup({'pipeline': [out, None, bg]}, 3)
    assert normalise and n_in == 3
    assert clean == [frontend.FrameClean(outliers=(3, 5.)), None, frontend.FrameClean(bgsubtract=True)]
    assert record == [[{'ImageOutliers': {'sigma': 3, 'threshold': 5.0}}, {'ImageNorm': {}}], [{'ImageNorm': {}}],
                      [{'ImageBGSubtract': {}}, {'ImageNorm': {}}]]
    clean, normalise, record, n_in = jobs._channel_setup({'pipeline': bg}, 2)
    assert clean == [frontend.FrameClean(bgsubtract=True)] * 2 and len(record) == 2
    # one channel: what the jobs did before there were channels
    assert jobs._channel_setup({}, None) == (None, True, None, None)
    clean, normalise, record, n_in = jobs._channel_setup({'pipeline': bg}, None)
    assert (clean, normalise, n_in) == (frontend.FrameClean(bgsubtract=True), True, None)
    assert record == [{'ImageBGSubtract': {}}, {'ImageNorm': {}}]


def test_train_job_takes_channels_only_with_num_inputs(tmp_path):
    np.save(str(tmp_path / "im2c.npy"), np.zeros((2, 40, 48, 2), np.float32))
    np.save(str(tmp_path / "bf.npy"), np.zeros((2, 40, 48), np.uint16))
    np.save(str(tmp_path / "gfp.npy"), np.zeros((2, 40, 47), np.uint16))
    np.save(str(tmp_path / "lab.npy"), np.zeros((2, 40, 48), np.uint8))
    base = {'images': str(tmp_path / "im2c.npy"), 'labels': str(tmp_path / "lab.npy"), 'output': str(tmp_path),
            'num_outputs': 2, 'tile': (32, 32)}
    with pytest.raises(ValueError, match="num_inputs'\\] is 3, the images have 2 channel"):
        jobs.SERVER_train(dict(base, num_inputs=3), {'gpu': 0})
    with pytest.raises(ValueError, match='share one length, shape and pixel type'):
        jobs.SERVER_train(dict(base, images=[str(tmp_path / "bf.npy"), str(tmp_path / "gfp.npy")], num_inputs=2), {'gpu': 0})
    with pytest.raises(ValueError, match="the images have 2 channel"):
        jobs.SERVER_train(dict(base, images=[str(tmp_path / "bf.npy")] * 2, num_inputs=1), {'gpu': 0})


def test_frame_stats_ask_for_the_pixel_types_alignment():
    """sq_frame_stats takes a channel's slice wherever it starts; what it still refuses is a pointer its pixel type cannot
    be read from"""
    lib = _lib.load()
    keep, p = _buf()
    for dtype, off in ((1, 1), (2, 1), (2, 2)):                 # uint16 at an odd address, float32 off a 4-byte boundary
        assert lib.sq_frame_stats(p + off, dtype, p, p, p, 2, 37, 53, None) == -1
        assert b"frames not aligned to their pixel type" in lib.sq_last_error(), (dtype, off)
    assert lib.sq_frame_stats(None, 0, p, p, p, 2, 37, 53, None) == -1 and b"null" in lib.sq_last_error()
