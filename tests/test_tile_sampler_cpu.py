"""CPU: the host half of the tile sampler -- the numpy restatement of the sampling definition (tests/tile_sampler_cases.py)
against scipy, against its own float64 evaluation and against plain slicing, frontend.tile_sample_plan, and the host-side
refusals of sq_tile_sample_affine and of SERVER_train's tile mode.  Nothing here launches a kernel."""
import ctypes

import numpy as np
import pytest
from scipy import ndimage

from sequitr_amd import _lib
from sequitr_amd.frontend import covering_tiles, tile_sample_plan
from tests import tile_sampler_cases as tc

F, H, W = tc.FRAMES_SHAPE


def _zero_padded(frame, oy, ox, tile):
    out = np.zeros(tile, frame.dtype)
    for i in range(tile[0]):
        for j in range(tile[1]):
            if 0 <= oy + i < frame.shape[0] and 0 <= ox + j < frame.shape[1]:
                out[i, j] = frame[oy + i, ox + j]
    return out


def test_rounding_is_half_away_from_zero():
    v = np.asarray([-2.5, -1.5, -0.5, -0.49999997, 0.0, 0.49999997, 0.5, 1.5, 2.5, 8388607.5, -8388607.5, 3.2, -3.7], np.float32)
    want = np.asarray([-3, -2, -1, 0, 0, 0, 1, 2, 3, 8388608, -8388608, 3, -4], np.float32)
    assert np.array_equal(tc.np_round(v), want)
    assert np.array_equal(tc.np_round(v.astype(np.float64)), want.astype(np.float64))
    assert not np.array_equal(np.round(v), want)                # np.round goes to even: not this definition


def test_float64_evaluation_equals_scipy_map_coordinates():
    """120 random angles and origins that leave the frame: the bilinear part in float64 against scipy's order-1 spline with
    mode='grid-constant', cval=0 at the same coordinates -- pins the fill convention independently"""
    rng = np.random.default_rng(0)
    frames = tc.random_frames(tc.FRAMES_SHAPE, np.float32, 1)
    tile = (24, 24)
    plan = np.zeros((120, 4), np.int32)
    plan[:, 0] = rng.integers(0, F, 120)
    plan[:, 1] = rng.integers(-30, H + 6, 120)
    plan[:, 2] = rng.integers(-30, W + 6, 120)
    coef = tc.rotation_coef(rng.uniform(0, 2 * np.pi, 120), (H, W))
    got, _, _ = tc.np_sample(frames, None, None, plan, coef, tile, 2, dtype=np.float64)
    worst = 0.0
    for k in range(120):
        sx, sy, ok = tc.np_coords(plan[k], coef[k], tile, np.float64)
        assert ok.all()
        ref = ndimage.map_coordinates(frames[plan[k, 0]].astype(np.float64), [sy, sx], order=1, mode='grid-constant', cval=0.0)
        worst = max(worst, float(np.abs(got[k, ..., 0] - ref).max()))
    print("float64 restatement vs scipy: max abs %.3g" % worst)
    assert worst <= 1e-12


def test_float32_stays_within_the_stated_bound_of_float64():
    """|f32 - f64| <= 2 L delta + 8 * 2^-24 * max|img|: L the largest neighbour difference of the zero-padded frame (the
    bilinear surface's slope along either axis), delta the largest coordinate difference of the case, and eight roundings of
    values no larger than max|img| in the interpolation itself"""
    rng = np.random.default_rng(1)
    worst = 0.0
    for dtype, seed in ((np.uint8, 2), (np.uint16, 3), (np.float32, 4)):
        normed = tc.np_normalised(tc.random_frames(tc.FRAMES_SHAPE, dtype, seed))
        plan, coef = tc.random_rows(tc.FRAMES_SHAPE, (40, 40), 12, seed)
        plan, coef = plan[:12], coef[:12]
        a32, _, _ = tc.np_sample(normed, None, None, plan, coef, (40, 40), 2, dtype=np.float32)
        a64, _, _ = tc.np_sample(normed, None, None, plan, coef, (40, 40), 2, dtype=np.float64)
        for k in range(12):
            x32, y32, _ = tc.np_coords(plan[k], coef[k], (40, 40), np.float32)
            x64, y64, _ = tc.np_coords(plan[k], coef[k], (40, 40), np.float64)
            delta = max(np.abs(x32 - x64).max(), np.abs(y32 - y64).max())
            pad = np.pad(normed[plan[k, 0]].astype(np.float64), 1)
            L = max(np.abs(np.diff(pad, axis=0)).max(), np.abs(np.diff(pad, axis=1)).max())
            bound = 2 * L * delta + 8 * 2.0 ** -24 * np.abs(pad).max()
            err = np.abs(a32[k].astype(np.float64) - a64[k]).max()
            worst = max(worst, err / bound)
            assert err <= bound, (np.dtype(dtype).name, k, err, bound)
    print("float32 vs float64 restatement: worst error / bound %.3f" % worst)


def test_identity_rows_give_the_zero_padded_crop():
    frames = tc.random_frames(tc.FRAMES_SHAPE, np.float32, 5)
    labels = tc.random_labels(tc.FRAMES_SHAPE, 6) + 1           # no label 0 inside: the fill shows
    weights = tc.random_weights(tc.FRAMES_SHAPE, 7)
    origins = [(0, 0), (-4, -7), (H - 10, W - 10), (-30, 3), (5, W)]
    plan, coef = tc.identity_rows(origins, f=1)
    tile = (24, 24)
    img, hot, wts = tc.np_sample(frames, labels, weights, plan, coef, tile, 8)
    for k, (oy, ox) in enumerate(origins):
        assert np.array_equal(img[k, ..., 0], _zero_padded(frames[1], oy, ox, tile))
        lab = _zero_padded(labels[1], oy, ox, tile)
        assert np.array_equal(hot[k], (lab[..., None] == np.arange(8)).astype(np.uint8))
        inside = _zero_padded(np.ones((H, W), np.float32), oy, ox, tile)
        assert np.array_equal(wts[k, ..., 0], _zero_padded(weights[1], oy, ox, tile) + (1 - inside))
    assert hot[4, ..., 0].all() and not hot[4, ..., 1:].any()   # wholly outside: label 0, weight 1, image 0
    assert np.all(wts[4] == 1) and not img[4].any()


def test_exact_quarter_turn_is_rot90():
    S = 37
    frames = tc.random_frames((1, S, S), np.float32, 8)
    labels = tc.random_labels((1, S, S), 9)
    weights = tc.random_weights((1, S, S), 10)
    plan, coef = tc.quarter_turn_rows(S)
    img, hot, wts = tc.np_sample(frames, labels, weights, plan, coef, (S, S), 7)
    assert np.array_equal(img[0, ..., 0], np.rot90(frames[0], 1))
    assert np.array_equal(hot[0].argmax(-1), np.rot90(labels[0], 1)) and np.all(hot[0].sum(-1) == 1)
    assert np.array_equal(wts[0, ..., 0], np.rot90(weights[0], 1))          # the added term is exactly 0
    # cos(pi/2) does not round to 0: the plan function's quarter turn is close, not exact -- hence the hand-made rows
    _, near = tile_sample_plan((S, S), (S, S), 1, 1, np.random.default_rng(0), theta=[np.pi / 2])
    assert near[0, 0] != 0 and abs(near[0, 0]) < 1e-7


def test_bad_rows_are_all_fill():
    frames = tc.random_frames(tc.FRAMES_SHAPE, np.float32, 11)
    labels = tc.random_labels(tc.FRAMES_SHAPE, 12) + 1
    weights = tc.random_weights(tc.FRAMES_SHAPE, 13)
    plan, coef = tc.bad_rows()
    img, hot, wts = tc.np_sample(frames, labels, weights, plan, coef, (24, 24), 3)
    assert not img.any() and np.all(wts == 1) and hot[..., 0].all() and not hot[..., 1:].any()


def test_plan_is_seeded_with_inclusive_origins_and_the_float64_formula():
    a = tile_sample_plan((H, W), (24, 24), 3, 600, np.random.default_rng(7))
    b = tile_sample_plan((H, W), (24, 24), 3, 600, np.random.default_rng(7))
    c = tile_sample_plan((H, W), (24, 24), 3, 600, np.random.default_rng(8))
    plan, coef = a
    assert plan.dtype == np.int32 and plan.shape == (600, 4) and plan.flags['C_CONTIGUOUS']
    assert coef.dtype == np.float32 and coef.shape == (600, 6) and coef.flags['C_CONTIGUOUS']
    assert np.array_equal(plan, b[0]) and np.array_equal(coef, b[1]) and not np.array_equal(plan, c[0])
    assert set(plan[:, 0]) == {0, 1, 2} and not plan[:, 3].any()
    assert plan[:, 1].min() == 0 and plan[:, 1].max() == H - 24 and plan[:, 2].min() == 0 and plan[:, 2].max() == W - 24
    # the rows are rotations: recover the angle, then the offsets must be the float64 formula rounded once
    theta = np.arctan2(coef[:, 3].astype(np.float64), coef[:, 0].astype(np.float64))
    assert len(np.unique(np.round(theta, 3))) > 500 and theta.min() < -3 and theta.max() > 3
    assert np.array_equal(coef[:, 1], -coef[:, 3]) and np.array_equal(coef[:, 0], coef[:, 4])
    th = np.random.default_rng(3).uniform(0, 2 * np.pi, 50)
    p2, c2 = tile_sample_plan((H, W), (16, 40), 2, 50, np.random.default_rng(1), theta=th)
    assert np.array_equal(c2, tc.rotation_coef(th, (H, W)))
    assert p2[:, 1].max() <= H - 16 and p2[:, 2].max() <= W - 40
    # tiny ranges: both ends occur; an axis shorter than the tile has origin 0
    p3, c3 = tile_sample_plan((9, 8), (8, 12), 2, 400, np.random.default_rng(0), augment=())
    assert set(p3[:, 1]) == {0, 1} and set(p3[:, 2]) == {0}
    assert np.array_equal(c3, np.tile(np.asarray([1, 0, 0, 0, 1, 0], np.float32), (400, 1)))    # theta = 0: the identity
    assert covering_tiles((H, W), (24, 24)) == 4 and covering_tiles((H, W), (48, 48)) == 1
    assert covering_tiles((80, 96), (32, 32)) == 9


def test_flip_at_angle_zero_is_the_mirrored_crop_and_bad_augment_is_refused():
    frames = tc.random_frames(tc.FRAMES_SHAPE, np.float32, 14)
    tile = (16, 40)
    plan, coef = tile_sample_plan((H, W), tile, F, 64, np.random.default_rng(2), augment=('flip',))
    img, _, _ = tc.np_sample(frames, None, None, plan, coef, tile, 2)
    seen = set()
    for k in range(64):
        mx, my = coef[k, 0] < 0, coef[k, 4] < 0
        seen.add((bool(mx), bool(my)))
        crop = _zero_padded(frames[plan[k, 0]], plan[k, 1], plan[k, 2], tile)
        crop = crop[:, ::-1] if mx else crop
        crop = crop[::-1] if my else crop
        assert np.array_equal(img[k, ..., 0], crop), k
    assert len(seen) == 4
    # 'flip' composed with a rotation in float64: the mirrored tile of the unflipped row, up to the one rounding
    th = [0.3] * 8
    base = tc.rotation_coef(th, (H, W)).astype(np.float64)
    pf, cf = tile_sample_plan((H, W), tile, F, 8, np.random.default_rng(5), augment=('rotate', 'flip'), theta=th)
    for k in range(8):
        mx, my = np.sign(cf[k, 0]) != np.sign(base[k, 0]), np.sign(cf[k, 4]) != np.sign(base[k, 4])
        j, i = (tile[1] - 1 - 3 if mx else 3), (tile[0] - 1 - 2 if my else 2)
        x, y = float(pf[k, 2] + j), float(pf[k, 1] + i)
        want = base[k, 0] * x + base[k, 1] * y + base[k, 2], base[k, 3] * x + base[k, 4] * y + base[k, 5]
        x, y = float(pf[k, 2] + 3), float(pf[k, 1] + 2)
        got = cf[k].astype(np.float64)
        assert abs(got[0] * x + got[1] * y + got[2] - want[0]) < 1e-4 and abs(got[3] * x + got[4] * y + got[5] - want[1]) < 1e-4
    for bad in (('rot90',), 'mirror', ('rotate', 'zoom')):
        with pytest.raises(ValueError, match='augment'):
            tile_sample_plan((H, W), tile, F, 4, np.random.default_rng(0), augment=bad)
    with pytest.raises(ValueError):
        tile_sample_plan((H, W, 3), tile, F, 4, np.random.default_rng(0))
    with pytest.raises(ValueError):
        tile_sample_plan((H, W), tile, 0, 4, np.random.default_rng(0))
    with pytest.raises(ValueError):
        tile_sample_plan((H, W), tile, F, 0, np.random.default_rng(0))
    with pytest.raises(ValueError, match='theta'):
        tile_sample_plan((H, W), tile, F, 4, np.random.default_rng(0), theta=[0.1, 0.2])


def test_host_side_refusals_of_the_entry_point_need_no_gpu():
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15                     # any non-null aligned address: nothing is launched
    err = lib.sq_last_error
    dims = dict(F=2, H=37, W=45, TH=24, TW=24, C=2, count=4)

    def call(frames=p, mean=None, std=None, labels=p, weights=p, plan=p, coef=p, oi=p, oh=p, ow=p, dtype=1, **kw):
        t = dict(dims, **kw)
        return lib.sq_tile_sample_affine(frames, dtype, mean, std, labels, weights, plan, coef, oi, oh, ow,
                                         *([t[k] for k in ('F', 'H', 'W', 'TH', 'TW', 'C', 'count')] + [None]))

    for kw in (dict(plan=None), dict(coef=None), dict(frames=None), dict(oi=None), dict(labels=None), dict(oh=None),
               dict(weights=None), dict(ow=None), dict(frames=None, oi=None, labels=None, oh=None, weights=None, ow=None)):
        assert call(**kw) == -1 and b"null" in err() and b"sq_tile_sample_affine" in err(), kw
    assert call(mean=p) == -1 and b"both mean and std" in err()
    assert call(std=p) == -1 and b"both mean and std" in err()
    for bad in ('F', 'H', 'W', 'TH', 'TW'):
        for val in (0, -3):
            assert call(**{bad: val}) == -1 and b"positive" in err(), (bad, val)
    for C in (0, -1, 17):
        assert call(C=C) == -1 and b"classes" in err(), C
    for count in (0, -1, 65536):
        assert call(count=count) == -1 and b"count" in err(), count
    assert call(H=4097, W=4096) == -1 and b"2^24" in err()
    assert call(dtype=3) == -1 and b"pixel type 3" in err()
    assert call(dtype=-1) == -1 and b"pixel type" in err()
    assert call(frames=p + 1) == -1 and b"aligned" in err()    # uint16 pixels at an odd address
    assert call(ow=p + 2) == -1 and b"aligned" in err()
    assert call(coef=p + 2) == -1 and b"aligned" in err()


def test_job_tile_mode_refusals(tmp_path, monkeypatch):
    from sequitr_amd import jobs
    np.save(str(tmp_path / "im.npy"), np.zeros((2, 40, 48), np.uint16))
    np.save(str(tmp_path / "im64.npy"), np.zeros((2, 40, 48), np.float64))
    np.save(str(tmp_path / "im2c.npy"), np.zeros((2, 40, 48, 2), np.float32))
    np.save(str(tmp_path / "lab.npy"), np.zeros((2, 40, 48), np.uint8))
    np.save(str(tmp_path / "lab_hot.npy"), np.zeros((2, 40, 48, 2), np.uint8))
    np.save(str(tmp_path / "lab_bad.npy"), np.zeros((2, 40, 46), np.uint8))
    base = {'images': str(tmp_path / "im.npy"), 'labels': str(tmp_path / "lab.npy"), 'output': str(tmp_path),
            'num_outputs': 2, 'tile': (32, 32)}
    with pytest.raises(ValueError, match='one-hot'):
        jobs.SERVER_train(dict(base, labels=str(tmp_path / "lab_hot.npy")), {'gpu': 0})
    with pytest.raises(ValueError, match=r"\(TH, TW\)"):
        jobs.SERVER_train(dict(base, tile=(32, 32, 1)), {'gpu': 0})
    with pytest.raises(TypeError, match='uint8, uint16 or float32'):
        jobs.SERVER_train(dict(base, images=str(tmp_path / "im64.npy")), {'gpu': 0})
    with pytest.raises(ValueError, match='single-channel'):
        jobs.SERVER_train(dict(base, images=str(tmp_path / "im2c.npy")), {'gpu': 0})
    with pytest.raises(ValueError, match='do not match'):
        jobs.SERVER_train(dict(base, labels=str(tmp_path / "lab_bad.npy")), {'gpu': 0})
    with pytest.raises(ValueError, match='augment'):
        jobs.SERVER_train(dict(base, augment=('rot90',)), {'gpu': 0})
    with pytest.raises(ValueError, match='samples_per_epoch'):
        jobs.SERVER_train(dict(base, samples_per_epoch=0), {'gpu': 0})
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(RuntimeError, match='WORLD_SIZE'):       # before anything is read or uploaded
        jobs.SERVER_train(dict(base, images=str(tmp_path / "missing.npy")), {'gpu': 0})
