"""CPU: the host half of the volume sampler -- frontend.sample_plan, the numpy restatement of the sampling definition
(tests/volume_sampler_cases.py) against itself, and the host-side refusals of the three entry points and of the job's
brick mode.  Nothing here launches a kernel."""
import ctypes

import numpy as np
import pytest

from sequitr_amd import _lib
from sequitr_amd.frontend import sample_plan
from tests import volume_sampler_cases as sc


def test_sample_plan_is_seeded_and_stays_inside():
    shape, brick = (19, 37, 45), (8, 16, 16)
    a = sample_plan(shape, brick, 3, 500, np.random.default_rng(7))
    b = sample_plan(shape, brick, 3, 500, np.random.default_rng(7))
    c = sample_plan(shape, brick, 3, 500, np.random.default_rng(8))
    assert a.dtype == np.int32 and a.shape == (500, 5) and a.flags['C_CONTIGUOUS']
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert a[:, 0].min() == 0 and a[:, 0].max() == 2
    for ax in range(3):
        assert a[:, 1 + ax].min() >= 0 and a[:, 1 + ax].max() <= shape[ax] - brick[ax]
    assert a[:, 4].min() >= 0 and a[:, 4].max() <= 15


def test_sample_plan_reaches_both_extremes_and_every_op():
    """a tiny volume, a few thousand draws: origin 0 and the LAST origin L - T occur on every axis (ImageSample.update
    never draws the last one), an axis with L == T is sampled at origin 0, and all 16 ops occur"""
    shape, brick = (6, 9, 8), (4, 8, 8)
    p = sample_plan(shape, brick, 2, 4000, np.random.default_rng(0))
    assert set(p[:, 1]) == {0, 1, 2} and set(p[:, 2]) == {0, 1} and set(p[:, 3]) == {0}
    assert set(p[:, 4]) == set(range(16)) and set(p[:, 0]) == {0, 1}
    assert set(sample_plan(shape, brick, 2, 4000, np.random.default_rng(0), augment=('flip',))[:, 4]) == set(range(8))
    assert set(sample_plan(shape, brick, 2, 4000, np.random.default_rng(0), augment=('rot90',))[:, 4]) == {0, 8}
    assert set(sample_plan(shape, brick, 2, 4000, np.random.default_rng(0), augment='flip')[:, 4]) == set(range(8))


def test_sample_plan_without_augmentation_short_axes_and_refusals():
    p = sample_plan((5, 37, 45), (8, 16, 18), 1, 300, np.random.default_rng(1), augment=())
    assert not p[:, 4].any() and not p[:, 0].any()
    assert not p[:, 1].any()                                    # Z = 5 is shorter than the brick: origin 0, the box is padded
    assert p[:, 2].max() > 0 and p[:, 3].max() > 0
    assert set(sample_plan((5, 37, 45), (8, 16, 18), 1, 300, np.random.default_rng(1), augment=('flip',))[:, 4]) == set(range(8))
    with pytest.raises(ValueError, match='square'):
        sample_plan((19, 37, 45), (8, 16, 18), 1, 4, np.random.default_rng(0))           # the default asks for 'rot90'
    with pytest.raises(ValueError, match='square'):
        sample_plan((19, 37, 45), (8, 16, 18), 1, 4, np.random.default_rng(0), augment=('rot90',))
    with pytest.raises(ValueError, match='augment'):
        sample_plan((19, 37, 45), (8, 16, 16), 1, 4, np.random.default_rng(0), augment=('rotate',))
    with pytest.raises(ValueError):
        sample_plan((19, 37), (8, 16), 1, 4, np.random.default_rng(0))
    with pytest.raises(ValueError):
        sample_plan((19, 37, 45), (8, 16, 16), 0, 4, np.random.default_rng(0))
    with pytest.raises(ValueError):
        sample_plan((19, 37, 45), (8, 16, 16), 1, 0, np.random.default_rng(0))


def test_restatement_ops_are_a_group_of_16_and_invert():
    """np_unapply(np_apply(box)) is the box for every op; the 16 ops give 16 different arrangements of an asymmetric box,
    the in-plane quarter turns (np.rot90 in the (x, y) plane) among them"""
    box = np.arange(3 * 5 * 5, dtype=np.int32).reshape(3, 5, 5)
    seen = set()
    for op in range(16):
        out = sc.np_apply(box, op)
        assert np.array_equal(sc.np_unapply(out, op), box)
        seen.add(np.ascontiguousarray(out).tobytes())
    assert len(seen) == 16
    for k in (1, 2, 3):
        turned = np.ascontiguousarray(np.rot90(box, k, axes=(1, 2))).tobytes()
        assert any(np.ascontiguousarray(sc.np_apply(box, op)).tobytes() == turned for op in range(16) if not op & 1)
    with_tail = np.arange(3 * 4 * 4 * 2).reshape(3, 4, 4, 2)   # a trailing class axis rides along untouched
    for op in range(16):
        assert np.array_equal(sc.np_apply(with_tail, op)[..., 1], sc.np_apply(with_tail[..., 1], op))
    flat = np.arange(2 * 3 * 4).reshape(2, 3, 4)
    assert np.array_equal(sc.np_apply(flat, 5), flat[::-1, :, ::-1])                    # the flips need no square box


def test_restatement_crop_pads_coordinate_by_coordinate():
    vols = np.arange(2 * 5 * 6 * 7, dtype=np.float32).reshape(2, 5, 6, 7) + 1          # no zero inside
    brick = (4, 3, 3)
    assert np.array_equal(sc.np_crop(vols, [1, 1, 2, 3, 0], brick), vols[1, 1:5, 2:5, 3:6])
    box = sc.np_crop(vols, [0, 3, -1, 5, 0], brick)            # leaves the volume at z >= 5, x < 0 and y >= 7
    assert np.array_equal(box[:2, 1:, :2], vols[0, 3:5, 0:2, 5:7])
    assert not box[2:].any() and not box[:, 0].any() and not box[:, :, 2].any()
    for row in ([2, 0, 0, 0, 0], [-1, 0, 0, 0, 0], [0, 5, 0, 0, 0], [0, 0, -3, 0, 0], [0, 0, 0, 7, 0]):
        assert not sc.np_crop(vols, row, brick).any()
    outside, straddle = sc.hostile_plan(sc.VOL_SHAPE, (8, 16, 16))
    v = np.ones(sc.VOL_SHAPE, np.uint8)
    assert not sc.np_copy(v, outside, (8, 16, 16)).any()
    part = sc.np_copy(v, straddle, (8, 16, 16)).reshape(len(straddle), -1)
    assert np.all(part.any(1)) and not np.any(part.all(1))      # every straddling row holds voxels and fill
    lab = np.array([0, 1, 2, 3], np.uint8).reshape(1, 1, 2, 2)
    oh = sc.np_onehot(lab, 3, np.asarray([[0, 0, 0, 0, 0]], np.int32), (1, 2, 2))
    assert oh.shape == (1, 1, 2, 2, 3) and oh[0, 0, 1, 1].sum() == 0 and oh[0, 0, 1, 0, 2] == 1 and oh.sum() == 3


def test_host_side_refusals_of_the_entry_points_need_no_gpu():
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15                     # any non-null aligned address: nothing is launched
    err = lib.sq_last_error
    dims = dict(V=2, Z=19, X=37, Y=45, BZ=8, BX=16, BY=16, count=4, allow=1)

    def d(**kw):
        t = dict(dims, **kw)
        return [t[k] for k in ('V', 'Z', 'X', 'Y', 'BZ', 'BX', 'BY', 'count', 'allow')] + [None]

    calls = {
        'sq_volume_sample_f32': lambda a, pl, o, dm: lib.sq_volume_sample_f32(a, 1, None, None, pl, o, *dm),
        'sq_volume_sample_copy': lambda a, pl, o, dm: lib.sq_volume_sample_copy(a, 4, pl, o, *dm),
        'sq_volume_sample_onehot_u8': lambda a, pl, o, dm: lib.sq_volume_sample_onehot_u8(a, 2, pl, o, *dm),
    }
    for name, call in calls.items():
        for args in ((None, p, p), (p, None, p), (p, p, None)):
            assert call(*args, d()) == -1 and b"null" in err() and name.encode() in err(), name
        for bad in ('V', 'Z', 'X', 'Y', 'BZ', 'BX', 'BY'):
            for val in (0, -3):
                assert call(p, p, p, d(**{bad: val})) == -1 and b"positive" in err(), (name, bad)
        assert call(p, p, p, d(count=0)) == -1 and b"count" in err()
        assert call(p, p, p, d(count=65536)) == -1 and b"count" in err()
        assert call(p, p, p, d(BZ=65536)) == -1 and b"out of range" in err()
        assert call(p, p, p, d(BY=18)) == -1 and b"square" in err() and b"BX=16 BY=18" in err()
        assert call(p, p, p, d(BX=12, BY=24)) == -1 and b"square" in err()
    f32 = lib.sq_volume_sample_f32
    assert f32(p, 3, None, None, p, p, *d()) == -1 and b"voxel type 3" in err()
    assert f32(p, -1, None, None, p, p, *d()) == -1 and b"voxel type" in err()
    assert f32(p, 1, p, None, p, p, *d()) == -1 and b"both mean and std" in err()
    assert f32(p, 1, None, p, p, p, *d()) == -1 and b"both mean and std" in err()
    assert f32(p + 1, 1, None, None, p, p, *d()) == -1 and b"aligned" in err()        # uint16 voxels at an odd address
    assert f32(p, 0, None, None, p, p + 2, *d()) == -1 and b"aligned" in err()
    for nbytes in (0, -1, 5, 6, 7, 9, 16):
        assert lib.sq_volume_sample_copy(p, nbytes, p, p, *d()) == -1 and b"elem_bytes" in err(), nbytes
    assert lib.sq_volume_sample_copy(p + 2, 4, p, p, *d()) == -1 and b"aligned" in err()
    assert lib.sq_volume_sample_copy(p, 8, p, p + 4, *d()) == -1 and b"aligned" in err()
    for C in (0, -2, 17):
        assert lib.sq_volume_sample_onehot_u8(p, C, p, p, *d()) == -1 and b"classes" in err(), C


def test_job_brick_mode_refusals(tmp_path):
    from sequitr_amd import jobs
    np.save(str(tmp_path / "im.npy"), np.zeros((1, 8, 32, 32), np.uint16))
    np.save(str(tmp_path / "im64.npy"), np.zeros((1, 8, 32, 32), np.float64))
    np.save(str(tmp_path / "im2c.npy"), np.zeros((1, 8, 32, 32, 2), np.float32))
    np.save(str(tmp_path / "lab.npy"), np.zeros((1, 8, 32, 32), np.uint8))
    np.save(str(tmp_path / "lab_bad.npy"), np.zeros((1, 8, 32, 30), np.uint8))
    base = {'images': str(tmp_path / "im.npy"), 'labels': str(tmp_path / "lab.npy"), 'output': str(tmp_path),
            'num_outputs': 2, 'brick': (16, 16, 8)}
    with pytest.raises(ValueError, match="weightmap"):
        jobs.SERVER_train_volume(dict(base, weightmap='delaunay'), {'gpu': 0})
    with pytest.raises(ValueError, match=r"\(X, Y, Z\)"):
        jobs.SERVER_train_volume(dict(base, brick=(16, 16)), {'gpu': 0})
    with pytest.raises(TypeError, match='uint8, uint16 or float32'):
        jobs.SERVER_train_volume(dict(base, images=str(tmp_path / "im64.npy")), {'gpu': 0})
    with pytest.raises(ValueError, match='single-channel'):
        jobs.SERVER_train_volume(dict(base, images=str(tmp_path / "im2c.npy")), {'gpu': 0})
    with pytest.raises(ValueError, match='square'):
        jobs.SERVER_train_volume(dict(base, brick=(16, 24, 8), augment=('flip', 'rot90')), {'gpu': 0})
    with pytest.raises(ValueError, match='augment'):
        jobs.SERVER_train_volume(dict(base, augment=('rotate',)), {'gpu': 0})
    with pytest.raises(ValueError, match='samples_per_epoch'):
        jobs.SERVER_train_volume(dict(base, samples_per_epoch=0), {'gpu': 0})
    with pytest.raises(ValueError, match='do not match'):
        jobs.SERVER_train_volume(dict(base, labels=str(tmp_path / "lab_bad.npy")), {'gpu': 0})
