"""CPU: what the object measurements (sequitr_amd/objects.py, include/sequitr_hip.h "Object measurements") promise without
a GPU -- the scipy restatement agrees with an independent flood fill, the host-side checks of the new entry points fail
loudly before any launch, and ObjectTable orders, ranks and derives its columns as documented."""
import math
from fractions import Fraction

import numpy as np
import pytest

from sequitr_amd import _lib, frontend, objects
from tests import objects_cases as oc


def _compare_with_flood(mask):
    ref = oc.objects_ref(mask)
    rows = oc.flood_objects(mask)
    assert ref['found'] == len(rows) == len(ref['frame'])
    for k, row in enumerate(rows):
        f, v, key, area = row[:4]
        assert (ref['frame'][k], ref['cls'][k], ref['key'][k], ref['area'][k]) == (f, v, key, area), (k, row)
        assert tuple(ref['bbox'][k]) == row[4:10], (k, row)
        for a in range(3):                                      # centre = c * sum / (c * area), exact integers below 2^53
            assert ref['centroid'][k][a] == (v * row[10 + a]) / (v * area), (k, a)
        assert ref['label'][k] == 1 + sum(1 for r in rows[:k] if r[0] == f)


def test_restatement_agrees_with_flood_fill():
    rng = np.random.default_rng(0)
    for h, w in ((1, 1), (1, 12), (12, 1), (7, 9), (12, 12)):
        _compare_with_flood((rng.random((2, h, w)) < 0.55).astype(np.uint8))
        _compare_with_flood(rng.integers(0, 4, (2, h, w)).astype(np.uint8))
    _compare_with_flood(oc.disks(3, 2, 12, 12, 4, classes=2, rmax=4))
    _compare_with_flood(np.zeros((1, 5, 5), np.uint8))
    _compare_with_flood((rng.random((2, 3, 5, 7)) < 0.4).astype(np.uint8))
    _compare_with_flood(rng.integers(0, 3, (1, 3, 5, 7)).astype(np.uint8))
    _compare_with_flood(oc.sized_objects())


def test_restatement_filter_and_labels():
    m = oc.sized_objects()
    ref = oc.objects_ref(m, min_area=3, max_area=7)
    assert sorted(ref['area']) == [3, 4, 5, 6, 7] and ref['found'] == 9
    assert sorted(np.unique(ref['labels'])) == [0, 1, 2, 3, 4, 5]
    assert np.array_equal(ref['mask'] != 0, ref['labels'] != 0) and np.array_equal(ref['mask'][ref['mask'] != 0], m[ref['mask'] != 0])
    assert (m != 0).sum() - (ref['mask'] != 0).sum() == 1 + 2 + 8 + 9


def test_workspace_sizes():
    lib = _lib.load()
    assert lib.sq_objects_workspace(1, 1, 1, 1, 1) == 96 + 8   # one 88-byte record rounded to 16, 8 B per pixel
    assert lib.sq_objects_workspace(8, 1, 2048, 2048, 1 << 16) == 8 * 8 * 2048 * 2048 + 88 * (1 << 16)
    assert lib.sq_objects_workspace(2, 5, 9, 70, 3) == 2 * 5 * 9 * 70 * 8 + 272
    assert lib.sq_objects_workspace(1, 1, 1 << 16, 1 << 15, 16) == -1          # 2^31 elements
    assert lib.sq_objects_workspace(1, 2, 1 << 15, (1 << 15) - 1, 16) > 0      # just below
    for bad in ((0, 1, 4, 4, 4), (1, 0, 4, 4, 4), (1, 1, 0, 4, 4), (1, 1, 4, 0, 4), (1, 1, 4, 4, 0)):
        assert lib.sq_objects_workspace(*bad) == -1


P = 4096                                                         # a non-null, 16-byte aligned stand-in: never dereferenced


def _measure(lib, mask=P, dims=(1, 1, 8, 8), image=None, dtype=0, lo=1, hi=0, ws=P, count=P, found=P, ri=P, rf=P, slots=P,
             max_out=16):
    return lib.sq_objects_measure(mask, *dims, image, dtype, lo, hi, ws, count, found, ri, rf, slots, max_out, None)


def test_measure_host_side_validation():
    lib = _lib.load()
    for kw in ({'mask': None}, {'ws': None}, {'count': None}, {'found': None}, {'ri': None}, {'rf': None}, {'slots': None}):
        assert _measure(lib, **kw) == -1 and b"null pointer" in lib.sq_last_error(), kw
    assert _measure(lib, image=P, dtype=3) == -1 and b"dtype" in lib.sq_last_error()
    assert _measure(lib, image=P, dtype=-1) == -1 and b"dtype" in lib.sq_last_error()
    assert _measure(lib, lo=0) == -1 and b"min_area" in lib.sq_last_error()
    assert _measure(lib, max_out=0) == -1 and b"max_out" in lib.sq_last_error()
    assert _measure(lib, dims=(1, 1, 1 << 16, 1 << 15)) == -1 and b"2^31" in lib.sq_last_error()
    assert _measure(lib, dims=(2, 1 << 15, 1 << 15, 1)) == -1 and b"2^31" in lib.sq_last_error()
    assert _measure(lib, dims=(1, 1, 0, 8)) == -1 and b"2^31" in lib.sq_last_error()
    assert _measure(lib, ws=P + 8) == -1 and b"16-byte aligned" in lib.sq_last_error()


def test_relabel_host_side_validation():
    lib = _lib.load()

    def relabel(mask=P, dims=(1, 1, 8, 8), ws=P, rank=P, n_slots=16, labels=P, mask_out=P):
        return lib.sq_objects_relabel(mask, *dims, ws, rank, n_slots, labels, mask_out, None)

    for kw in ({'mask': None}, {'ws': None}, {'rank': None}):
        assert relabel(**kw) == -1 and b"null pointer" in lib.sq_last_error(), kw
    assert relabel(labels=None, mask_out=None) == -1 and b"both NULL" in lib.sq_last_error()
    assert relabel(dims=(1, 1, 1 << 16, 1 << 15)) == -1 and b"2^31" in lib.sq_last_error()
    assert relabel(ws=P + 4) == -1 and b"16-byte aligned" in lib.sq_last_error()
    # a workspace no measure call has filled: there is nothing n_slots could match
    assert relabel(ws=P + 4096, n_slots=16) == -1 and b"n_slots" in lib.sq_last_error()
    assert relabel(labels=None) == -1 and b"n_slots" in lib.sq_last_error()      # one output is enough to get this far


def _rows(objs, with_image=True):
    """hand-made rows of include/sequitr_hip.h from (frame, class, key, area, isum, isumsq, imin, imax)"""
    ri = np.zeros((len(objs), 12), np.int64)
    rf = np.zeros((len(objs), 7), np.float64)
    for k, (f, c, key, area, s, q, lo, hi) in enumerate(objs):
        ri[k, :4] = (f, c, key, area)
        ri[k, 4:10] = (0, key // 100, key % 100, 1, key // 100 + 1, key % 100 + area)
        rf[k, :3] = (0.0, key // 100, key % 100 + (area - 1) / 2)
        if with_image:
            ri[k, 10], ri[k, 11] = s, q
            rf[k, 3:] = (float(s), float(q), lo, hi)
    return ri, rf


_PIX7 = (3, 65535, 65535, 40000, 12, 999, 65534)                # the seven pixels of the object at key 950
OBJS = [(1, 2, 40, 3, 30, 302, 9, 11), (0, 2, 7, 1, 65535, 65535 ** 2, 65535, 65535), (1, 1, 300, 2, 5, 13, 2, 3),
        (0, 1, 950, 7, sum(_PIX7), sum(x * x for x in _PIX7), 3, 65535), (1, 1, 12, 5, 50, 510, 8, 12), (0, 1, 3, 4, 10, 30, 1, 4),
        (2, 3, 0, 90000, 65535 * 90000, 65535 ** 2 * 90000, 65535, 65535)]


def test_object_table_order_ranks_and_coords():
    ri, rf = _rows(OBJS)
    t = objects.ObjectTable(ri, rf, 4, image_dtype=np.uint16)
    want = sorted(range(len(OBJS)), key=lambda k: OBJS[k][:3])
    assert list(t.order) == want
    assert list(t.frame) == [0, 0, 0, 1, 1, 1, 2] and list(t.cls) == [1, 1, 2, 1, 1, 2, 3]
    assert list(t.key) == [3, 950, 7, 12, 300, 40, 0] and list(t.label) == [1, 2, 3, 1, 2, 3, 1]
    assert t.area.dtype == np.int64 and t.bbox.shape == (7, 6) and t.centroid.dtype == np.float64
    assert t.intensity_sum.dtype == np.int64 and t.intensity_min.dtype == np.int64 and list(t.intensity_max[:3]) == [4, 65535, 65535]
    per = t.frames()
    assert [len(p) for p in per] == [3, 3, 1, 0] and list(per[1].key) == [12, 300, 40] and list(per[1].label) == [1, 2, 3]
    coords = t.coords()
    assert [c.shape for c in coords] == [(3, 5), (3, 5), (1, 5), (0, 5)] and all(c.dtype == np.float32 for c in coords)
    assert list(coords[0][1]) == [0.0, 9.0, 53.0, 0.0, 1.0]                   # [frame, row, column, 0, class]
    assert np.array_equal(per[0].coords()[0], coords[0])
    cols = t.columns()
    assert set(cols) >= {'frame', 'cls', 'key', 'area', 'bbox', 'centroid', 'label', 'intensity_sum', 'intensity_sumsq',
                         'intensity_min', 'intensity_max', 'mean_intensity', 'std_intensity'}
    # volumetric: the three centres in order; no image: no intensity columns
    rf[:, 0] = np.arange(len(OBJS)) + 0.5
    v = objects.ObjectTable(ri, rf, 3, volumetric=True)
    k = want[0]
    assert list(v.coords()[0][0]) == [0.0, k + 0.5, rf[k, 1], rf[k, 2], 1.0]
    assert v.intensity_sum is None and v.mean_intensity is None and 'intensity_sum' not in v.columns()
    empty = objects.ObjectTable(np.zeros((0, 12)), np.zeros((0, 7)), 2)
    assert len(empty) == 0 and [c.shape for c in empty.coords()] == [(0, 5), (0, 5)] and len(empty.frames()) == 2


def test_object_table_mean_and_std_intensity():
    ri, rf = _rows(OBJS)
    t = objects.ObjectTable(ri, rf, 3, image_dtype=np.uint16)
    mean, var, std = t.mean_intensity, t.var_intensity, t.std_intensity
    assert mean.dtype == np.float64 and std.dtype == np.float64
    for pos, k in enumerate(t.order):
        _, _, _, area, s, q, _, _ = OBJS[k]
        assert mean[pos] == s / area                            # Python's correctly rounded int / int
        exact = Fraction(q, area) - Fraction(s, area) ** 2
        assert exact >= 0 and var[pos] >= 0.0 and std[pos] == math.sqrt(var[pos])
        # four float64 roundings of terms no larger than sumsq / area, doubled
        assert abs(Fraction(float(var[pos])) - exact) <= Fraction(8 * q, area) / 2 ** 53, (k, var[pos], float(exact))
    by_key = {OBJS[k][2]: (var[pos], std[pos]) for pos, k in enumerate(t.order)}
    assert by_key[7] == (0.0, 0.0)                               # area 1
    assert by_key[0][0] >= 0.0 and by_key[0][0] <= 8 * 65535.0 ** 2 * 2.0 ** -53   # 300 x 300 pixels of 65535: never negative
    f = objects.ObjectTable(ri, rf, 3, image_dtype=np.float32)
    assert f.intensity_sum.dtype == np.float64 and f.intensity_sum[0] == 10.0 and f.intensity_max[0] == 4.0


def test_segment_frames_refuses_two_sinks():
    with pytest.raises(ValueError, match='on_masks and on_batch'):
        frontend.segment_frames(None, None, on_masks=lambda *a: None, on_batch=lambda *a: None)
