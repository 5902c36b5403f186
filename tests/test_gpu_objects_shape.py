"""Shape columns on the GPU (sq_objects_shape, objects.measure_objects(shape=True)) against the scipy restatement of
tests/objects_shape_cases.py: every one of the 16 integer columns of every row equal, after sorting both by
(frame, class, key)."""
import numpy as np
import pytest
import torch

from sequitr_amd import _lib, objects
from tests import objects_shape_cases as sc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OLD = ('frame', 'cls', 'key', 'area', 'bbox', 'centroid', 'label')


def check(mask, min_area=1, max_area=None):
    """all 16 columns of all rows against the restatement; returns (table, reference)"""
    mask = np.ascontiguousarray(mask)
    ref = sc.shape_ref(mask, min_area, max_area)
    t = objects.measure_objects(torch.from_numpy(mask).to(DEV), min_area=min_area, max_area=max_area, shape=True)
    assert len(t) == len(ref['key']), (len(t), len(ref['key']))
    for name in ('frame', 'cls', 'key', 'area'):
        assert np.array_equal(getattr(t, name), ref[name]), name
    got = t._shape_rows()
    assert got.dtype == np.int64 and got.shape == ref['shape'].shape
    bad = np.argwhere(got != ref['shape'])
    assert len(bad) == 0, [(int(i), sc.NAMES[j], int(got[i, j]), int(ref['shape'][i, j])) for i, j in bad[:6]]
    assert np.array_equal(t.coord_sums, got[:, 0:3]) and np.array_equal(t.moments2, got[:, 3:9])
    assert np.array_equal(t.faces, got[:, 9:12]) and np.array_equal(t.boundary, got[:, 12])
    assert np.array_equal(t.perimeter_counts, got[:, 13:16])
    return t, ref


@pytest.mark.parametrize("W", [1, 2, 3, 63, 64, 65, 127, 128, 129, 130, 200])
def test_every_column_across_the_segment_width(W):
    for H in (1, 2, 5, 33):
        check(sc.noise(W * 7 + H, (2, H, W), 3))
        check(sc.noise(W * 5 + H, (1, H, W), 1, fill=0.62))     # one class near percolation: winding objects, many corners
        check(sc.disks(W + H, 2, H, W, 6, classes=2, rmax=7))


@pytest.mark.parametrize("H", [sc.PT_H - 1, sc.PT_H, sc.PT_H + 1, 2 * sc.PT_H + 1])
def test_every_column_across_the_perimeter_tile(H):
    for W in (sc.PT_W - 1, sc.PT_W, sc.PT_W + 1, 2 * sc.PT_W + 1):
        check(sc.noise(H * 3 + W, (1, H, W), 1, fill=0.62))
        check(sc.noise(H + W, (2, H, W), 2, fill=0.8))
        check(np.ones((1, H, W), np.uint8))


def test_runs_on_each_side_of_the_seams():
    t, _ = check(sc.seam_runs())
    assert np.all(t.faces[:, 2] == 2) and np.array_equal(t.faces[:, 1], 2 * t.area)   # one run each: two ends, never a seam
    check(np.ones((2, 3, 200), np.uint8))


def test_one_pixel_objects_and_the_checkerboard(monkeypatch):
    m = sc.checkerboard(33, 65)
    t, _ = check(m)
    assert len(t) == 33 * 65 and np.all(t.area == 1)
    assert np.all(t.faces == [0, 2, 2]) and np.all(t.boundary == 1) and np.all(t.perimeter_counts == 0)
    assert np.all(t.perimeter == 0.0) and np.all(t.circularity == 0.0) and np.all(t.crack_perimeter == 4.0)
    monkeypatch.setattr(objects, "_MAX_OUT", 16)                # found > max_out at first: the retry's workspace feeds the shape call
    t2, _ = check(m)
    assert t2.found == 33 * 65
    check(sc.noise(3, (2, 9, 70), 3, fill=0.08))                # sparse: mostly single pixels


def test_diagonal_strangers_and_the_long_way_round():
    t, ref = check(sc.diagonal_strangers())
    assert list(t.area[:2]) == [1, 1] and np.all(t.perimeter_counts[:2] == 0)       # strangers do not see each other
    for m in (sc.spiral(33, 70), sc.comb(33, 70)):
        t, _ = check(m)
        assert len(t) == 1
    check(np.concatenate([sc.spiral(33, 70, 1), sc.comb(33, 70), sc.spiral(33, 70, 3)[:, ::-1].copy()]))
    check(sc.walls())


def test_edges_corners_and_neighbouring_frames():
    check(sc.flush())
    t, _ = check(sc.stacked_frames())
    assert len(t) == 3 and np.array_equal(t.faces[0], t.faces[2]) and np.array_equal(t.moments2[0], t.moments2[1])
    one = sc.noise(4, (1, 6, 66), 2)
    t, _ = check(np.repeat(one, 3, axis=0))                     # the same frame three times: the same rows three times
    per = t.frames()
    assert np.array_equal(per[0]._shape_rows(), per[1]._shape_rows()) and np.array_equal(per[0]._shape_rows(), per[2]._shape_rows())
    v, _ = check(sc.stacked_volumes())
    assert len(v) == 2 and np.array_equal(v._shape_rows()[0], v._shape_rows()[1])


def test_perimeter_tile_seams_and_corners():
    m = sc.tile_seams()
    check(m)
    check(m[:, ::-1, ::-1])
    check(np.swapaxes(sc.tile_seams(2 * sc.PT_W + 7, 2 * sc.PT_H + 6), 1, 2))       # transposed: other pixels meet the seams


@pytest.mark.parametrize("planes", [1, 2, 3, 9])
def test_volumes(planes):
    m = sc.blobs3d(planes, 2, planes, 33, 70, 12, classes=2, rmax=5)
    t, ref = check(m)
    assert t.volumetric
    check(sc.noise(planes, (2, planes, 5, 66), 2))
    check(sc.noise(planes + 1, (1, planes, 9, 65), 1, fill=0.5))
    if planes == 1:                                             # the planar result, the three perimeter columns present
        flat, _ = check(m[:, 0])
        assert np.array_equal(flat._shape_rows(), t._shape_rows()) and t.perimeter_counts.sum() > 0
        assert t.perimeter is None and 'perimeter_counts' in t.columns()
    else:
        assert np.all(t.perimeter_counts == 0) and t.faces[:, 0].min() >= 2


def test_balls_plates_and_a_shell():
    t, _ = check(sc.plates_and_shell())
    shell = int(np.flatnonzero(t.area == 7 ** 3 - 5 ** 3)[0])
    assert t.faces[shell].tolist() == [2 * 49 + 2 * 25] * 3 and t.boundary[shell] == 7 ** 3 - 5 ** 3
    b, _ = check(np.concatenate([sc.ball(9), sc.ball(9, cls=2)]))
    assert np.array_equal(b._shape_rows()[0], b._shape_rows()[1]) and b.faces[0, 0] == b.faces[0, 1] == b.faces[0, 2]


def test_far_object_needs_64_bit_sums():
    t, _ = check(sc.far_object())
    assert len(t) == 1 and t.coord_sums[0, 1:].min() > 2 ** 27 and t.moments2[0, [1, 2, 5]].min() > 2 ** 38   # far beyond 32 bits
    want = np.cov((np.argwhere(sc.far_object()[0]) - [1700, 1710]).T, bias=True)   # box-relative: nothing to cancel
    assert np.abs(t.covariance()[0] - want).max() <= 1e-12 * (np.trace(want) + 1.0)   # exact integers: none here either


@pytest.mark.parametrize("lo,hi,kept", [(3, 7, [3, 4, 5, 6, 7]), (9, None, [9]), (2, 2, [2])])
def test_rows_follow_slots_behind_the_size_filter(lo, hi, kept):
    t, _ = check(sc.sized_objects(), min_area=lo, max_area=hi)
    assert sorted(t.area) == kept and t.found == 9


def test_shape_false_is_the_table_of_before():
    m = sc.disks(8, 3, 60, 150, 20, classes=2)
    md = torch.from_numpy(m).to(DEV)
    img = torch.from_numpy(np.random.default_rng(0).integers(0, 65536, m.shape).astype(np.uint16)).to(DEV)
    plain = objects.measure_objects(md, image=img, labels=True, filtered_mask=True, min_area=5)
    same = objects.measure_objects(md, image=img, labels=True, filtered_mask=True, min_area=5, shape=False)
    full = objects.measure_objects(md, image=img, labels=True, filtered_mask=True, min_area=5, shape=True)
    keys = list(OLD) + ['intensity_sum', 'intensity_sumsq', 'intensity_min', 'intensity_max', 'mean_intensity', 'std_intensity']
    assert list(plain.columns()) == list(same.columns()) == keys and not plain.with_shape and plain.moments2 is None
    assert set(keys) < set(full.columns()) and full.with_shape
    for k in keys:
        for other in (same, full):
            a, b = plain.columns()[k], other.columns()[k]
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b), k
    assert torch.equal(plain.labels, full.labels) and torch.equal(plain.mask, full.mask) and plain.found == full.found
    assert np.array_equal(full._shape_rows(), sc.shape_ref(m, min_area=5)['shape'])


# ---- the C ABI by hand ---------------------------------------------------------------------------------------------------
class Measured(object):
    """one sq_objects_measure call by hand: what sq_objects_shape reads"""

    def __init__(self, mask, max_out=64, min_area=1):
        self.lib = _lib.load()
        self.mask = torch.from_numpy(np.ascontiguousarray(mask)).to(DEV)
        m4 = mask if mask.ndim == 4 else mask[:, None]
        self.dims = tuple(int(s) for s in m4.shape)
        self.max_out = max_out
        self.ws = torch.empty(self.lib.sq_objects_workspace(*self.dims, max_out) // 4, dtype=torch.int32, device=DEV)
        self.ctr = torch.zeros(2, dtype=torch.int32, device=DEV)
        self.rows_i = torch.empty((max_out, 12), dtype=torch.int64, device=DEV)
        self.rows_f = torch.empty((max_out, 7), dtype=torch.float64, device=DEV)
        self.slots = torch.empty(max_out, dtype=torch.int32, device=DEV)
        _lib.check(self.lib.sq_objects_measure(self.mask.data_ptr(), *self.dims, None, 0, min_area, 0, self.ws.data_ptr(),
                                               self.ctr.data_ptr(), self.ctr[1:].data_ptr(), self.rows_i.data_ptr(),
                                               self.rows_f.data_ptr(), self.slots.data_ptr(), max_out,
                                               torch.cuda.current_stream().cuda_stream), "sq_objects_measure")
        self.n, self.found = (int(v) for v in self.ctr.cpu().numpy())
        assert self.found <= max_out
        self.sbytes = int(self.lib.sq_objects_shape_workspace(max_out))
        self.sws = torch.full((self.sbytes // 4 + 8,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)     # 32 guard bytes behind
        self.out = torch.full((self.n + 2, 16), -77, dtype=torch.int64, device=DEV)                   # two guard rows behind

    def shape(self, **kw):
        a = dict(mask=self.mask.data_ptr(), dims=self.dims, ws=self.ws.data_ptr(), n_slots=self.max_out,
                 slots=self.slots.data_ptr(), n=self.n, sws=self.sws.data_ptr(), out=self.out.data_ptr())
        a.update(kw)
        return self.lib.sq_objects_shape(a['mask'], *a['dims'], a['ws'], a['n_slots'], a['slots'], a['n'], a['sws'], a['out'],
                                         torch.cuda.current_stream().cuda_stream)

    def sorted_rows(self):
        ri = self.rows_i[:self.n].cpu().numpy()
        return self.out[:self.n].cpu().numpy()[np.lexsort((ri[:, 2], ri[:, 1], ri[:, 0]))]


def test_guards_twice_and_graph_replay():
    m = np.concatenate([sc.tile_seams()[:1, :40, :70], sc.noise(2, (1, 40, 70), 2, fill=0.6)])
    c = Measured(m, max_out=1024)
    ref = sc.shape_ref(m)['shape']
    assert c.sbytes == (1024 * 104 + 15) // 16 * 16 and c.lib.sq_objects_shape_workspace(0) == -1
    assert c.lib.sq_objects_shape_workspace(3) == 320
    _lib.check(c.shape(), "sq_objects_shape")
    first = c.out.clone()
    assert np.array_equal(c.sorted_rows(), ref)
    assert torch.all(c.out[c.n:] == -77) and torch.all(c.sws[c.sbytes // 4:] == 0x5A5A5A5A)
    c.out[:c.n].fill_(-1)
    _lib.check(c.shape(), "sq_objects_shape")                   # twice: the same bits, whatever the workspace held
    assert torch.equal(c.out, first)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        _lib.check(c.shape(), "sq_objects_shape")               # warm up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _lib.check(c.shape(), "sq_objects_shape")
    for _ in range(2):
        c.out[:c.n].fill_(-1)
        c.sws[:c.sbytes // 4].fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(c.out, first)
    assert torch.all(c.sws[c.sbytes // 4:] == 0x5A5A5A5A)


def test_nothing_to_write_and_refusals():
    m = sc.disks(2, 2, 20, 70, 5, classes=2)
    c = Measured(m)
    assert c.n > 2
    before = c.out.clone()
    assert c.shape(n=0) == 0 and torch.equal(c.out, before)     # n == 0 succeeds and writes nothing
    e = Measured(np.zeros((1, 4, 5), np.uint8))
    assert e.n == 0 and e.shape() == 0 and torch.all(e.out == -77)
    other = Measured(m[:, :10].copy())                          # a workspace filled under another geometry
    N, P, H, W = c.dims
    refused = [dict(mask=None), dict(ws=None), dict(slots=None), dict(sws=None), dict(out=None),
               dict(n=-1), dict(n=c.max_out + 1), dict(n_slots=c.max_out - 1), dict(n_slots=c.max_out + 1),
               dict(dims=(N, P, W, H)), dict(dims=(1, P, H, W)), dict(dims=(N, 2, H // 2, W)),
               dict(ws=other.ws.data_ptr()), dict(ws=c.ws.data_ptr() + 16),     # ... and one never filled
               dict(ws=c.ws.data_ptr() + 4), dict(sws=c.sws.data_ptr() + 8),
               dict(dims=(0, P, H, W)), dict(dims=(N, P, H, -1))]
    for kw in refused:
        assert c.shape(**kw) == -1, kw                          # SQ_EINVAL
        assert c.lib.sq_last_error().decode().startswith("sq_objects_shape: "), kw
    torch.cuda.synchronize()
    assert torch.equal(c.out, before)                           # refused before any launch
    _lib.check(c.shape(), "sq_objects_shape")                   # and the call still works afterwards
    assert np.array_equal(c.sorted_rows(), sc.shape_ref(m)['shape'])
    wide = Measured(np.ones((1, 1, 65537), np.uint8), max_out=4)             # sq_objects_measure takes it ...
    assert wide.n == 1 and int(wide.rows_i[0, 3]) == 65537
    assert wide.shape() != 0 and torch.all(wide.out == -77)                  # ... sq_objects_shape does not
    edge = Measured(np.ones((1, 1, 65536), np.uint8), max_out=4)
    _lib.check(edge.shape(), "sq_objects_shape")
    assert edge.sorted_rows()[0].tolist() == sc.shape_ref(np.ones((1, 1, 65536), np.uint8))['shape'][0].tolist()
    with pytest.raises(_lib.SequitrHipError):
        objects.measure_objects(wide.mask, shape=True)
    assert len(objects.measure_objects(wide.mask)) == 1
