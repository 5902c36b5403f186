"""GPU: sq_label_zones_i32, sq_zone_graph and sequitr_amd/analysis/neighbors.py against the restatements of
tests/neighbors_cases.py.  Integer work: every byte of zones, d2, stats and the sorted pairs must be equal, and every
column of the neighbour table, floats bit for bit."""
import numpy as np
import pytest
import torch

from sequitr_amd import _lib
from sequitr_amd.analysis import neighbors as nb
from sequitr_amd.objects import measure_objects
from tests import neighbors_cases as nc
from tests import objects_cases as oc

pytestmark = pytest.mark.gpu
GUARD = 64                                                      # int32 elements in front of and behind every buffer


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Guarded(object):
    """an int32 buffer of n elements between two guard bands; .t is the 16-byte aligned payload"""

    def __init__(self, n, fill=0x5A5A5A5A):
        self.n, self.fill = n, fill
        self.buf = torch.full((n + 2 * GUARD,), fill, dtype=torch.int32, device="cuda")
        self.t = self.buf[GUARD:GUARD + n]
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        b = self.buf.cpu().numpy()
        return bool(np.all(b[:GUARD] == self.fill) and np.all(b[GUARD + self.n:] == self.fill))


def zones_guarded(lab_d, ml, R, want_d2):
    """label_zones into guarded outputs and a guarded workspace -> (zones, d2 or None) as numpy"""
    N, H, W = lab_d.shape
    nws = int(_lib.load().sq_label_zones_workspace(N, H, W))
    z, d, ws = Guarded(N * H * W), Guarded(N * H * W), Guarded(nws // 4)
    got = nb.label_zones(lab_d, R or None, return_distance=want_d2, max_label=ml, out=z.t.view(N, H, W),
                         distance_out=d.t.view(N, H, W) if want_d2 else None, workspace=ws.t)
    torch.cuda.synchronize()
    assert z.intact() and d.intact() and ws.intact(), "a guard band was written"
    if want_d2:
        return got[0].cpu().numpy(), got[1].cpu().numpy()
    assert np.all(d.t.cpu().numpy() == d.fill)                  # d2 NULL: nothing is written
    return got.cpu().numpy(), None


@pytest.mark.parametrize("case", nc.zone_cases(), ids=lambda c: c[0])
def test_zones_equal_the_restatement(case):
    name, lab, ml, reaches = case
    lab_d = dev(lab)
    for R in reaches:
        want_z, want_d = nc.zones_ref(lab, ml, R)
        for want_d2 in (True, False):
            z, d = zones_guarded(lab_d, ml, R, want_d2)
            assert z.dtype == np.int32 and np.array_equal(z, want_z), "%s R=%d d2=%s: %d zones differ" % (
                name, R, want_d2, int((z != want_z).sum()))
            if want_d2:
                assert d.dtype == np.int32 and np.array_equal(d, want_d), "%s R=%d: %d distances differ" % (
                    name, R, int((d != want_d).sum()))
    assert np.array_equal(lab_d.cpu().numpy(), lab)             # the input is not written


def graph_raw(z_d, ml, max_pairs):
    """one sq_zone_graph call into guarded buffers -> (stats, pairs sorted, count, dropped)"""
    lib = _lib.load()
    N, H, W = z_d.shape
    nws = int(lib.sq_zone_graph_workspace(max_pairs))
    stats, pairs, ctr, ws = Guarded(N * (ml + 1) * 4), Guarded(max_pairs * 4), Guarded(4), Guarded(nws // 4)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.sq_zone_graph(z_d.data_ptr(), N, H, W, ml, stats.t.data_ptr(), pairs.t.data_ptr(), max_pairs,
                                 ctr.t.data_ptr(), ctr.t[1:].data_ptr(), ws.t.data_ptr(), st), "sq_zone_graph")
    torch.cuda.synchronize()
    assert stats.intact() and pairs.intact() and ctr.intact() and ws.intact(), "a guard band was written"
    count, dropped, g2, g3 = ctr.t.cpu().numpy()
    assert g2 == g3 == ctr.fill
    rows = pairs.t.cpu().numpy().reshape(max_pairs, 4)
    assert 0 <= count <= max_pairs and np.all(rows[count:] == pairs.fill)
    rows = rows[:count].astype(np.int64)
    rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
    return stats.t.cpu().numpy().view(np.int64).reshape(N, ml + 1, 2), rows, int(count), int(dropped)


@pytest.mark.parametrize("case", nc.graph_cases(), ids=lambda c: c[0])
def test_graph_equals_the_restatement(case):
    name, z, ml = case
    want_s, want_p = nc.graph_ref(z, ml)
    z_d = dev(z)
    for max_pairs in (max(1, len(want_p)), 4 * len(want_p) + 3):            # the table at full load, and roomy
        s, p, count, dropped = graph_raw(z_d, ml, max_pairs)
        assert dropped == 0 and count == len(want_p), (name, max_pairs, count, dropped)
        assert np.array_equal(s, want_s) and np.array_equal(p, want_p), (name, max_pairs)
    s, p = nb.zone_graph(z_d, ml)
    assert s.dtype == np.int64 and p.dtype == np.int64 and np.array_equal(s, want_s) and np.array_equal(p, want_p)
    assert np.array_equal(z_d.cpu().numpy(), z)


def test_too_little_room_is_reported_and_the_wrapper_comes_back_with_more():
    name, z, ml = nc.five_pairs()
    want_s, want_p = nc.graph_ref(z, ml)
    assert len(want_p) == 5
    z_d = dev(z)
    s, p, count, dropped = graph_raw(z_d, ml, 1)
    assert dropped != 0 and count <= 1 and np.array_equal(s, want_s)
    assert all(row.tolist() in want_p.tolist() for row in p)
    s, p = nb.zone_graph(z_d, ml, max_pairs=1)
    assert np.array_equal(s, want_s) and np.array_equal(p, want_p)


def test_twice_is_bit_identical_and_captured_graphs_replay_the_eager_bits():
    lab = np.concatenate([nc.random_labels(5, 2, 129, 200, 9, 0.01), nc.seam_case()[1].repeat(15, 1)[:, :129]])
    ml = 9
    lab_d = dev(lab)
    want_z, want_d = nc.zones_ref(lab, ml, 40)
    want_s, want_p = nc.graph_ref(want_z, ml)
    a, b = nb.label_zones(lab_d, 40, True, ml), nb.label_zones(lab_d, 40, True, ml)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert np.array_equal(a[0].cpu().numpy(), want_z) and np.array_equal(a[1].cpu().numpy(), want_d)
    g1, g2 = nb.zone_graph(a[0], ml), nb.zone_graph(a[0], ml)
    assert np.array_equal(g1[0], g2[0]) and np.array_equal(g1[1], g2[1]) and np.array_equal(g1[1], want_p)

    lib = _lib.load()
    N, H, W = lab.shape
    max_pairs = 256
    zones, d2 = torch.empty_like(lab_d), torch.empty_like(lab_d)
    ws = torch.empty(int(lib.sq_label_zones_workspace(N, H, W)) // 4, dtype=torch.int32, device="cuda")
    stats = torch.empty((N, ml + 1, 2), dtype=torch.int64, device="cuda")
    pairs = torch.empty((max_pairs, 4), dtype=torch.int32, device="cuda")
    ctr = torch.empty(2, dtype=torch.int32, device="cuda")
    gws = torch.empty(int(lib.sq_zone_graph_workspace(max_pairs)) // 4, dtype=torch.int32, device="cuda")

    def both():                                                 # one linear chain of launches on the current stream
        nb.label_zones(lab_d, 40, max_label=ml, out=zones, distance_out=d2, workspace=ws)
        _lib.check(lib.sq_zone_graph(zones.data_ptr(), N, H, W, ml, stats.data_ptr(), pairs.data_ptr(), max_pairs,
                                     ctr.data_ptr(), ctr[1:].data_ptr(), gws.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream), "sq_zone_graph")

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        both()                                                  # warm up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    for _ in range(2):
        for t in (zones, d2, pairs, ctr):
            t.fill_(-1)
        stats.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(zones, a[0]) and torch.equal(d2, a[1])
        count, dropped = ctr.cpu().numpy()
        rows = pairs[:count].cpu().numpy().astype(np.int64)
        assert dropped == 0 and np.array_equal(rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))], want_p)
        assert np.array_equal(stats.cpu().numpy(), want_s)


def test_python_argument_checks():
    lab = torch.zeros((2, 8, 70), dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="contiguous"):
        nb.label_zones(lab[:, :, :50])
    with pytest.raises(ValueError, match="contiguous"):
        nb.label_zones(lab.to(torch.int64))
    with pytest.raises(ValueError, match="workspace holds"):
        nb.label_zones(lab, workspace=torch.empty(4, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="max_distance"):
        nb.label_zones(lab, 0)
    with pytest.raises(_lib.SequitrHipError, match="max_label"):
        nb.label_zones(lab, max_label=1 << 21)
    with pytest.raises(ValueError, match="sorted"):
        nb.neighbors(lab, [1, 1], np.zeros((2, 2)), [1, 0], 2)
    with pytest.raises(ValueError, match="num_classes"):
        nb.neighbors(lab, [1, 2], np.zeros((2, 2)), [0, 1], 2)
    z, d = nb.label_zones(lab, return_distance=True)             # no seed anywhere
    assert not z.any() and bool((d == nc.NO_SEED).all())
    t = nb.neighbors(lab, [], np.zeros((0, 2)), [], 2)
    assert len(t) == 0 and t.indptr.tolist() == [0] and t.n_class.shape == (0, 2)


@pytest.fixture(scope="module", params=[1, 2], ids=["C2", "C3"])
def objects(request):
    classes = request.param
    mask, labels, cls, centroid, frame = nc.object_frames(seed=3 + classes, classes=classes)
    free = nc.neighbors_ref(labels, cls, centroid, frame, classes + 1, np.inf)
    return classes + 1, mask, labels, cls, centroid, frame, free


def test_neighbors_equal_the_restatement(objects):
    C, mask, labels, cls, centroid, frame, free = objects
    table = measure_objects(dev(mask), labels=True)
    assert np.array_equal(table.labels.cpu().numpy(), labels)   # scipy's objects: pinned in tests/test_gpu_objects.py
    labels_d = dev(labels)
    assert free["n_pairs"] > 20
    at, below, above = nc.threshold_values(free)
    kept = {}
    for seeds in nb.SEEDS:
        for d_thresh, reach in ((at, None), (below, None), (above, None), (100.0, None), (30.0, 6)):
            want = nc.neighbors_ref(labels, cls, centroid, frame, C, d_thresh, reach, seeds)
            what = "C=%d %s d_thresh=%r reach=%r" % (C, seeds, d_thresh, reach)
            got = nb.neighbors(labels_d, cls, centroid[:, 1:], frame, C, d_thresh, reach, seeds, return_zones=True)
            nc.assert_table(got.columns(), want, "neighbors " + what)
            assert np.array_equal(got.zones.cpu().numpy(), want["zones"]), what
            assert (got.n_pairs, got.n_pairs_removed) == (want["n_pairs"], want["n_pairs_removed"]), what
            got = nb.neighbors_from_objects(table, C, d_thresh, reach, seeds)
            nc.assert_table(got.columns(), want, "neighbors_from_objects " + what)
            assert got.zones is None
            kept[(seeds, d_thresh)] = want["n_pairs"]
    assert kept[("objects", below)] < kept[("objects", at)] == kept[("objects", above)]


def test_two_objects_with_one_seed_pixel():
    mask = nc.shared_seed_objects()
    ref = oc.objects_ref(mask)
    table = measure_objects(dev(mask), labels=True)
    for seeds in nb.SEEDS:
        want = nc.neighbors_ref(ref["labels"], ref["cls"], ref["centroid"], ref["frame"], 3, 100.0, None, seeds)
        got = nb.neighbors_from_objects(table, 3, seeds=seeds, return_zones=True)
        nc.assert_table(got.columns(), want, seeds)
        assert np.array_equal(got.zones.cpu().numpy(), want["zones"])
    assert want["zone_area"][2] == 0 and np.isinf(got.local_density[2])   # the dot lost its seed pixel to the ring
    with pytest.raises(ValueError, match="labels=True"):
        nb.neighbors_from_objects(measure_objects(dev(mask)), 3)
