"""GPU: sq_label_zones3d_i32, sq_zone_graph3d and the volumetric half of sequitr_amd/analysis/neighbors.py against the
restatements of tests/neighbors3d_cases.py.  A minimum of fixed expressions and integer sums: every byte of zones, d2, stats
and the sorted pairs must be equal, and every column of the neighbour table, floats bit for bit.  Every zone case runs in
the LDS form and, with SQ_ZONES3D_LDS=0 flipped in-process, in the global-memory form."""
import os

import numpy as np
import pytest
import torch

from sequitr_amd import _lib, ops
from sequitr_amd.analysis import neighbors as nb
from sequitr_amd.objects import measure_objects
from tests import neighbors3d_cases as n3
from tests import neighbors_cases as nc
from tests import objects_cases as oc
from tests.test_gpu_neighbors import Guarded, dev
from tests.test_gpu_neighbors import graph_raw as planar_graph_raw

pytestmark = pytest.mark.gpu
SQ_EINVAL = -1


class lds_form(object):
    """SQ_ZONES3D_LDS for the calls inside: '0' selects the global-memory form; the variable is read per launch"""

    def __init__(self, on):
        self.value = None if on else "0"

    def __enter__(self):
        self.old = os.environ.pop("SQ_ZONES3D_LDS", None)
        if self.value is not None:
            os.environ["SQ_ZONES3D_LDS"] = self.value

    def __exit__(self, *exc):
        os.environ.pop("SQ_ZONES3D_LDS", None)
        if self.old is not None:
            os.environ["SQ_ZONES3D_LDS"] = self.old


def zones_guarded(lab_d, ml, R, dz, want_d2):
    """label_zones3d into guarded outputs and a guarded workspace -> (zones, d2 or None) as numpy"""
    N, D, H, W = lab_d.shape
    V = N * D * H * W
    nws = int(_lib.load().sq_label_zones3d_workspace(N, D, H, W))
    z, d, ws = Guarded(V), Guarded(2 * V), Guarded(nws // 4)
    d_out = d.t.view(torch.float64).view(N, D, H, W) if want_d2 else None
    got = nb.label_zones3d(lab_d, R or None, dz, return_distance=want_d2, max_label=ml, out=z.t.view(N, D, H, W),
                           distance_out=d_out, workspace=ws.t)
    torch.cuda.synchronize()
    assert z.intact() and d.intact() and ws.intact(), "a guard band was written"
    if want_d2:
        return got[0].cpu().numpy(), got[1].cpu().numpy()
    assert np.all(d.t.cpu().numpy() == d.fill)                  # d2 NULL: nothing is written
    return got.cpu().numpy(), None


def same_bits(a, b):
    return a.dtype == b.dtype == np.float64 and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("case", n3.zone_cases(), ids=lambda c: c[0])
def test_zones_equal_the_restatement(case):
    name, lab, ml, reaches, dzs = case
    lab_d = dev(lab)
    planar = n3.planar_ref(lab, ml)                             # once per case: it depends on neither dz nor the reach
    seeds = nc.seeds_of(lab, ml)
    has_seed = seeds.reshape(len(lab), -1).any(1)
    indicator = dev((seeds > 0).astype(np.float32))
    for dz in dzs:
        edt = ops.edt3d_squared(indicator, spacing=dz).cpu().numpy()
        for R in reaches:
            want_z, want_d = n3.zones3d_from_planar(*planar, dz=dz, max_distance=R)
            assert same_bits(want_d[has_seed], edt[has_seed]), "%s dz=%r: the restatement's d2 is not edt3d_squared" % (name, dz)
            for lds in (True, False):
                for want_d2 in (True, False):
                    with lds_form(lds):
                        z, d = zones_guarded(lab_d, ml, R, dz, want_d2)
                    what = "%s dz=%r R=%d lds=%s d2=%s" % (name, dz, R, lds, want_d2)
                    assert z.dtype == np.int32 and np.array_equal(z, want_z), "%s: %d zones differ" % (
                        what, int((z != want_z).sum()))
                    if want_d2:
                        assert same_bits(d, want_d), "%s: %d distances differ" % (what, int((d != want_d).sum()))
                        assert same_bits(d[has_seed], edt[has_seed]), what
                        assert np.all(np.isposinf(d[~has_seed])) and not z[~has_seed].any()
    assert np.array_equal(lab_d.cpu().numpy(), lab)             # the input is not written


def graph_raw(z_d, ml, max_pairs):
    """one sq_zone_graph3d call into guarded buffers -> (stats, pairs sorted, count, dropped)"""
    lib = _lib.load()
    N, D, H, W = z_d.shape
    nws = int(lib.sq_zone_graph3d_workspace(max_pairs))
    assert nws == 16 * max(2, 1 << (2 * max_pairs - 1).bit_length())
    stats, pairs, ctr, ws = Guarded(N * (ml + 1) * 4), Guarded(max_pairs * 5), Guarded(4), Guarded(nws // 4)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.sq_zone_graph3d(z_d.data_ptr(), N, D, H, W, ml, stats.t.data_ptr(), pairs.t.data_ptr(), max_pairs,
                                   ctr.t.data_ptr(), ctr.t[1:].data_ptr(), ws.t.data_ptr(), st), "sq_zone_graph3d")
    torch.cuda.synchronize()
    assert stats.intact() and pairs.intact() and ctr.intact() and ws.intact(), "a guard band was written"
    count, dropped, g2, g3 = ctr.t.cpu().numpy()
    assert g2 == g3 == ctr.fill
    rows = pairs.t.cpu().numpy().reshape(max_pairs, 5)
    assert 0 <= count <= max_pairs and np.all(rows[count:] == pairs.fill)
    rows = rows[:count].astype(np.int64)
    rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
    return stats.t.cpu().numpy().view(np.int64).reshape(N, ml + 1, 2), rows, int(count), int(dropped)


@pytest.mark.parametrize("case", n3.graph_cases(), ids=lambda c: c[0])
def test_graph_equals_the_restatement(case):
    name, z, ml = case
    want_s, want_p = n3.graph3d_ref(z, ml)
    z_d = dev(z)
    for max_pairs in (max(1, len(want_p)), 4 * len(want_p) + 3):            # the table at full load, and roomy
        s, p, count, dropped = graph_raw(z_d, ml, max_pairs)
        assert dropped == 0 and count == len(want_p), (name, max_pairs, count, dropped)
        assert np.array_equal(s, want_s) and np.array_equal(p, want_p), (name, max_pairs)
    s, p = nb.zone_graph3d(z_d, ml)
    assert s.dtype == np.int64 and p.dtype == np.int64 and p.shape[1] == 5
    assert np.array_equal(s, want_s) and np.array_equal(p, want_p)
    assert np.array_equal(z_d.cpu().numpy(), z)


def test_a_frame_is_a_volume_of_one_slice():
    """sq_zone_graph and sq_zone_graph3d are one program: at D = 1 the volume call gives the frame call's rows, no axial
    contact, and a border column equal to the area column -- every voxel of a one-slice volume lies on a face"""
    name, z, ml = nc.random_zones(6, 2, 37, 130, 20)            # about 20 zones over three 64-lane segments a row
    z = z.copy()
    z[0, 5:9, 40:60] = 0                                        # no zone: borders nothing
    z[1, 20, 100:] = ml + 3                                     # out of range either way: counts as 0
    z[1, 30:, 64] = -2
    assert z.shape == (2, 37, 130) and 15 <= len(np.unique(z[(z >= 1) & (z <= ml)])) <= ml
    want_s, want_p = nc.graph_ref(z, ml)
    assert len(want_p) > 20
    s2, p2, count2, dropped2 = planar_graph_raw(dev(z), ml, 4 * len(want_p) + 3)
    s3, p3, count3, dropped3 = graph_raw(dev(z[:, None]), ml, 4 * len(want_p) + 3)
    assert dropped2 == 0 and dropped3 == 0 and count2 == count3 == len(want_p)
    assert np.array_equal(s2, want_s) and np.array_equal(p2, want_p)
    assert np.array_equal(p3[:, :4], p2) and not p3[:, 4].any()
    assert np.array_equal(s3[:, :, 0], s2[:, :, 0]) and np.array_equal(s3[:, :, 1], s3[:, :, 0])


def test_too_little_room_is_reported_and_the_wrapper_comes_back_with_more():
    name, z, ml = n3.five_pairs()
    want_s, want_p = n3.graph3d_ref(z, ml)
    assert len(want_p) == 5
    z_d = dev(z)
    s, p, count, dropped = graph_raw(z_d, ml, 1)
    assert dropped != 0 and count <= 1 and np.array_equal(s, want_s)
    assert all(row.tolist() in want_p.tolist() for row in p)
    s, p = nb.zone_graph3d(z_d, ml, max_pairs=1)
    assert np.array_equal(s, want_s) and np.array_equal(p, want_p)


def test_twice_is_bit_identical_and_captured_graphs_replay_the_eager_bits():
    lab = n3.random_volume(5, 2, 9, 5, 130, 9, 0.02)
    ml, dz, R = 9, 2.5, 12
    lab_d = dev(lab)
    want_z, want_d = n3.zones3d_ref(lab, ml, R, dz)
    want_s, want_p = n3.graph3d_ref(want_z, ml)
    a, b = nb.label_zones3d(lab_d, R, dz, True, ml), nb.label_zones3d(lab_d, R, dz, True, ml)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int64), b[1].view(torch.int64))
    assert np.array_equal(a[0].cpu().numpy(), want_z) and same_bits(a[1].cpu().numpy(), want_d)
    g1, g2 = nb.zone_graph3d(a[0], ml), nb.zone_graph3d(a[0], ml)
    assert np.array_equal(g1[0], g2[0]) and np.array_equal(g1[1], g2[1]) and np.array_equal(g1[1], want_p)

    lib = _lib.load()
    N, D, H, W = lab.shape
    max_pairs = 256
    zones, d2 = torch.empty_like(lab_d), torch.empty(lab.shape, dtype=torch.float64, device="cuda")
    ws = torch.empty(int(lib.sq_label_zones3d_workspace(N, D, H, W)) // 4, dtype=torch.int32, device="cuda")
    stats = torch.empty((N, ml + 1, 2), dtype=torch.int64, device="cuda")
    pairs = torch.empty((max_pairs, 5), dtype=torch.int32, device="cuda")
    ctr = torch.empty(2, dtype=torch.int32, device="cuda")
    gws = torch.empty(int(lib.sq_zone_graph3d_workspace(max_pairs)) // 4, dtype=torch.int32, device="cuda")

    def both():                                                 # one linear chain of launches on the current stream
        nb.label_zones3d(lab_d, R, dz, max_label=ml, out=zones, distance_out=d2, workspace=ws)
        _lib.check(lib.sq_zone_graph3d(zones.data_ptr(), N, D, H, W, ml, stats.data_ptr(), pairs.data_ptr(), max_pairs,
                                       ctr.data_ptr(), ctr[1:].data_ptr(), gws.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream), "sq_zone_graph3d")

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
        assert torch.equal(zones, a[0]) and torch.equal(d2.view(torch.int64), a[1].view(torch.int64))
        count, dropped = ctr.cpu().numpy()
        rows = pairs[:count].cpu().numpy().astype(np.int64)
        assert dropped == 0 and np.array_equal(rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))], want_p)
        assert np.array_equal(stats.cpu().numpy(), want_s)


def test_python_argument_checks():
    lab = torch.zeros((2, 3, 8, 70), dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="contiguous"):
        nb.label_zones3d(lab[:, :, :, :50])
    with pytest.raises(ValueError, match="contiguous"):
        nb.label_zones3d(lab[0])                                 # three dimensions: the planar call's shape
    with pytest.raises(ValueError, match="contiguous"):
        nb.label_zones3d(lab.to(torch.int64))
    with pytest.raises(ValueError, match="contiguous"):
        nb.zone_graph3d(lab[0], 3)
    with pytest.raises(ValueError, match="workspace holds"):
        nb.label_zones3d(lab, workspace=torch.empty(4, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="max_distance"):
        nb.label_zones3d(lab, 0)
    for bad in (0.0, -2.0, float("inf"), float("nan"), None):
        with pytest.raises(ValueError, match="spacing"):
            nb.label_zones3d(lab, spacing=bad)
    with pytest.raises(ValueError, match="distance_out"):
        nb.label_zones3d(lab, distance_out=torch.empty_like(lab))       # int32: the planar call's type
    with pytest.raises(_lib.SequitrHipError, match="max_label"):
        nb.label_zones3d(lab, max_label=1 << 21)
    with pytest.raises(ValueError, match="sorted"):
        nb.neighbors3d(lab, [1, 1], np.zeros((2, 3)), [1, 0], 2)
    with pytest.raises(ValueError, match="num_classes"):
        nb.neighbors3d(lab, [1, 2], np.zeros((2, 3)), [0, 1], 2)
    with pytest.raises(ValueError, match=r"\(k,3\)"):
        nb.neighbors3d(lab, [1, 1], np.zeros((2, 2)), [0, 1], 2)
    with pytest.raises(ValueError, match="spacing"):
        nb.neighbors3d(lab, [], np.zeros((0, 3)), [], 2, spacing=0)
    z, d = nb.label_zones3d(lab, return_distance=True)           # no seed anywhere
    assert not z.any() and d.dtype == torch.float64 and bool(torch.isposinf(d).all())
    t = nb.neighbors3d(lab, [], np.zeros((0, 3)), [], 2)
    assert len(t) == 0 and t.volumetric and t.indptr.tolist() == [0] and t.n_class.shape == (0, 2)
    assert tuple(t.columns()) == n3.TABLE_COLUMNS


def test_c_abi_refusals():
    lib = _lib.load()
    lab = torch.zeros((1, 2, 4, 8), dtype=torch.int32, device="cuda")
    out = torch.full_like(lab, 7)
    d2 = torch.zeros((1, 2, 4, 8), dtype=torch.float64, device="cuda")
    ws = torch.empty(int(lib.sq_label_zones3d_workspace(1, 2, 4, 8)) // 4 + 4, dtype=torch.int32, device="cuda")
    assert lib.sq_label_zones3d_workspace(1, 2, 4, 8) == (16 + 3 * 256 + 128)
    assert lib.sq_label_zones3d_workspace(0, 2, 4, 8) == lib.sq_label_zones3d_workspace(1, 30000, 1, 1) == -1
    assert lib.sq_label_zones3d_workspace(2, 64, 4096, 4096) == -1 and lib.sq_zone_graph3d_workspace(0) == -1
    p = lambda t: t.data_ptr()                                  # noqa: E731

    def zones(labels=p(lab), zo=p(out), dd=p(d2), dims=(1, 2, 4, 8), ml=3, R=0, dz=1.0, w=p(ws)):
        return lib.sq_label_zones3d_i32(labels, zo, dd, *dims, ml, R, dz, w, None)

    assert zones() == 0
    for kw in (dict(labels=None), dict(zo=None), dict(w=None), dict(dims=(1, 0, 4, 8)), dict(dims=(1, 2, 30000, 8)),
               dict(dims=(2, 64, 4096, 4096)), dict(ml=0), dict(ml=1 << 21), dict(R=-1), dict(R=46341), dict(dz=0.0),
               dict(dz=float("inf")), dict(dz=float("nan")), dict(w=p(ws) + 4), dict(w=p(lab)), dict(zo=p(d2)),
               dict(dd=p(d2) + 4), dict(w=p(d2))):
        out.fill_(7)
        assert zones(**kw) == SQ_EINVAL and lib.sq_last_error(), kw
        torch.cuda.synchronize()
        assert bool((out == 7).all()), kw                       # refused before any launch
    stats = torch.zeros((1, 4, 2), dtype=torch.int64, device="cuda")
    pairs = torch.zeros((8, 5), dtype=torch.int32, device="cuda")
    ctr = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    gws = torch.empty(int(lib.sq_zone_graph3d_workspace(8)) // 4 + 4, dtype=torch.int32, device="cuda")

    def graph(z=p(lab), dims=(1, 2, 4, 8), ml=3, s=p(stats), pr=p(pairs), mp=8, c=p(ctr), dr=p(ctr) + 4, w=p(gws)):
        return lib.sq_zone_graph3d(z, *dims, ml, s, pr, mp, c, dr, w, None)

    assert graph() == 0
    torch.cuda.synchronize()
    for kw in (dict(z=None), dict(s=None), dict(pr=None), dict(c=None), dict(dr=None), dict(w=None), dict(dims=(1, 2, 0, 8)),
               dict(dims=(1 << 21, 1, 1, 1)), dict(dims=(2, 64, 4096, 4096)), dict(ml=0), dict(ml=1 << 21), dict(mp=0),
               dict(mp=(1 << 28) + 1), dict(w=p(gws) + 4), dict(s=p(stats) + 4), dict(w=p(pairs)), dict(w=p(lab))):
        ctr.fill_(7)
        assert graph(**kw) == SQ_EINVAL and lib.sq_last_error(), kw
        torch.cuda.synchronize()
        assert ctr.tolist() == [7, 7], kw


@pytest.fixture(scope="module", params=[1, 2], ids=["C2", "C3"])
def objects(request):
    classes = request.param
    mask, labels, cls, centroid, volume = n3.object_volumes(seed=3 + classes, classes=classes)
    return classes + 1, mask, labels, cls, centroid, volume


def test_neighbors_equal_the_restatement(objects):
    C, mask, labels, cls, centroid, volume = objects
    table = measure_objects(dev(mask), labels=True)
    assert table.volumetric and np.array_equal(table.labels.cpu().numpy(), labels)   # scipy's objects: tests/test_gpu_objects.py
    labels_d = dev(labels)
    kept = {}
    for dz in (1.0, 2.5):
        free = n3.neighbors3d_ref(labels, cls, centroid, volume, C, np.inf, spacing=dz)
        assert free["n_pairs"] > 10 and free["border_axial"].any() and free["border_lateral"].any()
        at, below, above = nc.threshold_values(free)
        for seeds in nb.SEEDS:
            for d_thresh, reach in ((at, None), (below, None), (above, None), (100.0, None), (30.0, 6)):
                if seeds == "centroids" and d_thresh in (below, above):
                    continue                                    # the threshold's three sides: once per spacing
                want = n3.neighbors3d_ref(labels, cls, centroid, volume, C, d_thresh, reach, seeds, dz)
                what = "C=%d %s dz=%r d_thresh=%r reach=%r" % (C, seeds, dz, d_thresh, reach)
                got = nb.neighbors3d(labels_d, cls, centroid, volume, C, d_thresh, reach, seeds, dz, return_zones=True)
                n3.assert_table(got.columns(), want, "neighbors3d " + what)
                assert tuple(got.columns()) == n3.TABLE_COLUMNS and got.volumetric and got.spacing == dz
                assert np.array_equal(got.zones.cpu().numpy(), want["zones"]), what
                assert (got.n_pairs, got.n_pairs_removed) == (want["n_pairs"], want["n_pairs_removed"]), what
                got = nb.neighbors_from_objects(table, C, d_thresh, reach, seeds, spacing=dz)
                n3.assert_table(got.columns(), want, "neighbors_from_objects " + what)
                assert got.zones is None
                kept[(dz, seeds, d_thresh)] = want["n_pairs"]
        assert kept[(dz, "objects", below)] < kept[(dz, "objects", at)] == kept[(dz, "objects", above)]


def test_two_objects_with_one_seed_voxel():
    mask = n3.shared_seed_volume()
    ref = oc.objects_ref(mask)
    assert len(ref["frame"]) == 3
    table = measure_objects(dev(mask), labels=True)
    for seeds in nb.SEEDS:
        want = n3.neighbors3d_ref(ref["labels"], ref["cls"], ref["centroid"], ref["frame"], 3, 100.0, None, seeds, 2.0)
        got = nb.neighbors_from_objects(table, 3, seeds=seeds, return_zones=True, spacing=2.0)
        n3.assert_table(got.columns(), want, seeds)
        assert np.array_equal(got.zones.cpu().numpy(), want["zones"])
    assert want["zone_area"][2] == 0 and np.isinf(got.local_density[2])   # the dot lost its seed voxel to the shell
    with pytest.raises(ValueError, match="labels=True"):
        nb.neighbors_from_objects(measure_objects(dev(mask)), 3)
