"""CPU: the restatements of tests/neighbors_cases.py against pure-Python all-pairs versions, the consequences the header
states, that every GPU case does what it is there for, NeighborTable's host half, the C-ABI's argument checks (no launch)
and the job's validation (before any input is opened)."""
import ctypes

import numpy as np
import pytest
import torch

from sequitr_amd import _lib, jobs
from sequitr_amd.analysis import neighbors as nb
from tests import neighbors_cases as nc


def small_frames():
    out = []
    for seed, (N, H, W) in enumerate(((1, 12, 13), (2, 7, 9), (1, 1, 11), (1, 10, 1), (3, 5, 5))):
        lab = nc.random_labels(seed, N, H, W, max_label=4, density=0.12)
        out.append(lab)
    lab = np.zeros((2, 9, 9), np.int32)                         # ties: left / right and up / down at once, both label orders
    lab[0, 4, 1], lab[0, 4, 7], lab[0, 0, 4], lab[0, 8, 4] = 2, 1, 3, 4
    lab[1, 4, 1], lab[1, 4, 7], lab[1, 0, 4], lab[1, 8, 4] = 1, 2, 4, 3
    out.append(lab)
    return out


@pytest.mark.parametrize("R", [0, 1, 3])
def test_zones_ref_equals_the_all_pairs_definition(R):
    ties = 0
    for lab in small_frames():
        z, d = nc.zones_ref(lab, 4, R)
        z2, d2 = nc.zones_allpairs(lab, 4, R)
        assert np.array_equal(z, z2) and np.array_equal(d, d2)
        ties += int(nc.tie_pixels(lab, 4).sum())
    assert ties > 20


def test_graph_ref_equals_the_all_pairs_definition():
    for lab in small_frames():
        z, _ = nc.zones_ref(lab, 4)
        z[0, 0, 0] = -2                                         # out of range: counts as 0
        s, p = nc.graph_ref(z, 4)
        s2, p2 = nc.graph_allpairs(z, 4)
        assert np.array_equal(s, s2) and np.array_equal(p, p2)
    for name, z, ml in nc.graph_cases()[:3]:
        s, p = nc.graph_ref(z, ml)
        s2, p2 = nc.graph_allpairs(z, ml)
        assert np.array_equal(s, s2) and np.array_equal(p, p2), name


def test_stated_consequences():
    for name, lab, ml, reaches in nc.zone_cases()[:8] + [nc.seam_case(), nc.label_value_case()]:
        seeds = nc.seeds_of(lab, ml)
        z, d = nc.zones_ref(lab, ml)
        assert np.array_equal(z[seeds > 0], seeds[seeds > 0]), name        # every seed lies in its own zone
        assert np.all(d[seeds > 0] == 0)
        has = seeds.reshape(len(seeds), -1).any(1)
        assert np.all(z[has] > 0) and np.all(z[~has] == 0) and np.all(d[~has] == nc.NO_SEED)
        stats, pairs = nc.graph_ref(z, ml)
        assert stats[:, :, 0].sum() == (z > 0).sum() and np.all(stats[:, 0] == 0)   # the areas add up to the covered pixels
        assert np.all(pairs[:, 3] > 0) and np.all(pairs[:, 1] < pairs[:, 2])


def test_every_zone_case_does_what_it_is_there_for():
    cases = {c[0]: c for c in nc.zone_cases()}
    assert {c[2] for c in cases.values() if c[0].startswith("rand")} == {6}
    widths = {c[1].shape[2] for c in cases.values()}
    heights = {c[1].shape[1] for c in cases.values()}
    assert widths >= set(nc.SIZES) and heights >= set(nc.SIZES)
    assert {c[1].shape[0] for c in cases.values()} >= {1, 3}
    for name in ("ties_12", "ties_21", "tie_le_12", "tie_le_21", "seams"):
        _, lab, ml, _ = cases[name]
        t = nc.tie_pixels(lab, ml)
        assert t.reshape(len(t), -1).any(1).all() or name == "seams" and t.any(), name
    for name, first in (("tie_le_12", 5), ("tie_le_21", 1)):    # the in-row seed is at distance 3, the other 3 rows away
        _, lab, ml, _ = cases[name]
        z, d = nc.zones_ref(lab, ml)
        assert lab[0, 3, 66] == first and lab[0, 0, 63] == 2 and d[0, 3, 63] == 9 and z[0, 3, 63] == min(first, 2)
        assert d[1, 3, 63] == 9 and z[1, 3, 63] == min(first, 2) and not nc.seeds_of(lab, ml)[:, 1:3, 63].any()
    _, lab, ml, reaches = cases["reach"]
    assert reaches == (0, 1, 5, 64)
    for R in reaches[1:]:
        z, d = nc.zones_ref(lab, ml, R)
        assert d[0, 70, 70 + R] == R * R and z[0, 70, 70 + R] == 2          # d2 == R*R is kept
        assert d[0, 71, 70 + R] == R * R + 1 and z[0, 71, 70 + R] == 0      # R*R + 1 is dropped
    _, lab, ml, _ = cases["label_values"]
    assert lab.min() < 0 and (lab == ml).any() and (lab == ml + 1).any() and (nc.seeds_of(lab, ml) > 0).sum() == 3
    _, lab, ml, _ = cases["seams"]
    z, d = nc.zones_ref(lab, ml)
    assert (lab[0, 4] > 0).sum() == 1 and (lab[0, 5] > 0).sum() == 1 and lab[0, 4, 3] and lab[0, 5, 197]
    _, lab, ml, _ = cases["no_seed_one_seed"]
    assert [(nc.seeds_of(lab, ml)[n] > 0).sum() for n in range(3)] == [0, 1, 0]
    _, lab, ml, _ = cases["frame_leak"]
    z, d = nc.zones_ref(lab, ml)
    assert np.all(z[1] == 3) and d[1, 0, 63] == 32 * 32 + 63 * 63             # a leak would find a seed at distance 1
    z, d = nc.zones_ref(cases["frame_leak_empty"][1], ml)
    assert not z[1].any() and np.all(d[1] == nc.NO_SEED)


def test_every_graph_case_does_what_it_is_there_for():
    cases = {c[0]: c for c in nc.graph_cases()}
    _, z, ml = cases["straight_border"]
    s, p = nc.graph_ref(z, ml)
    assert z.shape[2] > 3 * 64 and p.tolist() == [[0, 1, 2, 200]]
    _, z, ml = cases["corner_both_ways_two_frames"]
    s, p = nc.graph_ref(z, ml)
    assert p.tolist() == [[0, 1, 2, 5], [1, 1, 2, 3]]                       # 3 vertical + 2 horizontal; zone 0 makes no pair
    assert s[0, 1].tolist() == [6, 4] and s[0, 4].tolist() == [1, 1]        # corners count once
    assert s[0, 3].tolist() == [5, 2] and s[1, 4].tolist() == [0, 0]
    _, z, ml = cases["five_pairs"]
    assert nc.graph_ref(z, ml)[1].tolist() == [[0, k, k + 1, 3] for k in range(1, 6)]
    _, z, ml = cases["own_labels"]
    H, W = z.shape[1:]
    s, p = nc.graph_ref(z, ml)
    assert len(p) == 2 * H * W - H - W and np.all(p[:, 3] == 1) and np.all(s[0, 1:, 0] == 1)
    assert len(nc.graph_ref(*cases["zones_3x65x130"][1:])[1]) > 20


def host_table(labels, cls, centroid, frame, C, d_thresh, seeds="objects", reach=None):
    """NeighborTable from the restatement's zones and graph: its host half, without a GPU"""
    k = len(frame)
    bounds = np.searchsorted(frame, np.arange(labels.shape[0] + 1))
    label = np.arange(1, k + 1) - bounds[frame]
    ml = max(1, int(np.diff(bounds).max()))
    src = labels if seeds == "objects" else nc.centroid_seed_image(frame, label, centroid, labels.shape)
    z, _ = nc.zones_ref(src, ml, reach or 0)
    stats, pairs = nc.graph_ref(z, ml)
    rng = np.random.default_rng(0)
    return nb.NeighborTable(frame, label, cls, centroid, C, stats, pairs[rng.permutation(len(pairs))], labels.shape[0],
                            d_thresh, reach, seeds)


def test_neighbor_table_host_half_equals_the_restatement():
    mask, labels, cls, centroid, frame = nc.object_frames()
    free = nc.neighbors_ref(labels, cls, centroid, frame, 3, np.inf)
    assert free["n_pairs"] > 20 and free["n_pairs_removed"] == 0
    at, below, above = nc.threshold_values(free)
    counts = []
    for d in (at, below, above, 100.0):
        for seeds in ("objects", "centroids"):
            want = nc.neighbors_ref(labels, cls, centroid, frame, 3, d, None, seeds)
            t = host_table(labels, cls, centroid, frame, 3, d, seeds)
            nc.assert_table(t.columns(), want, "d_thresh %r %s" % (d, seeds))
            assert (t.n_pairs, t.n_pairs_removed) == (want["n_pairs"], want["n_pairs_removed"])
            assert np.array_equal(t.n_class.sum(1), t.n_total) and len(t.indices) == 2 * t.n_pairs
            for i in range(len(t)):                             # symmetric in CSR
                for j in t.indices[t.indptr[i]:t.indptr[i + 1]]:
                    assert i in t.indices[t.indptr[j]:t.indptr[j + 1]]
            if seeds == "objects":
                counts.append(want["n_pairs"])
    assert counts[1] < counts[0] == counts[2]                   # a pair is removed iff distance > d_thresh
    # batches: frames 0-1 and frame 2 concatenated equal the whole stack
    sel = frame < 2
    a = host_table(labels[:2], cls[sel], centroid[sel], frame[sel], 3, at)
    b = host_table(labels[2:], cls[~sel], centroid[~sel], frame[~sel] - 2, 3, at)
    whole = nb.NeighborTable.concatenate([a, b], [0, 2], 3)
    nc.assert_table(whole.columns(), nc.neighbors_ref(labels, cls, centroid, frame, 3, at), "concatenate")
    empty = nb.NeighborTable.concatenate([], [], 0)
    assert len(empty) == 0 and empty.indptr.tolist() == [0]
    none = nb.NeighborTable([], [], [], np.zeros((0, 3)), 3, np.zeros((2, 2, 2), np.int64), np.zeros((0, 4)), 2)   # no object
    both = nb.NeighborTable.concatenate([none, b], [0, 2], 3)
    assert len(none) == 0 and none.n_class.shape == (0, 3) and len(both) == len(b) and np.array_equal(both.indices, b.indices)


def test_shared_seed_pixel_goes_to_the_smallest_label():
    from tests import objects_cases as oc
    mask = nc.shared_seed_objects()
    ref = oc.objects_ref(mask)
    seeds = nc.centroid_seed_image(ref["frame"], ref["label"], ref["centroid"], mask.shape)
    assert len(ref["label"]) == 3 and (seeds > 0).sum() == 2 and seeds[0, 20, 20] == 1   # ring (1) and dot (3) share (20,20)
    want = nc.neighbors_ref(ref["labels"], ref["cls"], ref["centroid"], ref["frame"], 3, 100.0, None, "centroids")
    assert want["zone_area"][2] == 0 and np.isinf(want["local_density"][2]) and want["n_total"].tolist() == [1, 1, 0]


def test_delaunay_agreement_is_computed():
    zp, de, both = nc.delaunay_agreement(0, 40, 96, 96)
    assert 0 < both <= min(zp, de)
    print("40 points: %d zone pairs, %d Delaunay edges, %d shared" % (zp, de, both))


def test_abi_argument_checks_need_no_launch():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096 + 64)
    p = (ctypes.addressof(buf) + 63) // 64 * 64                 # host memory: no call below gets as far as a launch

    def zones(labels=p, zones_=p + 1024, d2=None, N=1, H=4, W=4, ml=3, R=0, ws=p + 2048):
        return lib.sq_label_zones_i32(labels, zones_, d2, N, H, W, ml, R, ws, None), lib.sq_last_error()

    for kw, word in ((dict(labels=None), b"null"), (dict(zones_=None), b"null"), (dict(ws=None), b"null"), (dict(N=0), b"N*H*W"),
                     (dict(H=30000), b"30000"), (dict(W=30000), b"30000"), (dict(N=8, H=20000, W=20000), b"2^31"),
                     (dict(ml=0), b"max_label"), (dict(ml=1 << 21), b"max_label"), (dict(R=-1), b"max_distance"),
                     (dict(R=46341), b"max_distance"), (dict(ws=p + 2052), b"aligned"), (dict(ws=p + 1024), b"overlap"),
                     (dict(d2=p + 1024), b"overlap")):
        rc, msg = zones(**kw)
        assert rc == -1 and word in msg, (kw, msg)
    assert lib.sq_label_zones_workspace(3, 10, 10) == 16 + 1808 and lib.sq_label_zones_workspace(1, 30000, 4) == -1
    assert lib.sq_label_zones_workspace(0, 4, 4) == -1 and lib.sq_label_zones_workspace(8, 20000, 20000) == -1

    def graph(z=p, N=1, H=4, W=4, ml=3, stats=p + 512, pairs=p + 1024, mp=4, count=p + 1536, dropped=p + 1540, ws=p + 2048):
        return lib.sq_zone_graph(z, N, H, W, ml, stats, pairs, mp, count, dropped, ws, None), lib.sq_last_error()

    for kw, word in ((dict(z=None), b"null"), (dict(stats=None), b"null"), (dict(pairs=None), b"null"), (dict(count=None), b"null"),
                     (dict(dropped=None), b"null"), (dict(ws=None), b"null"), (dict(H=0), b"N, H, W"), (dict(N=1 << 21, H=1, W=1), b"2^21"),
                     (dict(ml=0), b"max_label"), (dict(ml=1 << 21), b"max_label"), (dict(mp=0), b"max_pairs"),
                     (dict(mp=(1 << 28) + 1), b"max_pairs"), (dict(ws=p + 2056), b"aligned"), (dict(stats=p + 516), b"aligned"),
                     (dict(ws=p + 1024), b"overlap")):
        rc, msg = graph(**kw)
        assert rc == -1 and word in msg, (kw, msg)
    assert lib.sq_zone_graph_workspace(1) == 32 and lib.sq_zone_graph_workspace(1024) == 2048 * 12
    assert lib.sq_zone_graph_workspace(1025) == 4096 * 12 and lib.sq_zone_graph_workspace(0) == -1


def test_python_argument_checks_and_no_cpu_path():
    lab = torch.zeros((1, 4, 4), dtype=torch.int32)
    with pytest.raises(_lib.SequitrHipError, match="GPU memory"):
        nb.label_zones(lab)
    with pytest.raises(_lib.SequitrHipError, match="GPU memory"):
        nb.neighbors(lab, [], np.zeros((0, 2)), [], 2)
    with pytest.raises(TypeError):
        nb.label_zones(np.zeros((1, 4, 4), np.int32))
    for bad in (dict(d_thresh=-1.0), dict(d_thresh=float("nan")), dict(d_thresh="far"), dict(max_distance=0),
                dict(max_distance=2.5), dict(max_distance=46341), dict(max_distance=True), dict(seeds="voronoi")):
        with pytest.raises(ValueError, match=list(bad)[0]):
            nb.check_params(**bad)
    assert nb.check_params() == (100.0, None, "objects") and nb.check_params(0, np.int64(7), "centroids") == (0.0, 7, "centroids")


@pytest.mark.parametrize("bad", [{"d_thresh": -5}, {"d_thresh": "x"}, {"zone_reach": 0}, {"zone_reach": 1.5},
                                 {"neighbor_seeds": "delaunay"}])
def test_job_validates_before_any_input_is_opened(bad, tmp_path):
    params = dict({"input": str(tmp_path / "no_such_frames.npy"), "output": str(tmp_path)}, **bad)
    word = {"zone_reach": "max_distance", "neighbor_seeds": "seeds"}.get(list(bad)[0], list(bad)[0])
    with pytest.raises(ValueError, match=word):
        jobs.SERVER_segment_frames(params, {"neighbors": True})
