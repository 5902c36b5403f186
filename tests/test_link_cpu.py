"""CPU: the restatements of tests/link_cases.py against a brute force, the consequences the module text of
sequitr_amd/analysis/linking.py states, link_pairs / FrameLinker (fed by the restated overlap instead of the device) against
the rule written as plain loops, the host pieces (tracker JSON, lineage trees) and the C-ABI refusals."""
import ctypes
import json
import os

import numpy as np
import pytest

from sequitr_amd import _lib
from sequitr_amd.analysis import lineage, linking
from sequitr_amd.dataio import tracker
from tests import link_cases as lc
from tests import neighbors_cases as nc


def host_linker(**options):
    """a FrameLinker whose two device calls are the restatements, on numpy frames"""
    return linking.FrameLinker(overlap=lambda a, b, ml: lc.overlap_ref(a, b, ml),
                               zones=lambda labels, reach, ml: nc.zones_ref(labels, ml, reach)[0], **options)


def link_host(labels, cls=None, cuts=None, **options):
    counts = lc.counts_of(labels)
    cls = [np.zeros(k, np.int64) for k in counts] if cls is None else cls
    linker = host_linker(**options)
    F = len(labels)
    step = cuts or max(F, 1)
    for first in range(0, F, step):
        linker.push_frames(labels[first:first + step], cls[first:first + step])
    return linker.finish()


# ---- restatements -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (2, 5, 6), (3, 12, 13), (2, 2, 3, 4)])
def test_overlap_ref_equals_the_brute_force(shape):
    rng = np.random.default_rng(sum(shape))
    a = rng.integers(-1, 6, size=shape).astype(np.int32)
    b = rng.integers(-1, 6, size=shape).astype(np.int32)
    for ml in (1, 4, 5):
        got, want = lc.overlap_ref(a, b, ml), lc.brute_overlap(a, b, ml)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)
    p, aa, ab = lc.overlap_ref(a, a, 4)                         # a == b: only the diagonal, overlap = area
    assert np.array_equal(p[:, 1], p[:, 2]) and np.array_equal(p[:, 3], aa[p[:, 0], p[:, 1]]) and np.array_equal(aa, ab)
    assert not aa[:, 0].any()


def test_relabel_ref_is_the_definition():
    labels = np.array([[0, 1, 2, 3, -1], [2, 1, 0, 9, 1], [1, 1, 1, 1, 1]], np.int32)
    offsets, lut = np.array([0, 2, 2, 3]), np.array([7, 8, 9], np.int32)   # frame 1 is empty
    assert lc.relabel_ref(labels, offsets, lut).tolist() == [[0, 7, 8, 0, 0], [0, 0, 0, 0, 0], [9, 9, 9, 9, 9]]
    assert lc.relabel_ref(labels, np.array([0, 2, 2, 9]), lut).tolist()[2] == [9] * 5   # a range past the table reads as 0
    assert lc.relabel_ref(labels[:1], np.array([2, 9]), lut).tolist() == [[0, 9, 0, 0, 0]]


# ---- the rule ---------------------------------------------------------------------------------------------------------
def test_stated_consequences_hold_on_the_restated_rule():
    labels, cls, _ = lc.disk_movie()
    for reach in (0, 5):
        t = lc.link_ref_labels(labels, cls, reach)
        lc.check_consequences(t, lc.counts_of(labels))
        assert (t['children'] > 0).any() and t['generation'].max() == 1
    for name, labels, cls, opts in lc.scenarios():
        lc.check_consequences(lc.link_ref_labels(labels, cls, **opts), lc.counts_of(labels))


SCENARIOS = {s[0]: s for s in lc.scenarios()}


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_frame_linker_equals_the_restated_rule(name):
    _, labels, cls, opts = SCENARIOS[name]
    want = lc.link_ref_labels(labels, cls, **opts)
    got = link_host(labels, cls, **opts)
    lc.assert_tracks(got.columns(), want, name)
    assert got.options == dict(lc.DEFAULTS, **opts)
    t = got.columns()
    tracks, parent, children = t['track'].tolist(), t['parent'].tolist(), t['children'].tolist()
    if name in ("stationary", "moving_with_overlap"):
        assert tracks == [1, 1, 1] and t['end'].tolist() == [2] and t['links'][:, 3].tolist() == [0, 0]
    elif name in ("moving_without_overlap", "class_change_same_class", "min_iou_above", "min_overlap"):
        assert tracks == [1, 2] and parent == [1, 2] and len(t['links']) == 0       # two roots
    elif name in ("class_change_any_class", "min_iou_at", "min_iou_below"):
        assert tracks == [1, 1]
    elif name == "division":
        assert tracks == [1, 2, 3, 2, 3] and parent == [1, 1, 1] and children == [[2, 3], [0, 0], [0, 0]]
        assert t['end'].tolist() == [0, 2, 2] and t['links'][:, 3].tolist() == [1, 1, 0, 0]
        assert t['root'].tolist() == [1, 1, 1] and t['generation'].tolist() == [0, 1, 1]
    elif name == "division_continued_child_first":
        assert tracks == [1, 3, 2] and children[0] == [2, 3]    # label 2 continued the mother: it comes first
    elif name == "tie":
        assert tracks == [1, 2, 1] and t['end'].tolist() == [1, 0]
    elif name == "three_claimants":
        assert sorted(tracks[1:]) == [2, 3, 4] and parent.count(1) == 3 and parent[3] == 4   # the third is a root
        assert children[0][0] and children[0][1]
    elif name == "merge":
        assert tracks == [1, 2, 1] and t['end'].tolist() == [1, 0] and children == [[0, 0], [0, 0]]
    elif name == "no_divisions":
        assert tracks == [1, 1, 2] and parent == [1, 2]
    elif name == "empty_frame_in_the_middle":
        assert tracks == [1, 2] and t['start'].tolist() == [0, 2]
    elif name == "one_frame":
        assert tracks == [1, 2] and t['cls'].tolist() == [1, 0] and len(t['links']) == 0
    elif name in ("min_child_fraction_at", "min_child_fraction_below"):
        assert children[0] == [2, 3]
    elif name == "min_child_fraction_above":
        assert tracks == [1, 1, 2] and parent == [1, 2]


def test_random_many_to_many_movies_equal_the_restated_rule():
    """boxes thrown over one another: an object overlaps several successors and the greedy order matters"""
    rng = np.random.default_rng(0)
    for trial in range(12):
        labels = np.zeros((4, 24, 30), np.int32)
        for t in range(4):
            img = np.zeros((24, 30), np.int32)
            for l in range(1, int(rng.integers(0, 9)) + 1):
                y, x = int(rng.integers(0, 18)), int(rng.integers(0, 24))
                img[y:y + int(rng.integers(2, 7)), x:x + int(rng.integers(2, 7))] = l
            for r, v in enumerate(np.unique(img[img > 0])):
                labels[t][img == v] = r + 1
        cls = [rng.integers(0, 2, k) for k in lc.counts_of(labels)]
        for opts in ({}, {"same_class": False}, {"reach": 2, "min_iou": 0.1}):
            want = lc.link_ref_labels(labels, cls, **opts)
            lc.assert_tracks(link_host(labels, cls, **opts).columns(), want, "trial %d %r" % (trial, opts))
            lc.check_consequences(want, lc.counts_of(labels))


def test_link_pairs_is_one_step_of_the_rule():
    labels, cls, _ = lc.disk_movie()
    counts = lc.counts_of(labels)
    t = 2                                                       # the step in which cell 2 divides and cell 3 vanishes
    ml = max(counts[t], counts[t + 1])
    pairs, aa, ab = lc.overlap_ref(labels[t:t + 1], labels[t + 1:t + 2], ml)
    s = linking.link_pairs(pairs, aa[0], ab[0], cls[t], cls[t + 1])
    assert (s.kind == 1).sum() == 2 and (s.kind == -1).sum() == 1          # cell 4 jumps: a root
    assert len(s.created) == 3 and sorted(s.created.tolist()) == sorted(np.nonzero(s.kind != 0)[0] + 1)
    assert np.array_equal(s.source > 0, s.kind >= 0)
    same = linking.link_pairs(pairs[:, 1:], aa[0], ab[0], cls[t], cls[t + 1])                # (m,3) rows alike
    assert np.array_equal(s.source, same.source) and np.array_equal(s.created, same.created)


@pytest.mark.parametrize("reach", [0, 5])
def test_batch_cuts_give_identical_tables(reach):
    labels, cls, who = lc.disk_movie()
    want = lc.link_ref_labels(labels, cls, reach)
    for cuts in (1, 2, 3, len(labels)):
        got = link_host(labels, cls, cuts=cuts, reach=reach)
        lc.assert_tracks(got.columns(), want, "cuts of %d" % cuts)
    # cell 4 never overlaps itself: one track per frame without a reach, one track with it
    ids = [got.track[sum(len(w) for w in who[:t]) + who[t].index(4)] for t in range(len(labels))]
    assert len(set(ids)) == (1 if reach else len(labels))


def test_push_takes_batches_in_order_and_object_tables():
    labels, cls, _ = lc.disk_movie()

    class Table(object):
        def __init__(self, lo, hi):
            self.frame = np.repeat(np.arange(hi - lo), [len(c) for c in cls[lo:hi]])
            self.cls = np.concatenate(cls[lo:hi])

    linker = host_linker()
    linker.push(0, labels[:4], Table(0, 4))
    with pytest.raises(ValueError, match="order"):
        linker.push(5, labels[5:], Table(5, 6))
    linker.push(4, labels[4:], Table(4, 6))
    lc.assert_tracks(linker.finish().columns(), lc.link_ref_labels(labels, cls), "push")


def test_options_are_checked():
    for bad in ({"reach": -1}, {"reach": 1.5}, {"reach": True}, {"min_iou": 1.5}, {"min_iou": float("nan")},
                {"min_iou": "x"}, {"min_overlap": 0}, {"divisions": 1}, {"min_child_fraction": -0.1}, {"same_class": None}):
        with pytest.raises(ValueError, match=list(bad)[0]):
            linking.FrameLinker(**bad)
    with pytest.raises(ValueError, match="not built"):
        host_linker(reach=2).push_frames(np.zeros((2, 2, 4, 4), np.int32), [[], []])
    assert linking.check_options() == lc.DEFAULTS


def test_empty_movie_and_lut():
    t = host_linker().finish()
    assert len(t) == 0 and all(len(v) == 0 for v in t.columns().values())
    labels, cls, _ = lc.disk_movie()
    t = link_host(labels, cls)
    offsets, lut = t.lut()
    assert offsets.dtype == np.int64 and lut.dtype == np.int32
    assert offsets.tolist() == np.cumsum([0] + lc.counts_of(labels)).tolist()
    video = lc.relabel_ref(labels, offsets, lut)                # one value per track, and that value is its ID
    assert np.array_equal(video > 0, labels > 0)
    for f in range(len(labels)):
        for l in range(1, lc.counts_of(labels)[f] + 1):
            assert set(video[f][labels[f] == l].tolist()) == {int(t.track[offsets[f] + l - 1])}


# ---- host pieces ------------------------------------------------------------------------------------------------------
class _Objects(object):
    """the columns of an ObjectTable to_tracks reads"""
    volumetric = False

    def __init__(self, labels, cls):
        counts = lc.counts_of(labels)
        self.frame = np.repeat(np.arange(len(counts)), counts)
        self.cls = np.concatenate(cls)
        cen = []
        for f, k in enumerate(counts):
            for l in range(1, k + 1):
                y, x = np.nonzero(labels[f] == l)
                cen.append([0.0, y.mean(), x.mean()])
        self.centroid = np.array(cen).reshape(-1, 3)

    def __len__(self):
        return len(self.frame)


def _three_generations():
    """a mother (frames 0-1) that divides, and whose first daughter divides again at frame 4"""
    S = (8, 32)
    frames = [[(1, 1, 7, 4, 20)]] * 2 + [[(1, 1, 7, 4, 12), (2, 1, 7, 14, 20)]] * 2 + \
        [[(1, 1, 7, 4, 7), (2, 1, 7, 9, 12), (3, 1, 7, 14, 20)]] * 2
    return lc.boxes(S, frames)


def test_tracks_round_trip_through_json(tmp_path):
    labels, cls, _ = lc.disk_movie()
    table = link_host(labels, cls)
    tracks = table.to_tracks(_Objects(labels, cls), cell_type="GFP")
    assert [t.ID for t in tracks] == table.ID.tolist() and all(len(t) == len(t.t) == len(t.x) == len(t.label) for t in tracks)
    assert all(t.in_frame(t.t[0]) and not t.in_frame(-1) for t in tracks)
    assert sorted(set(l for t in tracks for l in t.label)) == [0, 1]
    for zipped in (True, False):
        folder = str(tmp_path / ("zipped" if zipped else "plain"))
        tracker.write_JSON(folder, tracks, "GFP", zipped=zipped)
        index = json.load(open(os.path.join(folder, "tracks_GFP.json")))["GFP"]
        assert index["zipped"] is zipped and len(index["files"]) == len(tracks) and index["path"] == folder
        assert os.path.exists(os.path.join(folder, "tracks_GFP.zip")) == zipped
        back = tracker.read_JSON(folder, "GFP")
        assert len(back) == len(tracks)
        for a, b, fn in zip(tracks, back, index["files"]):
            for name in ("ID", "x", "y", "z", "t", "length", "label", "parent", "children", "fate", "neighborhood"):
                assert getattr(a, name) == getattr(b, name), name
            assert b.cell_type == "GFP" and b.filename == fn
    with pytest.raises(IOError):
        tracker.read_JSON(str(tmp_path), "RFP")


def test_lineage_tree_of_three_generations():
    labels = _three_generations()
    cls = [np.zeros(k, np.int64) for k in lc.counts_of(labels)]
    table = link_host(labels, cls)
    assert table.generation.tolist() == [0, 1, 1, 2, 2] and table.root.tolist() == [1] * 5
    tracks = table.to_tracks(_Objects(labels, cls))
    trees = lineage.LineageTree(tracks).create()
    assert len(trees) == 1 and trees[0].root and not trees[0].leaf and trees[0].left.depth == 1
    assert json.loads(json.dumps(lineage.tree_to_dict(trees[0]))) == {
        "name": "1", "start": 0, "end": 1, "children": [
            {"name": "2", "start": 2, "end": 3, "children": [{"name": "4", "start": 4, "end": 5},
                                                             {"name": "5", "start": 4, "end": 5}]},
            {"name": "3", "start": 2, "end": 5}]}
    assert [n.ID for n in lineage.linearise_tree(trees[0])] == [1, 2, 3, 4, 5]
    with pytest.raises(TypeError):
        lineage.LineageTree([1, 2])


# ---- the C ABI's refusals need no GPU ---------------------------------------------------------------------------------
def test_overlap_refusals():
    lib = _lib.load()
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.addressof(buf)
    p += (-p) % 16                                              # 16-byte aligned host memory: nothing is launched
    a, b, pairs, cnt, drp, ws = p, p + 64, p + 128, p + 192, p + 196, p + 256

    def call(a=a, b=b, N=1, P=4, ml=3, aa=None, ab=None, pairs=pairs, mp=1, cnt=cnt, drp=drp, ws=ws):
        rc = lib.sq_label_overlap(a, b, N, P, ml, aa, ab, pairs, mp, cnt, drp, ws, None)
        return rc, lib.sq_last_error()

    for kw in ({"a": None}, {"b": None}, {"pairs": None}, {"cnt": None}, {"drp": None}, {"ws": None}):
        rc, msg = call(**kw)
        assert rc == -1 and b"null" in msg, kw
    for kw in ({"N": 0}, {"N": 1 << 21}, {"P": 0}, {"P": 1 << 31}):
        rc, msg = call(**kw)
        assert rc == -1 and b"2^31" in msg, kw
    for ml in (0, 1 << 21):
        rc, msg = call(ml=ml)
        assert rc == -1 and b"max_label" in msg
    for mp in (0, (1 << 28) + 1):
        rc, msg = call(mp=mp)
        assert rc == -1 and b"max_pairs" in msg
    rc, msg = call(ws=ws + 8)
    assert rc == -1 and b"16-byte" in msg
    rc, msg = call(aa=p + 324, ab=p + 400)
    assert rc == -1 and b"8-byte" in msg
    for kw in ({"ws": a}, {"ws": b - 16}, {"pairs": ws + 16}, {"cnt": ws}, {"drp": ws + 4}, {"aa": ws, "ab": p + 400}):
        rc, msg = call(**kw)
        assert rc == -1 and b"overlap" in msg, kw
    assert lib.sq_label_overlap_workspace(0) == -1 and lib.sq_label_overlap_workspace((1 << 28) + 1) == -1
    assert lib.sq_label_overlap_workspace(1) == 32 and lib.sq_label_overlap_workspace(1024) == 2048 * 12


def test_relabel_refusals():
    lib = _lib.load()
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.addressof(buf)
    p += (-p) % 16
    labels, out, off, lut = p, p + 64, p + 128, p + 192

    def call(labels=labels, out=out, N=2, P=4, off=off, lut=lut, n=3):
        rc = lib.sq_relabel_lut_i32(labels, out, N, P, off, lut, n, None)
        return rc, lib.sq_last_error()

    for kw in ({"labels": None}, {"out": None}, {"off": None}, {"lut": None}):
        rc, msg = call(**kw)
        assert rc == -1 and b"null" in msg, kw
    rc, msg = call(n=-1)
    assert rc == -1 and b"lut_len" in msg
    for kw in ({"N": 0}, {"N": 1 << 21}, {"P": 0}, {"P": 1 << 31}):
        rc, msg = call(**kw)
        assert rc == -1 and b"2^31" in msg, kw
    rc, msg = call(off=off + 4)
    assert rc == -1 and b"8-byte" in msg
    for kw in ({"out": labels + 4}, {"out": labels + 28}, {"off": out + 8}, {"lut": out}):
        rc, msg = call(**kw)
        assert rc == -1 and b"overlap" in msg, kw
