"""GPU: sq_label_overlap (both SQ_LINK_VEC forms, flipped in-process), sq_relabel_lut_i32 and
sequitr_amd/analysis/linking.py against the restatements of tests/link_cases.py.  Integer work: every byte of the sorted
pairs and of both area arrays must be equal, and every column of the track table, floats bit for bit."""
import os

import numpy as np
import pytest
import torch

from sequitr_amd import _lib
from sequitr_amd.analysis import linking
from tests import link_cases as lc

pytestmark = pytest.mark.gpu
GUARD = 64                                                      # int32 elements in front of and behind every buffer
FORMS = ("0", "1")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Form(object):
    """SQ_LINK_VEC for the calls inside: '0' the one-lane form, '1' the four-lane form; the variable is read per call"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.pop("SQ_LINK_VEC", None)
        os.environ["SQ_LINK_VEC"] = self.value

    def __exit__(self, *exc):
        os.environ.pop("SQ_LINK_VEC", None)
        if self.old is not None:
            os.environ["SQ_LINK_VEC"] = self.old


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


def overlap_raw(a_d, b_d, ml, max_pairs, areas=True):
    """one sq_label_overlap call into guarded buffers -> (pairs sorted, area_a, area_b, count, dropped)"""
    lib = _lib.load()
    N = a_d.shape[0]
    P = a_d.numel() // N
    nws = int(lib.sq_label_overlap_workspace(max_pairs))
    area = [Guarded(N * (ml + 1) * 2) for _ in range(2)]
    pairs, ctr, ws = Guarded(max_pairs * 4), Guarded(4), Guarded(nws // 4)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.sq_label_overlap(a_d.data_ptr(), b_d.data_ptr(), N, P, ml, area[0].t.data_ptr() if areas else None,
                                    area[1].t.data_ptr() if areas else None, pairs.t.data_ptr(), max_pairs, ctr.t.data_ptr(),
                                    ctr.t[1:].data_ptr(), ws.t.data_ptr(), st), "sq_label_overlap")
    torch.cuda.synchronize()
    assert all(g.intact() for g in area + [pairs, ctr, ws]), "a guard band was written"
    count, dropped, g2, g3 = ctr.t.cpu().numpy()
    assert g2 == g3 == ctr.fill
    rows = pairs.t.cpu().numpy().reshape(max_pairs, 4)
    assert 0 <= count <= max_pairs and np.all(rows[count:] == pairs.fill)
    rows = rows[:count].astype(np.int64)
    rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
    if not areas:                                               # NULL areas: nothing is written
        assert all(np.all(g.t.cpu().numpy() == g.fill) for g in area)
        return rows, None, None, int(count), int(dropped)
    aa, ab = (g.t.cpu().numpy().view(np.int64).reshape(N, ml + 1) for g in area)
    return rows, aa, ab, int(count), int(dropped)


def check_overlap(a_d, b_d, ml, what):
    """both forms, areas given and NULL, the rows exactly full and roomy, and the wrapper: every byte equals overlap_ref"""
    a, b = a_d.cpu().numpy(), b_d.cpu().numpy()
    want_p, want_a, want_b = lc.overlap_ref(a, b, ml)
    for form in FORMS:
        with Form(form):
            for max_pairs in (max(1, len(want_p)), 4 * len(want_p) + 3):
                for areas in (True, False):
                    p, aa, ab, count, dropped = overlap_raw(a_d, b_d, ml, max_pairs, areas)
                    assert dropped == 0 and count == len(want_p), (what, form, max_pairs, count, dropped)
                    assert p.tobytes() == want_p.tobytes(), (what, form, max_pairs)
                    if areas:
                        assert aa.tobytes() == want_a.tobytes() and ab.tobytes() == want_b.tobytes(), (what, form)
            p, aa, ab = linking.overlap_table(a_d, b_d, ml)
            assert p.dtype == aa.dtype == ab.dtype == np.int64
            assert p.tobytes() == want_p.tobytes() and aa.tobytes() == want_a.tobytes() and ab.tobytes() == want_b.tobytes()
    assert np.array_equal(a_d.cpu().numpy(), a) and np.array_equal(b_d.cpu().numpy(), b)   # the inputs are not written
    return want_p


@pytest.mark.parametrize("P", lc.WIDTHS)
def test_overlap_at_every_width(P):
    for N in (1, 3):
        a, b = lc.random_stack(P + N, N, P, 5), lc.random_stack(7 * P + N, N, P, 5, run=9)
        a[-1, :] = 1                                            # the last frame: one label that no other frame has in a
        b[-1, -1] = 5
        want = check_overlap(dev(a), dev(b), 5, "P=%d N=%d" % (P, N))
        if N == 3:                                              # nothing leaks between frames
            for n in range(N):
                alone = lc.overlap_ref(a[n:n + 1], b[n:n + 1], 5)[0]
                assert np.array_equal(want[want[:, 0] == n][:, 1:], alone[:, 1:])


@pytest.mark.parametrize("P", [64, 65, 128, 129, 256, 257, 1000])
def test_overlap_of_the_two_views_of_one_stack(P):
    stack = dev(lc.random_stack(P, 4, P, 6, density=0.7))
    a, b = stack[:-1], stack[1:]                                # b starts P elements in: 16-byte aligned iff P % 4 == 0
    assert a.data_ptr() % 16 == 0 and (b.data_ptr() % 16 == 0) == (P % 4 == 0)
    check_overlap(a, b, 6, "views P=%d" % P)


def run_cases():
    P = 1000
    ramp = (np.arange(P) // 7 % 5 + 1).astype(np.int32)
    cases = [("one_run_across_every_boundary", np.full((2, P), 3, np.int32), np.full((2, P), 2, np.int32), 3),
             ("a_changes_b_holds", np.stack([ramp, ramp[::-1]]), np.ones((2, P), np.int32), 5),
             ("b_changes_a_holds", np.full((2, P), 4, np.int32), np.stack([ramp[::-1], ramp]), 5),
             ("changes_inside_every_quad", np.tile(np.array([1, 1, 2, 2, 2, 3], np.int32), 200)[None, :1000],
              np.tile(np.array([1, 2, 2], np.int32), 334)[None, :1000], 3)]
    vals = np.array([-7, 0, 1, 6, 7, 8, -1, 2 ** 31 - 1, -2 ** 31, 6, 6, 7], np.int32)
    rng = np.random.default_rng(3)
    cases.append(("values_outside_the_range", rng.choice(vals, (2, 516)).astype(np.int32),
                  rng.choice(vals, (2, 516)).astype(np.int32), 7))
    same = lc.random_stack(11, 3, 260, 9)
    cases.append(("a_is_b", same, same, 9))
    cases.append(("all_zero", np.zeros((2, 300), np.int32), np.zeros((2, 300), np.int32), 4))
    return cases


@pytest.mark.parametrize("case", run_cases(), ids=lambda c: c[0])
def test_overlap_runs_and_values(case):
    name, a, b, ml = case
    a_d = dev(a)
    want = check_overlap(a_d, a_d if a is b else dev(b), ml, name)
    if name == "all_zero":
        assert len(want) == 0
    if name == "a_is_b":
        assert np.array_equal(want[:, 1], want[:, 2])


def test_every_position_its_own_label():
    n = 33 * 65
    a = np.arange(1, n + 1, dtype=np.int32).reshape(1, n)
    b = a[:, ::-1].copy()
    want = check_overlap(dev(a), dev(b), n, "unique labels")    # max_pairs == the number of pairs: every row is used
    assert len(want) == n and np.all(want[:, 3] == 1)
    for form in FORMS:                                          # fewer slots than pairs: the table itself fills up
        with Form(form):
            p, aa, ab, count, dropped = overlap_raw(dev(a), dev(b), n, 512)
            assert dropped != 0 and count <= 512 and np.array_equal(aa, lc.overlap_ref(a, b, n)[1])
            assert set(map(tuple, p.tolist())) <= set(map(tuple, want.tolist()))


def test_too_little_room_is_reported_and_the_wrapper_comes_back_with_more():
    a = np.array([[1, 1, 2, 2, 3, 0, 0, 3]], np.int32)
    b = np.array([[1, 2, 2, 3, 3, 1, 0, 0]], np.int32)
    want_p, want_a, want_b = lc.overlap_ref(a, b, 3)
    assert len(want_p) == 5
    a_d, b_d = dev(a), dev(b)
    for form in FORMS:
        with Form(form):
            p, aa, ab, count, dropped = overlap_raw(a_d, b_d, 3, 1)
            assert dropped != 0 and count <= 1 and np.array_equal(aa, want_a) and np.array_equal(ab, want_b)
            assert all(row in want_p.tolist() for row in p.tolist())
            p, aa, ab = linking.overlap_table(a_d, b_d, 3, max_pairs=1)
            assert np.array_equal(p, want_p) and np.array_equal(aa, want_a) and np.array_equal(ab, want_b)
            p, aa, ab = linking.overlap_table(a_d, b_d, max_pairs=1, areas=False)      # max_label from the data
            assert np.array_equal(p, want_p) and aa is None and ab is None


def test_twice_is_bit_identical_and_captured_graphs_replay_the_eager_bits():
    stack = dev(lc.random_stack(5, 5, 1028, 40, density=0.8))
    a, b, ml, max_pairs = stack[:-1], stack[1:], 40, 8192
    want_p, want_a, want_b = lc.overlap_ref(a.cpu().numpy(), b.cpu().numpy(), ml)
    lib = _lib.load()
    N, P = a.shape
    area = torch.empty((2, N, ml + 1), dtype=torch.int64, device="cuda")
    pairs = torch.empty((max_pairs, 4), dtype=torch.int32, device="cuda")
    ctr = torch.empty(2, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(lib.sq_label_overlap_workspace(max_pairs)) // 4, dtype=torch.int32, device="cuda")
    out = torch.empty_like(stack)
    offsets = dev(np.arange(6, dtype=np.int64) * 40)
    lut = dev(np.arange(200, dtype=np.int32)[::-1].copy())

    def both():                                                 # one linear chain of launches on the current stream
        st = torch.cuda.current_stream().cuda_stream
        _lib.check(lib.sq_label_overlap(a.data_ptr(), b.data_ptr(), N, P, ml, area[0].data_ptr(), area[1].data_ptr(),
                                        pairs.data_ptr(), max_pairs, ctr.data_ptr(), ctr[1:].data_ptr(), ws.data_ptr(), st),
                   "sq_label_overlap")
        linking.relabel(stack, offsets, lut, out=out)

    def result():
        count, dropped = ctr.cpu().numpy()
        rows = pairs[:count].cpu().numpy().astype(np.int64)
        assert dropped == 0
        return rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))], area.cpu().numpy(), out.cpu().numpy()

    for form in FORMS:
        with Form(form):
            both()
            first = result()
            both()
            second = result()
            assert all(x.tobytes() == y.tobytes() for x, y in zip(first, second))
            assert first[0].tobytes() == want_p.tobytes() and np.array_equal(first[1][0], want_a) \
                and np.array_equal(first[1][1], want_b)
            stream = torch.cuda.Stream()
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                both()                                          # warm up outside the capture
            torch.cuda.current_stream().wait_stream(stream)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                both()
            for _ in range(2):
                for t in (pairs, ctr, area, out):
                    t.fill_(-1)
                graph.replay()
                torch.cuda.synchronize()
                assert all(x.tobytes() == y.tobytes() for x, y in zip(first, result()))


# ---- relabel ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", lc.WIDTHS)
def test_relabel_at_every_width(P):
    N = 3
    labels = lc.random_stack(P, N, P, 9, density=0.8)
    labels[0, ::5] = -3                                         # negative, and beyond the frame's range
    labels[2, ::3] = 12
    offsets = np.array([0, 9, 9, 16], np.int64)                 # frame 1 is empty; frame 2 holds 7 objects: 8 and 9 read 0
    lut = (np.arange(16, dtype=np.int32) * 3 + 100)
    want = lc.relabel_ref(labels, offsets, lut)
    assert not want[1].any() and (P < 63 or (want[0].any() and want[2].any() and (want[2] == 0).any()))
    for shift in (0, 1):                                        # 16-byte aligned, and 4 bytes off it
        src, dst = Guarded(N * P + 1), Guarded(N * P + 1)
        s = src.t[shift:shift + N * P].view(N, P)
        s.copy_(dev(labels))
        d = dst.t[shift:shift + N * P].view(N, P)
        got = linking.relabel(s, offsets, lut, out=d)
        torch.cuda.synchronize()
        assert got is d and np.array_equal(d.cpu().numpy(), want) and np.array_equal(s.cpu().numpy(), labels)
        assert src.intact() and dst.intact()
        assert int(dst.t[N * P if shift == 0 else 0]) == dst.fill
        assert linking.relabel(s, offsets, lut, out=s) is s      # in place
        torch.cuda.synchronize()
        assert np.array_equal(s.cpu().numpy(), want) and src.intact()
    assert np.array_equal(linking.relabel(dev(labels), dev(offsets), dev(lut)).cpu().numpy(), want)
    # device data cannot be validated: a range that leaves the table reads as 0 beyond it
    beyond = np.array([0, 9, 9, 30], np.int64)
    assert np.array_equal(linking.relabel(dev(labels), beyond, lut).cpu().numpy(), lc.relabel_ref(labels, beyond, lut))
    assert not linking.relabel(dev(labels), np.zeros(4, np.int64), np.zeros(0, np.int32)).any()   # an empty table


# ---- link_labels ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reach", [0, 5])
def test_link_labels_equals_the_restated_rule(reach):
    labels, cls, who = lc.disk_movie()
    assert labels.shape == (6, 96, 130)
    want = lc.link_ref_labels(labels, cls, reach)
    lab_d = dev(labels)
    for form in FORMS:
        with Form(form):
            got = linking.link_labels(lab_d, cls, reach=reach)
            lc.assert_tracks(got.columns(), want, "reach %d form %s" % (reach, form))
    lc.check_consequences(got.columns(), lc.counts_of(labels))
    assert (got.children > 0).any() and (got.end < 5).any()     # a division, and a cell that vanished
    rows = [sum(len(w) for w in who[:t]) + who[t].index(4) for t in range(6)]
    assert len(set(got.track[rows].tolist())) == (1 if reach else 6)   # the jumping cell is rescued only by the reach
    # batches of 1, 2, 3 and F frames: identical tables
    for cut in (1, 2, 3, 6):
        linker = linking.FrameLinker(reach=reach)
        for first in range(0, 6, cut):
            linker.push_frames(lab_d[first:first + cut], cls[first:first + cut])
        lc.assert_tracks(linker.finish().columns(), want, "cut %d" % cut)
    # without classes every object is of class 0: the counts come from the frames
    lc.assert_tracks(linking.link_labels(lab_d, reach=reach, min_iou=0.1).columns(),
                     lc.link_ref_labels(labels, None, reach, min_iou=0.1), "no classes")
    # the relabelled video has one value per track, and that value is its ID
    offsets, lut = got.lut()
    video = linking.relabel(lab_d, offsets, lut).cpu().numpy()
    assert np.array_equal(video, lc.relabel_ref(labels, offsets, lut)) and np.array_equal(video > 0, labels > 0)
    for t in range(6):
        for l in range(1, len(who[t]) + 1):
            assert set(video[t][labels[t] == l].tolist()) == {int(got.track[offsets[t] + l - 1])}


def test_link_labels_on_volumes_in_time():
    labels, who = lc.volume_movie()
    assert labels.shape == (4, 3, 20, 33)
    want = lc.link_ref_labels(labels)
    got = linking.link_labels(dev(labels))
    lc.assert_tracks(got.columns(), want, "volumes")
    assert (got.children > 0).any()
    with pytest.raises(ValueError, match="not built"):
        linking.link_labels(dev(labels), reach=3)


def test_python_argument_checks():
    lab = torch.zeros((2, 8, 70), dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="contiguous"):
        linking.overlap_table(lab[:, :, :50], lab[:, :, :50])
    with pytest.raises(ValueError, match="one shape"):
        linking.overlap_table(lab, lab[:1])
    with pytest.raises(ValueError, match="max_label"):
        linking.overlap_table(lab, lab, max_label=1 << 21)
    with pytest.raises(_lib.SequitrHipError, match="GPU memory"):
        linking.overlap_table(lab.cpu(), lab.cpu())
    with pytest.raises(ValueError, match="offsets"):
        linking.relabel(lab, [0, 1], [1])
    with pytest.raises(ValueError, match="out must"):
        linking.relabel(lab, [0, 0, 0], [], out=lab[:1])
    with pytest.raises(_lib.SequitrHipError, match="overlap"):
        flat = torch.zeros(2 * 8 * 70 + 4, dtype=torch.int32, device="cuda")
        linking.relabel(flat[:1120].view(2, 8, 70), [0, 0, 0], [], out=flat[4:1124].view(2, 8, 70))
    p, aa, ab = linking.overlap_table(lab, lab)                 # nothing anywhere
    assert p.shape == (0, 4) and not aa.any() and not ab.any()
