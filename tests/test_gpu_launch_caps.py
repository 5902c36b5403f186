"""GPU: the mask-analysis kernels on launches above their grid caps (tests/launch_cap_cases.py is the table, and
tests/test_launch_cap_plan.py shows on the CPU that its rows do what this file relies on): the second trip of every
grid-stride loop, the ragged last trip, a third trip, and the index arithmetic between trips -- for the component
operations, both splitters in both forms of the regrowth, the zones and contact graphs in a plane and in a volume, the
overlap table in both SQ_LINK_VEC forms (WaveWalk's carry), the relabelling at V = 1 and V = 4, and the mask stitcher.

Integer work throughout: every comparison is equality of every byte, word and row with the existing references
(mask_cleanup_cases, volume_cleanup_cases, mask_split_cases, volume_split_cases, neighbors_cases, neighbors3d_cases,
link_cases, oracle.frontend_ref; the overlap of 5 * 10^7 positions against launch_cap_cases.overlap_packed, which the plan
test shows equal to link_cases.overlap_ref).  A mismatch is reported with its first flat index, the trip it lies in and its
offset within the trip.  Every output is a view inside a larger buffer of 0xA5 bytes and is itself 0xA5 before the call: a
trip that wrote nothing leaves the sentinel, and the 4 KiB on either side must come back untouched.  Workspaces are passed
in, 0xFF before the call, and once per family a call is repeated on a workspace of other bytes: the result does not
depend on what the workspace held.

Times measured on the MI355X host; each test prints its own with -s.  GPU: HIP events round the calls under test, all
forms and repeats of a test together.  Whole test: generation, references, uploads, downloads and comparisons; a reference
that several tests share is charged to the first.  The file takes 15 s there, of which the GPU works 0.08 s.

    test                                         GPU ms               whole test s
    fill_holes + clear_border   plane2 / plane3  1.8 / 1.8            0.49 / 0.30
    fill_cavities + clear_border3d
                     volume2 / volume3 / thin    2.1 / 2.8 / 1.7      0.47 / 0.76 / 0.23
    split                       plane2 / plane3  1.2 / 1.1            0.23 / 0.38
    split3d                   volume2 / volume3  2.2 / 2.7            0.38 / 0.48
    label_zones               labels2 / labels3  1.7 / 0.7            1.21 / 1.14
    label_zones3d         labelvol2 / labelvol3  5.2 / 3.1            1.05 / 1.04
    zone_graph labels2, zone_graph3d labelvol2   3.1, 3.9             0.36, 1.26
    tables of 2^23 slots                         0.3                  0.15
    overlap                one-lane / four-lane  32.0 / 4.0           0.51 / 0.92
    relabel    relabel1 / relabel1x3 / relabel4  0.6 / 0.8 / 0.7      0.12 / 0.21 / 0.59
    stitch                    stitch2 / stitch3  1.8 / 0.2            0.05 / 0.06

The CPU side is the references; it is nearly all of the "whole test" column above.  (The thin volume's fill is not run
slice by slice: its 140 002 slices of 3 x 5 hold no hole, and scipy took 12 s of that column for them.)  On `thin` the
face enumerator's own launch passes the cap as well; its `late` content -- runs and pockets that only face items of the
second trip reach -- is what shows that trip in the outputs (the plan test proves that it does).
"""
import time

import numpy as np
import pytest
import torch

from oracle import frontend_ref
from sequitr_amd import _lib, maskops, volumeops
from sequitr_amd.analysis import linking, neighbors
from sequitr_amd.frontend import FrameTiler
from tests import launch_cap_cases as lcc
from tests import link_cases as lc
from tests import mask_cleanup_cases as mc
from tests import mask_split_cases as sc
from tests import neighbors3d_cases as n3
from tests import neighbors_cases as nc
from tests import volume_cleanup_cases as vc
from tests import volume_split_cases as vs

pytestmark = pytest.mark.gpu
PAD = 4096                                                      # bytes on either side of every output
SENTINEL, WS_BYTE = 0xA5, 0xFF
C = 3
CC, NB, FE = (lcc.cap_items(h) for h in ('cc_grid', 'nb_grid', 'fe_grid'))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Guarded(object):
    """a tensor of `shape` and `dtype` filled with the byte `fill`, a 16-byte aligned view inside a larger buffer of it"""

    def __init__(self, shape, dtype=torch.uint8, fill=SENTINEL):
        self.fill = fill
        self.nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        self.buf = torch.full((self.nbytes + 2 * PAD,), fill, dtype=torch.uint8, device="cuda")
        self.out = self.buf[PAD:PAD + self.nbytes].view(dtype).view(*shape)
        assert self.out.data_ptr() % 16 == 0 and self.out.is_contiguous()

    def refill(self, byte=None):
        self.fill = self.fill if byte is None else byte
        self.buf.fill_(self.fill)
        return self

    def check(self, what):
        lo, hi = self.buf[:PAD], self.buf[PAD + self.nbytes:]
        assert bool((lo == self.fill).all()), "%s wrote in front of its buffer" % what
        assert bool((hi == self.fill).all()), "%s wrote past its buffer" % what
        return self.out

    def numpy(self, what):
        return self.check(what).cpu().numpy()


def workspace(nbytes, byte=WS_BYTE):
    return Guarded(((int(nbytes) + 15) // 16 * 4,), torch.int32, byte)


class Clock(object):
    """GPU time of the calls under test, by events round each"""

    def __init__(self):
        self.ms, self.t0 = 0.0, time.time()

    def __call__(self, fn, *args, **kwargs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn(*args, **kwargs)
        e1.record()
        e1.synchronize()
        self.ms += e0.elapsed_time(e1)
        return out


@pytest.fixture
def clock(request):
    c = Clock()
    yield c
    print("%s: GPU %.2f ms, whole test %.2f s" % (request.node.name, c.ms, time.time() - c.t0))


_CACHE = {}


def cached(key, make):
    """inputs and references are computed once per module and never written"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


@pytest.fixture(scope="module", autouse=True)
def release_the_cache():
    yield
    _CACHE.clear()                                              # some 0.5 GB of inputs and references, host and device


def mask_input(name):
    def make():
        kind, shape = lcc.INPUTS[name]
        gen = {'mask': lcc.plane_mask, 'volume': lcc.volume_mask, 'thin': lcc.thin_volume}[kind]
        m, info = gen(shape, CC)
        md = dev(m)
        m.setflags(write=False)
        return m, info, md
    return cached(('input', name), make)


def label_input(name):
    def make():
        kind, shape = lcc.INPUTS[name]
        lab, info = (lcc.label_frames if kind == 'labels' else lcc.label_volumes)(shape, NB)
        lab_d = dev(lab)
        lab.setflags(write=False)
        return lab, info, lab_d
    return cached(('input', name), make)


def window_box(w):
    return (w['frame'], slice(*w['rows'])) + ((slice(*w['box']),) if 'box' in w else ())


def run_mask_op(clock, fn, md, ws_bytes, what, want, again=False, **kw):
    """fn(mask, ..., out=, workspace=) into a guarded output on a 0xFF workspace; with `again` once more on other bytes"""
    g, ws = Guarded(tuple(md.shape)), workspace(ws_bytes)
    for byte in (WS_BYTE, 0x5A)[:2 if again else 1]:
        g.refill()
        ws.refill(byte)
        assert clock(fn, md, out=g.out, workspace=ws.out, classes=C, **kw) is g.out
        torch.cuda.synchronize()
        ws.check(what + ": the workspace")
        lcc.first_difference(g.numpy(what), want, CC, "%s (workspace of 0x%02X)" % (what, byte))


# ---- the component operations ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plane2", "plane3"])
def test_fill_holes_and_clear_border_of_frames(clock, name):
    m, info, md = mask_input(name)
    lib = _lib.load()
    wants = []
    for limit in (None, lcc.SMALL_AREA):                        # the small limit also runs count_kernel
        want = cached(('fill', name, limit), lambda: mc.fill_holes_ref(m, limit, C))
        wants.append(want)
        assert all((want[window_box(w)] != m[window_box(w)]).any() for w in info['windows'])
        run_mask_op(clock, maskops.fill_holes, md, lib.sq_mask_fill_holes_workspace(*m.shape), "fill_holes %s max_area %s"
                    % (name, limit), want, again=limit is None, max_area=limit)
    assert not np.array_equal(*wants)
    want = cached(('clear', name), lambda: mc.clear_border_ref(m, C))
    assert all((want[window_box(w)] != m[window_box(w)]).any() for w in info['windows'])
    run_mask_op(clock, maskops.clear_border, md, lib.sq_mask_clear_border_workspace(*m.shape), "clear_border " + name, want,
                again=True)
    assert np.array_equal(md.cpu().numpy(), m)


@pytest.mark.parametrize("name", ["volume2", "volume3", "thin"])
def test_fill_cavities_and_clear_border3d(clock, name):
    m, info, md = mask_input(name)
    lib = _lib.load()
    N, D, H, W = m.shape
    for planar in (False, True)[:1 if name == 'thin' else 2]:   # 3 x 5 slices hold no hole, and 140 002 of them cost scipy 12 s
        nws = lib.sq_mask_fill_holes_workspace(N * D, H, W) if planar else lib.sq_volume_fill_holes_workspace(N, D, H, W)
        wants = []
        for limit in (None, lcc.SMALL_AREA):
            want = cached(('fill', name, limit, planar), lambda: vc.fill_ref(m, limit, C, planar))
            wants.append(want)
            assert all((want[window_box(w)] != m[window_box(w)]).any() for w in info['windows'] if name != 'thin')
            what = "fill_cavities %s max_voxels %s planar %s" % (name, limit, planar)
            run_mask_op(clock, volumeops.fill_cavities, md, nws, what, want, again=limit is None and not planar,
                        max_voxels=limit, planar=planar)
        assert planar or not np.array_equal(*wants)        # a slice's holes are small: the limit tells cavities apart
        assert not np.array_equal(wants[0], m)
    cleared = []
    for faces in vc.FACES:                                      # on `thin`, N * face_count passes the cap too: FACE_ROWS
        want = cached(('clear', name, faces), lambda: vc.clear_border_ref(m, C, faces))
        cleared.append(want)
        run_mask_op(clock, volumeops.clear_border3d, md, lib.sq_volume_clear_border_workspace(N, D, H, W),
                    "clear_border3d %s faces %s" % (name, faces), want, again=faces == 'lateral', faces=faces)
    assert not np.array_equal(*cleared) and cleared[1].any()
    if name == 'thin':                                          # what only face_roots_kernel's second trip reaches
        late = info['late']
        v, W = late['frame'], m.shape[3]
        for c, z0, z1 in late['runs']:
            assert (m[v, z0:z1, 1, W - 1] == c).all() and not any(want[v, z0:z1, 1, W - 1].any() for want in cleared)
        filled = cached(('fill', name, None, False), lambda: vc.fill_ref(m, None, C))   # computed above
        for c, z0, z1 in late['pockets']:
            assert not filled[v, z0:z1, 1, 2:].any() and (filled[v, z0 - 1, 1, 2:] == c).all()
    assert np.array_equal(md.cpu().numpy(), m)


# ---- the splitters ---------------------------------------------------------------------------------------------------
def forms(monkeypatch, switch, fn):
    """fn(what) in the default form and with the one-step-per-launch regrowth; the switch is read per call"""
    monkeypatch.delenv(switch, raising=False)
    fn("default form")
    monkeypatch.setenv(switch, "0")
    fn(switch + "=0")
    monkeypatch.delenv(switch, raising=False)


@pytest.mark.parametrize("name", ["plane2", "plane3"])
def test_split_of_frames(clock, monkeypatch, name):
    m, info, md = mask_input(name)
    r = lcc.PLANE_FULL['r']
    want = cached(('split', name), lambda: sc.split_ref(m, r, 'cross', None, C))
    for w in info['windows']:                                   # cuts are really made in every trip
        assert (want[window_box(w)] != m[window_box(w)]).any(), w['name']
    nws = _lib.load().sq_mask_split_workspace(*m.shape)
    forms(monkeypatch, "SQ_SPLIT_LDS", lambda what: run_mask_op(clock, maskops.split, md, nws, "split %s, %s" % (name, what),
                                                                 want, again=True, erosions=r, structure='cross'))


@pytest.mark.parametrize("name", ["volume2", "volume3"])
def test_split3d_of_volumes(clock, monkeypatch, name):
    m, info, md = mask_input(name)
    r = lcc.VOLUME_FULL['r']
    want = cached(('split', name), lambda: vs.split3d_ref(m, r, 'cross', None, C))
    for w in info['windows']:
        assert (want[window_box(w)] != m[window_box(w)]).any(), w['name']
    nws = _lib.load().sq_volume_split_workspace(*m.shape)
    forms(monkeypatch, "SQ_SPLIT3D_LDS", lambda what: run_mask_op(clock, volumeops.split3d, md, nws,
                                                                   "split3d %s, %s" % (name, what), want, again=True,
                                                                   erosions=r, structure='cross'))


# ---- zones -----------------------------------------------------------------------------------------------------------
REACH = 6


def run_zones(clock, fn, lab_d, nws, want, what, d2_dtype, ws_byte=WS_BYTE, **kw):
    """zones (and the distance when `want` holds one) into guarded outputs on a filled workspace"""
    zones, ws = Guarded(tuple(lab_d.shape), torch.int32), workspace(nws, ws_byte)
    d2 = Guarded(tuple(lab_d.shape), d2_dtype) if want[1] is not None else None
    clock(fn, lab_d, out=zones.out, distance_out=None if d2 is None else d2.out, workspace=ws.out,
          max_label=lcc.MAX_LABEL, **kw)
    torch.cuda.synchronize()
    ws.check(what + ": the workspace")
    lcc.first_difference(zones.numpy(what), want[0], NB, what + " zones")
    if d2 is not None:
        lcc.first_difference(d2.numpy(what), want[1], NB, what + " distance")


@pytest.mark.parametrize("name", ["labels2", "labels3"])
def test_label_zones_of_frames(clock, name):
    lab, info, lab_d = label_input(name)
    nws = _lib.load().sq_label_zones_workspace(*lab.shape)
    full = cached(('zones', name, 0), lambda: nc.zones_ref(lab, lcc.MAX_LABEL, 0))
    for f, y, x, small in info['ties']:                         # an equidistant pair of seeds in every window
        assert full[0][f, y, x] == small and full[1][f, y, x] == 9
    run_zones(clock, neighbors.label_zones, lab_d, nws, (full[0], None), "label_zones " + name, torch.int32)
    for byte in (WS_BYTE, 0x5A):
        run_zones(clock, neighbors.label_zones, lab_d, nws, full, "label_zones %s with the distance" % name, torch.int32, byte)
    if name == "labels2":                                       # within a finite reach: the other form of the column kernel
        near = cached(('zones', name, REACH), lambda: nc.zones_ref(lab, lcc.MAX_LABEL, REACH))
        assert (near[0] != full[0]).any()
        run_zones(clock, neighbors.label_zones, lab_d, nws, (near[0], None), "label_zones %s within %d" % (name, REACH),
                  torch.int32, max_distance=REACH)
        run_zones(clock, neighbors.label_zones, lab_d, nws, near, "label_zones %s within %d with the distance" % (name, REACH),
                  torch.int32, max_distance=REACH)
    assert np.array_equal(lab_d.cpu().numpy(), lab)


def planar_half(name, lab):
    return cached(('planar', name), lambda: n3.planar_ref(lab, lcc.MAX_LABEL))


@pytest.mark.parametrize("name", ["labelvol2", "labelvol3"])
def test_label_zones3d_of_volumes(clock, monkeypatch, name):
    lab, info, lab_d = label_input(name)
    nws = _lib.load().sq_label_zones3d_workspace(*lab.shape)
    full = cached(('zones3d', name, 0), lambda: n3.zones3d_from_planar(*planar_half(name, lab)))
    for v, z, y, x, small in info['ties']:
        assert full[0][v, z, y, x] == small and full[1][v, z, y, x] == 9.0

    def run(what):
        what = "label_zones3d %s, %s" % (name, what)
        run_zones(clock, neighbors.label_zones3d, lab_d, nws, (full[0], None), what, torch.float64)
        run_zones(clock, neighbors.label_zones3d, lab_d, nws, full, what + ", with the distance", torch.float64, 0x5A)
        if name == "labelvol2":
            near = cached(('zones3d', name, REACH),
                          lambda: n3.zones3d_from_planar(*planar_half(name, lab), max_distance=REACH))
            assert (near[0] != full[0]).any()
            run_zones(clock, neighbors.label_zones3d, lab_d, nws, (near[0], None), "%s, within %d" % (what, REACH),
                      torch.float64, max_distance=REACH)
            run_zones(clock, neighbors.label_zones3d, lab_d, nws, near, "%s, within %d, with the distance" % (what, REACH),
                      torch.float64, 0x5A, max_distance=REACH)

    forms(monkeypatch, "SQ_ZONES3D_LDS", run)                   # =0: zones3d_depth_kernel, the global-memory form
    assert np.array_equal(lab_d.cpu().numpy(), lab)


# ---- contact graphs and the overlap table: one raw call into guarded buffers ----------------------------------------
def table_call(entry, width, tensors, dims, ml, max_pairs, stats_shape, ws_byte=WS_BYTE, areas=True, clock=None):
    """sq_zone_graph / sq_zone_graph3d / sq_label_overlap -> (rows sorted, stats or (area_a, area_b), count, dropped)"""
    lib = _lib.load()
    nws = int(getattr(lib, entry + "_workspace")(max_pairs))
    ws = workspace(nws, ws_byte)
    pairs, ctr = Guarded((max_pairs, width), torch.int32), Guarded((4,), torch.int32)
    st = torch.cuda.current_stream().cuda_stream
    if entry == "sq_label_overlap":
        stats = [Guarded(stats_shape, torch.int64) for _ in range(2)]
        args = [t.data_ptr() for t in tensors] + list(dims) + [ml] + [s.out.data_ptr() if areas else None for s in stats]
    else:
        stats = [Guarded(stats_shape, torch.int64)]
        args = [tensors[0].data_ptr()] + list(dims) + [ml, stats[0].out.data_ptr()]
    args += [pairs.out.data_ptr(), max_pairs, ctr.out.data_ptr(), ctr.out[1:].data_ptr(), ws.out.data_ptr(), st]
    call = lambda: _lib.check(getattr(lib, entry)(*args), entry)   # noqa: E731
    clock(call) if clock is not None else call()
    torch.cuda.synchronize()
    ws.check(entry + ": the workspace")
    count, dropped, g2, g3 = (int(v) for v in ctr.numpy(entry + " counters"))
    assert g2 == g3 == np.frombuffer(bytes([SENTINEL] * 4), np.int32)[0]
    rows = pairs.numpy(entry + " pairs")
    assert 0 <= count <= max_pairs and np.all(rows[count:].view(np.uint8) == SENTINEL), "rows beyond count were written"
    rows = rows[:count].astype(np.int64)
    rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
    if entry == "sq_label_overlap" and not areas:
        assert all(np.all(s.numpy(entry).view(np.uint8) == SENTINEL) for s in stats)
        return rows, None, count, dropped
    got = [s.numpy(entry + " stats") for s in stats]
    return rows, got[0] if len(got) == 1 else got, count, dropped


def same_rows(got, want, what):
    assert got.shape == want.shape, "%s: %d rows, want %d" % (what, len(got), len(want))
    if not np.array_equal(got, want):
        i = int(np.flatnonzero((got != want).any(1))[0])
        raise AssertionError("%s: row %d is %s, want %s" % (what, i, got[i], want[i]))


def test_zone_graph_of_big_frames(clock):
    """launch_cap_cases.BIG_INPUT_ROWS: the row kernel's grid is not capped; the capped launches are in the table test below"""
    lab, info, lab_d = label_input("labels2")
    zones = cached(('zones', "labels2", 0), lambda: nc.zones_ref(lab, lcc.MAX_LABEL, 0))[0]
    stats, pairs = cached(('graph', "labels2"), lambda: nc.graph_ref(zones, lcc.MAX_LABEL))
    zd = dev(zones)
    N = zones.shape[0]
    for byte in (WS_BYTE, 0x5A):
        rows, st, count, dropped = table_call("sq_zone_graph", 4, [zd], zones.shape, lcc.MAX_LABEL, 1024,
                                              (N, lcc.MAX_LABEL + 1, 2), byte, clock=clock)
        assert dropped == 0 and count == len(pairs)
        same_rows(rows, pairs, "zone_graph labels2")
        lcc.first_difference(st, stats, NB, "zone_graph labels2 stats")
    st, rows = neighbors.zone_graph(zd, lcc.MAX_LABEL)
    assert np.array_equal(st, stats) and np.array_equal(rows, pairs)


def test_zone_graph3d_of_a_big_volume(clock):
    """launch_cap_cases.BIG_INPUT_ROWS, as above"""
    lab, info, lab_d = label_input("labelvol2")
    zones = cached(('zones3d', "labelvol2", 0), lambda: n3.zones3d_from_planar(*planar_half("labelvol2", lab)))[0]
    stats, pairs = n3.graph3d_ref(zones, lcc.MAX_LABEL)
    zd = dev(zones)
    rows, st, count, dropped = table_call("sq_zone_graph3d", 5, [zd], zones.shape, lcc.MAX_LABEL, 1024,
                                          (zones.shape[0], lcc.MAX_LABEL + 1, 2), clock=clock)
    assert dropped == 0 and count == len(pairs)
    same_rows(rows, pairs, "zone_graph3d labelvol2")
    lcc.first_difference(st, stats, NB, "zone_graph3d labelvol2 stats")
    st, rows = neighbors.zone_graph3d(zd, lcc.MAX_LABEL)
    assert np.array_equal(st, stats) and np.array_equal(rows, pairs)


def test_tables_of_2_to_the_23_slots_give_the_rows_of_the_default_capacity(clock):
    """max_pairs = 2^22 on small inputs: the clear and the compaction walk the table in several trips (TABLE_ROWS)"""
    ml = 6
    z2 = nc.random_zones(3, 2, 33, 70, ml)[1]
    z3 = n3.random_zones(3, 2, 5, 17, 70, ml)[1]
    a, b = lcc.overlap_stacks(3, 1028)
    cases = [("sq_zone_graph", 4, [dev(z2)], z2.shape, ml, (2, ml + 1, 2), nc.graph_ref(z2, ml)),
             ("sq_zone_graph3d", 5, [dev(z3)], z3.shape, ml, (2, ml + 1, 2), n3.graph3d_ref(z3, ml)),
             ("sq_label_overlap", 4, [dev(a), dev(b)], (3, 1028), lcc.OVERLAP_MAX_LABEL, (3, lcc.OVERLAP_MAX_LABEL + 1),
              lc.overlap_ref(a, b, lcc.OVERLAP_MAX_LABEL))]
    for entry, width, tensors, dims, label, stats_shape, want in cases:
        small = table_call(entry, width, tensors, dims, label, 1024, stats_shape)
        for byte in (WS_BYTE, 0x5A):
            big = table_call(entry, width, tensors, dims, label, lcc.BIG_PAIRS, stats_shape, byte, clock=clock)
            assert big[2] == small[2] and big[3] == small[3] == 0, (entry, big[2:], small[2:])
            same_rows(big[0], small[0], entry + " with 2^23 slots")
            if entry == "sq_label_overlap":
                same_rows(big[0], want[0], entry)
                assert all(np.array_equal(g, s) and np.array_equal(g, w) for g, s, w in zip(big[1], small[1], want[1:]))
            else:
                same_rows(big[0], want[1], entry)
                assert np.array_equal(big[1], small[1]) and np.array_equal(big[1], want[0])


# ---- the overlap table past chunk_grid's cap -------------------------------------------------------------------------
def check_overlap(clock, monkeypatch, name, form):
    N, P = lcc.INPUTS[name][1]
    ml = lcc.OVERLAP_MAX_LABEL
    a, b = lcc.overlap_stacks(N, P)
    want_p, want_a, want_b = lcc.overlap_packed(a, b, ml)
    a_d, b_d = dev(a), dev(b)
    del a, b
    assert a_d.data_ptr() % 16 == 0 and b_d.data_ptr() % 16 == 0
    monkeypatch.setenv("SQ_LINK_VEC", form)
    room = max(4096, 2 * len(want_p))                           # a table that fills up probes every slot: give it room at once
    for areas in (True, False):
        rows, area, count, dropped = table_call("sq_label_overlap", 4, [a_d, b_d], (N, P), ml, room, (N, ml + 1),
                                                WS_BYTE if areas else 0x5A, areas, clock)
        what = "overlap %s SQ_LINK_VEC=%s areas %s" % (name, form, areas)
        assert dropped == 0 and count == len(want_p), (what, count, dropped, len(want_p))
        same_rows(rows, want_p, what)
        if areas:
            for got, want, side in zip(area, (want_a, want_b), "ab"):
                if not np.array_equal(got, want):
                    n, l = (int(v[0]) for v in np.nonzero(got != want))
                    raise AssertionError("%s: area_%s of frame %d, label %d is %d, want %d" % (what, side, n, l, got[n, l],
                                                                                              want[n, l]))
    p, aa, ab = linking.overlap_table(a_d, b_d, ml, max_pairs=room)
    assert np.array_equal(p, want_p) and np.array_equal(aa, want_a) and np.array_equal(ab, want_b)
    monkeypatch.delenv("SQ_LINK_VEC", raising=False)


def test_overlap_one_lane_past_the_cap(clock, monkeypatch):
    """3 frames of 65 600 wave-chunks: 65 472 of the steps a wave takes carry into the next frame, 256 do not"""
    check_overlap(clock, monkeypatch, "overlap1", "0")


def test_overlap_four_lane_past_the_cap(clock, monkeypatch):
    """45 000 frames of 3 wave-chunks of 512 positions (P % 4 == 0, both stacks on 16 bytes)"""
    check_overlap(clock, monkeypatch, "overlap4", "1")


# ---- relabel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["relabel1", "relabel1x3", "relabel4"])
def test_relabel_past_the_cap(clock, name):
    N, P = lcc.INPUTS[name][1]
    chunk = 1024 if name == "relabel4" else 256
    cap = lcc.cap_items('chunk_grid/relabel') * chunk           # positions of a trip, but for the ragged last chunk of a frame
    labels, offsets, lut = lcc.relabel_case(N, P)
    want = lc.relabel_ref(labels, offsets, lut)
    assert (P % 4 == 0) == (name == "relabel4") and all(want[n].any() for n in range(N) if n % 7 != 2)
    src, dst = Guarded((N, P), torch.int32), Guarded((N, P), torch.int32)
    src.out.copy_(dev(labels))
    assert clock(linking.relabel, src.out, offsets, lut, out=dst.out) is dst.out
    torch.cuda.synchronize()
    lcc.first_difference(dst.numpy("relabel"), want, cap, "relabel %s, out of place" % name)
    assert np.array_equal(src.numpy("relabel"), labels)
    assert clock(linking.relabel, src.out, offsets, lut, out=src.out) is src.out
    torch.cuda.synchronize()
    lcc.first_difference(src.numpy("relabel in place"), want, cap, "relabel %s, in place" % name)


# ---- the mask stitcher -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stitch2", "stitch3"])
def test_stitch_past_the_cap(clock, name):
    F, H, W = lcc.INPUTS[name][1]
    tl = FrameTiler((H, W), tile=512, margin=32, device="cuda:0")
    rng = np.random.default_rng(F)
    masks = rng.integers(0, 3, (F * tl.TR * tl.TC, 512, 512), dtype=np.uint8)
    want = frontend_ref.stitch(masks, tl.oy, tl.ox, tl.ymap, tl.xmap, H, W)
    md, g = dev(masks), Guarded((F, H, W))
    lib = _lib.load()
    clock(lambda: _lib.check(lib.sq_stitch_masks_u8(md.data_ptr(), tl._ymap.data_ptr(), tl._xmap.data_ptr(), g.out.data_ptr(),
                                                    F, H, W, tl.TR, tl.TC, tl.T, torch.cuda.current_stream().cuda_stream),
                             "sq_stitch_masks_u8"))
    torch.cuda.synchronize()
    lcc.first_difference(g.numpy("stitch"), want, FE, "stitch " + name)
    lcc.first_difference(clock(tl.stitch, md).cpu().numpy(), want, FE, "FrameTiler.stitch " + name)
    # a tiling of the frames stitched back is the frames themselves
    ident = ((np.arange(H)[:, None] * 7 + np.arange(W)[None]) % 251 + np.arange(F)[:, None, None]).astype(np.uint8)
    tiles = tl.tiles(dev(ident), normalise=False).to(torch.uint8).reshape(-1, 512, 512).contiguous()
    lcc.first_difference(clock(tl.stitch, tiles).cpu().numpy(), ident, FE, "tile then stitch " + name)
