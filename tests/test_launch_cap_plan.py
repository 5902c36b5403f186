"""CPU: the plan behind tests/test_gpu_launch_caps.py.  The four grid caps of tests/launch_cap_cases.py are the ones in the
source; every row of its table passes its cap by a ragged amount, with placed content round every trip boundary and a
component across it; the restated WaveWalk of sq_link.hip visits every wave-chunk once, with steps that carry and steps
that do not; and the generators, run at a cap of a few blocks, give references equal to the pure-Python restatements of
the case files."""
import os
import re

import numpy as np
import pytest
from scipy import ndimage

from tests import launch_cap_cases as lcc
from tests import link_cases as lc
from tests import mask_cleanup_cases as mc
from tests import mask_split_cases as sc
from tests import neighbors3d_cases as n3
from tests import neighbors_cases as nc
from tests import volume_cleanup_cases as vc
from tests import volume_split_cases as vs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERATORS = {'mask': (lcc.plane_mask, 'cc_grid'), 'volume': (lcc.volume_mask, 'cc_grid'), 'thin': (lcc.thin_volume, 'cc_grid'),
              'labels': (lcc.label_frames, 'nb_grid'), 'labelvol': (lcc.label_volumes, 'nb_grid')}


def helper_text(helper):
    name = helper.split('/')[0]
    text = open(os.path.join(ROOT, lcc.CAPS[helper]['file'])).read()
    m = re.search(r'inline unsigned %s\(int64_t \w+\) \{(.*?)\n?\}' % name, text, re.S)
    assert m, "%s is no longer defined in %s" % (name, lcc.CAPS[helper]['file'])
    line = text[:m.start()].count('\n') + 1
    assert line == lcc.CAPS[helper]['line'], "%s now stands at %s:%d: move the table's pointer" % (
        name, lcc.CAPS[helper]['file'], line)
    return m.group(1)


# ---- the caps ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("helper", sorted(lcc.CAPS))
def test_the_table_restates_the_caps_of_the_source(helper):
    body = helper_text(helper)
    m = re.search(r'> (\d+) \? (\d+)', body)
    assert m and m.group(1) == m.group(2), body
    assert int(m.group(1)) == lcc.CAPS[helper]['blocks'], "%s caps at %s blocks, the table says %d: move its rows" % (
        helper, m.group(1), lcc.CAPS[helper]['blocks'])
    if not helper.startswith('chunk_grid'):
        assert '(items + 255) / 256' in body and lcc.CAPS[helper]['per_block'] == lcc.THREADS
    assert lcc.cap_items(helper) == lcc.CAPS[helper]['blocks'] * lcc.CAPS[helper]['per_block']


def test_what_a_block_of_the_link_kernels_covers():
    text = open(os.path.join(ROOT, 'sequitr_amd/csrc/sq_link.hip')).read()
    assert 'step = (int64_t)gridDim.x * 4;' in text              # four waves of a block, a wave-chunk each
    assert text.count('chunk_grid((waves + 3) / 4)') == 2
    assert 'constexpr int LANE_U = 4;' in text and 'constexpr int VEC_U = 2;' in text   # chunks of 64 * 4 and 256 * 2 positions
    assert 'for (int64_t c = blockIdx.x; c < total; c += gridDim.x)' in text             # relabel: a block-chunk per block
    assert 'chunk_grid((P + 1023) / 1024 * N)' in text and 'chunk_grid((P + 255) / 256 * N)' in text


def test_the_capped_launches_are_the_ones_the_table_names():
    """which helper sizes which launch: a launch moved to another helper must move its rows"""
    src = lambda f: open(os.path.join(ROOT, 'sequitr_amd/csrc', f)).read()   # noqa: E731
    assert 'tgrid(cc_grid(total)), fgrid(cc_grid(N * face_count(D, H, W, lateral)))' in src('sq_component_ops.hip')
    assert 'tgrid(cc_grid(total))' in src('sq_split.hip')       # both splits: one driver
    assert src('sq_neighbors.hip').count('dim3(nb_grid(px))') == 2
    n3d = src('sq_neighbors3d.hip')
    assert 'dim3(nb_grid(vox))' in n3d and 'dim3(nb_grid((int64_t)N * D * H * W))' in n3d
    for f in ('sq_zones.h', 'sq_link.hip'):                     # sq_zones.h: both zone graphs, one driver
        assert 'dim3(nb_grid(slots))' in src(f) and 'nb_grid(table_words >' in src(f)
    for f, run in (('sq_neighbors.hip', 'zone_graph_run<false>('), ('sq_neighbors3d.hip', 'zone_graph_run<true>(')):
        assert run in src(f)
    assert 'dim3(fe_grid((int64_t)F * H * W))' in src('sq_frontend.hip')


# ---- the rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", lcc.ROWS, ids=lambda r: "%s-%s" % (r[0], r[1]))
def test_a_row_passes_its_cap_by_a_ragged_amount(row):
    entry, name, helper, items, trips = row
    cap = lcc.cap_items(helper)
    kind, shape = lcc.INPUTS[name]
    assert items == lcc.row_items(entry, name)
    assert trips == -(-items // cap) and trips >= 2
    r = items - (trips - 1) * cap
    assert 0 < r < cap and r % 256 != 0, (items, cap, r)
    assert int(np.prod(shape)) < 2 ** 31 and shape[0] < 2 ** 21
    if kind == 'link':
        assert shape[1] < 2 ** 31
        if entry.endswith('V=1'):
            assert shape[1] % 4 != 0
        if entry.endswith('V=4') or entry.endswith('four-lane'):
            assert shape[1] % 4 == 0
        assert shape[1] % {'linking.overlap_table/one-lane': 256, 'linking.overlap_table/four-lane': 512,
                           'linking.relabel/V=1': 256, 'linking.relabel/V=4': 1024}[entry] != 0      # a ragged last chunk
    elif kind != 'thin':
        assert shape[-1] % 64 != 0                              # the row scans keep their carry


def test_every_family_has_three_trips_and_a_frame_that_starts_in_the_second():
    for family in ('cc_grid', 'nb_grid', 'fe_grid', 'chunk_grid'):
        rows = [r for r in lcc.ROWS if r[2].split('/')[0] == family]
        assert any(r[4] >= 3 for r in rows), family
        starts = False
        for entry, name, helper, items, trips in rows:
            shape, cap = lcc.INPUTS[name][1], lcc.cap_items(helper)
            per = items // shape[0]
            starts = starts or any(cap <= n * per < 2 * cap for n in range(1, shape[0]))
        assert starts, family


def test_face_and_table_rows():
    cap = lcc.cap_items('cc_grid')
    for name, lateral, items, trips in lcc.FACE_ROWS:
        N, D, H, W = lcc.INPUTS[name][1]
        assert items == N * lcc.face_count(D, H, W, lateral) and trips == -(-items // cap) == 2
        assert (items - cap) % 256 != 0
    slots = 2
    while slots < 2 * lcc.BIG_PAIRS:                            # graph_slots of sq_zones.h
        slots *= 2
    assert slots == 1 << 23
    text = open(os.path.join(ROOT, 'sequitr_amd/csrc/sq_zones.h')).read()
    assert 'while (s < 2 * max_pairs) s *= 2;' in text
    cap = lcc.cap_items('nb_grid')
    assert all(lcc.INPUTS[name][0] in ('labels', 'labelvol') for entry, name in lcc.BIG_INPUT_ROWS)
    for entry, kernel, items, trips in lcc.TABLE_ROWS:
        words = 1 if 'compact' in kernel else (4 if entry.endswith('3d') else 3)
        assert items == words * slots and trips == items // cap >= 2


def check_windows(arr, info, cap, min_patches):
    flat = arr.reshape(-1)
    inner = int(np.prod(arr.shape[2:]))
    for w in info['windows']:
        f, (lo, hi) = w['frame'], w['rows']
        patches = w.get('patches')
        if patches is not None:
            assert len(patches) >= min_patches and len(set(p[1] for p in patches)) >= 2, w['name']
            for p in patches:
                box = tuple(slice(p[i], p[i + 1]) for i in range(2, len(p), 2))
                assert box[0].start >= lo and box[0].stop <= hi
                assert (arr[f][box] == p[1]).any(), "%s: the %s of class %d is not there" % (w['name'], p[0], p[1])
        b = w['boundary']
        if b is None:
            continue
        first = (f * arr.shape[1] + lo) * inner
        assert first < b < first + (hi - lo) * inner, "%s does not straddle item %d" % (w['name'], b)
        cls, s0, s1 = w['bar'][0], w['bar'][-2], w['bar'][-1]
        where = w['bar'][1:-2]                                  # (x) in a frame, (y, x) in a volume
        comp, _ = ndimage.label(arr[f] == cls)
        a, z = (s0,) + tuple(where), (s1 - 1,) + tuple(where)
        assert comp[a] != 0 and comp[a] == comp[z], "%s: the bar is not one component" % w['name']
        ia = np.ravel_multi_index((f,) + a, arr.shape)
        iz = np.ravel_multi_index((f,) + z, arr.shape)
        assert ia // cap == b // cap - 1 and iz // cap == b // cap, "%s: the bar stays within one trip" % w['name']
    last = info['last']
    assert flat[-1] == last[0]
    names = [w['name'] for w in info['windows']]
    want = ['trip%d' % k for k in range(1, -(-arr.size // cap))]
    assert [n for n in names if n.startswith('trip')] == want
    if min_patches:
        assert names[0] == 'first' and names[-1] == 'last'
        assert info['windows'][0]['rows'][0] == 0 and info['windows'][-1]['rows'][1] == arr.shape[1]


def check_late_faces(m, info, cap):
    """face_roots_kernel's second trip shows in the outputs: for both settings of `faces`, on the mask and on a complement
    plane, some roots are flagged by face items >= cap and by no item below it, and the references differ from ones that
    enumerate the first `cap` face items only"""
    N, D, H, W = m.shape
    late = info['late']
    v = late['frame']
    for lateral in (True, False):
        vox = lcc.face_voxels(D, H, W, lateral)
        assert len(vox) == lcc.face_count(D, H, W, lateral)
        on_face = np.zeros((D, H, W), bool)
        on_face[:, 0] = on_face[:, -1] = on_face[:, :, 0] = on_face[:, :, -1] = True
        if not lateral:
            on_face[0] = on_face[-1] = True
        assert np.array_equal(np.unique(vox), np.flatnonzero(on_face))
        early, only_late = lcc.face_items_of(m.shape, lateral, v, cap)
        assert len(early) and len(only_late)
        for c in (1, 2):
            for P in (m[v] == c, m[v] != c):
                lab, _ = ndimage.label(P)
                lo = set(np.unique(lab.reshape(-1)[early]).tolist()) - {0}
                hi = set(np.unique(lab.reshape(-1)[only_late]).tolist()) - {0}
                assert hi - lo, "lateral %s class %d: no root is flagged by the second trip alone" % (lateral, c)
    box = (v, slice(*late['rows']))
    for faces in vc.FACES:
        want = vc.clear_border_ref(m, 3, faces)
        assert np.array_equal(want, lcc.clear_border_limited(m, 3, faces))
        cut = lcc.clear_border_limited(m, 3, faces, cap)
        assert (cut[box] != want[box]).any()
        assert not want[box][:, 1, W - 1].any() and m[box][:, 1, W - 1].any()      # the runs go, by the late items alone
    want = vc.fill_ref(m, None, 3)
    assert np.array_equal(want, lcc.fill_limited(m, 3))
    cut = lcc.fill_limited(m, 3, cap)
    for c, z0, z1 in late['pockets']:                           # a pocket stays open, by the late items alone
        assert not want[v, z0:z1, 1, 2:].any() and (cut[v, z0:z1, 1, 2:] == c).all()
    for c, z0, z1 in late['runs']:
        assert (m[v, z0:z1, 1, W - 1] == c).all()


@pytest.mark.parametrize("name", [n for n, v in lcc.INPUTS.items() if v[0] in GENERATORS])
def test_the_windows_of_a_full_size_input_hold_what_they_record(name):
    kind, shape = lcc.INPUTS[name]
    gen, helper = GENERATORS[kind]
    cap = lcc.cap_items(helper)
    arr, info = gen(shape, cap)
    assert arr.shape == shape
    check_windows(arr, info, cap, 3 if kind == 'thin' else 5)
    if kind == 'thin':
        check_late_faces(arr, info, cap)
    if kind == 'labels':
        for f, y, x, small in info['ties']:
            crop = arr[f:f + 1, y - 8:y + 9, x - 11:x + 12]
            assert nc.tie_pixels(crop, lcc.MAX_LABEL)[0, 8, 11]
    if kind == 'labelvol':
        for v, z, y, x, small in info['ties']:
            assert not arr[v, max(0, z - 4):z + 5, y - 8:y + 9, x - 11:x + 12].sum() - arr[v, z, y, x - 3] - arr[v, z, y, x + 3]
            assert nc.tie_pixels(arr[v, z:z + 1, y - 8:y + 9, x - 11:x + 12], lcc.MAX_LABEL)[0, 8, 11]


# ---- WaveWalk ---------------------------------------------------------------------------------------------------------
def link_rows():
    out = []
    for entry, name, helper, items, trips in lcc.ROWS:
        if helper == 'chunk_grid/overlap':
            N, P = lcc.INPUTS[name][1]
            out.append((name, N, items // N, lcc.cap_items(helper)))
    return out + [('scaled_few_frames', 3, 17, 32), ('scaled_many_frames', 40, 3, 32), ('scaled_three_trips', 5, 15, 32)]


@pytest.mark.parametrize("name,N,cpf,waves", link_rows(), ids=lambda v: v if isinstance(v, str) else "")
def test_the_wave_walk_visits_every_chunk_once_with_and_without_a_carry(name, N, cpf, waves):
    q, dc = divmod(waves, cpf)
    assert dc != 0 and N >= q + 2
    seen, carried, plain = lcc.walk(N, cpf, waves)
    assert len(seen) == N * cpf and sorted(seen) == [(n, c) for n in range(N) for c in range(cpf)]
    assert carried > 0 and plain > 0
    assert (carried, plain) == lcc.walk_counts(N, cpf, waves)
    if name == 'overlap1':
        assert (carried, plain) == (65472, 256)
    # a walk that drops the carry leaves frames' chunks out and counts others twice: the model tells the two apart
    broken, _, _ = lcc.walk(N, cpf, waves, carry=False)
    assert sorted(broken) != sorted(seen)


def test_a_dropped_carry_changes_the_table_of_a_scaled_down_stack():
    """the overlap case's sensitivity, on the CPU: count the chunks the broken walk visits, frame by frame"""
    N, cpf, waves, chunk = 3, 17, 32, 256
    P = (cpf - 1) * chunk + 77
    a, b = lcc.overlap_stacks(N, P)
    want = lcc.overlap_packed(a, b, lcc.OVERLAP_MAX_LABEL)

    def table(carry):
        pairs, aa, ab = {}, np.zeros_like(want[1]), np.zeros_like(want[2])
        for n, c in lcc.walk(N, cpf, waves, carry)[0]:
            if n >= N or c * chunk >= P:                        # c >= cpf: the kernel's `p < P` reads nothing there
                continue
            sl = slice(c * chunk, min(P, (c + 1) * chunk))
            p, x, y = lcc.overlap_packed(a[n:n + 1, sl], b[n:n + 1, sl], lcc.OVERLAP_MAX_LABEL)
            aa[n] += x[0]
            ab[n] += y[0]
            for _, la, lb, k in p:
                pairs[(n, la, lb)] = pairs.get((n, la, lb), 0) + k
        rows = np.array([list(k) + [v] for k, v in sorted(pairs.items())], np.int64).reshape(-1, 4)
        return rows, aa, ab

    good, bad = table(True), table(False)
    assert all(np.array_equal(g, w) for g, w in zip(good, want))
    assert not np.array_equal(bad[0], want[0]) and not np.array_equal(bad[1], want[1])


# ---- the generators at a cap of a few blocks -------------------------------------------------------------------------
def test_plane_masks_scaled_down():
    cap = lcc.cap_items('cc_grid', 9)
    obj = lcc.PLANE_SMALL
    m, info = lcc.plane_mask((3, 30, 67), cap, obj)
    assert m.size == 2 * cap + 1422
    check_windows(m, info, cap, 5)
    for limit in (None, lcc.SMALL_AREA):
        want = mc.fill_holes_ref(m, limit, 3)
        assert np.array_equal(want, mc.brute(m, {'op': 'fill_holes', 'max_area': limit}, 3))
        for w in info['windows']:
            assert (want[w['frame'], w['rows'][0]:w['rows'][1]] != m[w['frame'], w['rows'][0]:w['rows'][1]]).any()
    assert not np.array_equal(mc.fill_holes_ref(m, None, 3), mc.fill_holes_ref(m, lcc.SMALL_AREA, 3))
    want = mc.clear_border_ref(m, 3)
    assert np.array_equal(want, mc.brute(m, {'op': 'clear_border'}, 3)) and not np.array_equal(want, m)
    want = sc.split_ref(m, obj['r'], 'cross', None, 3)
    assert np.array_equal(want, sc.brute_split(m, obj['r'], 'cross', None, 3))
    for w in info['windows']:
        assert (want[w['frame'], w['rows'][0]:w['rows'][1]] != m[w['frame'], w['rows'][0]:w['rows'][1]]).any(), w['name']


def test_volume_masks_scaled_down():
    cap = lcc.cap_items('cc_grid', 16)
    obj = lcc.VOLUME_SMALL
    m, info = lcc.volume_mask((1, 7, 34, 47), cap, obj)
    assert m.size == 2 * cap + 2994
    check_windows(m, info, cap, 5)
    for limit in (None, lcc.SMALL_AREA):
        want = vc.fill_ref(m, limit, 3)
        assert np.array_equal(want, vc.brute(m, {'op': 'fill_holes', 'max_voxels': limit}, 3)) and not np.array_equal(want, m)
    assert not np.array_equal(vc.fill_ref(m, None, 3), vc.fill_ref(m, lcc.SMALL_AREA, 3))
    for faces in vc.FACES:
        want = vc.clear_border_ref(m, 3, faces)
        assert np.array_equal(want, vc.brute(m, {'op': 'clear_border', 'faces': faces}, 3)) and not np.array_equal(want, m)
    want = vs.split3d_ref(m, obj['r'], 'cross', None, 3)
    assert np.array_equal(want, vs.brute_split3d(m, obj['r'], 'cross', None, 3))
    for w in info['windows']:
        box = (w['frame'], slice(*w['rows']), slice(*w['box']))
        assert (want[box] != m[box]).any(), w['name']


def test_thin_volumes_scaled_down():
    cap = lcc.cap_items('cc_grid', 8)
    m, info = lcc.thin_volume((2, 150, 3, 5), cap)
    assert m.size == 2 * cap + 404
    check_windows(m, info, cap, 3)
    assert 2 * lcc.face_count(150, 3, 5, True) > cap
    check_late_faces(m, info, cap)
    for limit in (None, lcc.SMALL_AREA):
        want = vc.fill_ref(m, limit, 3)
        assert np.array_equal(want, vc.brute(m, {'op': 'fill_holes', 'max_voxels': limit}, 3)) and not np.array_equal(want, m)
    both = [vc.clear_border_ref(m, 3, faces) for faces in vc.FACES]
    for faces, want in zip(vc.FACES, both):
        assert np.array_equal(want, vc.brute(m, {'op': 'clear_border', 'faces': faces}, 3))
    assert not np.array_equal(both[0], both[1]) and both[1].any()


def test_label_frames_scaled_down():
    cap = lcc.cap_items('nb_grid', 20)
    lab, info = lcc.label_frames((3, 60, 71), cap)
    assert lab.size == 2 * cap + 2540
    check_windows(lab, info, cap, 5)
    for reach in (0, 5):
        zones, d2 = nc.zones_ref(lab, lcc.MAX_LABEL, reach)
        zb, db = nc.zones_allpairs(lab, lcc.MAX_LABEL, reach)
        assert np.array_equal(zones, zb) and np.array_equal(d2, db)
        for f, y, x, small in info['ties']:
            assert zones[f, y, x] == small and d2[f, y, x] == 9
        stats, pairs = nc.graph_ref(zones, lcc.MAX_LABEL)
        sb, pb = nc.graph_allpairs(zones, lcc.MAX_LABEL)
        assert np.array_equal(stats, sb) and np.array_equal(pairs, pb) and len(pairs)


def test_label_volumes_scaled_down():
    cap = lcc.cap_items('nb_grid', 32)
    lab, info = lcc.label_volumes((1, 5, 68, 71), cap)
    assert lab.size == 2 * cap + 7756
    check_windows(lab, info, cap, 5)
    zones, d2 = n3.zones3d_ref(lab, lcc.MAX_LABEL)
    zb, db = n3.zones3d_allpairs(lab, lcc.MAX_LABEL)
    assert np.array_equal(zones, zb) and np.array_equal(d2, db)
    for v, z, y, x, small in info['ties']:
        assert zones[v, z, y, x] == small and d2[v, z, y, x] == 9.0
    stats, pairs = n3.graph3d_ref(zones, lcc.MAX_LABEL)
    sb, pb = n3.graph3d_allpairs(zones, lcc.MAX_LABEL)
    assert np.array_equal(stats, sb) and np.array_equal(pairs, pb) and len(pairs)


@pytest.mark.parametrize("N,P", [(3, 16 * 256 + 77), (40, 1028), (5, 14 * 256 + 77)])
def test_label_stacks_scaled_down_and_the_packed_reference(N, P):
    a, b = lcc.overlap_stacks(N, P)
    ml = lcc.OVERLAP_MAX_LABEL
    assert a.shape == b.shape == (N, P) and a.dtype == b.dtype == np.int32
    want = lc.overlap_ref(a, b, ml)
    for got, w, bw in zip(lcc.overlap_packed(a, b, ml), want, lc.brute_overlap(a, b, ml)):
        assert got.dtype == w.dtype and got.shape == w.shape and np.array_equal(got, w) and np.array_equal(w, bw)
    own = [set(np.unique(a[n])) - set(np.unique(np.delete(a, n, 0)[[k for k in range(N - 1) if abs(k + (k >= n) - n) == 1]]))
           for n in range(N)]
    assert all(own), "every frame carries a label its neighbours do not have"
    if N <= 8:
        assert all(10 + n in set(np.unique(a[n])) and not (np.delete(a, n, 0) == 10 + n).any() for n in range(N))
    assert len(want[0]) >= 8 * N                                # dense: many pairs in every frame


def test_relabel_case_scaled_down():
    labels, offsets, lut = lcc.relabel_case(5, 9 * 256 + 77)
    want = lc.relabel_ref(labels, offsets, lut)
    counts = np.diff(offsets)
    assert len(set(counts.tolist())) == 5 and 0 in counts
    for n in range(5):                                          # the definition, position by position
        row = [int(lut[offsets[n] + v - 1]) if 1 <= v <= counts[n] else 0 for v in labels[n].tolist()]
        assert want[n].tolist() == row
    assert all(want[n].any() for n in range(5) if counts[n]) and not want[2].any()
