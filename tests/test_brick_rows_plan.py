"""CPU: the plan behind tests/test_gpu_brick_rows_sweep.py.  The constants of tests/brick_rows_cases.py are the ones in the
sources; the launch arithmetic restated there gives the figures the tables were chosen for; every table reaches every
regime it names, and the tables of the feature tests (volume_frontend on its three volumes, volume_sampler_cases.
IMAGE_CASES) reach none of the new ones -- which is why this sweep exists, and what fails if someone makes it redundant;
the references at the new shapes equal a voxel-by-voxel loop on the smallest cases."""
import os
import re

import numpy as np
import pytest

from sequitr_amd.frontend import volume_bricks
from tests import brick_rows_cases as br
from tests import volume_frontend_cases as vc
from tests import volume_sampler_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def source(path):
    return open(os.path.join(ROOT, path)).read()


def nvecs(tags):
    return {int(t[5:]) for t in tags if t.startswith('nvec=')}


# ---- the constants and the loops ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(br.CONSTANTS))
def test_the_table_restates_the_constants_of_the_source(name):
    path, pattern, value, places = br.CONSTANTS[name]
    found = re.findall(pattern, source(path))
    assert len(found) == places, "%s: %r matches %d places in %s, not %d" % (name, pattern, len(found), path, places)
    for got in found:
        assert int(got) == value, "%s is %s in %s, the table says %d: move its cases" % (name, got, path, value)


def test_the_kernels_are_the_ones_the_restatement_describes():
    fe, sm, py = source(br.FE), source(br.SM), source(br.PY)
    for src in (fe, sm):
        assert 'unsigned tx = 4;' in src and 'while (tx < 64 && tx < pieces) tx *= 2;' in src
        assert 'return h < n ? h : n;' in src
    assert fe.count('for (int j = tx; j < nvec; j += TX) {') == 2 and sm.count('for (int j = tx; j < nvec; j += TX) {') == 1
    assert 'const int head = head_elems(dst, n), nvec = (n - head) >> 2;' in fe          # float rows: four to a store
    assert 'const int head = head_elems(dst, n), nvec = (n - head) / VE;' in fe
    assert 'const int head = head_units(dst, n), nvec = (n - head) / VE;' in sm
    assert fe.count('const int i = head + VE * j;') == 1 and 'const int i = head + 4 * j;' in fe
    assert 'const int i = head + VE * j;' in sm and 'if (++sub == K) {' in sm
    assert fe.count('const dim3 grid((g.BX + block.y - 1) / block.y, g.BZ, count);') == 2
    assert 'const dim3 grid((g.BX + block.y - 1) / block.y, g.BZ, count);' in sm
    assert 'const dim3 block = row_block((int64_t)g.BY * 4);' in fe
    assert 'const dim3 block = row_block((int64_t)g.BY * C * sizeof(E));' in fe
    assert 'const dim3 block = row_block((int64_t)g.BY * K * sizeof(typename P::U));' in sm
    assert 'const int B = g.BX, nt = (B + TILE - 1) / TILE;' in sm and 'const int nt = (g.BX + TILE - 1) / TILE;' in sm
    assert 'const int ni = min(TILE, B - x0), n = min(TILE, B - y0) * K;' in sm and 'for (int k = tx; k < n; k += TILE) {' in sm
    assert 'SQ_REQUIRE(C > 0 && C <= %d,' % br.SCATTER_MAX_C in fe and 'SQ_REQUIRE(C >= 1 && C <= 16,' in sm
    # the second launch of the three host loops: the offsets the split tests hold
    assert py.count('out[lo:].data_ptr()') == 2 and py.count('values[lo:].data_ptr()') == 2 and 'x[lo:].data_ptr()' in py
    assert py.count('first + lo, n') == 3


def test_row_block_and_the_split_restated():
    assert [br.row_block(b)[0] for b in (1, 48, 49, 112, 113, 240, 241, 496, 497, 1 << 20)] == [4, 4, 8, 8, 16, 16, 32, 32, 64, 64]
    assert all(tx * rows == 256 for tx, rows in map(br.row_block, range(1, 3000)))
    assert br.row_split(0, 4, 16) == (0, 4, 0) and br.row_split(4, 4, 16) == (3, 3, 1) and br.row_split(12, 4, 2) == (1, 0, 1)
    assert br.row_split(12, 4, 1) == (1, 0, 0) and br.row_split(1, 1, 131) == (15, 7, 4) and br.row_split(8, 8, 131) == (1, 65, 0)
    assert br.row_split(14, 2, 531) == (1, 66, 2)
    assert [br.lane_trips(n, 64) for n in (0, 1, 64, 65, 128, 129)] == [0, 1, 1, 2, 2, 3]
    assert br.x_groups(70, 64) == (2, 6) and br.x_groups(3, 4) == (1, 3) and br.x_groups(8, 4) == (2, 4)
    assert [br.tile_grid(B) for B in (64, 65, 128, 70)] == [(1, 64), (2, 1), (2, 64), (2, 6)]
    assert br.launches(67584) == [(0, 65535), (65535, 2049)] and br.launches(65535) == [(0, 65535)]
    for K in (5, 7):                                            # over the starts of a vector, the carry falls everywhere
        assert set().union(*(br.carry_positions(s, K) for s in range(K))) == set(range(16))
    assert br.carry_positions(0, 16) == {15} and br.carry_positions(0, 1) == set(range(16))


# ---- volume_to_bricks_kernel ------------------------------------------------------------------------------------------
def test_the_to_bricks_table_reaches_every_regime():
    seen, by_brick = set(), {}
    for brick, kind, shape in br.TO_BRICKS_CASES:
        g = volume_bricks(shape[1:], brick, br.TO_BRICKS_MARGIN)
        if kind == 'rows':                                      # two bricks along z and y, x shorter than the brick
            assert g.counts[0] == 2 and g.counts[2] >= 2 and shape[2] < brick[1]
        else:
            assert shape[3] < brick[2] and g.counts[2] == 1
        tags = br.to_bricks_tags(shape, brick, br.TO_BRICKS_MARGIN)
        by_brick.setdefault(brick, set()).update(tags)
        seen |= tags
        assert int(np.prod(shape)) * 4 + shape[0] * g.per_volume * int(np.prod(brick)) * 4 < 1 << 20       # small
    assert br.TO_BRICKS_NEEDED <= seen, br.TO_BRICKS_NEEDED - seen
    figures = {b: (min(t for t in br.TXS if 'TX=%d' % t in tags), max(nvecs(tags)), 'groups>=2' in tags)
               for b, tags in by_brick.items()}
    assert figures == {(2, 70, 5): (4, 1, True), (2, 20, 27): (8, 6, False), (2, 10, 61): (32, 15, True),
                       (2, 5, 131): (64, 32, True), (1, 5, 263): (64, 65, True), (1, 3, 519): (64, 129, False),
                       (2, 20, 45): (16, 11, True)}
    for brick, tags in by_brick.items():                        # every brick: every head, rows of fill, fill inside a row
        assert {'head=%d' % h for h in range(4)} | {'fill_row', 'row_fill', 'oy>0'} <= tags, brick
    assert 'trips=2' in by_brick[(1, 5, 263)] and 'trips=3' in by_brick[(1, 3, 519)]
    assert 'row_fill@trip>=2' in by_brick[(1, 5, 263)] and 'row_fill@trip>=2' in by_brick[(1, 3, 519)]


def test_the_feature_tests_of_the_front_end_reach_none_of_it():
    brick, margin = (8, 16, 16), (2, 4, 4)
    old_b, old_u8, old_f32 = set(), set(), set()
    for shape in ((2, 19, 37, 45), (1, 5, 37, 16), (2, 11, 26, 37)):
        total = shape[0] * volume_bricks(shape[1:], brick, margin).per_volume
        old_b |= br.to_bricks_tags(shape, brick, margin)
        for first in range(0, total, 7):                        # test_gpu_volume_frontend.batches
            old_b |= br.to_bricks_tags(shape, brick, margin, first, min(7, total - first))
        old_u8 |= br.scatter_tags(shape[1:], brick, margin, 1, 1, V=shape[0])
        for C in (1, 2, 3):
            old_f32 |= br.scatter_tags(shape[1:], brick, margin, C, 4, V=shape[0])
    assert not old_b & br.TO_BRICKS_NEW, old_b & br.TO_BRICKS_NEW
    assert {t for t in old_b if t.startswith(('TX=', 'head=', 'tail=', 'nvec='))} == {'TX=8', 'head=0', 'head=0+body', 'tail=0+body', 'nvec=4'}
    assert not old_u8 & br.SCATTER_U8_NEW, old_u8 & br.SCATTER_U8_NEW
    assert nvecs(old_u8) == {0, 1} and nvecs(br.scatter_tags((19, 37, 45), brick, margin, 1, 1)) == {0}
    assert not old_f32 & br.SCATTER_F32_NEW, old_f32 & br.SCATTER_F32_NEW
    assert max(nvecs(old_f32)) == 12                            # far from a second trip of TX >= 8 lanes
    for table, new in ((br.TO_BRICKS_NEEDED, br.TO_BRICKS_NEW), (br.SCATTER_U8_NEEDED, br.SCATTER_U8_NEW),
                       (br.SCATTER_F32_NEEDED, br.SCATTER_F32_NEW)):
        assert new <= table, new - table                        # and the new tables reach all of it (tests above and below)


# ---- bricks_scatter_kernel --------------------------------------------------------------------------------------------
def test_the_scatter_tables_reach_every_regime():
    seen, per_case = set(), []
    for case in br.SCATTER_U8_CASES:
        tags = set().union(*(br.scatter_tags(*case, unit=1, offset=off) for off in br.SCATTER_U8_OFFSETS))
        per_case.append(br.scatter_tags(*case, unit=1))
        seen |= tags
    assert br.SCATTER_U8_NEEDED <= seen, br.SCATTER_U8_NEEDED - seen
    even = {'head=%d+body' % h for h in range(0, 16, 2)}
    assert {t for t in per_case[0] if t.startswith('head=') and t.endswith('+body')} == even and 'TX=16' in per_case[0]
    assert {'tail=%d+body' % h for h in range(0, 16, 2)} <= per_case[0] and max(nvecs(per_case[0])) == 8
    assert {t for t in per_case[1] if t.startswith('head=') and t.endswith('+body')} == {'head=%d+body' % h for h in (0, 4, 8, 12)}
    assert 'TX=64' in per_case[1] and max(nvecs(per_case[1])) == 68 and 'trips=2' in per_case[1]
    assert {'TX=4', 'groups>=2', 'last_group=partial'} <= per_case[2] and nvecs(per_case[2]) == {0}
    seen, per_case = set(), []
    for case in br.SCATTER_F32_CASES:
        tags = set().union(*(br.scatter_tags(*case, unit=4, offset=off) for off in br.SCATTER_F32_OFFSETS))
        per_case.append(br.scatter_tags(*case, unit=4))
        seen |= tags
    assert br.SCATTER_F32_NEEDED <= seen, br.SCATTER_F32_NEEDED - seen
    assert [max(nvecs(t)) for t in per_case[:3]] == [67, 66, 132] and all('TX=64' in t for t in per_case[:3])
    assert 'trips=2' in per_case[0] and 'trips=2' in per_case[1] and 'trips=3' in per_case[2]
    assert {'head=0+body', 'head=1+body', 'tail=0+body', 'tail=3+body'} <= per_case[2]
    assert {'TX=4', 'groups>=2', 'last_group=partial'} | {'head=%d' % h for h in range(4)} <= per_case[3]
    assert [c[3] for c in br.SCATTER_F32_CASES[4:]] == [2, 5, 8, br.SCATTER_MAX_C] and 'TX=32' in per_case[6]
    for case in br.SCATTER_U8_CASES + br.SCATTER_F32_CASES:
        picks = br.interior_bricks(*case[:3])
        total = br.SCATTER_V * volume_bricks(*case[:3]).per_volume
        assert len(picks) == 3 and picks[0] == 0 and picks[-1] == total - 1 and total >= 4


# ---- the sampler ------------------------------------------------------------------------------------------------------
def _sampler_case_tags(kind, param, brick):
    shape = br.sampler_volume(brick)
    plan = br.sampler_plan(shape, brick)
    unit, K = br.sampler_unit(kind, param)
    tags = set().union(*(br.sampler_row_tags(kind, param, brick, len(plan), off) for off in br.sampler_offsets(kind, param)))
    return tags | br.plan_fill_tags(plan, shape, brick, unit, K, 7), plan


def test_the_sampler_row_table_reaches_every_regime():
    per_unit, onehot, copies = {}, set(), set()
    for kind, param, brick in br.SAMPLER_ROW_CASES:
        assert brick[1] != brick[2]                             # no transposed op reaches the kernel: every row is a row-path row
        tags, plan = _sampler_case_tags(kind, param, brick)
        assert set(plan[:, 4]) == set(sc.FLIPS) and len(plan) <= 64
        L = br.sampler_volume(brick)[1:]
        for a in range(3):                                      # both extreme origins, as case_plan makes them
            assert 0 in plan[:, 1 + a] and max(L[a] - brick[a], 0) in plan[:, 1 + a]
        per_unit.setdefault(br.sampler_unit(kind, param)[0], set()).update(tags)
        if kind == 'onehot':
            onehot |= tags
        if kind == 'copy':
            copies.add(param)
    for unit in br.SAMPLER_UNITS:
        need = br.SAMPLER_PER_UNIT | br.HEADS_WITH_BODY[unit] | {'row_fill', 'row_fill@trip>=2'}
        assert need <= per_unit[unit], (unit, need - per_unit[unit])
    assert {'trips=2', 'tail>0+body'} | br.HEADS_WITH_BODY[2] <= per_unit[2]           # the 2-byte copy: one case
    assert copies == {1, 2, 3, 4, 8}
    assert br.SAMPLER_ONEHOT_NEEDED <= onehot, br.SAMPLER_ONEHOT_NEEDED - onehot
    assert br.labels((1, 2, 3, 400)).max() >= 16                # labels >= C are present for every C
    two_trips = {(k, p): max(nvecs(_sampler_case_tags(k, p, b)[0])) for k, p, b in br.SAMPLER_ROW_CASES}
    assert two_trips[('copy', 1)] >= 65 and two_trips[('copy', 3)] >= 65 and two_trips[('onehot', 5)] >= 65
    assert two_trips[('copy', 8)] >= 65 and two_trips[('copy', 2)] >= 65 and two_trips[('images', np.float32)] >= 65


def test_the_feature_tests_of_the_sampler_reach_none_of_it():
    for kind, param, brick, ops in br.OLD_SAMPLER_CASES:
        count = len(sc.case_plan(sc.VOL_SHAPE, brick, ops))
        tags = br.sampler_row_tags(kind, param, brick, count)
        assert not tags & br.SAMPLER_NEW, (kind, param, brick, tags & br.SAMPLER_NEW)
        if ops != sc.TRANSPOSED:                                # rows of 70 floats run under transposed ops only
            assert not tags & br.SAMPLER_NEW_ON_PLAIN_ROWS, (kind, param, brick)
        assert max(nvecs(tags)) <= 18
    old_tiles = set()
    for brick, ops in sc.IMAGE_CASES + [sc.BIG_TILE_CASE]:
        if ops != sc.FLIPS:
            old_tiles |= set().union(*(br.tile_tags(brick[1], K) for K in (1, 2, 3)))
    assert not old_tiles & br.TILE_NEW, old_tiles & br.TILE_NEW
    assert br.TILE_NEW <= br.TILE_NEEDED | {'last=whole', 'last=1'}


def test_the_tile_and_gather_cases_reach_their_regimes():
    seen = set()
    for kind, param, B in br.TILE_CASES:
        seen |= br.tile_tags(B, br.sampler_unit(kind, param)[1])
        shape = br.tile_volume(B)
        plan = br.sampler_plan(shape, (1, B, B), sc.TRANSPOSED, random_rows=0)
        assert set(plan[:, 4]) == set(sc.TRANSPOSED) and len(plan) * B * B * 16 <= 12 << 20
    assert br.TILE_NEEDED <= seen, br.TILE_NEEDED - seen
    B = br.GATHER_BRICK[1]
    tags = br.sampler_row_tags('images', br.GATHER_DTYPE, br.GATHER_BRICK, 1)
    assert {'TX=64', 'trips=2', 'groups>=2'} <= tags and br.tile_grid(B) == (5, 7)


# ---- the host's splits ------------------------------------------------------------------------------------------------
def test_the_split_cases_start_a_second_launch_inside_the_second_volume():
    g = volume_bricks(br.SPLIT_VOLUME, br.SPLIT_BRICK, br.SPLIT_MARGIN)
    assert g.counts == (48, 32, 22) and g.per_volume == 33792
    total = br.SPLIT_V * g.per_volume
    assert total == 67584 and br.launches(total) == [(0, 65535), (65535, 2049)]
    assert g.per_volume < br.MAX_COUNT < total                  # brick 65535 lies in volume 1
    assert br.launches(total - br.SPLIT_FIRST)[1] == (65535, 2044)
    assert br.SPLIT_FRAMES == 65540 and br.launches(br.SPLIT_FRAMES) == [(0, 65535), (65535, 5)]
    assert total * 6 * 4 < 2 << 20


# ---- the references at the new shapes, against loops ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", br.DTYPES, ids=br._name)
def test_np_bricks_equals_the_voxel_loop_on_the_smallest_brick(dtype):
    brick = br.TO_BRICKS_BRICKS[0]
    for kind, shape in br.to_bricks_volumes(brick).items():
        vols = br.volume(shape, dtype)
        g = volume_bricks(shape[1:], brick, br.TO_BRICKS_MARGIN)
        for normalise in (True, False):
            want = br.loop_bricks(vols, g, normalise)
            assert vc.np_bricks(vols, g, normalise).tobytes() == want.tobytes(), (kind, normalise)
            assert (want == 0).any() and (want != 0).any()


def test_np_scatter_equals_the_voxel_loop_on_the_smallest_cases():
    for (shape, brick, margin, C), dtype in ((br.SCATTER_U8_CASES[2], np.uint8), (br.SCATTER_F32_CASES[5], np.float32)):
        g = volume_bricks(shape, brick, margin)
        total = br.SCATTER_V * g.per_volume
        values = br.masks((total,) + brick) if dtype == np.uint8 else br.logits((total,) + brick + (C,))
        tail = () if dtype == np.uint8 else (C,)
        blank = np.full((br.SCATTER_V,) + shape + tail, 255, dtype)
        assert vc.np_scatter(values, blank.copy(), g).tobytes() == br.loop_scatter(values, blank.copy(), g).tobytes()
        k = total - 1
        one = vc.np_scatter(values[k:k + 1], blank.copy(), g, first=k)
        assert one.tobytes() == br.loop_scatter(values[k:k + 1], blank.copy(), g, first=k).tobytes()
        assert (one == 255).any() and (one != 255).any()


def test_the_sampler_references_equal_the_voxel_loop_on_small_cases():
    brick = (2, 3, 5)
    shape = br.sampler_volume(brick)
    plan = br.sampler_plan(shape, brick)
    src = br.copy_source(shape, 3)
    assert sc.np_copy(src, plan, brick).tobytes() == br.loop_sample(src, plan, brick).tobytes()
    lab = br.labels(shape)
    full = (lab[..., None] == np.arange(7, dtype=np.uint8)).astype(np.uint8)
    assert sc.np_onehot(lab, 7, plan, brick).tobytes() == br.loop_sample(full, plan, brick).tobytes()
    sq = (1, 5, 5)
    tplan = br.sampler_plan(br.tile_volume(5), sq, sc.TRANSPOSED, random_rows=0)
    vols = br.volume(br.tile_volume(5), np.uint16)
    norm = br.normalised(br.tile_volume(5), np.uint16, True)
    assert sc.np_images(vols, tplan, sq, normalised=norm).tobytes() == br.loop_sample(norm, tplan, sq)[..., None].tobytes()
