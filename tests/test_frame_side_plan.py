"""CPU: the plan behind tests/test_gpu_frame_side_sweep.py.  The constants of tests/frame_side_cases.py are the ones in the
source; every table reaches the regimes it names; the chunked pairwise order restated in plain float32 numpy is np.mean /
np.std bit for bit on every statistics case (so the cases exercise the order the kernel copies, and a tail summed left to
right would show); the strip layout of the background fit gives the regimes the table names, and a float64 emulation of
the kernel's fit stays far inside the surface bound on them; the hot-pixel definition restated index by index equals the
host pipe on every hot-pixel case, and the tie case has pixels exactly on its threshold."""
import os
import re

import numpy as np
import pytest

from oracle import frontend_ref
from sequitr_amd.frontend import axis_tiles
from tests import confusion_cases as cc
from tests import frame_clean_cases as fc
from tests import frame_side_cases as fsc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def source(path):
    return open(os.path.join(ROOT, path)).read()


# ---- the constants ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(fsc.CONSTANTS))
def test_the_table_restates_the_constants_of_the_source(name):
    path, pattern, value = fsc.CONSTANTS[name]
    found = re.findall(pattern, source(path))
    assert len(found) == 1, "%s: %r matches %d places in %s" % (name, pattern, len(found), path)
    expr = found[0].strip()
    assert re.fullmatch(r'\d+( << \d+)?', expr), expr
    got = int(expr.split(' << ')[0]) << int(expr.split(' << ')[1]) if ' << ' in expr else int(expr)
    assert got == value, "%s is %d in %s, the table says %d: move its cases" % (name, got, path, value)


def test_the_launches_are_the_ones_the_cases_assume():
    pw, fe, vf = (source('sequitr_amd/csrc/' + f) for f in ('sq_pairwise.h', 'sq_frontend.hip', 'sq_volume_frontend.hip'))
    assert 'if (left >= CHUNK) {' in pw and 'pw_rec<T, SQ>(a, (int)left, m)' in pw      # whole chunks: the tree; else pw_rec
    assert 'if (n <= LEAF) return pw_block<T, SQ>(a, n, mean);' in pw and 'n2 -= n2 % 8;' in pw and 'if (n < 8) {' in pw
    assert 'dim3 grid((nchunks + 3) / 4, F);' in fe
    assert 'const int m = nchunks - base < 64 ? nchunks - base : 64;' in vf and 'if (m == 64) {' in vf
    clean = source('sequitr_amd/csrc/sq_frame_clean.hip')
    assert 'const int n = (H + BG_MIN_ROWS - 1) / BG_MIN_ROWS;' in clean and 'return n < BG_MAX_STRIPS ? n : BG_MAX_STRIPS;' in clean
    assert clean.count('const int rows = (H + nstrips - 1) / nstrips;') == 2
    assert 'const int vec = (W % 4 == 0) && SQ_ALIGNED16(out);' in clean
    assert 'res[p] = fabsf(v - med) > threshold ? med : v;' in clean
    score = source('sequitr_amd/csrc/sq_score.hip')
    assert score.count('for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {') == 2
    assert 'L.grid = (unsigned)std::min(L.units, MAX_GRID);' in score
    assert 'if (idx >= max_out) continue;' in source('sequitr_amd/csrc/sq_centroids.hip')
    assert 'max_out = n ' in source('sequitr_amd/centroids.py')


# ---- statistics -------------------------------------------------------------------------------------------------------
def test_the_statistics_table_reaches_every_regime():
    seen = set().union(*(tags for _, _, tags in fsc.STATS_CASES))
    assert fsc.STATS_NEEDED <= seen, fsc.STATS_NEEDED - seen
    for name, tails in fsc.TAILS.items():
        assert all(fsc.tail_class(t) == name for t in tails), name
        rows = [(s, d) for s, d, tags in fsc.STATS_CASES if name in tags]
        assert {fsc._name(d) for _, d in rows} == {'uint8', 'uint16', 'float32'}, name
        assert {s[1] * s[2] // fsc.CHUNK for s, _ in rows} >= set(fsc.FULLS) - {0 if name == 'tail=0' else None}, name
    for (F, H, W), dtype, _ in fsc.STATS_CASES:
        assert H * W <= 5 * fsc.CHUNK + fsc.CHUNK - 1 and F == (3 if (H * W) % 2 else 2)
        T = min(H, W)
        assert len(axis_tiles(H, T, 0)[0]) >= 1 and len(axis_tiles(W, T, 0)[0]) >= 1       # the tiler accepts the shape
    assert {129, 200, 255} == set(fsc.TAILS['tail=129..255'])   # just above LEAF: the first split, at a whole and a ragged half
    vseen = set()
    for shape, _ in fsc.VOLUME_CASES:
        vseen |= fsc.volume_tags(shape)
    assert fsc.VOLUME_NEEDED <= vseen, fsc.VOLUME_NEEDED - vseen
    assert [-(-int(np.prod(s[1:])) // fsc.CHUNK) for s, _ in fsc.VOLUME_CASES] == [64, 65, 128]


@pytest.mark.parametrize("case", range(len(fsc.STATS_CASES)), ids=fsc.STATS_IDS)
def test_the_restated_pairwise_order_is_numpys(case):
    shape, dtype, tags = fsc.STATS_CASES[case]
    fr = fsc.stats_frames(shape, dtype, case)
    differs = False
    for f in range(shape[0]):
        a = fsc.as_float32(fr[f])
        mean, std = fsc.pairwise_stats(fr[f])
        assert mean.dtype == np.float32 and mean.tobytes() == np.mean(a).tobytes(), (f, mean, np.mean(a))
        assert std.dtype == np.float32 and std.tobytes() == np.std(a).tobytes(), (f, std, np.std(a))
        wrong = fsc.pairwise_stats(fr[f], fsc.leftright_sum_tail)
        differs = differs or wrong[0].tobytes() != mean.tobytes() or wrong[1].tobytes() != std.tobytes()
    # a long ragged chunk of float32 pixels: its order shows in the result (sums of small integers are exact in any order)
    if dtype == np.float32 and ('tail=8191' in tags or 'tail>256,half%8' in tags):
        assert differs, "a tail summed left to right gives the same statistics: the case does not hold pw_rec"


@pytest.mark.parametrize("case", range(len(fsc.VOLUME_CASES)))
def test_the_restated_order_is_numpys_on_the_volumes(case):
    shape, dtype = fsc.VOLUME_CASES[case]
    vols = fsc.stats_frames(shape, dtype, 70 + case)
    for v in range(shape[0]):
        a = fsc.as_float32(vols[v])
        mean, std = fsc.pairwise_stats(vols[v])
        assert mean.tobytes() == np.mean(a).tobytes() and std.tobytes() == np.std(a).tobytes(), v


# ---- background -------------------------------------------------------------------------------------------------------
def test_the_strip_layout_gives_the_regimes():
    assert fsc.strip_layout(2049) == (256, 9, 28)
    assert fsc.strip_layout(2100) == (256, 9, 22)
    assert fsc.strip_layout(2305) == (256, 10, 25)
    assert fsc.strip_layout(4096) == (256, 16, 0)
    assert fsc.strip_layout(2048) == (256, 8, 0)
    assert fsc.strip_layout(257) == (33, 8, 0)                  # the tallest frame of tests/frame_clean_cases.py: no cap
    assert fsc.strip_layout(3) == (1, 3, 0) and fsc.strip_layout(9) == (2, 5, 0)
    seen = set()
    for shape, _ in fsc.BG_CASES:
        seen |= fsc.bg_tags(shape)
        strips, rows, empty = fsc.strip_layout(shape[1])
        assert (strips - empty - 1) * rows < shape[1] <= (strips - empty) * rows       # the strips cover the rows once
    assert fsc.BG_NEEDED <= seen, fsc.BG_NEEDED - seen
    assert [s[1:] for s, _ in fsc.BG_CASES] == [(2049, 5), (2100, 3), (2305, 4), (4096, 3), (2048, 6), (3, 2100), (9, 9)]


@pytest.mark.parametrize("case", range(len(fsc.BG_CASES)), ids=fsc.BG_IDS)
def test_the_emulated_fit_is_far_inside_the_bound(case):
    (F, H, W), _ = fsc.BG_CASES[case]
    fr = fsc.bg_frames(case)
    for f in range(F):
        x = fc.as_float32(fr[f])
        want = fc.oracle_fit(x)[0]
        err = np.abs(fc.basis_surface(fsc.fit_emulated(x), H, W) - want).max()
        print("case %s frame %d: emulated surface error %.3g = %.3g delta" % (fsc.BG_IDS[case], f, err, err / fc.delta(x)))
        assert err <= 1e-3 * fc.delta(x), (f, err, fc.delta(x))
        if H >= 9:                                              # rows dropped from the moments move the surface past the bound
            cut = np.abs(fc.basis_surface(fsc.fit_emulated(x, skip_last_row=True), H, W) - want).max()
            assert cut > fc.delta(x), (f, cut, fc.delta(x))


def test_the_zero_coefficient_frame_cancels_and_stays_inside_the_bound():
    x = fsc.zero_coef_frame()
    assert x.shape == (96, 80) and x.dtype == np.float32
    mean, std = fsc.two_pass_stats(x)
    assert abs(mean - fsc.ZERO_COEF_LEVEL) < 0.1 and abs(std - fsc.ZERO_COEF_NOISE) < 0.05
    rel = abs(fsc.one_pass_std(x) - std) / std
    print("one-pass float64 std of the zero-coefficient frame: relative error %.3g, float32 half-ulp %.3g" % (rel, 2.0 ** -25))
    assert abs(fsc.one_pass_std(x) - std) <= fc.delta(x)
    assert rel > 2.0 ** -30                                     # the cancellation is there to see: far above fp64 rounding


# ---- hot pixels -------------------------------------------------------------------------------------------------------
def test_the_hot_pixel_table_reaches_every_regime():
    seen = set().union(*(tags for *_, tags in fsc.HOT_CASES))
    assert fsc.HOT_NEEDED <= seen, fsc.HOT_NEEDED - seen
    assert {(H, W, s) for H, W, s, _, _ in fsc.HOT_CASES} == {(H, W, s) for s in (2, 3, 4, 5) for H in (s, 32, 33, 64)
                                                               for W in (256, 257, 259, 260, 512)}
    for size in fc.SIZES:                                       # every window meets every pixel type, both store paths
        rows = [(W, d) for H, W, s, d, _ in fsc.HOT_CASES if s == size]
        assert {fsc._name(d) for _, d in rows} == {'uint8', 'uint16', 'float32'}
        assert {W % 4 == 0 for W, _ in rows} == {True, False}


@pytest.mark.parametrize("case", range(len(fsc.HOT_CASES)), ids=fsc.HOT_IDS)
def test_outliers_restated_equals_the_host_pipe(case):
    H, W, size, dtype, _ = fsc.HOT_CASES[case]
    fr = fsc.hot_frames(H, W, dtype)
    assert fr.shape == (fsc.HOT_F, H, W) and not np.isnan(fr.astype(np.float64)).any()
    assert not (np.signbit(fr.astype(np.float64)) & (fr == 0)).any()          # no -0.0
    changed = 0
    for f in range(fsc.HOT_F):
        want = fc.outliers_host(fr[f], size, fsc.HOT_THRESHOLD)
        assert want.tobytes() == fc.outliers_restated(fr[f], size, fsc.HOT_THRESHOLD).tobytes(), f
        changed += int((want != fc.as_float32(fr[f])).sum())
    assert changed > 0                                          # hot pixels were there and went


def test_the_tie_case_has_pixels_exactly_on_the_threshold():
    H, W, size, dtype, thr = fsc.TIE_CASE
    fr = fsc.hot_frames(H, W, dtype, seed=1)
    assert np.issubdtype(fr.dtype, np.integer) and W % 4 == 0
    on = 0
    for f in range(fsc.HOT_F):
        x = fc.as_float32(fr[f])
        med = fc.median_restated(x, size)
        want = fc.outliers_host(fr[f], size, thr)
        assert want.tobytes() == fc.outliers_restated(fr[f], size, thr).tobytes()
        tie = np.abs(x - med) == np.float32(thr)
        on += int(tie.sum())
        assert (want[tie] == x[tie]).all() and (want[tie] != med[tie]).all()  # kept: a `>=` would replace them
    assert on >= 20, on


# ---- confusion, centroids, the blank frame ----------------------------------------------------------------------------
def test_the_confusion_cases_pass_the_grid_cap_by_five_units():
    assert fsc.CONFUSION_ITEMS == 65536 + 5
    assert [c[:2] + (c[2],) for c in fsc.CONFUSION_CASES] == [('mask-index', 1, 3), ('mask-index', 5, 3), ('logits-onehot', 2, 2)]
    for case, (pair, n, C) in enumerate(fsc.CONFUSION_CASES):
        chunk, units = fsc.confusion_units(fsc.CONFUSION_ITEMS, n)
        assert chunk == fsc.MIN_CHUNK and units == fsc.CONFUSION_ITEMS and 0 < units - fsc.MAX_GRID < 256
        p, t = fsc.confusion_inputs(case)
        assert p.shape[:2] == (fsc.CONFUSION_ITEMS, n) and t.shape[:2] == p.shape[:2]
        counts, ignored = cc.confusion_ref(p, t, C)
        late = counts[fsc.MAX_GRID:].sum() + ignored[fsc.MAX_GRID:].sum()
        assert late == 5 * n and counts[fsc.MAX_GRID:].sum() > 0, "the items of the second trip count nothing"
        assert ignored.sum() > 0


@pytest.mark.parametrize("kind", ["planar", "volumetric"])
def test_the_centroid_cases_hold_well_over_eight_components(kind):
    mask, ref, total = fsc.centroid_case(kind)
    assert mask.shape == ((3, 40, 70) if kind == 'planar' else (2, 5, 24, 40)) and mask.dtype == np.uint8
    assert total >= 3 * fsc.SMALL_MAX_OUT and all(len(r) > 0 for r in ref)
    assert {1.0, 2.0} <= set(np.concatenate(ref)[:, 4].tolist())


def test_the_host_pipeline_gives_nan_tiles_for_the_blank_frame():
    fr = fsc.blank_frames()
    H, W = fsc.BLANK_SHAPE[1:]
    oy, ox = axis_tiles(H, fsc.BLANK_TILE, fsc.BLANK_MARGIN)[0], axis_tiles(W, fsc.BLANK_TILE, fsc.BLANK_MARGIN)[0]
    a = fsc.as_float32(fr[1])
    assert np.mean(a) == fsc.BLANK_VALUE and np.std(a) == 0
    with np.errstate(invalid='ignore'):
        tiles = frontend_ref.tiles(fr, oy, ox, fsc.BLANK_TILE)
    per = len(oy) * len(ox)
    assert tiles.shape == (3 * per, 32, 32, 1) and per == 4
    assert np.isnan(tiles[per:2 * per]).all() and np.isfinite(tiles[:per]).all() and np.isfinite(tiles[2 * per:]).all()
