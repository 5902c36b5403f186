"""CPU: what tests/test_gpu_weightmap_sweep.py relies on, shown without a GPU -- the case tables of tests/weightmap_cases.py
reach every launch regime of the planar weight-map kernels (asserted from the launch arithmetic restated there), the
replay of the v2 column search takes every one of its branches and equals scipy, the float32-product reading of the map
expression is the reference's bit for bit while the all-double reading is not, and no reference value sits where a
last-bit difference in exp() could change its float32 rounding."""
import numpy as np
import pytest

from oracle import weightmap_ref
from tests import weightmap_cases as wc


def _regime(name):
    return wc.regime(*wc.edt_labels(name).shape)


def _all_regimes():
    return {n: _regime(n) for n in wc.EDT_CASES}


# ---- every regime is reached ----------------------------------------------------------------------------------------------
def test_case_names_carry_their_shapes():
    for name in wc.EDT_CASES:
        assert wc.edt_labels(name).shape == wc.shape_of(name) and wc.edt_labels(name).dtype == np.float32, name
    for name in wc.WM2_CASES:
        assert wc.wm2_case(name)[0].shape == wc.shape_of(name), name
    for name in wc.POINTS_CASES:
        assert wc.points_labels(name).shape == wc.shape_of(name), name


def test_launch_arithmetic_restated():
    r = wc.regime(1, 2048, 40)
    assert r["form"] == "v2" and r["nblk8"] == 256 and r["lds_bytes"] == 147456 and r["lds_above_48k"]
    assert wc.regime(1, 682, 33)["lds_bytes"] == 49152 and not wc.regime(1, 682, 33)["lds_above_48k"]
    assert wc.regime(1, 683, 33)["lds_bytes"] == 49216 and wc.regime(1, 683, 33)["lds_above_48k"]
    assert wc.regime(1, 2048, 1024)["form"] == "v2" and wc.regime(1, 2049, 3)["form"] == "v1" and wc.regime(1, 3, 1025)["form"] == "v1"
    assert wc.regime(1, 5, 9)["empty_parts"] == (5, 6, 7) and wc.regime(1, 9, 9)["empty_parts"] == (5, 6, 7)
    assert wc.regime(1, 17, 9)["empty_parts"] == (6, 7) and wc.regime(1, 8, 9)["empty_parts"] == ()
    assert wc.regime(1, 16384, 256)["v1_trips"] == 1 and wc.regime(1, 16385, 256)["v1_trips"] == 2
    assert wc.regime(5, 3, 1026)["flag_ints"] == 8 and wc.regime(4, 3, 1026)["flag_ints"] == 4


def test_v2_row_pass_regimes_are_reached():
    R = {n: _regime(n) for n in wc.ROW_PASS_CASES}
    assert all(r["form"] == "v2" and r["idle_row_waves"] for r in R.values())      # rows % 4 != 0 everywhere
    assert {r["nseg"] for r in R.values()} >= {1, 2, 16}
    assert {wc.edt_labels(n).shape[2] for n in R} == {1, 63, 64, 65, 1023, 1024}
    assert any(r["nseg"] == 16 and r["last_seg_partial"] for r in R.values())
    assert any(r["nseg"] == 16 and not r["last_seg_partial"] for r in R.values())
    for name in ("rows_1x3x1023", "rows_1x5x1024"):
        f = wc.is_feature(wc.edt_labels(name)[0])
        W = f.shape[1]
        rows = [set(np.nonzero(r)[0]) for r in f]
        assert {0} in rows                                      # `last` carried over the 15 later segments
        assert {W - 1} in rows                                  # `nxt` carried over the 15 earlier ones
        k = rows.index(set())                                   # a featureless row between featured ones
        assert 0 < k < len(rows) - 1 and rows[k - 1] and rows[k + 1]
    assert {63, 64} in [set(np.nonzero(r)[0]) for r in wc.is_feature(wc.edt_labels("rows_1x5x1024")[0])]


def test_v2_column_pass_regimes_are_reached():
    R = {n: r for n, r in _all_regimes().items() if r["form"] == "v2"}
    grid = {(wc.edt_labels(n).shape[1], wc.edt_labels(n).shape[2]) for n in R if n.startswith("cols_")}
    assert grid == {(h, w) for h in (1, 5, 8, 9, 17) for w in (9, 32, 33, 70)}
    assert any(r["empty_parts"] for r in R.values()) and any(not r["empty_parts"] and r["rows_per"] > 1 for r in R.values())
    assert any(r["last_block_partial"] and r["nblk8"] > 1 for r in R.values())
    assert any(not r["last_block_partial"] for r in R.values())
    assert any(r["last_strip_padded"] and r["strips"] > 1 for r in R.values())
    assert any(not r["last_strip_padded"] for r in R.values())
    assert R["lds_1x682x33"]["lds_bytes"] == 48 * 1024 and not R["lds_1x682x33"]["lds_above_48k"]
    assert R["lds_1x683x33"]["lds_above_48k"]
    for name in ("tall_corner_1x2048x40", "tall_dense_row_1x2048x40"):
        assert R[name]["lds_bytes"] == 147456 and R[name]["nblk8"] == 256 and R[name]["last_strip_padded"]
    corner = wc.edt_labels("tall_corner_1x2048x40")
    assert corner.sum() == 1 and corner[0, 0, 0] == 1
    b = wc.edt_labels("batch_empty_middle_3x9x70")             # "no feature" is a block-local fact in v2
    assert b[0].any() and not b[1].any() and b[2].any() and R["batch_empty_middle_3x9x70"]["strips"] > 1


def test_v1_regimes_are_reached():
    R = {n: r for n, r in _all_regimes().items() if r["form"] == "v1"}
    shapes = {wc.edt_labels(n).shape for n in R}
    assert shapes >= {(1, 3, 1025), (2, 5, 1100), (1, 2049, 3), (1, 2050, 33), (1, 2049, 2050)}
    assert any(wc.edt_labels(n).shape[2] > 1024 and wc.edt_labels(n).shape[1] <= 2048 for n in R)    # too wide only
    assert any(wc.edt_labels(n).shape[1] > 2048 and wc.edt_labels(n).shape[2] <= 1024 for n in R)    # too tall only
    assert R["v1_stride_1x2049x2050"]["v1_trips"] == 2
    assert wc.stream_trips(2049 * 2050) == 2 and wc.stream_trips(2049 * 2050, wc.POINTS_GRID_CAP) == 3
    assert all(r["v1_trips"] == 1 for n, r in R.items() if "stride" not in n)
    f = wc.edt_labels("v1_flags_5x3x1026")
    assert R["v1_flags_5x3x1026"]["flags_padded"] and R["v1_flags_5x3x1026"]["flag_ints"] == 8
    assert [bool(v.any()) for v in f] == [True, True, False, True, True]
    c = wc.edt_labels("v1_corner_1x2049x3")
    assert c.sum() == 1 and c[0, 2048, 2] == 1
    assert 0.005 < wc.edt_labels("v1_stride_1x2049x2050").mean() < 0.02            # dense: no thread walks a whole column


def test_nonbinary_cases_hold_every_value():
    forms = set()
    for name in ("nonbinary_1x6x70", "nonbinary_v1_1x2x1030"):
        v = wc.edt_labels(name)
        forms.add(_regime(name)["form"])
        for val in wc.NONBINARY_VALUES + (1.0, 0.0):
            assert (v == np.float32(val)).any(), (name, val)
        assert np.signbit(v[v == 0]).any()                      # -0.0 is there
        # only == 1.0f is a feature, in float32 and in double alike
        assert np.array_equal(1. - v.astype(np.float64) == 0, wc.is_feature(v))
        assert np.array_equal(np.float32(1) - v == 0, wc.is_feature(v))
    assert forms == {"v1", "v2"}
    assert np.float32(wc.NONBINARY_VALUES[-1]) < 1 and np.float32(wc.NONBINARY_VALUES[-2]) > 1


# ---- the search replay -------------------------------------------------------------------------------------------------------
def _replay_inputs():
    """(case, image index, g, columns, scipy's D2 on those columns) of every v2 image that has a feature"""
    for name in wc.EDT_CASES:
        if _regime(name)["form"] != "v2":
            continue
        cols = wc.REPLAY_COLUMNS.get(name)
        for i, v in enumerate(wc.edt_labels(name)):
            if wc.is_feature(v).any():
                ref = wc.edt_reference_sq(name)[i]
                yield name, i, wc.row_distances(v), cols, ref if cols is None else ref[:, list(cols)]


def test_search_replay_equals_scipy_and_takes_every_branch():
    total = dict.fromkeys(wc.COUNTERS, 0)
    per_case = {}
    for name, i, g, cols, ref in _replay_inputs():
        d2, cnt = wc.column_search_replay(g, cols=cols)
        assert np.array_equal(d2, ref), (name, i)
        for k, v in cnt.items():
            total[k] += v
            per_case.setdefault(name, dict.fromkeys(wc.COUNTERS, 0))[k] += v
    assert all(total[k] > 0 for k in wc.COUNTERS), total
    # the corner feature is seen from the far end of the column: the search crosses every one of the 256 blocks
    assert per_case["tall_corner_1x2048x40"]["skip_block_minimum"] >= 255 * 8 and per_case["tall_corner_1x2048x40"]["down_off_image"] > 0
    # one dense row far from sparse ones: the block-minimum skip and the scan both occur
    dense = per_case["tall_dense_row_1x2048x40"]
    assert dense["skip_block_minimum"] > 0 and dense["scan_neighbour"] > 0 and dense["up_stop_distance"] > 0


def test_search_replay_notices_a_wrong_comparison():
    """`du * du >= best` -> `>` and `du * du + m * m < best` -> `<=` only make the search look at more blocks: the minimum cannot
    change, and the counters show the extra work.  What loses candidates is either test taken one row too far (the nearest row
    of the next block is 8 b + 7 above, 8 b below) and a scan without its tail: each must break the equality with scipy."""
    inputs = [t for t in _replay_inputs() if t[0] != "tall_corner_1x2048x40"]      # 256 steps a pixel: replayed once, above
    base = [wc.column_search_replay(g, cols=cols) for _, _, g, cols, _ in inputs]
    for m in wc.BENIGN_MUTATIONS:
        more = 0
        for (name, i, g, cols, ref), (_, c0) in zip(inputs, base):
            d2, c = wc.column_search_replay(g, mutate=m, cols=cols)
            assert np.array_equal(d2, ref), (m, name, i)
            visited0 = c0["scan_neighbour"] + c0["skip_block_minimum"]
            assert c["scan_neighbour"] >= c0["scan_neighbour"] and c["scan_neighbour"] + c["skip_block_minimum"] >= visited0
            more += (c["scan_neighbour"] - c0["scan_neighbour"]) + (c["scan_neighbour"] + c["skip_block_minimum"] - visited0)
        assert more > 0, m                                      # the table holds the equalities on which the two forms differ
    for m in wc.LOSING_MUTATIONS:
        wrong = [name for name, i, g, cols, ref in inputs if not np.array_equal(wc.column_search_replay(g, mutate=m, cols=cols)[0], ref)]
        assert wrong, m
        print(m, "loses the minimum on", len(wrong), "images, e.g.", wrong[:3])


def test_brute_force_equals_scipy_on_the_tiny_cases():
    n = 0
    for name in wc.EDT_CASES:
        lab = wc.edt_labels(name)
        if lab.shape[1] * lab.shape[2] <= wc.TINY:
            for i, v in enumerate(lab):
                assert np.array_equal(wc.brute_force_sq(v), wc.edt_reference_sq(name)[i]), (name, i)
                n += 1
    assert n >= 25
    e = np.zeros((3, 4), np.float32)                            # scipy's artefact for an image without a feature
    assert np.array_equal(wc.brute_force_sq(e), weightmap_ref.edt_squared(e))


# ---- the map expression ------------------------------------------------------------------------------------------------------
def _case_params():
    for name in wc.EDT_CASES:
        for w0, sigma in wc.params_of(wc.edt_labels(name).shape):
            yield name, w0, sigma


def test_float32_product_is_the_reference_bit_for_bit_and_the_double_product_is_not():
    seen = set()
    for name, w0, sigma in _case_params():
        lab, ref, sq = wc.edt_labels(name), wc.edt_reference_map(name, w0, sigma), wc.edt_reference_sq(name)
        f32 = wc.map_expr_f32(lab, sq, w0, sigma)
        assert np.array_equal(f32.view(np.int64), ref.view(np.int64)), (name, w0, sigma, wc.ulps64(f32, ref))
        f64 = wc.map_expr_f64(lab, sq, w0, sigma)
        differs = int((f64 != ref).sum())
        if w0 in wc.NEW_W0:
            assert differs > 0, (name, w0, sigma)
            seen.add(w0)
        elif set(np.unique(lab)) <= {0.0, 1.0}:                 # 10 and 30 are float32 numbers: on binary labels nothing changes
            assert differs == 0, (name, w0, sigma)
    assert seen == set(wc.NEW_W0)
    assert {p[0] for p in wc.PARAMS} == {10., 30.} | set(wc.NEW_W0)


def test_the_issue_measurement():
    """40 x 70 random label, w0 = 12.3, sigma = 3: the double product is off by ~1e8 float64 ulps and changes hundreds of the
    float32 pixels that are written to disk; the float32 product changes none"""
    lab = (np.random.default_rng(0).random((40, 70)) < 0.05).astype(np.float32)
    ref = weightmap_ref.image_weight_map(lab, 12.3, 3.)[..., 0]
    sq = weightmap_ref.edt_squared(lab)
    f64, f32 = wc.map_expr_f64(lab, sq, 12.3, 3.), wc.map_expr_f32(lab, sq, 12.3, 3.)
    assert wc.ulps64(f32, ref) == 0
    assert wc.ulps64(f64, ref) > 10 ** 7 and (f64.astype(np.float32) != ref.astype(np.float32)).sum() > 100


def test_no_reference_value_sits_on_a_float32_rounding_edge():
    """The GPU float64 map may differ from the reference by 2 float64 ulps (exp's last bit).  Its float32 rounding is then
    the reference's unless the reference lies within 2 ulps of the midpoint of two float32 numbers: no case has such a
    value, so the sweep asserts the float32 maps EQUAL.  (If a new case has one, change its seed.)"""
    for name, w0, sigma in _case_params():
        ref = wc.edt_reference_map(name, w0, sigma)
        bad = wc.near_f32_midpoint(ref, 2 * np.spacing(np.abs(ref)))
        assert not bad.any(), (name, w0, sigma, np.argwhere(bad)[:3].tolist())
    # the ImageWeightMap2 maps are held to 1e-12 in float64: the same condition with that margin
    for name in wc.WM2_CASES:
        for w0, sigma in wc.wm2_params_of(name):
            bad = wc.near_f32_midpoint(wc.wm2_reference(name, w0, sigma), 1e-12)
            assert not bad.any(), (name, w0, sigma, np.argwhere(bad)[:3].tolist())
    for name, make in wc.SCIPY_TILES.items():
        for w0, sigma in wc.WM2_PARAMS:
            assert not wc.near_f32_midpoint(weightmap_ref.image_weight_map2_raster(make(), w0, sigma)[0], 1e-12).any(), (name, w0)
    # the condition does exclude something: the midpoint itself and a value one ulp from it
    mid = 1.0 + 2.0 ** -24
    assert wc.near_f32_midpoint(np.array([mid, np.nextafter(mid, 2.), 1.0 + 2.0 ** -23, 1.5]), 2 * np.spacing(1.0)).tolist() == [True, True, False, False]


# ---- ImageWeightMap2 ---------------------------------------------------------------------------------------------------------
def test_weightmap2_cases_are_what_the_sweep_needs():
    shapes = {wc.wm2_case(n)[0].shape for n in wc.WM2_CASES}
    assert shapes == {(1, 3, 40), (1, 40, 3), (1, 2, 9), (2, 37, 90), (3, 90, 37), (1, 2049, 2050)}
    assert {len(wc.wm2_case(n)[1]) for n in ("narrow_1x3x40", "narrow_1x40x3", "narrow_1x2x9")} == {1, 5}
    sides = set()
    for name in wc.WM2_CASES:
        img, simp, lng = wc.wm2_case(name)
        N, H, W = img.shape
        assert H != W and set(np.unique(img)) <= {0.0, 1.0} and len(lng) == len(simp) and simp.max() < 2 ** 15
        real = simp[simp[:, 0] >= 0]
        assert set(real[:, 0]) == set(range(N))                 # every tile index is used
        V = real[:, 1:].reshape(-1, 3, 2)
        sides |= {s for s, hit in (("top", (V[..., 0] < 0).any()), ("bottom", (V[..., 0] >= H).any()),
                                   ("left", (V[..., 1] < 0).any()), ("right", (V[..., 1] >= W).any())) if hit}
        fg = img != 0
        if name in ("wide_2x37x90", "tall_3x90x37"):
            assert (simp[:, 0] < 0).any() and len(simp) % 4 != 0
            assert fg[:, 0].any() and fg[:, -1].any() and fg[:, :, 0].any() and fg[:, :, -1].any()     # objects on every border
            box = (V[..., 0].max(1) - V[..., 0].min(1) + 1) * (V[..., 1].max(1) - V[..., 1].min(1) + 1)
            assert (box > 64).any()                             # more than one pixel per lane
            area2 = np.abs((V[:, 1, 0] - V[:, 0, 0]) * (V[:, 2, 1] - V[:, 0, 1]) - (V[:, 1, 1] - V[:, 0, 1]) * (V[:, 2, 0] - V[:, 0, 0]))
            assert (area2 == 0).any()                           # a collinear simplex
            last = V[real[:, 0] == N - 1]
            count = wc.raster_clipped(fg[N - 1], last, 10., 5.)[1]
            tie = (count >= 2) & ~fg[N - 1]
            assert tie.sum() >= 5                               # background pixels on a shared edge: the larger key wins
    assert sides == {"top", "bottom", "left", "right"}
    assert wc.stream_trips(2049 * 2050) == 2
    for name, make in wc.SCIPY_TILES.items():
        lab = make()
        assert lab.shape in ((48, 96), (96, 48)) and lab[0].any() and lab[-1].any() and lab[:, 0].any() and lab[:, -1].any()


def test_clipped_raster_equals_the_oracle_on_simplices_inside_the_tile():
    n = 0
    for name in wc.WM2_CASES:
        if name.startswith("stride"):
            continue
        img, simp, _ = wc.wm2_case(name)
        N, H, W = img.shape
        for t in range(N):
            V = simp[simp[:, 0] == t, 1:].reshape(-1, 3, 2)
            V = V[wc.in_tile(V, H, W)]
            if len(V):
                for w0, sigma in wc.WM2_PARAMS:
                    a, ca = wc.raster_clipped(img[t] != 0, V, w0, sigma)
                    b, cb = weightmap_ref.image_weight_map2_raster(img[t], w0, sigma, vertices=V)
                    assert np.array_equal(a, b) and np.array_equal(ca, cb), (name, t)
                n += 1
    assert n >= 6
    # a simplex that sticks out covers, on the tile, what the same simplex covers on a larger tile around it
    V = np.array([[(-5, 10), (8, 4), (6, 30)]])
    small = wc.raster_clipped(np.zeros((37, 90), bool), V, 10., 300.)[1]
    large = wc.raster_clipped(np.zeros((57, 110), bool), V + 10, 10., 300.)[1]
    assert np.array_equal(small, large[10:47, 10:100]) and small.sum() > 0


def test_gaussian_of_the_kernels_equals_scipy_on_narrow_tiles():
    """Tiles narrower than the 9-tap window: scipy's 'reflect' bounces more than once.  The restated accumulation order is the
    kernels'; scipy's pass over the length-1 channel axis adds nine equal taps where the kernels multiply by their sum, so
    the two are not bit-equal: positive terms, three passes of nine products and eight sums on either side, 3 * 2 * 9 * 2^-53
    relative at the most = 27 ulp (observed: 2)."""
    from scipy.ndimage import gaussian_filter
    assert [wc.reflect(i, 3) for i in range(-4, 8)] == [2, 2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1]
    assert [wc.reflect(i, 2) for i in range(-4, 6)] == [0, 1, 1, 0, 0, 1, 1, 0, 0, 1] and wc.reflect(-3, 1) == 0
    rng = np.random.default_rng(5)
    for shape in ((3, 40), (40, 3), (2, 9), (1, 12), (37, 90)):
        a = np.where(rng.random(shape) < 0.5, 1024., rng.random(shape) * 30)
        ref = gaussian_filter(a[..., None], 1.)[..., 0]
        assert wc.ulps64(wc.gauss9_reflect(a), ref) <= 27, shape


# ---- boundary points ---------------------------------------------------------------------------------------------------------
def test_boundary_point_cases():
    assert {wc.points_labels(n).shape for n in wc.POINTS_CASES} == {(2, 5, 70), (2, 70, 5), (3, 6, 6), (1, 1, 20), (1, 2049, 2050)}
    assert wc.stream_trips(2049 * 2050, wc.POINTS_GRID_CAP) > 1
    for name in wc.POINTS_CASES:
        lab, ref = wc.points_labels(name), wc.points_reference(name)
        assert ref.shape == lab.shape and ref.any()
        if 1 not in lab.shape[1:] and "stride" not in name:     # the restatement without np.squeeze is the oracle's
            for v in lab:
                assert np.array_equal(wc.boundary_points_2d(v), weightmap_ref.boundary_points(v))
    for name in ("points_2x5x70", "points_2x70x5"):
        v = wc.points_labels(name)
        assert v[0, 0].any() and v[0, -1].any() and v[0, :, 0].any() and v[0, :, -1].any()          # objects on every border
    v = wc.points_labels("points_2x5x70")
    assert v[0, -1].all() and v[1, 0].all()                     # filled rows on both sides of the batch boundary
    # a kernel reading across it would compute the outline of the two images glued together, which differs on those rows
    glued = wc.boundary_points_2d(v.reshape(10, 70)).reshape(2, 5, 70)
    ref = wc.points_reference("points_2x5x70")
    assert (glued[0, -1] != ref[0, -1]).any() and (glued[1, 0] != ref[1, 0]).any()
