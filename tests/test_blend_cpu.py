"""CPU: the geometry of seam blending (include/sequitr_hip.h "Seam blending") swept by brute force, frontend.axis_blend and
the library's sq_blend_axis_slots against the dense restatement of tests/blend_cases.py, that restatement against a
pure-Python per-pixel loop, and the properties that make it a blend: B = 0 is the owner-map stitch, a seam between two
constant tiles becomes the exact linear ramp, and tiles cut from one field come back as that field."""
import ctypes

import numpy as np
import pytest

from sequitr_amd import _lib
from sequitr_amd.frontend import axis_blend, axis_tiles, check_blend, segment_frames
from tests import blend_cases as bc
from tests import tta_cases as tc


def sweep(sizes):
    """for every tile size T given: every admissible margin and blend, L = T .. 3T + 2 and 5T + 1"""
    for T in sizes:
        for m in range(0, (T + 1) // 2):
            for B in range(0, m + 1):
                if bc.admissible(T, m, B):
                    for L in list(range(T, 3 * T + 3)) + [5 * T + 1]:
                        yield L, T, m, B


SWEPT = tuple(range(4, 25)) + (32, 33, 64)


def check_geometry(L, T, m, B):
    """the six consequences the header states, at one geometry; returns whether some coordinate has three tiles"""
    origins, s, w = bc.axis_weights(L, T, m, B)
    n, what = len(origins), (L, T, m, B)
    owner = axis_tiles(L, T, m)[1] >> 16
    p = np.arange(L)
    live, o = w > 0, origins.astype(np.int64)[:, None]
    assert not (live & ((p < o) | (p >= o + T))).any(), what                                # only inside tile k
    assert not (live[1:] & (p - o[1:] < m - B)).any(), what                                 # the outer m - B pixels: never
    assert (w[owner, p] >= B + 1).all(), what                                               # the owner's weight
    count = live.sum(0)
    first, last = live.argmax(0), n - 1 - live[::-1].argmax(0)
    assert count.min() >= 1 and count.max() <= 3 and np.array_equal(last - first + 1, count), what   # consecutive
    three = count.max() == 3
    if three:
        assert live[n - 1, count == 3].all() and origins[n - 1] == L - T and s[n - 1] - s[n - 2] < 2 * B, what
    if B > 0 and n > 1:                                                                     # regular seams: both runs >= 2B
        k = np.arange(1, n)
        run = np.diff(s)
        regular = (run[k - 1] >= np.where(k > 1, 2 * B, B)) & (run[k] >= np.where(k < n - 1, 2 * B, B))
        k, j = k[regular], np.arange(-B, B)
        at = s[k][:, None] + j[None, :]
        assert np.array_equal(w[(k - 1)[:, None], at], np.broadcast_to(B - j, at.shape)), what
        assert np.array_equal(w[k[:, None], at], np.broadcast_to(B + j + 1, at.shape)), what
        assert (w[:, at.reshape(-1)].sum(0) == 2 * B + 1).all(), what
    if B == 0:
        assert np.array_equal(w, (owner[None] == np.arange(n)[:, None]).astype(w.dtype)), what
    return three


def test_geometry_sweep():
    """Every geometry of T = 4 .. 24 and of T = 32, 33, 64.  The same function has passed the whole range the header
    names, T = 4 .. 64 (645 966 geometries, a minute and a half): the sizes kept here hold every regime of it -- runs shorter
    than 2B, a last tile clamped to L - T at every offset, one tile, margins 0 .. (T - 1) / 2 -- within a few seconds."""
    geometries = list(sweep(SWEPT))
    assert len(geometries) > 45426
    assert sum(check_geometry(*g) for g in geometries) > 0


def test_the_header_s_example_of_three_tiles():
    origins, s, w = bc.axis_weights(53, 16, 4, 4)
    assert origins.tolist() == [0, 8, 16, 24, 32, 37]
    assert w[:, 37:40].sum(0).tolist() == [10, 11, 10] and ((w[:, 37:40] > 0).sum(0) == 3).all()
    assert [c for c in bc.contributors(bc.axis_blend(53, 16, 4, 4)[1], 37)] == [(3, 13, 3), (4, 5, 6), (5, 0, 1)]


def library_slots(L, T, m, B):
    slots = np.full((L, 3, 2), -7, np.int32)
    n = _lib.load().sq_blend_axis_slots(L, T, m, B, slots.ctypes.data_as(ctypes.c_void_p))
    return n, slots


def test_axis_blend_three_writings_agree():
    """frontend.axis_blend (tile by tile), sq_blend_axis_slots (coordinate by coordinate) and the dense restatement"""
    for L, T, m, B in sweep(range(4, 17)):
        origins, slots = bc.axis_blend(L, T, m, B)
        o2, s2 = axis_blend(L, T, m, B)
        assert s2.dtype == np.int32 and s2.shape == (L, 3, 2)
        assert np.array_equal(o2, origins) and np.array_equal(s2, slots), (L, T, m, B)
        n, s3 = library_slots(L, T, m, B)
        assert n == len(origins) and np.array_equal(s3, slots), (L, T, m, B)
    o, slots = axis_blend(2048, 512, 32, 32)
    assert np.array_equal(slots, bc.axis_blend(2048, 512, 32, 32)[1]) and library_slots(2048, 512, 32, 32)[0] == len(o) == 5
    band = ((slots[:, :, 1] > 0).sum(1) > 1).mean()
    assert abs(band - 4 * 64 / 2048.0) < 1e-12                  # four seams of 2 * 32 coordinates


def test_bad_blends_are_refused_on_the_host_and_in_the_library():
    lib = _lib.load()
    for L, T, m, B in ((64, 16, 4, 5), (64, 16, 4, -1), (64, 16, 6, 3), (64, 16, 0, 1), (4096, 1024, 300, 256)):
        with pytest.raises(ValueError):
            axis_blend(L, T, m, B)
        n, slots = library_slots(L, T, m, B)
        assert n == -1 and (slots == -7).all() and b"blend" in lib.sq_last_error(), (L, T, m, B)
    assert library_slots(15, 16, 4, 1)[0] == -1 and library_slots(64, 16, 8, 0)[0] == -1
    assert lib.sq_blend_axis_slots(64, 16, 4, 1, None) == -1
    for bad in (True, 1.0, "2", (1,)):
        with pytest.raises(ValueError):
            check_blend(bad, 16, 4)
    assert check_blend(None, 16, 4) == 0 and check_blend(np.int64(4), 16, 4) == 4 and check_blend(255, 1024, 255) == 255
    assert axis_blend(64, 16, 4, 2)[1].shape == (64, 3, 2) and library_slots(4096, 1024, 255, 255)[0] > 0


def pixel_loop(acc, H, W, T, m, B):
    """the definition one pixel and one class at a time, in Python scalars of numpy float32"""
    (oy, ys), (ox, xs) = bc.axis_blend(H, T, m, B), bc.axis_blend(W, T, m, B)
    TR, TC, K = len(oy), len(ox), acc.shape[-1]
    F = acc.shape[0] // (TR * TC)
    b = np.zeros((F, H, W, K), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for f in range(F):
            for y in range(H):
                for x in range(W):
                    KY, KX = bc.contributors(ys, y), bc.contributors(xs, x)
                    for c in range(K):
                        S = np.float32(0.0)
                        for ky, ly, wy in KY:
                            for kx, lx, wx in KX:
                                S = np.float32(S + np.float32(np.float32(wy * wx) * acc[(f * TR + ky) * TC + kx, ly, lx, c]))
                        b[f, y, x, c] = np.float32(S / np.float32(sum(k[2] for k in KY) * sum(k[2] for k in KX)))
    return b


@pytest.mark.parametrize("H,W,T,m,B", [(12, 13, 4, 1, 1), (9, 13, 5, 1, 1), (12, 11, 6, 2, 1), (6, 13, 6, 1, 1),
                                       (12, 13, 6, 2, 0), (11, 12, 4, 1, 0)])
def test_restatement_against_a_pixel_loop(H, W, T, m, B):
    rng = np.random.default_rng(H * W + T)
    TR, TC = len(axis_tiles(H, T, m)[0]), len(axis_tiles(W, T, m)[0])
    K = 3
    acc = tc.special_values((2 * TR * TC, T, T, K), rng)
    got, want = bc.blend_rows(acc, H, W, T, m, B), pixel_loop(acc, H, W, T, m, B)
    assert tc.same_bits_nan_aware(got, want)
    assert np.isnan(want).any() and np.isfinite(want).any()


@pytest.mark.parametrize("H,W,T,m", [(37, 53, 16, 4), (16, 80, 16, 2), (12, 13, 6, 1)])
def test_no_blend_is_the_owner_map_stitch(H, W, T, m):
    rng = np.random.default_rng(W)
    TR, TC = len(axis_tiles(H, T, m)[0]), len(axis_tiles(W, T, m)[0])
    acc = tc.special_values((2 * TR * TC, T, T, 4), rng)
    b, owner = bc.blend_rows(acc, H, W, T, m, 0), tc.stitch(acc, H, W, T, m)
    nan = np.isnan(owner)
    assert np.array_equal(np.isnan(b), nan) and np.array_equal(b[~nan], owner[~nan])       # -0 becomes +0: equal as numbers
    mask, p = bc.stitch_blend(acc, 0.25, H, W, T, m, 0)
    want_mask, want_p = tc.stitch_probs(acc, 0.25, H, W, T, m)
    assert np.array_equal(mask, want_mask) and np.array_equal(p, want_p, equal_nan=True)


@pytest.mark.parametrize("B", [1, 3, 4])
def test_constant_tiles_give_the_exact_linear_ramp(B):
    H, W, T, m = 16, 40, 16, 4                                 # tiles at 0, 8, 16, 24: seams at 12, 20, 28
    ox, _ = axis_tiles(W, T, m)
    values = np.array([3, -5, 7, 2], np.float32)
    acc = np.broadcast_to(values[:, None, None, None], (4, T, T, 1)).copy()
    b = bc.blend_rows(acc, H, W, T, m, B)[0, :, :, 0]
    assert (b == b[0]).all()
    for k, s in enumerate((12, 20, 28)):
        lo, hi = float(values[k]), float(values[k + 1])
        for j in range(-B, B):
            want = np.float32(np.float32(lo * (B - j) + hi * (B + j + 1)) / np.float32(2 * B + 1))
            assert b[0, s + j] == want, (s, j)
        if B < 4:
            assert b[0, s - B - 1] == lo and b[0, s + B] == hi


@pytest.mark.parametrize("H,W,T,m,B", [(37, 53, 16, 4, 4), (53, 37, 16, 4, 2), (70, 45, 32, 8, 8)])
def test_tiles_cut_from_one_field_come_back_as_that_field(H, W, T, m, B):
    rng = np.random.default_rng(B)
    field = rng.integers(-50, 51, (2, H, W, 3)).astype(np.float32)          # products with weights <= 17^2 stay exact
    oy, ox = axis_tiles(H, T, m)[0], axis_tiles(W, T, m)[0]
    acc = np.stack([field[f, y:y + T, x:x + T] for f in range(2) for y in oy for x in ox])
    assert np.array_equal(bc.blend_rows(acc, H, W, T, m, B), field)


def test_the_gpu_cases_keep_their_promises():
    """what tests/test_gpu_blend.py relies on, checked without a GPU: at least 99 % of the uint8 values are compared, the
    special rows are there, and NaN at the unused positions changes nothing"""
    for H, W, T, m, B in bc.geometry_cases():
        for K in (1, 2, 16):
            acc, poisoned = bc.blend_case(H, W, T, m, B, 1, K, 0.25, seed=1000 * B + 10 * K + H)
            mask, p = bc.stitch_blend(acc, 0.25, H, W, T, m, B)
            mask2, p2 = bc.stitch_blend(poisoned, 0.25, H, W, T, m, B)
            assert np.array_equal(mask, mask2) and np.array_equal(p, p2, equal_nan=True)
            assert np.isnan(poisoned).sum() > np.isnan(acc).sum() or not (~bc.used_positions(H, W, T, m, B)).any()
            assert bc.u8_boundary_share(p, K) < 0.01, (H, W, B, K)
            assert np.isnan(p).any() and np.isfinite(p).any()
    assert (~bc.used_positions(64, 64, 16, 4, 1)).any()


class Untouchable(object):
    shape, dtype = (3, 70, 90), np.dtype("uint16")

    def __getitem__(self, key):
        raise AssertionError("a frame was read")


class NoNet(object):
    n_outputs, n_inputs, device = 2, 1, "cpu"


def test_segment_frames_checks_blend_before_a_frame_is_read():
    fr = Untouchable()
    for tile, margin, blend in ((32, 4, 5), (32, 4, -1), (32, 0, 1), (32, 12, 5), (32, 4, True), (32, 4, 2.0), (32, 4, "2")):
        with pytest.raises(ValueError, match="blend"):
            segment_frames(NoNet(), fr, tile=tile, margin=margin, blend=blend)
