"""CPU: the fragment-order f32 filter pack without a device -- the size query, the argument checks of the two new entry points
(no launch is reached), the host-side "does the packed kernel take this call" rule, and the numpy statement of the pack order
(tests/conv_packed_cases.py, which tests/test_gpu_conv_packed.py compares the device pack against bit for bit) as a permutation."""
import numpy as np
import pytest

from sequitr_amd import _lib
from tests import conv_packed_cases as pc
from tests import f32_walk_cases as wc

EINVAL, EALIGN = -1, -3


@pytest.mark.parametrize("K,Cin,Cout", [(3, 16, 64), (3, 32, 64), (3, 48, 192), (3, 256, 256), (3, 128, 128)])
def test_elems_of_eligible_filters(K, Cin, Cout):
    assert _lib.load().sq_conv_packed_filter_elems_f32(K, Cin, Cout) == 9 * Cin * Cout


@pytest.mark.parametrize("K,Cin,Cout", [(1, 64, 64), (3, 8, 64), (3, 24, 64), (3, 64, 96), (3, 64, 32), (3, 0, 64), (3, 64, 0),
                                        (5, 64, 64), (3, -16, 64)])
def test_elems_reports_ineligible_filters_like_the_other_size_queries(K, Cin, Cout):
    lib = _lib.load()
    assert lib.sq_conv_packed_filter_elems_f32(K, Cin, Cout) == -1
    assert lib.sq_conv_packed_weights_elems_bf16(5, 64, 64) == -1          # the convention it follows


def test_pack_entry_validates_without_a_device():
    lib = _lib.load()
    assert lib.sq_conv_pack_filter_f32(None, 256, 3, 16, 64, None) == EINVAL and b"null" in lib.sq_last_error()
    assert lib.sq_conv_pack_filter_f32(256, None, 3, 16, 64, None) == EINVAL and b"null" in lib.sq_last_error()
    for K, Cin, Cout in [(1, 16, 64), (3, 24, 64), (3, 16, 96)]:
        assert lib.sq_conv_pack_filter_f32(256, 512, K, Cin, Cout, None) == EINVAL
        assert b"unsupported" in lib.sq_last_error()
    assert lib.sq_conv_pack_filter_f32(256 + 4, 512, 3, 16, 64, None) == EALIGN
    assert lib.sq_conv_pack_filter_f32(256, 512 + 8, 3, 16, 64, None) == EALIGN and b"aligned" in lib.sq_last_error()


def test_packed_conv_entries_validate_without_a_device():
    lib = _lib.load()
    shape = (2, 256, 256, 32, 64)                                          # a call the packed kernel takes
    assert lib.sq_conv_packed_takes_f32(*shape, 3) == 1
    # x, w, wp, bias, y
    assert lib.sq_conv2d_packed_nhwc_fwd_f32(None, 256, 512, None, 768, *shape, 3, 1.0, 1, None) == EINVAL
    assert b"null" in lib.sq_last_error()
    assert lib.sq_conv2d_packed_nhwc_fwd_f32(256, 512, 768, None, None, *shape, 3, 1.0, 1, None) == EINVAL
    assert lib.sq_conv2d_packed_nhwc_fwd_f32(256, 512, 768, None, 1024, *shape, 3, 1.0, 7, None) == EINVAL
    assert b"activation" in lib.sq_last_error()
    assert lib.sq_conv2d_packed_nhwc_fwd_f32(256, 512, 768 + 4, None, 1024, *shape, 3, 1.0, 1, None) == EALIGN
    assert lib.sq_conv2d_packed_nhwc_fwd_f32(256, 512, 768, 1024 + 4, 2048, *shape, 3, 1.0, 1, None) == EALIGN
    # a tensor of 2 GiB or more is no packed call: it goes to the unpacked entry and its 64-bit-addressed kernel, as without a pack
    big = (64, 1024, 1024, 32, 64)
    assert lib.sq_conv_packed_takes_f32(*big, 3) == 0 and lib.sq_conv_packed_takes_f32(7, 1024, 1024, 32, 64, 3) == 1
    assert lib.sq_conv2d_packed_nhwc_fwd_f32(None, 256, 512, None, 768, *big, 3, 1.0, 1, None) == EINVAL
    assert b"sq_conv2d_nhwc_fwd_f32: null" in lib.sq_last_error()
    assert lib.sq_conv3x3_pool_packed_fwd_f32(256, 512, 768, None, 1024, 2048, *big, 1, None) == EINVAL
    assert b"sq_conv3x3_pool_fwd_f32" in lib.sq_last_error() and b"2 GiB" in lib.sq_last_error()      # as the pooled entry always did
    # x, w, wp, bias, y, pooled
    assert lib.sq_conv3x3_pool_packed_fwd_f32(None, 256, 512, None, 768, 1024, *shape, 1, None) == EINVAL
    assert lib.sq_conv3x3_pool_packed_fwd_f32(256, 512, 768, None, 1024, 2048 + 4, *shape, 1, None) == EALIGN
    # calls the pack is not used for are the unpacked entry points, with their checks: no pack, a shape off the 64-block plan
    assert lib.sq_conv2d_packed_nhwc_fwd_f32(None, None, None, None, None, *shape, 3, 1.0, 1, None) == EINVAL
    assert b"sq_conv2d_nhwc_fwd_f32" in lib.sq_last_error()
    assert lib.sq_conv2d_packed_nhwc_fwd_f32(None, 256, 512, None, 768, 1, 64, 64, 32, 64, 3, 1.0, 1, None) == EINVAL
    assert b"sq_conv2d_nhwc_fwd_f32" in lib.sq_last_error()
    assert lib.sq_conv3x3_pool_packed_fwd_f32(256, 512, 768, None, 1024, 2048, 2, 255, 256, 32, 64, 1, None) == EINVAL
    assert b"even" in lib.sq_last_error()


def test_takes_follows_the_plan_and_the_switch(monkeypatch):
    lib = _lib.load()
    monkeypatch.delenv("SQ_CONV_PACKED", raising=False)
    for N, H, W, Cin, Cout in [(2, 256, 256, 16, 64), (4, 128, 128, 64, 128), (2, 128, 128, 256, 256), (3, 250, 250, 32, 64),
                               (1, 64, 64, 64, 64), (2, 256, 256, 64, 96), (1, 128, 128, 128, 128)]:
        eligible = Cin % 16 == 0 and Cout % 64 == 0
        want = eligible and pc.on_64_blocks(wc.PLAIN, N, H, W, Cin, Cout)[0]
        assert lib.sq_conv_packed_takes_f32(N, H, W, Cin, Cout, 3) == int(want), (N, H, W, Cin, Cout)
    assert lib.sq_conv_packed_takes_f32(2, 256, 256, 32, 64, 1) == 0          # K = 1 has no pack
    monkeypatch.setenv("SQ_CONV_PACKED", "0")                                 # read per call
    assert lib.sq_conv_packed_takes_f32(2, 256, 256, 32, 64, 3) == 0
    monkeypatch.setenv("SQ_CONV_PACKED", "1")
    assert lib.sq_conv_packed_takes_f32(2, 256, 256, 32, 64, 3) == 1


@pytest.mark.parametrize("c", pc.PACKED_WALKS, ids=pc.packed_case_id)
def test_walk_cases_reach_the_regimes_they_declare(c, monkeypatch):
    """every case of the walk sweep (tests/test_gpu_conv_packed.py): the tags it declares are the ones the walk plan and the
    shape give, the 64-channel-block plan and the packed kernel take it, and the walk is the unpacked kernel's"""
    monkeypatch.delenv("SQ_CONV_PACKED", raising=False)
    lib = _lib.load()
    assert set(c.tags) == pc.packed_tags(c)
    on64, p = pc.on_64_blocks(c.form, c.N, c.H, c.W, c.Cin, c.Cout, c.act)
    assert on64, p
    assert lib.sq_conv_packed_takes_f32(c.N, c.H, c.W, c.Cin, c.Cout, 3) == 1
    assert c.form in (wc.PLAIN, wc.POOL) and (c.form == wc.PLAIN or (c.H % 2 == 0 and c.W % 2 == 0))
    assert c.N * c.H * c.W * max(c.Cin, c.Cout) * 4 <= 140e6            # no tensor much over 130 MB
    tiles_x, tiles_y = wc.tiles_xy(c)
    counts = [wc.block_count(p, b) for b in range(p["G"])]
    assert (min(counts), max(counts), sum(counts)) == (p["tmin"], p["tmax"], p["items"]) and p["items"] == c.N * tiles_x * tiles_y
    assert p["G"] == (p["gn"] * tiles_y + p["gy"]) * tiles_x + p["gx"]
    for b in range(p["G"]):
        wc.carries_of_block(p, tiles_x, tiles_y, b)                     # asserts every step lands on tile b + k G
    monkeypatch.setenv("SQ_CONV_PACKED", "0")                           # the switch changes the kernel, never the walk
    assert lib.sq_conv_packed_takes_f32(c.N, c.H, c.W, c.Cin, c.Cout, 3) == 0
    assert pc.packed_walk(c) == p


def test_walk_table_reaches_every_needed_regime():
    """a regime that loses its last case fails here"""
    carried = {}
    for c in pc.PACKED_WALKS:
        for t in c.tags:
            carried.setdefault(t, []).append(pc.packed_case_id(c))
    assert set(carried) == pc.PACKED_NEEDED, (pc.PACKED_NEEDED - set(carried), set(carried) - pc.PACKED_NEEDED)
    assert len({pc.packed_case_id(c) for c in pc.PACKED_WALKS}) == len(pc.PACKED_WALKS)
    nf = pc.NONFINITE_CASE
    assert nf.act == "relu" and nf.bias == "rand" and pc.packed_walk(nf)["tmax"] >= 2 and nf.H % 2 == 0 and nf.W % 2 == 0
    assert pc.on_64_blocks(wc.PLAIN, nf.N, nf.H, nf.W, nf.Cin, nf.Cout, "relu")[0]      # it also runs plain


def test_the_oracle_stores_a_non_finite_pre_activation_under_relu_as_the_kernels_do():
    """oracle/sq_oracle.c applies ReLU as v > 0.0f ? v : 0.0f: a NaN or -inf pre-activation gives +0, +inf stays +inf, as
    fmaxf(v, 0) on the kernels' fast paths.  The non-finite GPU tests still use it only where the whole neighbourhood is finite;
    pc.neighbourhoods marks exactly the outputs a planted value can reach."""
    from oracle import c_oracle as co
    x = np.zeros((1, 6, 6, 16), np.float32)
    x[0, 1, 1, 0], x[0, 4, 4, 15], x[0, 1, 4, 3] = np.nan, np.inf, -np.inf
    w = np.ones((3, 3, 16, 4), np.float32)
    w[..., 1] = -1.0
    y = co.conv2d(x, w, np.full(4, 0.5, np.float32), act="relu")
    finite, has_nan = (m.numpy() for m in pc.neighbourhoods(x))
    assert has_nan.sum() == 9 and (~finite).sum() == 27
    assert not np.isnan(y).any() and not np.signbit(y).any()
    assert (y[has_nan].view(np.uint32) == 0).all()                     # NaN -> +0
    assert np.isposinf(y[0, 3:6, 3:6, 0]).all() and (y[0, 3:6, 3:6, 1].view(np.uint32) == 0).all()     # +inf stays, -inf -> +0
    assert (y[0, 0:3, 3:6, 0].view(np.uint32) == 0).all() and np.isposinf(y[0, 0:3, 3:6, 1]).all()
    assert (y[finite] == 0.5).all()
    assert np.isnan(co.conv2d(x, w, None, act=None)[has_nan]).all()     # the NaN is there before the activation


def test_a_mismatch_names_its_block_and_its_place_in_the_walk():
    """the report of the GPU sweeps (pc.mismatch), on arrays made to differ in one known element"""
    c = pc.PACKED_WALKS[0]
    p, (tiles_x, tiles_y) = pc.packed_walk(c), wc.tiles_xy(c)
    assert (p["G"], p["tmin"], p["tmax"]) == (87, 2, 3)
    t = 5 + 2 * p["G"]                                                  # the third tile of block 5
    n, tyi, txi = t // (tiles_x * tiles_y), (t // tiles_x) % tiles_y, t % tiles_x
    b, pos, cnt = wc.tile_position(p, tiles_x, tiles_y, n, tyi, txi)
    assert (b, pos, cnt) == (5, 2, 3)
    ref = np.zeros((c.N, c.H, c.W, c.Cout), np.float32)
    assert pc.mismatch(ref.copy(), ref, p, c.H, c.W) is None
    got = ref.copy()
    y, x, ch = 16 * tyi + 3, 16 * txi + 15, 200
    got[n, y, x, ch] = 1.0
    msg = pc.mismatch(got, ref, p, c.H, c.W)
    assert "y: 1 of %d elements differ" % ref.size in msg, msg
    assert "(n %d, y %d, x %d, channel %d)" % (n, y, x, ch) in msg, msg
    assert "tile (n %d, ty %d, tx %d), item %d of %d of block %d (of 87 blocks), channel block 3" % (n, tyi, txi, pos, cnt, b) in msg, msg
    assert "[((2, 3), 1)]" in msg, msg
    got[n, y, x, ch] = -0.0                                             # equal as floats, not in bits: still a mismatch
    assert "1 of %d elements differ" % ref.size in pc.mismatch(got, ref, p, c.H, c.W)
    # a pooled pixel (y, x) lies in the tile of (2 y, 2 x); the 32 -> 32 kernel's channel blocks are 32 wide
    got = np.zeros((c.N, c.H // 2, c.W // 2, 32), np.float32)
    ref = got.copy()
    got[n, 8 * tyi + 7, 8 * txi, 31] = np.nan
    msg = pc.mismatch(got, ref, p, c.H, c.W, name="pooled", bn=32)
    assert "tile (n %d, ty %d, tx %d), item 2 of 3 of block 5 (of 87 blocks), channel block 0" % (n, tyi, txi) in msg, msg
    # the last block of the uneven walk: two tiles
    t = 86 + p["G"]
    n, tyi, txi = t // (tiles_x * tiles_y), (t // tiles_x) % tiles_y, t % tiles_x
    assert wc.tile_position(p, tiles_x, tiles_y, n, tyi, txi) == (86, 1, 2)
    ref = np.zeros((c.N, c.H, c.W, c.Cout), np.float32)
    got = ref.copy()
    got[n, 16 * tyi, 16 * txi, 0] = 2.0
    assert "item 1 of 2 of block 86 (of 87 blocks), channel block 0" in pc.mismatch(got, ref, p, c.H, c.W)


@pytest.mark.parametrize("Cin", [16, 48])
@pytest.mark.parametrize("Cout", [64, 192])
def test_pack_order_is_a_permutation(Cin, Cout):
    idx = pc.pack_index(Cin, Cout)
    assert idx.shape == (9 * Cin * Cout,)
    assert np.array_equal(np.sort(idx), np.arange(9 * Cin * Cout))           # every weight exactly once
    # spot checks of the definition: element nb of lane (kk, li) of step (cb, c, tap, s)
    w = np.arange(9 * Cin * Cout, dtype=np.float32).reshape(3, 3, Cin, Cout)
    wp = pc.pack_numpy(w).reshape(Cout // 64, Cin // 16, 9, 4, 4, 16, 4)
    rng = np.random.default_rng(Cin * 1000 + Cout)
    for _ in range(200):
        cb, c, tap, s = rng.integers(Cout // 64), rng.integers(Cin // 16), rng.integers(9), rng.integers(4)
        kk, li, nb = rng.integers(4), rng.integers(16), rng.integers(4)
        assert wp[cb, c, tap, s, kk, li, nb] == w[tap // 3, tap % 3, 16 * c + 4 * s + kk, 64 * cb + 16 * nb + li]
    # one MFMA step is 1 KiB contiguous, an item's 36 steps follow each other, a tile's chunks follow each other
    assert wp.strides[3] == 1024 and wp.strides[2] == 4096 and wp.strides[1] == 36 * 1024
