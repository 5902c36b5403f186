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
