"""Numpy restatement and case table for ImageBlur on the GPU (include/sequitr_hip.h "Frame cleaning", sq_frame_blur_f32).

The definition of record is pipeline.ImageBlur: scipy's gaussian_filter of the float32 plane.  Restated here tap by tap, with
no scipy, and checked against scipy and the host pipe bit for bit in tests/test_frame_blur_cpu.py; the GPU tests compare the
kernel with this restatement.
"""
import os

import numpy as np

GOLDEN = np.load(os.path.join(os.path.dirname(__file__), "golden", "pipeline_golden.npz"))

# sigma -> R: 0.1 -> 0, 0.124 -> 0, 0.125 -> 1, 0.3 -> 1, 0.5 -> 2, 0.7 -> 3, 0.8 -> 3, 1 -> 4, 1.5 -> 6, 2 -> 8, 2.2 -> 9,
# 3.3 -> 13, 4 -> 16, 4.2 -> 17, 8 -> 32, 8.124 -> 32.  2 / 2.2, 4 / 4.2 and 8.124 are the largest radius of each radius class
# of the kernel (8, 16, 32: the three tile widths) and the next one up; the kernel has one instance per radius.
SIGMAS_CPU = (0.1, 0.124, 0.125, 0.3, 0.5, 0.8, 1, 1.5, 2, 3.3, 8, 8.124)
SIGMAS_GPU = (0.1, 0.125, 0.5, 0.7, 1.5, 2, 2.2, 3.3, 4, 4.2, 8.124)
SHAPES_CPU = ((1, 1), (1, 7), (7, 1), (2, 3), (5, 64), (37, 53), (64, 65), (130, 129), (3, 200))


def radius(sigma):
    return int(4.0 * float(sigma) + 0.5)


def weights(sigma):
    """w[0 .. R] in float64, w[0] the centre, with scipy's own expressions (_gaussian_kernel1d)"""
    R = radius(sigma)
    x = np.arange(-R, R + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi /= phi.sum()
    return phi[R:].copy()


def refl(i, L):
    """scipy's mode='reflect' on an index array, repeated until every index is inside"""
    i = np.array(i, dtype=np.int64)
    if L == 1:
        return np.zeros_like(i)
    while True:
        low, high = i < 0, i >= L
        if not (low.any() or high.any()):
            return i
        i = np.where(low, -i - 1, np.where(high, 2 * L - 1 - i, i))


def one_pass(a, w, axis):
    """a float32 array filtered along `axis`: float64 taps added in the order k = R .. 1, one rounding to float32"""
    a = np.moveaxis(np.asarray(a, np.float32), axis, 0)
    L, R = a.shape[0], len(w) - 1
    a64, i = a.astype(np.float64), np.arange(L)
    with np.errstate(invalid="ignore", over="ignore"):
        acc = a64 * w[0]
        for k in range(R, 0, -1):
            acc = acc + (a64[refl(i - k, L)] + a64[refl(i + k, L)]) * w[k]
        out = acc.astype(np.float32)
    return np.moveaxis(out, 0, axis)


def blur_restated(plane, sigma):
    """ImageBlur(sigma) of one (H, W) plane of any pixel type: axis 0 first, over the pixel cast to float32, then axis 1
    over the float32 result"""
    w = weights(sigma)
    x = np.array(plane, dtype="float").astype("float32") if np.asarray(plane).dtype != np.float32 else np.asarray(plane)
    return one_pass(one_pass(x, w, 0), w, 1)


def plane(shape, kind, seed):
    """a seeded (H, W) plane: 'u8' / 'u16' counts, 'f32' of order 1000, 'big' float32 scaled to 1e30"""
    rng = np.random.default_rng(seed)
    if kind == "u8":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == "u16":
        return rng.integers(0, 65536, shape, dtype=np.uint16)
    x = (1000.0 * rng.standard_normal(shape)).astype(np.float32)
    return x * np.float32(1e30 / 1000.0) if kind == "big" else x


def special_plane(shape, seed):
    """float32 with +-0, +-inf, NaN, 1e30 and subnormals sprinkled over noise"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape).astype(np.float32)
    vals = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e30, -1e30, 1e-40, -3e-45, 1.17549435e-38], np.float32)
    n = max(1, x.size // 5)
    flat = x.reshape(-1)
    flat[rng.integers(0, x.size, n)] = vals[rng.integers(0, len(vals), n)]
    return x


def seams(shape, tile_h, tile_w, F=1, seed=0, dtype=np.uint16):
    """F frames of noise with a bright pixel on either side of every tile seam of the first row / column of tiles and in
    every frame corner; the frames differ"""
    H, W = shape
    rng = np.random.default_rng(seed)
    fr = rng.integers(100, 200, (F, H, W)).astype(dtype)
    top = 250 if np.dtype(dtype) == np.uint8 else 60000
    for f in range(F):
        for y in sorted(set([0, H - 1] + [v for s in range(tile_h, H, tile_h) for v in (s - 1, s)])):
            for x in sorted(set([0, W - 1] + [u for s in range(tile_w, W, tile_w) for u in (s - 1, s)])):
                fr[f, y, x] = top - 7 * f
    return fr


def equal_bits(got, want):
    """float32 arrays equal bit for bit, NaN positions equal (a NaN's payload is not part of the contract)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (got.shape, want.shape, got.dtype, want.dtype)
    gn, wn = np.isnan(got), np.isnan(want)
    if not np.array_equal(gn, wn):
        return False
    return np.array_equal(got.view(np.uint32)[~gn], want.view(np.uint32)[~wn])
