"""Shared by tests/test_weightmap3d_definitions.py (CPU) and tests/test_gpu_weightmap3d.py (GPU): the numpy definition of
the device form of the volumetric EDT weight map (sq_edt3d_sq_f64 / sq_weightmap3d_edt_f32) and the case list.

Device form, per volume (Z, X, Y) with depth spacing dz:
    D3(z,x,y) = min over z' of fl(A(|z - z'|) + P(z',x,y)),   A(k) = fl(fl(k dz) fl(k dz))
P = the exact planar squared distance of slice z' (an integer, here taken per slice from scipy's 2-D transform), +inf for
a slice without a feature.  A volume without any feature takes scipy's artefact, the distance to index (-1, 0, 0):
D3 = fl(fl(((z+1) dz)^2 + x^2) + y^2).  The map is ImageWeightMap.pipe's float64 expression (sequitr/pipeline.py:475-479)
on d = sqrt(D3)."""
import functools

import numpy as np
from scipy.ndimage import distance_transform_edt

SPACINGS = (1.0, 2.5, 1.7)


def planar_sq(vol):
    """(Z,X,Y) binary -> float64 (Z,X,Y): exact squared planar distance per slice, +inf where the slice has no feature"""
    vol = np.asarray(vol, np.float64)
    P = np.full(vol.shape, np.inf)
    for z in range(vol.shape[0]):
        if (1. - vol[z] == 0).any():
            d = distance_transform_edt(1. - vol[z])
            P[z] = np.rint(d * d)
    return P


def edt3d_sq_def(vol, dz=1.0):
    """the device form of the squared 3-D distance of one volume, float64"""
    vol = np.asarray(vol, np.float64)
    Z, X, Y = vol.shape
    dz = np.float64(dz)
    if not (1. - vol == 0).any():
        z, x, y = np.meshgrid(np.arange(Z, dtype=np.float64), np.arange(X, dtype=np.float64),
                              np.arange(Y, dtype=np.float64), indexing='ij')
        t = (z + 1.) * dz
        return (t * t + x * x) + y * y
    P = planar_sq(vol)
    t = np.arange(Z, dtype=np.float64) * dz
    A = t * t
    zs = np.arange(Z)
    out = np.full(vol.shape, np.inf)
    for zp in range(Z):
        if np.isfinite(P[zp, 0, 0]):
            np.minimum(out, A[np.abs(zs - zp)][:, None, None] + P[zp][None], out=out)
    return out


def weight_expr(vol, d, w0=10., sigma=5.):
    """pipeline.py:477-479 on a given distance array, with numpy's types: on a float32 volume (what the device takes) w0 is a
    Python scalar and w0 * (1. - image) the float32 product fl32(fl32(w0) * fl32(1 - image)), widened where it meets the
    float64 exp(...); on a float64 volume everything is float64"""
    image = np.asarray(vol)
    if image.dtype == np.float32:
        wb = (np.float32(w0) * (np.float32(1.) - image)).astype(np.float64)
    else:
        image = image.astype(np.float64)
        wb = w0 * (1. - image)
    return wb * np.exp(-(d * d) / (2. * sigma ** 2 + 1e-99)) + image + 1.


def weightmap3d_def(vol, w0=10., sigma=5., dz=1.0):
    return weight_expr(vol, np.sqrt(edt3d_sq_def(vol, dz)), w0, sigma)


def ulps64(a, b):
    """largest distance in float64 units in the last place between two arrays of non-negative finite doubles"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return int(np.abs(a.view(np.int64) - b.view(np.int64)).max())


def _random(seed, shape, p):
    return (np.random.default_rng(seed).random(shape) < p).astype(np.float32)


def _single():
    v = np.zeros((1, 40, 8, 33), np.float32)
    v[0, 39, 7, 32] = 1                                      # the search runs the full depth from z = 0
    return v


def _gap():
    v = _random(7, (2, 12, 20, 24), 0.05)
    v[0, 3:9] = 0                                            # featureless slices between featured ones
    return v


def _empty_and_corner():
    v = np.zeros((2, 4, 10, 10), np.float32)                 # volume 0 empty: the per-volume artefact
    v[1, 0, 0, 0] = 1                                        # volume 1: nothing may leak across the batch boundary
    return v


def _featureless_slice(seed, shape, p, z):
    v = _random(seed, shape, p)
    v[0, z] = 0                                              # P_INF from the first form of the planar passes
    return v


# name -> labels (N, D, H, W) float32; the shapes and densities of the sweep
_CASES = {
    "planar_1x1x6x6": lambda: _random(1, (1, 1, 6, 6), 0.1),
    "column_1x6x1x1": lambda: _random(2, (1, 6, 1, 1), 0.3),
    "odd_1x5x9x11": lambda: _random(3, (1, 5, 9, 11), 0.03),
    "batch_2x8x16x16": lambda: _random(4, (2, 8, 16, 16), 0.01),
    "wide_1x3x7x70": lambda: _random(5, (1, 3, 7, 70), 0.02),
    "single_1x40x8x33": _single,
    "gap_2x12x20x24": _gap,
    "empty_2x4x10x10": _empty_and_corner,
    "deep_1x300x4x40": lambda: _random(6, (1, 300, 4, 40), 0.002),
    # slices wider than 1024 / taller than 2048: the planar half runs edt_rows_kernel + edt_cols_weight_kernel<true, true>
    "wideplane_1x2x3x1030": lambda: _featureless_slice(8, (1, 2, 3, 1030), 0.004, 1),
    "tallplane_1x3x2050x3": lambda: _featureless_slice(9, (1, 3, 2050, 3), 0.004, 1),
}
CASE_NAMES = tuple(_CASES)


@functools.lru_cache(maxsize=None)
def labels(name):
    v = _CASES[name]()
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def reference_sq(name, dz):
    """edt3d_sq_def of every volume of a case, computed once and shared (read-only)"""
    r = np.stack([edt3d_sq_def(v, dz) for v in labels(name)])
    r.setflags(write=False)
    return r
