"""CPU: the numpy definition of the volumetric EDT weight map's device form (tests/weightmap3d_cases.py) against scipy's
own 3-D transform -- distance_transform_edt(1 - image, sampling=(dz, 1, 1)), what ImageWeightMap.pipe
(sequitr/pipeline.py:475-479) computes on a (Z, X, Y) array -- and the host-side validation of the new entry points.

Bounds.  For dz in {1, 2, 2.5, 0.5} every k dz, its square and every sum with an integer below 2^31 is exact in double:
the two must be EQUAL.  For other spacings the device form rounds A + P once where scipy rounds (dz^2 + dx^2) + dy^2
twice: the squared distances differ by at most 2 roundings (relative 2^-52), the square root halves that, and each side
then rounds its root once => <= 2 ulp of d."""
import ctypes

import numpy as np
import pytest
from scipy.ndimage import distance_transform_edt

from oracle import weightmap_ref
from sequitr_amd import _lib
from tests import weightmap3d_cases as wc

EXACT = (1.0, 2.0, 2.5, 0.5)
INEXACT = (1.7, 0.3, float(np.pi))


def _volumes():
    rng = np.random.default_rng(11)
    vols = []
    for shape, p in (((6, 9, 11), 0.03), ((12, 7, 5), 0.01), ((3, 16, 16), 0.1), ((20, 4, 6), 0.004), ((1, 8, 8), 0.1),
                     ((9, 1, 1), 0.3)):
        for _ in range(3):
            v = (rng.random(shape) < p).astype(np.float32)
            if not v.any():
                v[shape[0] // 2, shape[1] // 2, shape[2] // 2] = 1
            vols.append(v)
    gap = (rng.random((10, 8, 8)) < 0.05).astype(np.float32)
    gap[2:7] = 0                                             # featureless slices between featured ones
    vols.append(gap)
    return vols


def test_device_form_definition_against_scipy():
    for v in _volumes():
        for dz in EXACT + INEXACT:
            d = np.sqrt(wc.edt3d_sq_def(v, dz))
            ref = distance_transform_edt(1. - v, sampling=(dz, 1, 1))
            if dz in EXACT:
                assert np.array_equal(d, ref), (v.shape, dz, np.abs(d - ref).max())
            else:
                assert wc.ulps64(d, ref) <= 2, (v.shape, dz, wc.ulps64(d, ref))
        # dz == 1: the reference's own call on the 3-D array, and its exact integer squared distances
        assert np.array_equal(wc.edt3d_sq_def(v, 1.0).astype(np.int64), weightmap_ref.edt_squared(v))
        assert wc.ulps64(wc.weightmap3d_def(v), weightmap_ref.image_weight_map(v)) == 0


def test_volume_without_any_feature_reproduces_scipy():
    """scipy's feature transform points every voxel of a volume without a feature at index (-1, 0, 0)"""
    v = np.zeros((5, 6, 7), np.float32)
    for dz in (1.0, 1.7):
        d = np.sqrt(wc.edt3d_sq_def(v, dz))
        ref = distance_transform_edt(1. - v, sampling=(dz, 1, 1))
        assert np.array_equal(d, ref), (dz, np.abs(d - ref).max())
        assert d[0, 0, 0] == dz and d[4, 0, 0] == np.sqrt((5 * dz) * (5 * dz))
    assert np.array_equal(wc.weightmap3d_def(v), weightmap_ref.image_weight_map(v))


def test_case_list_is_what_the_sweep_needs():
    assert wc.labels("planar_1x1x6x6").any() and wc.labels("column_1x6x1x1").any()
    gap = wc.labels("gap_2x12x20x24")
    assert not gap[0, 3:9].any() and gap[0, :3].any() and gap[0, 9:].any()
    e = wc.labels("empty_2x4x10x10")
    assert not e[0].any() and e[1].sum() == 1
    for name in wc.CASE_NAMES:
        assert set(np.unique(wc.labels(name))) <= {0.0, 1.0}
    # slices outside the 1024 x 2048 box of the second form of the planar passes, each volume with one featureless slice
    for name, outside in (("wideplane_1x2x3x1030", lambda H, W: W > 1024 and H <= 2048),
                          ("tallplane_1x3x2050x3", lambda H, W: H > 2048 and W <= 1024)):
        v = wc.labels(name)
        assert outside(*v.shape[2:]) and [bool(z.any()) for z in v[0]].count(False) == 1 and v.dtype == np.float32


def test_map_expression_follows_numpy_types():
    """on a float32 volume the reference forms w0 * (1. - image) in float32 (w0 is a Python scalar): weight_expr equals the
    reference's call bit for bit at a w0 that is not a float32 number, and the all-double product does not"""
    for name in ("odd_1x5x9x11", "gap_2x12x20x24", "wideplane_1x2x3x1030", "tallplane_1x3x2050x3"):
        lab = wc.labels(name)
        d = np.sqrt(wc.reference_sq(name, 1.0))
        for w0, sigma in ((10., 5.), (12.3, 3.)):
            ref = np.stack([weightmap_ref.image_weight_map(v, w0, sigma) for v in lab])
            assert ref.dtype == np.float64 and wc.ulps64(wc.weight_expr(lab, d, w0, sigma), ref) == 0, (name, w0)
            double = wc.weight_expr(lab.astype(np.float64), d, w0, sigma)
            assert (double != ref).any() == (w0 == 12.3), (name, w0)


def test_host_side_validation_of_the_volumetric_entries_needs_no_gpu():
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15                   # any non-null, 16-byte aligned address: nothing is launched
    for call in (lambda img, out, ws, D, dz: lib.sq_edt3d_sq_f64(img, out, ws, 1, D, 4, 4, dz, None),
                 lambda img, out, ws, D, dz: lib.sq_weightmap3d_edt_f32(img, out, None, ws, 1, D, 4, 4, 10., 5., dz, None)):
        assert call(None, p, p, 2, 1.0) == -1 and b"null" in lib.sq_last_error()
        assert call(p, p, None, 2, 1.0) == -1 and b"null" in lib.sq_last_error()
        assert call(p, None, p, 2, 1.0) == -1
        assert call(p, p, p, 0, 1.0) == -1 and b"0 < D" in lib.sq_last_error()
        for dz in (0.0, -1.0, float("nan"), float("inf")):
            assert call(p, p, p, 2, dz) == -1 and b"spacing" in lib.sq_last_error(), dz
        assert call(p, p, p + 4, 2, 1.0) == -1 and b"aligned" in lib.sq_last_error()
    assert lib.sq_weightmap3d_edt_f32(p, None, None, p, 1, 2, 4, 4, 10., 5., 1.0, None) == -1
    assert b"no output" in lib.sq_last_error()
    ws = lib.sq_weightmap3d_workspace
    assert ws(0, 4, 4, 4) == -1 and ws(1, 0, 4, 4) == -1 and ws(1, 4, -1, 4) == -1 and ws(1, 4, 4, 0) == -1
    assert ws(1, 30000, 4, 4) == -1 and ws(1, 4, 30000, 4) == -1 and ws(1, 4, 4, 30000) == -1
    assert ws(2, 1024, 1024, 1024) == -1                     # N*D*H*W = 2^31
    assert ws(1, 29999, 4, 4) > 0
    n = ws(2, 3, 5, 7)                                       # flags (16 B per 4 slices), P int32 (16-B rounded), g uint16
    assert n == 32 + ((210 * 4 + 15) // 16) * 16 + 210 * 2 and n % 2 == 0


def test_python_layers_refuse_bad_arguments_before_any_launch():
    import torch
    from sequitr_amd import jobs, ops
    with pytest.raises(_lib.SequitrHipError):
        ops.weightmap_edt3d(torch.zeros(1, 2, 4, 4))         # host tensor: no CPU fall-back
    with pytest.raises(_lib.SequitrHipError):
        ops.edt3d_squared(torch.zeros(1, 2, 4, 4))
    with pytest.raises(ValueError, match="weightmap"):
        jobs.SERVER_train_volume({"weightmap": "delaunay", "images": "/nonexistent.npy"}, {})
