"""GPU: the planar weight-map kernels of sequitr_amd/csrc/sq_weightmap.hip (both forms of the row and column passes, the
ImageWeightMap2 raster and Gaussian kernels) and wm2_points_kernel of sq_delaunay.hip at every launch regime, against the
references of tests/weightmap_cases.py.  tests/test_weightmap_definitions.py shows without a GPU that the case tables reach
every regime, and why each bound below holds.

Bounds.  Squared distances: EQUAL to scipy's (exact integers).  EDT float64 map: the reference's expression operation by
operation on a correctly rounded sqrt, so only exp() may differ from numpy's in the last bit => <= 2 float64 ulp, the bound
of tests/test_gpu_weightmap.py.  EDT float32 map: EQUAL to the reference's float64 map rounded once (no reference value lies
within 2 ulp of a float32 rounding edge).  ImageWeightMap2: 1e-12 of the raster definition in float64, as in
tests/test_gpu_weightmap.py, and the float32 map EQUAL to that definition rounded once (no value within 1e-12 of an edge).
Boundary points: EQUAL."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import weightmap_ref
from sequitr_amd import ops
from tests import weightmap_cases as wc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def check_squared(name):
    img = dev(wc.edt_labels(name))
    got = ops.edt_squared(img).cpu().numpy().astype(np.int64)
    bad = got != wc.edt_reference_sq(name)
    assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    return img


def check_maps(name, img, w0, sigma):
    ref = wc.edt_reference_map(name, w0, sigma)
    got64 = ops.weightmap_edt(img, w0, sigma, dtype=torch.float64).cpu().numpy()
    got32 = ops.weightmap_edt(img, w0, sigma, dtype=torch.float32).cpu().numpy()
    u = wc.ulps64(got64, ref)
    bad = got32 != ref.astype(np.float32)
    print("%s w0=%g sigma=%g: float64 map %d ulp from the reference, %d of %d float32 pixels differ"
          % (name, w0, sigma, u, int(bad.sum()), bad.size))
    assert u <= 2, (name, w0, sigma, u)
    assert not bad.any(), (name, w0, sigma, int(bad.sum()), np.argwhere(bad)[:4].tolist())


# ---- planar EDT ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", wc.EDT_CASES)
def test_squared_distances_equal_scipy(name):
    check_squared(name)


# every (w0, sigma) on the cases up to wc.SMALL pixels, (10, 5) and (12.3, 3) on all of them
@pytest.mark.parametrize("name,w0,sigma", [(n, w0, s) for n in wc.EDT_CASES for w0, s in wc.params_of(wc.shape_of(n))],
                         ids=lambda v: v if isinstance(v, str) else "%.3g" % v)
def test_maps_equal_the_reference(name, w0, sigma):
    check_maps(name, dev(wc.edt_labels(name)), w0, sigma)


@pytest.mark.parametrize("shape", [(1, 9, 70), (1, 3, 1026)], ids=["v2", "v1"])
def test_nothing_stale_in_the_cached_workspace(shape):
    """feature -> empty -> feature batches of one shape back to back through the same cached workspace: a flag or a g left from
    the call before would show in the next"""
    assert wc.regime(*shape)["form"] == ("v2" if shape[2] <= 1024 else "v1")
    full = wc._random(71, shape, 0.02)
    other = wc._random(72, shape, 0.02)
    empty = np.zeros(shape, np.float32)
    for k, lab in enumerate((full, empty, other, empty, full)):
        img = dev(lab)
        d2 = ops.edt_squared(img).cpu().numpy()[0].astype(np.int64)
        assert np.array_equal(d2, weightmap_ref.edt_squared(lab[0])), (shape, k)
        for w0, sigma in wc.PARAMS_ALL:
            ref = weightmap_ref.image_weight_map(lab[0], w0, sigma)[..., 0]
            got = ops.weightmap_edt(img, w0, sigma, dtype=torch.float64).cpu().numpy()[0]
            assert wc.ulps64(got, ref) <= 2, (shape, k, w0)


def child_main():
    """run in a fresh process with SQ_EDT_V2=0: the row-pass cases, all narrower than 1025 pixels, through the first form"""
    assert os.environ.get("SQ_EDT_V2") == "0"
    failed = 0
    for name in wc.ROW_PASS_CASES + ("batch_empty_middle_3x9x70", "nonbinary_1x6x70"):
        try:
            img = check_squared(name)
            for w0, sigma in wc.PARAMS_ALL:
                check_maps(name, img, w0, sigma)
            print("pass", name)
        except AssertionError as e:
            failed += 1
            print("FAIL", name, e)
    return 1 if failed else 0


def test_first_form_on_narrow_images_in_a_child_process():
    """SQ_EDT_V2 is read once per process: one fresh child runs the W <= 1024 row-pass cases through edt_rows_kernel /
    edt_cols_weight_kernel"""
    code = "import sys; sys.path.insert(0, %r); from tests import test_gpu_weightmap_sweep as t; sys.exit(t.child_main())" % ROOT
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SQ_EDT_V2="0"), cwd=ROOT, capture_output=True,
                       text=True, timeout=240)
    print(r.stdout[-4000:], r.stderr[-2000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.count("pass ") == len(wc.ROW_PASS_CASES) + 2 and "FAIL" not in r.stdout


# ---- ImageWeightMap2 ---------------------------------------------------------------------------------------------------------
def check_wm2(name, got64, got32, ref, w0):
    err = np.abs(got64 - ref)
    bad = got32 != ref.astype(np.float32)
    print("%s w0=%g: float64 map within %.3g of the definition, %d of %d float32 pixels differ" % (name, w0, err.max(), int(bad.sum()), bad.size))
    assert got64.shape == ref.shape and err.max() <= 1e-12, (name, w0, err.max(), np.argwhere(err > 1e-12)[:4].tolist())
    assert not bad.any(), (name, w0, int(bad.sum()), np.argwhere(bad)[:4].tolist())


@pytest.mark.parametrize("name", wc.WM2_CASES)
def test_weightmap2_hand_made_simplices(name):
    img, simp, lng = wc.wm2_case(name)
    d_img, d_simp, d_lng = dev(img), dev(simp), dev(lng)
    for w0, sigma in wc.wm2_params_of(name):
        got64 = ops.weightmap_delaunay(d_img, d_simp, d_lng, w0, sigma, dtype=torch.float64).cpu().numpy()
        got32 = ops.weightmap_delaunay(d_img, d_simp, d_lng, w0, sigma, dtype=torch.float32).cpu().numpy()
        check_wm2(name, got64, got32, wc.wm2_reference(name, w0, sigma), w0)


@pytest.mark.parametrize("name", tuple(wc.SCIPY_TILES))
def test_weightmap2_reference_path_on_oblong_tiles(name):
    from sequitr_amd.weightmap import device_weightmaps2
    lab = wc.SCIPY_TILES[name]()
    for w0, sigma in wc.WM2_PARAMS:
        ref = weightmap_ref.image_weight_map2_raster(lab, w0, sigma)[0]
        got64 = device_weightmaps2(lab[None], w0, sigma, device="cuda:0", dtype=torch.float64, triangulation="scipy").cpu().numpy()[0]
        got32 = device_weightmaps2(lab[None], w0, sigma, device="cuda:0", triangulation="scipy").cpu().numpy()[0]
        check_wm2(name, got64, got32, ref, w0)


# ---- boundary points ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", wc.POINTS_CASES)
def test_boundary_points_equal_the_reference(name):
    got = ops.wm2_boundary_points(dev(wc.points_labels(name))).cpu().numpy()
    assert got.dtype == np.uint8 and got.max() <= 1
    bad = got.astype(bool) != wc.points_reference(name)
    assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:4].tolist())
