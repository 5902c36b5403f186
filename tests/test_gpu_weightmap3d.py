"""GPU: volumetric EDT weight maps (sq_edt3d_sq_f64 / sq_weightmap3d_edt_f32, ops.edt3d_squared / weightmap_edt3d,
weightmap.device_weightmaps3d, jobs.SERVER_train_volume weightmap='edt') against the numpy definition of the device form
in tests/weightmap3d_cases.py, which tests/test_weightmap3d_definitions.py pins against scipy's own 3-D transform, and
against oracle.weightmap_ref (the reference's call on a 3-D array) at spacing 1.

Bounds: the squared distances are the definition's bit for bit (the same correctly rounded float64 operations in the same
order); the float64 map is the reference's expression operation by operation on a correctly rounded sqrt, so only exp()
may differ from numpy's in the last bit => <= 2 ulp, the bound of tests/test_gpu_weightmap.py; the float32 map is that
expression rounded once.  Every output sits inside a guarded buffer and the workspace is pre-filled with 0xFF bytes."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import weightmap_ref
from sequitr_amd import _lib, ops
from sequitr_amd.weightmap import device_weightmaps3d
from tests import weightmap3d_cases as wc

pytestmark = pytest.mark.gpu
GUARD = 256
W0, SIGMA = 10., 5.
W0_F64, SIGMA_F64 = 12.3, 3.                                # a w0 that is not a float32 number


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


class Guarded:
    """an output of n elements between two runs of a known pattern that must survive the launch"""

    def __init__(self, n, dtype, pattern):
        self.n, self.pattern = n, pattern
        self.buf = torch.full((n + 2 * GUARD,), pattern, dtype=dtype, device="cuda:0")
        self.ptr = self.buf.data_ptr() + GUARD * self.buf.element_size()

    def take(self, shape):
        h = self.buf.cpu().numpy()
        assert np.all(h[:GUARD] == self.pattern) and np.all(h[GUARD + self.n:] == self.pattern), "guard overwritten"
        return h[GUARD:GUARD + self.n].reshape(shape).copy()


def _workspace(shape):
    nbytes = _lib.load().sq_weightmap3d_workspace(*shape)
    assert nbytes > 0
    ws = torch.full((nbytes + GUARD,), 0xFF, dtype=torch.uint8, device="cuda:0")     # stale contents cannot pass for results
    assert ws.data_ptr() % 16 == 0
    return ws, nbytes


def raw_sq(img, dz):
    lib, shape = _lib.load(), tuple(img.shape)
    ws, nbytes = _workspace(shape)
    out = Guarded(img.numel(), torch.float64, -7.0)
    _lib.check(lib.sq_edt3d_sq_f64(img.data_ptr(), out.ptr, ws.data_ptr(), *shape, dz, ops._stream()), "sq_edt3d_sq_f64")
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0xFF).all()), "wrote past the workspace"
    return out.take(shape)


def raw_map(img, dz, w0=W0, sigma=SIGMA):
    """both outputs of one launch: (float64 map, float32 map)"""
    lib, shape = _lib.load(), tuple(img.shape)
    ws, nbytes = _workspace(shape)
    o64, o32 = Guarded(img.numel(), torch.float64, -7.0), Guarded(img.numel(), torch.float32, -7.0)
    _lib.check(lib.sq_weightmap3d_edt_f32(img.data_ptr(), o64.ptr, o32.ptr, ws.data_ptr(), *shape, w0, sigma, dz,
                                          ops._stream()), "sq_weightmap3d_edt_f32")
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0xFF).all()), "wrote past the workspace"
    return o64.take(shape), o32.take(shape)


def check_case(name):
    lab = wc.labels(name)
    img = dev(lab)
    for dz in wc.SPACINGS:
        want = wc.reference_sq(name, dz)
        got = raw_sq(img, dz)
        bad = got.view(np.int64) != want.view(np.int64)
        assert not bad.any(), (name, dz, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        assert torch.equal(ops.edt3d_squared(img, dz), dev(got))
        if dz == 1.0:
            for i, v in enumerate(lab):
                assert np.array_equal(got[i].astype(np.int64), weightmap_ref.edt_squared(v)), (name, i)
        ref = wc.weight_expr(lab, np.sqrt(want), W0, SIGMA)
        m64, m32 = raw_map(img, dz)
        u = wc.ulps64(m64, ref)
        print("%s dz=%g: float64 map %d ulp from numpy's expression" % (name, dz, u))
        assert u <= 2, (name, dz, u)
        assert np.array_equal(m32, ref.astype(np.float32)), (name, dz, np.abs(m32 - ref).max())
        assert torch.equal(ops.weightmap_edt3d(img, W0, SIGMA, dz, dtype=torch.float64), dev(m64))
        assert torch.equal(ops.weightmap_edt3d(img.reshape(img.shape + (1,)), W0, SIGMA, dz), dev(m32))
    # the reference's own call on the 3-D array; W0_F64 is not a float32 number, so there the float32 product of
    # w0 * (1. - image) on a float32 volume differs from a double one in every background voxel near a feature
    for w0, sigma in ((W0, SIGMA), (W0_F64, SIGMA_F64)):
        w = device_weightmaps3d(lab, w0, sigma, device="cuda:0")
        assert w.dtype == torch.float32 and tuple(w.shape) == lab.shape + (1,) and w.is_cuda
        wn = w.cpu().numpy()[..., 0]
        for i, v in enumerate(lab):
            assert np.array_equal(wn[i], weightmap_ref.image_weight_map(v, w0, sigma).astype(np.float32)), (name, w0, i)
    ref = np.stack([weightmap_ref.image_weight_map(v, W0_F64, SIGMA_F64) for v in lab])
    assert wc.ulps64(wc.weight_expr(lab, np.sqrt(wc.reference_sq(name, 1.0)), W0_F64, SIGMA_F64), ref) == 0
    m64, m32 = raw_map(img, 1.0, W0_F64, SIGMA_F64)
    u = wc.ulps64(m64, ref)
    print("%s w0=%g: float64 map %d ulp from the reference" % (name, W0_F64, u))
    assert u <= 2, (name, W0_F64, u)
    assert np.array_equal(m32, ref.astype(np.float32)), (name, W0_F64)
    return img


@pytest.mark.parametrize("name", [n for n in wc.CASE_NAMES if not n.startswith("deep")])
def test_sweep_against_the_definition(name):
    img = check_case(name)
    if name.startswith("planar"):                            # one slice: the planar map, bit for bit
        for dt in (torch.float64, torch.float32):
            assert torch.equal(ops.weightmap_edt3d(img, W0, SIGMA, 2.5, dtype=dt)[:, 0], ops.weightmap_edt(img[:, 0], W0, SIGMA, dtype=dt))
        assert torch.equal(ops.edt3d_squared(img)[:, 0], ops.edt_squared(img[:, 0]).double())


@pytest.mark.parametrize("lds", ["1", "0"])
def test_both_forms_of_the_depth_pass(lds, monkeypatch):
    monkeypatch.setenv("SQ_EDT3D_LDS", lds)                  # read per launch
    check_case("deep_1x300x4x40")


def test_lds_and_global_forms_are_bit_identical(monkeypatch):
    for name in ("deep_1x300x4x40", "gap_2x12x20x24", "empty_2x4x10x10", "wide_1x3x7x70"):
        img = dev(wc.labels(name))
        res = {}
        for lds in ("1", "0"):
            monkeypatch.setenv("SQ_EDT3D_LDS", lds)
            res[lds] = (raw_sq(img, 1.7),) + raw_map(img, 1.7)
        for a, b in zip(res["1"], res["0"]):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), name


def test_strip_above_48k_of_lds():
    """D * 32 columns * 4 bytes = 64000 > 48 KiB: the launch that has to ask for its LDS; one feature at each end"""
    lab = np.zeros((1, 500, 2, 33), np.float32)
    lab[0, 0, 1, 32] = lab[0, 499, 0, 0] = 1
    got = raw_sq(dev(lab), 1.0)[0]
    assert np.array_equal(got.astype(np.int64), weightmap_ref.edt_squared(lab[0]))
    assert np.array_equal(got, wc.edt3d_sq_def(lab[0], 1.0))


def test_bad_arguments_are_refused():
    img = dev(np.zeros((1, 2, 4, 4), np.float32))
    with pytest.raises(ValueError, match="spacing"):
        ops.edt3d_squared(img, 0.0)
    with pytest.raises(ValueError, match="spacing"):
        ops.weightmap_edt3d(img, spacing=float("nan"))
    with pytest.raises(ValueError, match=r"\(N,D,H,W\)"):
        ops.weightmap_edt3d(img[0])
    with pytest.raises(TypeError):
        ops.weightmap_edt3d(img, dtype=torch.float16)


# ---- the job ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def job_runs(tmp_path_factory):
    """SERVER_train_volume on two 8 x 16 x 16 volumes, 3 steps, same seed: weightmap='edt' (spacing 2), 'uniform', neither,
    and a `weights` file made by the numpy definition"""
    from sequitr_amd import core, jobs
    root = tmp_path_factory.mktemp("wm3d_job")
    saved = core.TensorflowConfiguration.MODELDIR
    core.TensorflowConfiguration.MODELDIR = str(root / "models")
    os.mkdir(str(root / "models"))
    try:
        rng = np.random.default_rng(0)
        zz, xx, yy = np.mgrid[0:8, 0:16, 0:16]
        lab = np.zeros((2, 8, 16, 16), np.uint8)
        lab[0][(zz - 3) ** 2 * 4 + (xx - 5) ** 2 + (yy - 4) ** 2 < 14] = 1       # two cells with a narrow gap between them
        lab[0][(zz - 4) ** 2 * 4 + (xx - 5) ** 2 + (yy - 12) ** 2 < 14] = 1
        lab[1][(zz - 5) ** 2 * 4 + (xx - 10) ** 2 + (yy - 8) ** 2 < 20] = 1
        imgs = (lab * 2.0 + rng.standard_normal(lab.shape) * 0.4).astype(np.float32)
        np.save(str(root / "im.npy"), imgs)
        np.save(str(root / "lab.npy"), lab)
        wdef = np.stack([wc.weightmap3d_def(v, W0, SIGMA, 2.0) for v in lab.astype(np.float32)]).astype(np.float32)
        np.save(str(root / "w.npy"), wdef)
        runs = {}
        for key, extra in (("edt", {"weightmap": "edt", "spacing": 2.0}), ("uniform", {"weightmap": "uniform"}), ("default", {}),
                           ("file", {"weights": str(root / "w.npy"), "weightmap": "edt", "spacing": 7.0})):
            os.mkdir(str(root / key))
            params = dict({"images": str(root / "im.npy"), "labels": str(root / "lab.npy"), "num_outputs": 2, "num_epochs": 5,
                           "dropout": 0.0, "seed": 0, "filters": (16, 32), "output": str(root / key)}, **extra)
            info = jobs.SERVER_train_volume(params, {"gpu": 0, "max_steps": 3})
            runs[key] = (info, json.load(open(str(root / key / "train.json"))))
        return runs
    finally:
        core.TensorflowConfiguration.MODELDIR = saved


def test_job_computes_the_map_on_the_device(job_runs):
    info, tj = job_runs["edt"]
    assert info["steps"] == 3 and len(tj["losses"]) == 3 and np.isfinite(tj["losses"]).all()
    assert tj["weightmap"] == "edt" and tj["w0"] == 10. and tj["sigma"] == 5. and tj["spacing"] == 2.
    first = tj["losses"][0]
    assert first != job_runs["uniform"][1]["losses"][0]
    from_file = job_runs["file"][1]["losses"][0]             # a `weights` file wins over weightmap / spacing
    assert abs(first - from_file) <= 1e-5 * abs(from_file), (first, from_file)
    assert "weightmap" not in job_runs["file"][1]


def test_job_default_is_the_uniform_weight_bit_for_bit(job_runs):
    a, b = job_runs["default"][1]["losses"], job_runs["uniform"][1]["losses"]
    assert len(a) == 3 and a == b, (a, b)


def test_job_refuses_an_unknown_weightmap():
    from sequitr_amd import jobs
    with pytest.raises(ValueError, match="weightmap"):
        jobs.SERVER_train_volume({"weightmap": "delaunay", "images": "/nonexistent.npy"}, {"gpu": 0})
