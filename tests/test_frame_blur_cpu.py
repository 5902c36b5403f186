"""CPU: the contract of ImageBlur on the GPU, pinned without one -- the restatement of tests/frame_blur_cases.py against
scipy, the host pipe and the reference's own vector; FrameClean with a blur step and from_pipeline; the header."""
import itertools
import os
import re

import numpy as np
import pytest
from scipy import ndimage

from sequitr_amd import pipeline
from sequitr_amd.frontend import FrameClean, blur_weights
from tests import frame_blur_cases as fb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = fb.GOLDEN


@pytest.mark.parametrize("sigma", fb.SIGMAS_CPU)
def test_restatement_is_scipy_and_the_host_pipe(sigma):
    for n, shape in enumerate(fb.SHAPES_CPU):
        for kind in ("u16", "f32", "big"):
            x = fb.plane(shape, kind, 10 * n + 1)
            got = fb.blur_restated(x, sigma)
            x32 = np.array(x, dtype="float").astype("float32")
            with np.errstate(invalid="ignore", over="ignore"):
                want = ndimage.gaussian_filter(x32, sigma)
                host = pipeline.ImageBlur(sigma)(np.array(x))
            assert want.dtype == np.float32 and host.shape == shape + (1,) and host.dtype == np.float32
            assert fb.equal_bits(got, want), (shape, kind, sigma)
            assert fb.equal_bits(got, np.ascontiguousarray(host[..., 0])), (shape, kind, sigma)


def test_restatement_gives_the_reference_vector():
    got = fb.blur_restated(G["img_in"], 1.5)
    assert G["blur_out"].shape == G["img_in"].shape + (1,)
    assert fb.equal_bits(got, np.ascontiguousarray(G["blur_out"][..., 0]))
    assert (got != G["img_in"]).any()


def test_radius_follows_scipy():
    for sigma, R in ((0.124, 0), (0.125, 1), (8.124, 32), (8.125, 33), (0.5, 2), (1.5, 6)):
        assert fb.radius(sigma) == R, sigma
        if R <= 32:
            r, w = blur_weights(sigma)
            assert r == R and w.dtype == np.float64 and w.shape == (R + 1,)
            assert np.array_equal(w, fb.weights(sigma))
            # scipy's own kernel, where it can be reached
            full = ndimage.gaussian_filter1d(np.eye(1, 2 * R + 1, R, dtype=np.float64)[0], sigma, mode="constant")
            assert np.allclose(full[R:], w, rtol=1e-15, atol=0)
    assert blur_weights(0.1)[1].tolist() == [1.0]
    with pytest.raises(ValueError, match="ImageBlur"):
        blur_weights(8.125)


MAKE = {"O": lambda: pipeline.ImageOutliers(3, 40.), "G": lambda: pipeline.ImageBlur(1.5), "B": pipeline.ImageBGSubtract,
        "N": pipeline.ImageNorm}
LEGAL = ["".join(c) for n in range(5) for c in itertools.combinations("OGBN", n)]


def test_there_are_sixteen_subsequences():
    assert len(LEGAL) == 16 and len(set(LEGAL)) == 16


@pytest.mark.parametrize("letters", LEGAL, ids=[l or "empty" for l in LEGAL])
def test_from_pipeline_accepts_every_subsequence_of_the_four_pipes(letters, tmp_path):
    p = pipeline.ImagePipeline([MAKE[c]() for c in letters])
    want = FrameClean((3, 40.) if "O" in letters else None, "B" in letters, blur=1.5 if "G" in letters else None)
    p.save(str(tmp_path / "pipe.json"))
    for source in (p, str(tmp_path / "pipe.json")):
        clean, normalise = FrameClean.from_pipeline(source)
        assert normalise == ("N" in letters)
        assert (clean == want) if set(letters) & set("OGB") else clean is None
        chain = (clean or FrameClean()).pipes(normalise)
        assert [list(q)[0] for q in chain] == [q.__class__.__name__ for q in p.pipeline]
        if "G" in letters:
            assert clean.blur == 1.5 and {"ImageBlur": {"sigma": 1.5}} in chain


@pytest.mark.parametrize("letters", ["GO", "BG", "NG"])
def test_from_pipeline_rejects_a_blur_out_of_order(letters, tmp_path):
    p = pipeline.ImagePipeline([MAKE[c]() for c in letters])
    p.save(str(tmp_path / "bad.json"))
    for source in (p, str(tmp_path / "bad.json")):
        with pytest.raises(ValueError, match="ImageBlur"):
            FrameClean.from_pipeline(source)


@pytest.mark.parametrize("sigma", [0, -1, float("nan"), float("inf"), 8.125, "1.5"], ids=str)
def test_from_pipeline_rejects_a_sigma_outside_the_limits(sigma, tmp_path):
    p = pipeline.ImagePipeline([pipeline.ImageBlur(sigma), pipeline.ImageNorm()])
    with pytest.raises(ValueError, match="ImageBlur"):
        FrameClean.from_pipeline(p)
    p.save(str(tmp_path / "bad.json"))
    with pytest.raises(ValueError, match="ImageBlur"):
        FrameClean.from_pipeline(str(tmp_path / "bad.json"))
    with pytest.raises(ValueError, match="ImageBlur"):
        FrameClean(blur=sigma)


def test_a_duplicate_blur_is_rejected():
    with pytest.raises(ValueError, match="ImageBlur"):
        FrameClean.from_pipeline(pipeline.ImagePipeline([pipeline.ImageBlur(1.), pipeline.ImageBlur(1.)]))


def test_frame_clean_with_a_blur_is_a_plain_value():
    assert FrameClean(blur=None) == FrameClean() and not FrameClean(blur=None)
    assert hash(FrameClean(blur=None)) == hash(FrameClean())
    assert repr(FrameClean((2, 50.), True)) == "FrameClean(outliers=(2, 50.0), bgsubtract=True)"
    a, b = FrameClean(blur=0.5), FrameClean(blur=0.5)
    assert a and a == b and hash(a) == hash(b) and a != FrameClean(blur=1.5) and a != FrameClean()
    assert FrameClean((2, 50.), True, 1) == FrameClean((2, 50.), True, blur=1.0)
    assert FrameClean((2, 50.), True, blur=0.5) != FrameClean((2, 50.), True)
    assert "blur=0.5" in repr(a) and len({a, b, FrameClean()}) == 2
    assert FrameClean((2, 50.), True).blur is None and FrameClean((2, 50.), True).bgsubtract is True
    assert FrameClean((3, 40.), True, 2).pipes() == [{"ImageOutliers": {"sigma": 3, "threshold": 40.}},
                                                     {"ImageBlur": {"sigma": 2.0}}, {"ImageBGSubtract": {}}, {"ImageNorm": {}}]


def test_header_declares_the_blur():
    src = open(os.path.join(ROOT, "include", "sequitr_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bsq_frame_blur_f32\s*\(", code)
    assert "pipeline.py:244-263" in src
    from sequitr_amd import _lib
    assert "sq_frame_blur_f32" in _lib.SIGNATURES
