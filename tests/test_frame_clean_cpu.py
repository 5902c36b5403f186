"""CPU: the contract of frame cleaning on the GPU, pinned without one -- the restated definitions of
tests/frame_clean_cases.py against the host pipes and the reference's own vectors, FrameClean.from_pipeline, the header."""
import os
import re

import numpy as np
import pytest

from sequitr_amd import pipeline
from sequitr_amd.frontend import FrameClean
from tests import frame_clean_cases as fc
from tests.util import assert_bit_exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = fc.GOLDEN


@pytest.mark.parametrize("size", fc.SIZES)
def test_restated_median_is_the_host_pipe(size):
    for case, ((F, H, W), _) in enumerate(fc.CASES):
        if min(H, W) < size:
            continue
        for f, frame in enumerate(fc.frames(case)):
            for thr in (50., 4.):
                assert_bit_exact(fc.outliers_restated(frame, size, thr), fc.outliers_host(frame, size, thr),
                                 "case %d frame %d size %d threshold %g" % (case, f, size, thr))


def test_restated_median_gives_the_reference_vector():
    assert_bit_exact(fc.outliers_restated(G["img_in"], 2, 50.), G["outliers_out"][..., 0], "outliers_out")
    assert (fc.outliers_restated(G["img_in"], 2, 50.) != G["img_in"]).any()


def test_case_frames_hold_what_they_promise():
    for case, ((F, H, W), dtype) in enumerate(fc.CASES):
        fr = fc.frames(case)
        assert fr.shape == (F, H, W) and fr.dtype == dtype and np.isfinite(fr.astype(np.float64)).all()
        assert not np.signbit(fr.astype(np.float64)[fr == 0]).any()
        for f in range(F):
            if (H, W) == G["img_in"].shape and f == 0:
                continue
            cleaned = fc.outliers_host(fr[f], 3, 50.) if min(H, W) >= 3 else fc.outliers_host(fr[f], 2, 50.)
            hot = cleaned != fc.as_float32(fr[f])
            assert hot[0, 0] and hot[0, W - 1] and hot[H - 1, 0] and hot[H - 1, W - 1], (case, f)
    assert np.array_equal(fc.frames(1)[0], G["img_in"])


def test_oracle_fit_is_the_host_pipe_and_the_reference_vector():
    img = G["img_in"]
    surface, coef = fc.oracle_fit(img)
    d = fc.delta(img)
    assert np.abs((img.astype(np.float64) - surface) - G["bgsub_out"][..., 0]).max() <= d
    assert np.abs(fc.basis_surface(coef, *img.shape) - surface).max() <= d
    for case in range(len(fc.CASES)):
        for frame in fc.frames(case):
            x = fc.as_float32(frame)
            host = pipeline.ImageBGSubtract()(np.array(frame))[..., 0]
            assert host.dtype == np.float64
            got = x.astype(np.float64) - fc.oracle_fit(x)[0]
            assert np.abs(got - host).max() <= fc.delta(x), (case, np.abs(got - host).max(), fc.delta(x))


def test_oracle_chain_is_the_host_chain():
    frame = fc.frames(4)[0]
    chain = pipeline.ImagePipeline([pipeline.ImageOutliers(2, 50.), pipeline.ImageBGSubtract(), pipeline.ImageNorm()])
    host = chain(np.array(frame))[..., 0]
    z, std, d = fc.oracle_chain(frame, outliers=(2, 50.), bgsubtract=True)
    assert np.abs(z - host).max() <= (1 + np.abs(z).max()) * d / std
    z, std, d = fc.oracle_chain(fc.frames(1)[0], outliers=(2, 50.))
    assert_bit_exact(z.astype(np.float32), G["chain_out_0"][..., 0], "chain_out_0")


LEGAL = [[], ["O"], ["B"], ["N"], ["O", "B"], ["O", "N"], ["B", "N"], ["O", "B", "N"]]


def _pipes(letters, sigma=3, threshold=40.):
    make = {"O": lambda: pipeline.ImageOutliers(sigma, threshold), "B": pipeline.ImageBGSubtract, "N": pipeline.ImageNorm,
            "F": pipeline.ImageFlip}
    return [make[c]() for c in letters]


@pytest.mark.parametrize("letters", LEGAL, ids=["".join(l) or "empty" for l in LEGAL])
def test_from_pipeline_accepts_every_legal_subsequence(letters, tmp_path):
    p = pipeline.ImagePipeline(_pipes(letters))
    want_clean = FrameClean((3, 40.) if "O" in letters else None, "B" in letters)
    for source in (p, None):
        if source is None:
            p.save(str(tmp_path / "pipe.json"))
            source = str(tmp_path / "pipe.json")
            assert [q.__class__.__name__ for q in pipeline.ImagePipeline.load(source).pipeline] == \
                [q.__class__.__name__ for q in p.pipeline]
        clean, normalise = FrameClean.from_pipeline(source)
        assert normalise == ("N" in letters)
        assert (clean == want_clean) if ("O" in letters or "B" in letters) else clean is None
        names = [list(q)[0] for q in (clean or FrameClean()).pipes(normalise)]
        assert names == [q.__class__.__name__ for q in p.pipeline]
    if "O" in letters:
        assert clean.outliers == (3, 40.) and clean.pipes()[0] == {"ImageOutliers": {"sigma": 3, "threshold": 40.}}


@pytest.mark.parametrize("letters,sigma,named", [(["O", "F", "N"], 2, "ImageFlip"), (["F"], 2, "ImageFlip"),
                                                 (["N", "B"], 2, "ImageBGSubtract"), (["B", "O"], 2, "ImageOutliers"),
                                                 (["N", "N"], 2, "ImageNorm"), (["O", "N"], 6, "ImageOutliers"),
                                                 (["O"], 1, "ImageOutliers"), (["O"], 2.5, "ImageOutliers")])
def test_from_pipeline_rejects_what_the_device_does_not_run(letters, sigma, named, tmp_path):
    p = pipeline.ImagePipeline(_pipes(letters, sigma=sigma))
    with pytest.raises(ValueError, match=named):
        FrameClean.from_pipeline(p)
    if letters != ["N", "N"]:                                   # a JSON object holds a name once: save() cannot write this one
        p.save(str(tmp_path / "bad.json"))
        with pytest.raises(ValueError, match=named):
            FrameClean.from_pipeline(str(tmp_path / "bad.json"))


def test_frame_clean_is_a_plain_value():
    assert FrameClean((2, 50), True) == FrameClean((2, 50.), True) and not FrameClean()
    assert FrameClean((2, 50.)) != FrameClean((3, 50.)) and hash(FrameClean((2, 50.))) == hash(FrameClean((2, 50.)))
    for bad in (1, 6, 2.5):
        with pytest.raises(ValueError, match="ImageOutliers"):
            FrameClean(outliers=(bad, 5.))
    with pytest.raises(TypeError):
        FrameClean.from_pipeline([pipeline.ImageNorm()])


def test_header_declares_frame_cleaning():
    src = open(os.path.join(ROOT, "include", "sequitr_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("sq_frame_outliers_f32", "sq_frame_bgfit_workspace", "sq_frame_bgfit_f64", "sq_frame_bg_stats_f64",
                 "sq_frames_to_tiles_bg"):
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert "pipeline.py:266-295" in src and "pipeline.py:360-4" in src
