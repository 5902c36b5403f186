"""CPU: the scipy restatement of the splitting step (tests/mask_split_cases.py) against a pure-Python version on small
frames, the consequences include/sequitr_hip.h states, that every GPU case does what it is there for, MaskCleanup's
validation of the ``split`` step, the C-ABI's argument checks (no launch happens) and the jobs' rejection of a bad
``split`` step before any input is opened."""
import json
import os
import re

import numpy as np
import pytest
from scipy import ndimage

from sequitr_amd import _lib, jobs, maskops
from tests import mask_cleanup_cases as mc
from tests import mask_split_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = maskops.SPLIT_TILE


def small_masks():
    out = [(mc.random_mask(s, 2, h, w, C, d), C) for s, (h, w, C, d) in enumerate(
        [(12, 13, 2, 0.8), (12, 13, 3, 0.9), (11, 12, 5, 0.95), (1, 9, 2, 0.9), (7, 1, 3, 0.9), (2, 2, 2, 0.9), (9, 12, 2, 0.97)])]
    m = np.zeros((1, 12, 13), np.uint8)
    m[0, 1:6, 1:6] = m[0, 6:11, 7:12] = m[0, 3, 6:10] = m[0, 3:8, 9] = 1       # two blocks joined by a bent corridor
    m[0, 7:12, 0:5] = 2
    m[0, 9, 5:7] = 2                                            # class 2 touches class 1's second block
    out += [(m, 3), (np.ones((1, 6, 7), np.uint8), 2), (np.zeros((1, 5, 4), np.uint8), 2), (mc.unknown_bytes(), 3)]
    return out


def test_restatement_is_the_headers_text_in_plain_python():
    changed = 0
    for mask, C in small_masks():
        for r, st, reach in ((1, "cross", None), (1, "square", 1), (1, "cross", 3), (2, "cross", None), (2, "square", 64),
                             (1, "cross", 64)):
            want = sc.brute_split(mask, r, st, reach, C)
            assert np.array_equal(sc.split_ref(mask, r, st, reach, C), want), (mask.shape, C, r, st, reach)
            changed += int((want != mask).sum())
    assert changed > 20                                         # the small frames do get cut


def all_cases():
    cases = sc.splitting_cases(TILE) + sc.unchanged_cases(TILE)
    cases += [("random %dx%dx%d" % s, mc.random_mask(s[1] * 1000 + s[2], *s, 3, 0.95), 3, 1, "cross", None) for s in sc.split_shapes(TILE)[:8]]
    return cases


def test_stated_consequences_hold_on_every_case():
    for name, mask, C, r, st, reach in all_cases():
        T = 2 * r if reach is None else reach
        out = sc.split_ref(mask, r, st, reach, C)
        assert np.all((out == mask) | (out == 0)), name         # anti-extensive
        assert np.array_equal(out[mask >= C], mask[mask >= C]), name
        for f in range(mask.shape[0]):
            for c in range(1, C):
                P = mask[f] == c
                S, L0, L = sc.plane_labels(P, r, st, T)
                kept = np.where(out[f] == c, L, 0)
                # two surviving pixels with different non-zero labels are never 4-adjacent
                for a, b in ((kept[:-1], kept[1:]), (kept[:, :-1], kept[:, 1:])):
                    assert not np.any((a > 0) & (b > 0) & (a != b)), name
                comp, n = ndimage.label(P)
                seeds = [len(set(L0[(comp == k) & S].tolist())) for k in range(1, n + 1)]
                for k in range(1, n + 1):
                    if seeds[k - 1] <= 1:                       # no seed, or one: the component is unchanged
                        assert np.all(out[f][comp == k] == c), (name, k)
                assert np.all(out[f][P & (L == 0)] == c), name   # what T steps do not reach keeps its class
        if sc.most_seeds_in_a_component(mask, r, st, C) <= 1:
            assert np.array_equal(out, mask), name


def test_every_gpu_case_does_what_it_is_there_for():
    for name, mask, C, r, st, reach in sc.splitting_cases(TILE):
        out = sc.split_ref(mask, r, st, reach, C)
        assert sc.most_seeds_in_a_component(mask, r, st, C) >= 2, name
        assert (out != mask).sum() >= 1, name
        assert sc.count_objects(out, C) > sc.count_objects(mask, C), name
    for name, mask, C, r, st, reach in sc.unchanged_cases(TILE):
        assert np.array_equal(sc.split_ref(mask, r, st, reach, C), mask), name
    for r in (4, 8):
        for st in sc.STRUCTURES:
            m = sc.seam_pairs(TILE, r)
            assert sc.count_objects(m, 2) == sc.SEAM_OBJECTS and sc.count_objects(sc.split_ref(m, r, st, None, 2), 2) == sc.SEAM_DISKS
    # the issue's figures: two disks of radius 12, 18 .. 22 apart, become two objects at r = 8; a square r = 10 leaves no seed
    for d in (18, 20, 22):
        m = np.zeros((1, 40, 60), np.uint8)
        sc.chain(m[0], 20, 30, 12, d)
        out = sc.split_ref(m, 8, "cross", None, 2)
        assert sc.count_objects(m, 2) == 1 and sc.count_objects(out, 2) == 2 and 5 <= int((out != m).sum()) <= 20, d
        assert np.array_equal(sc.split_ref(m, 8, "cross", 64, 2), out)           # reach beyond 2 r makes no difference here
        assert np.array_equal(sc.split_ref(m, 10, "square", None, 2), m)
    # the gaps: a corridor of length g is cut iff the two growths meet within T steps, in its middle
    K = maskops.SPLIT_STEPS
    g = sc.gaps(TILE)
    cut = [int((sc.split_ref(g, 1, "cross", T, 2) != g).sum()) for T in (1, K - 1, K, K + 1, 2 * K + 3, 64)]
    assert cut == sorted(cut) and len(set(cut)) == len(cut), cut  # every reach the GPU test runs cuts more corridors
    # the elbows need more than 2 K + 3 steps, the stacked frames' blobs at the frame edge stay whole
    e = sc.elbows(TILE)
    assert np.array_equal(sc.split_ref(e, 1, "square", 2 * K + 3, 2), e) and (sc.split_ref(e, 1, "square", 64, 2) != e).sum() == 2
    s = sc.frames_stacked()
    out = sc.split_ref(s, 2, "cross", None, 2)
    assert np.array_equal(out[:, 14:20, 3:12], s[:, 14:20, 3:12]) and np.array_equal(out[:, 0:6, 3:12], s[:, 0:6, 3:12])
    # classes in contact: one cut inside each class, none along the line where they touch
    c = sc.contact()
    out = sc.split_ref(c, 3, "square", 12, 3)
    assert np.array_equal(out[0, :, 28:32], c[0, :, 28:32]) and (out != c)[0, :, :30].any() and (out != c)[0, :, 30:].any()
    # the wall of unknown bytes: the bar it cuts through is unchanged, the whole bar beside it is cut
    u = sc.unknown_wall()
    out = sc.split_ref(u, 2, "cross", 16, 3)
    assert np.array_equal(out[0, :15], u[0, :15]) and (out != u)[0, 15:].any()


def test_python_constants_are_the_headers():
    src = open(os.path.join(ROOT, "include", "sequitr_hip.h")).read()
    val = {k: int(v) for k, v in re.findall(r"#define (SQ_SPLIT_[A-Z_]+) (\d+)", src)}
    assert maskops.SPLIT_TILE == (val["SQ_SPLIT_TILE_ROWS"], val["SQ_SPLIT_TILE_COLS"])
    assert maskops.SPLIT_STEPS == val["SQ_SPLIT_STEPS"] and maskops.SPLIT_MAX_REACH == val["SQ_SPLIT_MAX_REACH"] == 64
    assert "Mask clean-up: splitting" in src


def test_mask_cleanup_validation_of_split():
    steps = [{"op": "open", "iterations": 2, "structure": "cross"}, {"op": "split", "erosions": 8, "structure": "square", "reach": 12},
             {"op": "clear_border"}]
    mcl = maskops.MaskCleanup(steps)
    assert mcl.record() == steps and json.loads(json.dumps(mcl.record())) == steps
    assert maskops.MaskCleanup([{"op": "split", "erosions": 4}]).record() == [
        {"op": "split", "erosions": 4, "structure": "cross", "reach": None}]          # None stays None
    assert maskops.MaskCleanup(mcl).record() == steps
    for bad, match in (([{"op": "split"}], "step 0 \\(split\\): erosions must be an integer 1 .. 16, got None"),
                       ([{"op": "open"}, {"op": "split", "erosions": 0}], "step 1 \\(split\\): erosions .* got 0"),
                       ([{"op": "split", "erosions": 17}], "got 17"),
                       ([{"op": "split", "erosions": True}], "got True"),
                       ([{"op": "split", "erosions": 2.0}], "got 2.0"),
                       ([{"op": "split", "erosions": 2, "structure": "disk"}], "structure must be one of .* got 'disk'"),
                       ([{"op": "split", "erosions": 2, "reach": 0}], "reach must be an integer 1 .. 64 or null, got 0"),
                       ([{"op": "split", "erosions": 2, "reach": 65}], "got 65"),
                       ([{"op": "split", "erosions": 2, "reach": False}], "got False"),
                       ([{"op": "split", "erosions": 2, "reach": 4.0}], "got 4.0"),
                       ([{"op": "split", "erosions": 2, "iterations": 2}], "unknown key\\(s\\) 'iterations'")):
        with pytest.raises(ValueError, match=match):
            maskops.MaskCleanup(bad)


def test_split_refuses_host_masks_and_bad_arguments():
    import torch
    m = torch.zeros((1, 4, 4), dtype=torch.uint8)
    for call in (lambda: maskops.split(m, 2), lambda: maskops.MaskCleanup([{"op": "split", "erosions": 2}]).apply(m, 2)):
        with pytest.raises(_lib.SequitrHipError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="one of"):
        maskops.split(m, 2, "disk")
    with pytest.raises(ValueError, match="erosions must be 1 .. 16"):
        maskops.split(m, 17)
    with pytest.raises(ValueError, match="reach must be 1 .. 64"):
        maskops.split(m, 2, reach=65)


def test_entry_point_checks_its_arguments_before_any_launch():
    lib = _lib.load()
    buf = np.zeros(8192 + 64, np.uint8)
    base = (buf.ctypes.data + 15) // 16 * 16                    # host memory will do: every call below is refused first
    a, b, ws = base, base + 1024, base + 2048
    CROSS = 0

    def refused(rc, word):
        assert rc == -1 and word.encode() in lib.sq_last_error(), (rc, lib.sq_last_error())

    fn = lib.sq_mask_split_u8
    refused(fn(None, b, 1, 8, 8, 2, 1, CROSS, 2, ws, None), "null")
    refused(fn(a, None, 1, 8, 8, 2, 1, CROSS, 2, ws, None), "null")
    refused(fn(a, b, 1, 8, 8, 2, 1, CROSS, 2, None, None), "null")
    refused(fn(a, b, 1, 8, 8, 1, 1, CROSS, 2, ws, None), "C must be")
    refused(fn(a, b, 1, 8, 8, 257, 1, CROSS, 2, ws, None), "C must be")
    refused(fn(a, b, 1, 8, 8, 2, 1, 2, 2, ws, None), "structure must be")
    refused(fn(a, b, 1, 8, 8, 2, 0, CROSS, 2, ws, None), "erosions must be 1 .. 16")
    refused(fn(a, b, 1, 8, 8, 2, 17, CROSS, 2, ws, None), "erosions must be 1 .. 16")
    refused(fn(a, b, 1, 8, 8, 2, 1, CROSS, 0, ws, None), "reach must be 1 .. 64")
    refused(fn(a, b, 1, 8, 8, 2, 1, CROSS, 65, ws, None), "reach must be 1 .. 64")
    refused(fn(a, b, 1, 0, 8, 2, 1, CROSS, 2, ws, None), "2^31")
    refused(fn(a, b, 0, 8, 8, 2, 1, CROSS, 2, ws, None), "2^31")
    refused(fn(a, b, 2, 32768, 32768, 2, 1, CROSS, 2, ws, None), "2^31")
    refused(fn(a, b, 1, 8, 8, 2, 1, CROSS, 2, ws + 8, None), "16-byte aligned")
    refused(fn(a, a + 63, 1, 8, 8, 2, 1, CROSS, 2, ws, None), "out must not overlap mask")
    refused(fn(a, a, 1, 8, 8, 2, 1, CROSS, 2, ws, None), "out must not overlap mask")
    refused(fn(a, b, 1, 8, 8, 2, 1, CROSS, 2, a + 48, None), "workspace must not overlap")
    refused(fn(a, b, 1, 8, 8, 2, 1, CROSS, 2, b - 512, None), "workspace must not overlap")
    # the workspace: two int32 label planes and the seed bytes, 9 B per pixel, rounded up to 16
    assert lib.sq_mask_split_workspace(3, 10, 11) == (330 * 9 + 15) // 16 * 16
    assert lib.sq_mask_split_workspace(1, 1, 1) == 16 and lib.sq_mask_split_workspace(8, 2048, 2048) == 8 * 2048 * 2048 * 9
    assert lib.sq_mask_split_workspace(2, 32768, 32768) == -1 and lib.sq_mask_split_workspace(0, 4, 4) == -1
    assert lib.sq_mask_split_workspace(1, 4, -1) == -1


class _Untouchable(np.ndarray):
    """an array whose pixels must not be touched: the jobs under test raise before they read one"""

    def __getitem__(self, key):
        raise AssertionError("the job read the input")


@pytest.mark.parametrize("job", ["segment_frames", "evaluate"])
def test_jobs_refuse_a_bad_split_step_before_any_input_is_opened(job, tmp_path):
    run = getattr(jobs, "SERVER_" + job)
    frames = np.zeros((2, 8, 8), np.uint16).view(_Untouchable)
    base = {"input": str(tmp_path / "missing.npy"), "labels": str(tmp_path / "missing_labels.npy"), "output": str(tmp_path)}
    for bad, match in (([{"op": "split"}], "erosions"),
                       ([{"op": "split", "erosions": 99}], "erosions must be an integer 1 .. 16, got 99"),
                       ([{"op": "open"}, {"op": "split", "erosions": 4, "reach": 100}], "step 1 \\(split\\): reach"),
                       ([{"op": "split", "erosions": 4, "radius": 2}], "unknown key")):
        with pytest.raises(ValueError, match=match):
            run(dict(base, postprocess=bad), {})                # the input does not even exist
        with pytest.raises(ValueError, match=match):
            run(dict(base, input=frames, labels=frames, postprocess=bad), {})
    path = str(tmp_path / "steps.json")
    json.dump([{"op": "split", "erosions": 4, "structure": "ring"}], open(path, "w"))
    with pytest.raises(ValueError, match="structure"):
        run(dict(base, postprocess=path), {})
    with pytest.raises(ValueError, match="volumes"):
        run(dict(base, postprocess=[{"op": "split", "erosions": 4}], brick=(16, 16, 8)), {})
    with pytest.raises(ValueError, match="volumes"):
        jobs.SERVER_segment_volume(dict(base, postprocess=[{"op": "split", "erosions": 4}]), {})
    assert os.listdir(str(tmp_path)) == ["steps.json"]
