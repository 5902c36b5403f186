"""CPU: the scipy restatement of the mask clean-up (tests/mask_cleanup_cases.py) against a pure-Python brute force on small
frames, the merge-rule cases of include/sequitr_hip.h, MaskCleanup's validation, the C-ABI's argument checks (no launch
happens) and the jobs' rejection of a bad ``postprocess`` before any input is opened."""
import json
import os
import re

import numpy as np
import pytest

from sequitr_amd import _lib, jobs, maskops
from tests import mask_cleanup_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small_masks():
    out = [(mc.random_mask(s, 2, h, w, C, d), C) for s, (h, w, C, d) in enumerate(
        [(12, 13, 2, 0.3), (12, 13, 3, 0.5), (11, 12, 5, 0.9), (1, 9, 2, 0.6), (7, 1, 3, 0.7), (2, 2, 2, 0.5), (9, 12, 3, 0.8)])]
    out += [(mc.object_in_ring(), 3), (mc.nested_rings(), 3), (mc.unknown_bytes(), 3), (np.ones((1, 6, 7), np.uint8), 2),
            (np.zeros((1, 5, 4), np.uint8), 2)]
    return out


@pytest.mark.parametrize("op", mc.OPS)
@pytest.mark.parametrize("structure", mc.STRUCTURES)
def test_morph_restatement_is_the_iterated_3x3_step(op, structure):
    for mask, C in small_masks():
        for r in (1, 2, 3):
            step = {"op": op, "iterations": r, "structure": structure}
            assert np.array_equal(mc.step_ref(mask, step, C), mc.brute(mask, step, C)), (mask.shape, C, r)


def test_component_restatements_are_the_flood_fill():
    for mask, C in small_masks():
        for step in ({"op": "fill_holes"}, {"op": "fill_holes", "max_area": 1}, {"op": "fill_holes", "max_area": 3},
                     {"op": "fill_holes", "max_area": 20}, {"op": "clear_border"}):
            assert np.array_equal(mc.step_ref(mask, step, C), mc.brute(mask, step, C)), (mask.shape, C, step)
    for name, mask, C, areas in mc.fill_cases():
        if mask.size <= 12 * 13 * 2:
            for a in areas:
                step = {"op": "fill_holes", "max_area": a}
                assert np.array_equal(mc.step_ref(mask, step, C), mc.brute(mask, step, C)), (name, a)
    for name, mask, C in mc.border_cases():
        if mask.size <= 20 * 30:
            assert np.array_equal(mc.clear_border_ref(mask, C), mc.brute(mask, {"op": "clear_border"}, C)), name


def test_merge_rules():
    # a class-2 object inside a class-1 ring stays and the ring's background fills with 1
    m = mc.object_in_ring()
    f = mc.fill_holes_ref(m, None, 3)
    assert np.array_equal(f[0, 4:7, 5:8], np.full((3, 3), 2)) and np.all(f[0, 2:10, 2:11][m[0, 2:10, 2:11] == 0] == 1)
    assert np.array_equal(f == 0, (m == 0) & ~np.pad(np.ones((8, 9), bool), ((2, 2), (2, 2)))[None])
    # max_area counts the enclosed foreign pixels: the hole has 72 - 9 background pixels and area 72
    assert np.array_equal(mc.fill_holes_ref(m, 71, 3), m) and np.array_equal(mc.fill_holes_ref(m, 72, 3), f)
    assert np.array_equal(mc.fill_holes_ref(m, 63, 3), m)
    # nested rings go to the lowest class that encloses the pixel
    n = mc.nested_rings()
    g = mc.fill_holes_ref(n, None, 3)
    assert np.all(g[0, 4:8, 4:9] == 1) and np.all(g[0, 2, 2:11] == 2) and np.all(g[0, 2:10, 2] == 2)
    assert np.array_equal(g[n > 0], n[n > 0]) and np.all(g[0, 0] == 0)
    assert np.all(mc.fill_holes_ref(n, 20, 3)[0, 2, 2:11] == 0) and np.all(mc.fill_holes_ref(n, 20, 3)[0, 4:8, 4:9] == 1)
    # bytes >= C and 255 are kept by every step, are never written over, and open a wall they stand in
    u = mc.unknown_bytes()
    unknown = u >= 3
    for step in ([{"op": o, "iterations": r, "structure": s} for o in mc.OPS for r in (1, 3) for s in mc.STRUCTURES]
                 + [{"op": "fill_holes"}, {"op": "clear_border"}]):
        got = mc.step_ref(u, step, 3)
        assert np.array_equal(got[unknown], u[unknown]), step
        if step["op"] in ("dilate", "close", "fill_holes"):
            assert np.array_equal(got[u > 0], u[u > 0]), step      # a pixel that carries a class is never changed
        else:
            assert np.all((got == u) | (got == 0)), step
    h = mc.fill_holes_ref(u, None, 3)
    assert np.all(h[0, 3:9, 3:10][u[0, 3:9, 3:10] == 0] == 1) and np.array_equal(h[1], u[1])
    assert np.array_equal(mc.fill_holes_ref(u, 41, 3)[0], u[0]) and np.array_equal(mc.fill_holes_ref(u, 42, 3)[0], h[0])
    d = mc.morph_ref(u, "dilate", 1, "cross", 3)
    assert d[0, 5, 11] == 1 and d[0, 4, 12] == 2 and d[0, 5, 12] == 2   # both reach (5, 11): the lowest class wins, on background only
    c = mc.clear_border_ref(u, 3)
    assert c[0, 5, 12] == 0 and c[0, 0, 3] == 255 and c[0, 7, 0] == 3 and np.array_equal(c[0, 2:10, 2:11], u[0, 2:10, 2:11])


def test_python_constants_are_the_headers():
    src = open(os.path.join(ROOT, "include", "sequitr_hip.h")).read()
    val = {k: int(v) for k, v in re.findall(r"#define (SQ_MORPH_[A-Z_]+) (\d+)", src)}
    assert maskops.MORPH_TILE == (val["SQ_MORPH_TILE_ROWS"], val["SQ_MORPH_TILE_COLS"])
    assert maskops.MORPH_MAX_ITER == val["SQ_MORPH_MAX_ITER"] == 16
    assert maskops.MORPH_OPS == {"erode": val["SQ_MORPH_ERODE"], "dilate": val["SQ_MORPH_DILATE"], "open": val["SQ_MORPH_OPEN"],
                                 "close": val["SQ_MORPH_CLOSE"]}
    assert maskops.STRUCTURES == {"cross": val["SQ_MORPH_CROSS"], "square": val["SQ_MORPH_SQUARE"]}


def test_mask_cleanup_validation():
    steps = [{"op": "open", "iterations": 2, "structure": "cross"}, {"op": "fill_holes", "max_area": 400}, {"op": "clear_border"}]
    mcl = maskops.MaskCleanup(steps)
    assert mcl.record() == steps and json.loads(json.dumps(mcl.record())) == steps
    assert maskops.MaskCleanup([{"op": "erode"}, {"op": "fill_holes"}]).record() == [
        {"op": "erode", "iterations": 1, "structure": "cross"}, {"op": "fill_holes", "max_area": None}]
    assert maskops.MaskCleanup(mcl).record() == steps
    for bad, match in (([{"op": "skeletonize"}], "unknown op 'skeletonize'"),
                       ([{"op": "open", "radius": 2}], "unknown key\\(s\\) 'radius'"),
                       ([{"op": "clear_border", "iterations": 1}], "unknown key\\(s\\) 'iterations'"),
                       ([{"op": "fill_holes", "structure": "cross", "size": 3}], "'size', 'structure'"),
                       ([{"op": "erode", "iterations": 0}], "iterations must be an integer 1 .. 16, got 0"),
                       ([{"op": "erode", "iterations": 17}], "got 17"),
                       ([{"op": "erode", "iterations": 2.0}], "got 2.0"),
                       ([{"op": "close", "structure": "disk"}], "structure must be one of .* got 'disk'"),
                       ([{"op": "fill_holes", "max_area": 0}], "max_area must be a positive integer or null, got 0"),
                       ([{"iterations": 2}], "must be a dict with an 'op'"),
                       (["open"], "must be a dict with an 'op'"),
                       ([], "non-empty list"), ({"op": "open"}, "non-empty list")):
        with pytest.raises(ValueError, match=match):
            maskops.MaskCleanup(bad)


def test_device_functions_refuse_host_masks():
    import torch
    m = torch.zeros((1, 4, 4), dtype=torch.uint8)
    for call in (lambda: maskops.morph(m, "open"), lambda: maskops.fill_holes(m), lambda: maskops.clear_border(m),
                 lambda: maskops.MaskCleanup([{"op": "open"}]).apply(m, 2)):
        with pytest.raises(_lib.SequitrHipError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="one of"):
        maskops.morph(m, "skeletonize")
    with pytest.raises(ValueError, match="1 .. 16"):
        maskops.morph(m, "open", iterations=17)


def test_entry_points_check_their_arguments_before_any_launch():
    lib = _lib.load()
    buf = np.zeros(4096 + 64, np.uint8)
    base = (buf.ctypes.data + 15) // 16 * 16                    # host memory will do: every call below is refused first
    a, b, ws = base, base + 1024, base + 2048
    E, D, CROSS, SQUARE = 0, 1, 0, 1

    def refused(rc, word):
        assert rc == -1 and word.encode() in lib.sq_last_error(), (rc, lib.sq_last_error())

    refused(lib.sq_mask_morph_u8(None, b, 1, 8, 8, 2, E, CROSS, 1, None), "null")
    refused(lib.sq_mask_morph_u8(a, None, 1, 8, 8, 2, E, CROSS, 1, None), "null")
    refused(lib.sq_mask_morph_u8(a, b, 1, 8, 8, 1, E, CROSS, 1, None), "C must be")
    refused(lib.sq_mask_morph_u8(a, b, 1, 8, 8, 2, 4, CROSS, 1, None), "op must be")
    refused(lib.sq_mask_morph_u8(a, b, 1, 8, 8, 2, D, 2, 1, None), "structure must be")
    refused(lib.sq_mask_morph_u8(a, b, 1, 8, 8, 2, D, SQUARE, 0, None), "iterations must be 1 .. 16")
    refused(lib.sq_mask_morph_u8(a, b, 1, 8, 8, 2, D, SQUARE, 17, None), "iterations must be 1 .. 16")
    refused(lib.sq_mask_morph_u8(a, b, 1, 0, 8, 2, E, CROSS, 1, None), "2^31")
    refused(lib.sq_mask_morph_u8(a, b, 2, 32768, 32768, 2, E, CROSS, 1, None), "2^31")
    refused(lib.sq_mask_morph_u8(a, a + 63, 1, 8, 8, 2, E, CROSS, 1, None), "overlap")
    refused(lib.sq_mask_morph_u8(a, a, 1, 8, 8, 2, E, CROSS, 1, None), "overlap")
    for fn, extra in ((lib.sq_mask_fill_holes_u8, (0,)), (lib.sq_mask_clear_border_u8, ())):
        refused(fn(None, b, 1, 8, 8, 2, *extra, ws, None), "null")
        refused(fn(a, b, 1, 8, 8, 2, *extra, None, None), "null")
        refused(fn(a, b, 1, 8, 8, 1, *extra, ws, None), "C must be")
        refused(fn(a, b, 2, 32768, 32768, 2, *extra, ws, None), "2^31")
        refused(fn(a, b, 1, 8, 8, 2, *extra, ws + 8, None), "16-byte aligned")
        refused(fn(a, a + 1, 1, 8, 8, 2, *extra, ws, None), "overlap")
    assert lib.sq_mask_fill_holes_workspace(3, 10, 11) == (330 * 9 + 15) // 16 * 16
    assert lib.sq_mask_clear_border_workspace(3, 10, 11) == 330 * 8
    assert lib.sq_mask_fill_holes_workspace(2, 32768, 32768) == -1 and lib.sq_mask_clear_border_workspace(0, 4, 4) == -1


class _Untouchable(np.ndarray):
    """an array whose pixels must not be touched: the jobs under test raise before they read one"""

    def __getitem__(self, key):
        raise AssertionError("the job read the input")


@pytest.mark.parametrize("job", ["segment_frames", "evaluate"])
def test_jobs_refuse_a_bad_postprocess_before_any_input_is_opened(job, tmp_path):
    run = getattr(jobs, "SERVER_" + job)
    frames = np.zeros((2, 8, 8), np.uint16).view(_Untouchable)
    base = {"input": str(tmp_path / "missing.npy"), "labels": str(tmp_path / "missing_labels.npy"), "output": str(tmp_path)}
    for bad, match in (([{"op": "skeletonize"}], "unknown op 'skeletonize'"),
                       ([{"op": "open", "radius": 2}], "unknown key"),
                       ([{"op": "open", "iterations": 99}], "iterations"),
                       ({"op": "open"}, "non-empty list")):
        with pytest.raises(ValueError, match=match):
            run(dict(base, postprocess=bad), {})                # the input does not even exist
        with pytest.raises(ValueError, match=match):
            run(dict(base, input=frames, labels=frames, postprocess=bad), {})
    path = str(tmp_path / "steps.json")
    json.dump([{"op": "fill_holes", "max_area": -3}], open(path, "w"))
    with pytest.raises(ValueError, match="max_area"):
        run(dict(base, postprocess=path), {})
    with pytest.raises(ValueError, match="volumes"):
        run(dict(base, postprocess=[{"op": "open"}], brick=(16, 16, 8)), {})
    with pytest.raises(ValueError, match="volumes"):
        jobs.SERVER_segment_volume(dict(base, postprocess=[{"op": "open"}]), {})
    assert os.listdir(str(tmp_path)) == ["steps.json"]
