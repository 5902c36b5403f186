"""CPU: the scipy restatement of the volume clean-up (tests/volume_cleanup_cases.py) against a pure-Python brute force on
small volumes, the consequences include/sequitr_hip.h ("Volume clean-up") states, VolumeCleanup's validation, the C-ABI's
argument checks (no launch happens) and the jobs' handling of ``volume_postprocess`` before any input is opened."""
import json
import os
import re

import numpy as np
import pytest

from sequitr_amd import _lib, jobs, volumeops
from tests import mask_cleanup_cases as mc
from tests import volume_cleanup_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small_volumes():
    """(mask (N, D, H, W) up to 4 x 5 x 6 a volume, C): densities 0.3 / 0.6 / 0.9, C = 2 and 3, unknown bytes"""
    out = [(vc.random_volume(s, 1, d, h, w, C, dens), C) for s, (d, h, w, C, dens) in enumerate(
        [(4, 5, 6, 2, 0.3), (4, 5, 6, 3, 0.6), (4, 5, 6, 2, 0.9), (3, 5, 6, 3, 0.9), (1, 5, 6, 2, 0.6), (4, 1, 6, 3, 0.6),
         (4, 5, 1, 2, 0.9), (2, 2, 2, 2, 0.6)])]
    m = vc.shell(4, 5, 6, 0, 0, 0, 4, 5, 6)
    m[0, 1, 2, 2] = 2
    m[0, 2, 3, 4] = 255
    out += [(m[:, :3], 3), (m, 3), (np.ones((1, 3, 4, 5), np.uint8), 2), (np.zeros((1, 2, 3, 4), np.uint8), 2)]
    return out


@pytest.mark.parametrize("op", vc.OPS)
@pytest.mark.parametrize("structure", vc.STRUCTURES)
def test_morph_restatement_is_the_iterated_elementary_step(op, structure):
    for mask, C in small_volumes():
        for r in (1, 2, 3):
            step = {"op": op, "iterations": r, "structure": structure}
            assert np.array_equal(vc.step_ref(mask, step, C), vc.brute(mask, step, C)), (mask.shape, C, r)


def test_component_restatements_are_the_flood_fill():
    for mask, C in small_volumes():
        for step in ({"op": "fill_holes"}, {"op": "fill_holes", "max_voxels": 1}, {"op": "fill_holes", "max_voxels": 3},
                     {"op": "fill_holes", "max_voxels": 20}, {"op": "clear_border"}, {"op": "clear_border", "faces": "lateral"}):
            assert np.array_equal(vc.step_ref(mask, step, C), vc.brute(mask, step, C)), (mask.shape, C, step)
    for name, mask, C, limits in vc.fill_cases():
        if mask.size <= 700:
            for a in limits:
                step = {"op": "fill_holes", "max_voxels": a}
                assert np.array_equal(vc.step_ref(mask, step, C), vc.brute(mask, step, C)), (name, a)
    for name, mask, C in vc.border_cases():
        if mask.size <= 1400:
            for faces in vc.FACES:
                step = {"op": "clear_border", "faces": faces}
                assert np.array_equal(vc.step_ref(mask, step, C), vc.brute(mask, step, C)), (name, faces)


def test_plane_structures_are_the_planar_restatement_slice_by_slice():
    for seed, C in ((1, 2), (2, 3)):
        mask = vc.random_volume(seed, 2, 4, 9, 11, C, 0.7)
        for op in ("erode", "open", "dilate", "close"):
            for r in (1, 2, 3):
                for st3, st2 in (("plane_cross", "cross"), ("plane_square", "square")):
                    want = mc.morph_ref(mask.reshape(8, 9, 11), op, r, st2, C).reshape(mask.shape)
                    assert np.array_equal(vc.morph_ref(mask, op, r, st3, C), want), (op, r, st3)
    m = dict((c[0], c) for c in vc.fill_cases())["open to the first plane"][1]
    assert np.array_equal(vc.fill_ref(m, None, 2, planar=True), mc.fill_holes_ref(m[0], None, 2)[None])


def test_stated_consequences():
    # iterated erosions (and dilations of one plane) compose: erode 2 twice is erode 4
    for seed, C, st in ((3, 2, "cross"), (4, 3, "cube"), (5, 2, "cube")):
        mask = vc.random_volume(seed, 1, 12, 13, 14, C, 0.97, unknown=False)
        for m in (mask, np.where(mask == 255, 0, 1).astype(np.uint8)):
            twice = vc.morph_ref(vc.morph_ref(m, "erode", 2, st, C), "erode", 2, st, C)
            assert np.array_equal(twice, vc.morph_ref(m, "erode", 4, st, C))
        assert twice.any()                                      # the solid volume keeps its core
    sparse = vc.random_volume(6, 1, 12, 13, 14, 2, 0.03, unknown=False)
    assert np.array_equal(vc.morph_ref(vc.morph_ref(sparse, "dilate", 2, "cross", 2), "dilate", 2, "cross", 2),
                          vc.morph_ref(sparse, "dilate", 4, "cross", 2))
    # D = 1: every voxel is on a face -- nothing is filled, and all faces remove everything
    one = np.stack([mc.object_in_ring()])
    assert one.shape[1] == 1 and np.array_equal(vc.fill_ref(one, None, 3), one)
    assert not vc.clear_border_ref(one, 3, "all").any()
    assert np.array_equal(vc.clear_border_ref(one, 3, "lateral")[0], mc.clear_border_ref(one[0], 3))
    assert not np.array_equal(vc.fill_ref(one, None, 3, planar=True), one)
    # a cavity open to the first plane is not filled; slice by slice it is
    cases = dict((c[0], c) for c in vc.fill_cases())
    m = cases["open to the first plane"][1]
    assert np.array_equal(vc.fill_ref(m, None, 2), m) and (vc.fill_ref(m, None, 2, planar=True) != m).any()
    assert np.array_equal(vc.fill_ref(cases["tunnel to a face"][1], None, 2), cases["tunnel to a face"][1])
    assert np.array_equal(vc.fill_ref(cases["pierced shell"][1], None, 2), cases["pierced shell"][1])
    # max_voxels counts the foreign voxel: 210 with it
    f = cases["foreign voxel inside"][1]
    full = vc.fill_ref(f, None, 3)
    assert full[0, 4, 5, 5] == 2 and int((full != f).sum()) == 209
    assert np.array_equal(vc.fill_ref(f, 209, 3), f) and np.array_equal(vc.fill_ref(f, 210, 3), full)
    # shells in shells go to the lowest class that encloses the voxel; the unknown byte stays
    s = cases["shells in shells"][1]
    g = vc.fill_ref(s, None, 3)
    assert np.all(g[0, 4:9, 4:10, 4:11][s[0, 4:9, 4:10, 4:11] == 0] == 1) and g[0, 6, 6, 6] == 7
    assert np.all(g[0, 2, 2:12, 2:13] == 2) and np.array_equal(g[s > 0], s[s > 0]) and not g[0, 0].any()
    # lateral keeps what touches only z-faces
    name, b, C = vc.border_cases()[0]
    lat, alls = vc.clear_border_ref(b, C, "lateral"), vc.clear_border_ref(b, C, "all")
    assert lat[0, 0, 3, 3] == 1 and lat[0, -1, 8, 4] == 2 and alls[0, 0, 3, 3] == 0 and alls[0, -1, 8, 4] == 0
    assert lat[0, 3, 0, 7] == 0 and lat[0, 5, 5, 0] == 0 and np.array_equal(alls[0, 3:5, 5:7, 5:8], b[0, 3:5, 5:7, 5:8])


def test_python_constants_are_the_headers():
    src = open(os.path.join(ROOT, "include", "sequitr_hip.h")).read()
    val = {k: int(v) for k, v in re.findall(r"#define (SQ_[A-Z0-9_]+) (\d+)", src)}
    assert volumeops.MORPH3D_TILE == (val["SQ_MORPH3D_TILE_D"], val["SQ_MORPH3D_TILE_H"], val["SQ_MORPH3D_TILE_W"])
    assert volumeops.MORPH3D_MAX_ITER == val["SQ_MORPH3D_MAX_ITER"] == 4
    assert volumeops.STRUCTURES3D == {"cross": val["SQ_MORPH3D_CROSS"], "cube": val["SQ_MORPH3D_CUBE"]}
    assert volumeops.FACES == {"all": val["SQ_FACES_ALL"], "lateral": val["SQ_FACES_LATERAL"]}


def test_volume_cleanup_validation():
    steps = [{"op": "open", "iterations": 2, "structure": "cube"}, {"op": "fill_holes", "max_voxels": 400, "planar": False},
             {"op": "clear_border", "faces": "lateral"}]
    vcl = volumeops.VolumeCleanup(steps)
    assert vcl.record() == steps and json.loads(json.dumps(vcl.record())) == steps
    assert volumeops.VolumeCleanup([{"op": "erode"}, {"op": "fill_holes"}, {"op": "clear_border"},
                                    {"op": "close", "structure": "plane_square", "iterations": 16}]).record() == [
        {"op": "erode", "iterations": 1, "structure": "cross"}, {"op": "fill_holes", "max_voxels": None, "planar": False},
        {"op": "clear_border", "faces": "all"}, {"op": "close", "iterations": 16, "structure": "plane_square"}]
    assert volumeops.VolumeCleanup(vcl).record() == steps
    for bad, match in (([{"op": "skeletonize"}], "unknown op 'skeletonize'"),
                       ([{"op": "split", "erosions": 3}], "a 3-D split is not built"),
                       ([{"op": "open", "radius": 2}], "unknown key\\(s\\) 'radius'"),
                       ([{"op": "clear_border", "iterations": 1}], "unknown key\\(s\\) 'iterations'"),
                       ([{"op": "fill_holes", "max_area": 3, "size": 3}], "'max_area', 'size'"),
                       ([{"op": "erode", "iterations": 0}], "iterations must be an integer 1 .. 4 for structure 'cross', got 0"),
                       ([{"op": "erode", "iterations": 5, "structure": "cube"}], "1 .. 4 for structure 'cube', got 5"),
                       ([{"op": "erode", "iterations": 17, "structure": "plane_cross"}], "1 .. 16 for structure 'plane_cross', got 17"),
                       ([{"op": "erode", "iterations": 2.0}], "got 2.0"),
                       ([{"op": "close", "structure": "square"}], "structure must be one of .* got 'square'"),
                       ([{"op": "fill_holes", "max_voxels": 0}], "max_voxels must be a positive integer or null, got 0"),
                       ([{"op": "fill_holes", "planar": 1}], "planar must be true or false, got 1"),
                       ([{"op": "clear_border", "faces": "top"}], "faces must be one of .* got 'top'"),
                       ([{"iterations": 2}], "must be a dict with an 'op'"),
                       (["open"], "must be a dict with an 'op'"),
                       ([], "non-empty list"), ({"op": "open"}, "non-empty list")):
        with pytest.raises(ValueError, match=match):
            volumeops.VolumeCleanup(bad)


def test_device_functions_refuse_host_and_planar_masks():
    import torch
    m = torch.zeros((1, 3, 4, 4), dtype=torch.uint8)
    for call in (lambda: volumeops.morph3d(m, "open"), lambda: volumeops.morph3d(m, "open", structure="plane_cross"),
                 lambda: volumeops.fill_cavities(m), lambda: volumeops.fill_cavities(m, planar=True),
                 lambda: volumeops.clear_border3d(m), lambda: volumeops.VolumeCleanup([{"op": "open"}]).apply(m, 2)):
        with pytest.raises(_lib.SequitrHipError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="one of"):
        volumeops.morph3d(m, "skeletonize")
    with pytest.raises(ValueError, match="1 .. 4"):
        volumeops.morph3d(m, "open", iterations=5)
    with pytest.raises(ValueError, match="1 .. 16"):
        volumeops.morph3d(m, "open", iterations=17, structure="plane_square")
    with pytest.raises(ValueError, match="structure must be one of"):
        volumeops.morph3d(m, "open", structure="square")
    with pytest.raises(ValueError, match="faces must be one of"):
        volumeops.clear_border3d(m, faces="top")


def test_entry_points_check_their_arguments_before_any_launch():
    lib = _lib.load()
    buf = np.zeros(4096 + 64, np.uint8)
    base = (buf.ctypes.data + 15) // 16 * 16                    # host memory will do: every call below is refused first
    a, b, ws = base, base + 1024, base + 2048
    E, D, CROSS, CUBE = 0, 1, 0, 1

    def refused(rc, word):
        assert rc == -1 and word.encode() in lib.sq_last_error(), (rc, lib.sq_last_error())

    refused(lib.sq_volume_morph_u8(None, b, 1, 4, 8, 8, 2, E, CROSS, 1, None), "null")
    refused(lib.sq_volume_morph_u8(a, None, 1, 4, 8, 8, 2, E, CROSS, 1, None), "null")
    refused(lib.sq_volume_morph_u8(a, b, 1, 4, 8, 8, 1, E, CROSS, 1, None), "C must be")
    refused(lib.sq_volume_morph_u8(a, b, 1, 4, 8, 8, 2, 4, CROSS, 1, None), "op must be")
    refused(lib.sq_volume_morph_u8(a, b, 1, 4, 8, 8, 2, D, 2, 1, None), "structure must be")
    refused(lib.sq_volume_morph_u8(a, b, 1, 4, 8, 8, 2, D, CUBE, 0, None), "iterations must be 1 .. 4")
    refused(lib.sq_volume_morph_u8(a, b, 1, 4, 8, 8, 2, D, CUBE, 5, None), "iterations must be 1 .. 4")
    refused(lib.sq_volume_morph_u8(a, b, 1, 0, 8, 8, 2, E, CROSS, 1, None), "2^31")
    refused(lib.sq_volume_morph_u8(a, b, 1, 4, 0, 8, 2, E, CROSS, 1, None), "2^31")
    refused(lib.sq_volume_morph_u8(a, b, 2, 64, 4096, 4096, 2, E, CROSS, 1, None), "2^31")
    refused(lib.sq_volume_morph_u8(a, b, 65536, 65536, 65536, 65536, 2, E, CROSS, 1, None), "2^31")
    refused(lib.sq_volume_morph_u8(a, a + 255, 1, 4, 8, 8, 2, E, CROSS, 1, None), "overlap")
    refused(lib.sq_volume_morph_u8(a, a, 1, 4, 8, 8, 2, E, CROSS, 1, None), "overlap")
    for fn, extra in ((lib.sq_volume_fill_holes_u8, (0,)), (lib.sq_volume_clear_border_u8, (0,))):
        refused(fn(None, b, 1, 4, 8, 8, 2, *extra, ws, None), "null")
        refused(fn(a, b, 1, 4, 8, 8, 2, *extra, None, None), "null")
        refused(fn(a, b, 1, 4, 8, 8, 1, *extra, ws, None), "C must be")
        refused(fn(a, b, 1, 0, 8, 8, 2, *extra, ws, None), "2^31")
        refused(fn(a, b, 2, 64, 4096, 4096, 2, *extra, ws, None), "2^31")
        refused(fn(a, b, 1, 4, 8, 8, 2, *extra, ws + 8, None), "16-byte aligned")
        refused(fn(a, a + 1, 1, 4, 8, 8, 2, *extra, ws, None), "overlap")
    refused(lib.sq_volume_clear_border_u8(a, b, 1, 4, 8, 8, 2, 2, ws, None), "faces must be")
    refused(lib.sq_volume_clear_border_u8(a, b, 1, 4, 8, 8, 2, -1, ws, None), "faces must be")
    assert not buf.any()                                        # `out` is untouched
    assert lib.sq_volume_fill_holes_workspace(3, 2, 5, 11) == (330 * 9 + 15) // 16 * 16
    assert lib.sq_volume_clear_border_workspace(3, 2, 5, 11) == 330 * 8
    assert lib.sq_volume_fill_holes_workspace(2, 64, 4096, 4096) == -1 and lib.sq_volume_clear_border_workspace(1, 0, 4, 4) == -1


class _Untouchable(np.ndarray):
    """an array whose voxels must not be touched: the jobs under test raise before they read one"""

    def __getitem__(self, key):
        raise AssertionError("the job read the input")


def test_jobs_refuse_a_bad_volume_postprocess_before_any_input_is_opened(tmp_path):
    vols = np.zeros((2, 4, 8, 8), np.uint16).view(_Untouchable)
    base = {"input": str(tmp_path / "missing.npy"), "labels": str(tmp_path / "missing_labels.npy"), "output": str(tmp_path)}
    path = str(tmp_path / "steps.json")
    json.dump([{"op": "fill_holes", "max_voxels": -3}], open(path, "w"))
    for run, more in ((jobs.SERVER_segment_volume, {}), (jobs.SERVER_segment_volume, {"brick": (8, 8, 4)}),
                      (jobs.SERVER_evaluate, {"brick": (8, 8, 4)})):
        for bad, match in (([{"op": "skeletonize"}], "unknown op 'skeletonize'"),
                           ([{"op": "split", "erosions": 2}], "3-D split is not built"),
                           ([{"op": "open", "radius": 2}], "unknown key"),
                           ([{"op": "open", "iterations": 5}], "iterations"),
                           ({"op": "open"}, "non-empty list"),
                           (path, "max_voxels")):
            with pytest.raises(ValueError, match=match):
                run(dict(base, volume_postprocess=bad, **more), {})     # the input does not even exist
            with pytest.raises(ValueError, match=match):
                run(dict(base, input=vols, labels=vols, volume_postprocess=bad, **more), {})
    assert os.listdir(str(tmp_path)) == ["steps.json"]


@pytest.mark.parametrize("job", ["evaluate", "segment_frames", "segment", "train", "train_volume", "train_gan"])
def test_jobs_refuse_the_key_where_it_does_not_apply(job, tmp_path):
    run = getattr(jobs, "SERVER_" + job)
    vols = np.zeros((2, 4, 8, 8), np.uint16).view(_Untouchable)
    good = [{"op": "open"}]
    base = {"output": str(tmp_path)}
    for key in ("input", "labels", "images", "weights", "training_data"):
        base[key] = str(tmp_path / ("missing_%s.npy" % key))
    with pytest.raises(ValueError, match="volume_postprocess"):
        run(dict(base, volume_postprocess=good), {})
    with pytest.raises(ValueError, match="volume_postprocess"):
        run(dict(base, volume_postprocess=good, **{k: vols for k in ("input", "labels", "images", "weights", "training_data")}), {})
    assert os.listdir(str(tmp_path)) == []
    # the planar key stays refused for volumes, with or without the new one
    for more in ({}, {"volume_postprocess": good}):
        with pytest.raises(ValueError, match="volumes"):
            jobs.SERVER_segment_volume(dict(base, postprocess=[{"op": "open"}], **more), {})
        with pytest.raises(ValueError, match="volumes"):
            jobs.SERVER_evaluate(dict(base, postprocess=[{"op": "open"}], brick=(8, 8, 4), **more), {})
