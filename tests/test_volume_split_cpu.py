"""CPU: the scipy restatement of the 3-D splitting step (tests/volume_split_cases.py) against a pure-Python version on
small volumes, the consequences include/sequitr_hip.h states, that every GPU case does what it is there for,
VolumeCleanup's validation of the ``split3d`` step, the C-ABI's argument checks (no launch happens) and the volume jobs'
rejection of a bad ``split3d`` step before any input is opened."""
import json
import os
import re

import numpy as np
import pytest
from scipy import ndimage

from sequitr_amd import _lib, jobs, volumeops
from tests import volume_cleanup_cases as vc
from tests import volume_split_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = volumeops.SPLIT3D_TILE
K = volumeops.SPLIT3D_STEPS


def small_volumes():
    out = [(vc.random_volume(s, n, d, h, w, C, dens), C) for s, (n, d, h, w, C, dens) in enumerate(
        [(2, 6, 7, 9, 2, 0.8), (1, 6, 7, 9, 3, 0.9), (1, 5, 7, 8, 3, 0.95), (1, 6, 6, 9, 2, 0.97), (1, 1, 7, 9, 2, 0.9),
         (1, 6, 1, 9, 3, 0.9), (2, 5, 6, 1, 2, 0.9), (1, 2, 2, 2, 2, 0.9)])]
    m = np.zeros((1, 6, 7, 9), np.uint8)
    m[0, 0:3, 0:3, 0:3] = m[0, 3:6, 4:7, 5:8] = 1               # two blocks joined by a bent corridor
    m[0, 1, 1, 3:7] = m[0, 1, 1:5, 6] = m[0, 1:4, 5, 6] = 1
    m[0, 3:6, 0:3, 0:3] = 2
    m[0, 4, 3:5, 1] = 2
    out += [(m, 3), (np.ones((1, 5, 6, 7), np.uint8), 2), (np.zeros((1, 3, 5, 4), np.uint8), 2),
            (np.full((1, 3, 4, 5), 7, np.uint8), 3)]
    return out


def test_restatement_is_the_headers_text_in_plain_python():
    changed = 0
    settings = [(1, st, reach) for st in sc.STRUCTURES for reach in (None, 1, 6)]
    settings += [(2, "cross", None), (2, "plane_cross", 3), (2, "cube", 5), (2, "plane_square", 4), (1, "cross", 2), (1, "cube", 4),
                 (1, "plane_cross", 5)]
    for mask, C in small_volumes():
        for r, st, reach in settings:
            want = sc.brute_split3d(mask, r, st, reach, C)
            assert np.array_equal(sc.split3d_ref(mask, r, st, reach, C), want), (mask.shape, C, r, st, reach)
            changed += int((want != mask).sum())
    assert changed > 20                                         # the small volumes do get cut


def all_cases():
    cases = sc.splitting_cases(TILE) + sc.unchanged_cases(TILE)
    cases += [(name, mask, C, r, st, None) for name, mask, C, r, st in sc.erosion_chain_cases()]
    cases += [("random %dx%dx%dx%d" % s, vc.random_volume(s[2] * 1000 + s[3], *s, 3, 0.95), 3, 1, "cross", None)
              for s in sc.split_shapes(TILE)[::4]]
    return cases


def test_stated_consequences_hold_on_every_case():
    for name, mask, C, r, st, reach in all_cases():
        T = sc.default_reach(r, st) if reach is None else reach
        out = sc.split3d_ref(mask, r, st, reach, C)
        assert np.all((out == mask) | (out == 0)), name         # anti-extensive
        assert np.array_equal(out[mask >= C], mask[mask >= C]), name
        for v in range(mask.shape[0]):
            for c in range(1, C):
                P = mask[v] == c
                S, L0, L = sc.volume_labels(P, r, st, T)
                kept = np.where(out[v] == c, L, 0)
                # two surviving voxels with different non-zero labels are never 6-adjacent
                for a, b in ((kept[:-1], kept[1:]), (kept[:, :-1], kept[:, 1:]), (kept[:, :, :-1], kept[:, :, 1:])):
                    assert not np.any((a > 0) & (b > 0) & (a != b)), name
                comp, n = ndimage.label(P)
                seeds = np.zeros(n + 1, np.int64)
                for k, _l in set(zip(comp[S].tolist(), L0[S].tolist())):
                    seeds[k] += 1
                assert np.all(out[v][P & (seeds[comp] <= 1)] == c), name     # no seed, or one: the component is unchanged
                assert np.all(out[v][P & (L == 0)] == c), name   # what T steps do not reach keeps its class
        if sc.most_seeds_in_a_component(mask, r, st, C) <= 1:
            assert np.array_equal(out, mask), name


def test_every_gpu_case_does_what_it_is_there_for():
    for name, mask, C, r, st, reach in sc.splitting_cases(TILE):
        out = sc.split3d_ref(mask, r, st, reach, C)
        assert sc.most_seeds_in_a_component(mask, r, st, C) >= 2, name
        assert (out != mask).sum() >= 1, name
        assert sc.count_objects(out, C) > sc.count_objects(mask, C), name
    for name, mask, C, r, st, reach in sc.unchanged_cases(TILE):
        assert np.array_equal(sc.split3d_ref(mask, r, st, reach, C), mask), name
    for name, mask, C, r, st in sc.erosion_chain_cases():
        out = sc.split3d_ref(mask, r, st, None, C)
        assert sc.count_objects(mask, C) == 1 and sc.count_objects(out, C) == 2 and (out != mask).sum() == 1, name
    # every seam pair becomes two objects
    for st in sc.STRUCTURES:
        m = sc.seam_pairs(TILE)
        out = sc.split3d_ref(m, 4, st, 12 if st == "cube" else 8, 2)
        assert m.shape[0] == sc.SEAM_VOLUMES and sc.count_objects(m, 2) == 12 and sc.count_objects(out, 2) == 24, st
    assert sc.count_objects(sc.split3d_ref(sc.chain_of_three(TILE), 4, "cross", None, 2), 2) == 3
    # the checked figures: two balls of radius 8, centres 14 apart, r = 4, on each of the three axes
    for axis in range(3):
        m = sc.pair((30, 30, 30) if axis else (34, 24, 24), (15, 15, 15) if axis else (17, 12, 12), axis, 4)[None]
        for st in ("cross", "plane_cross", "plane_square"):
            out = sc.split3d_ref(m, 4, st, 8, 2)
            assert sc.count_objects(out, 2) == 2 and int((out != m).sum()) == 45, (axis, st)
            assert np.array_equal(sc.split3d_ref(m, 4, st, None, 2), out)            # the default reach is 2 r
        out = sc.split3d_ref(m, 4, "cube", 8, 2)
        assert sc.count_objects(out, 2) == 1 and int((out != m).sum()) == 13, axis  # a bridge remains
        out = sc.split3d_ref(m, 4, "cube", 12, 2)
        assert sc.count_objects(out, 2) == 2 and int((out != m).sum()) == 45, axis
        assert np.array_equal(sc.split3d_ref(m, 4, "cube", None, 2), out)            # the default reach is 3 r
    m = sc.pair((20, 20, 30), (10, 10, 15), 2, 3)[None]         # radius 6, distance 10, r = 3, cube: split at 9, not at 6
    assert sc.count_objects(sc.split3d_ref(m, 3, "cube", 6, 2), 2) == 1 and sc.count_objects(sc.split3d_ref(m, 3, "cube", 9, 2), 2) == 2
    # the gaps: a corridor of length g is cut iff the two growths meet within T steps
    for axis in range(3):
        g = sc.gaps(TILE, axis)
        cut = [int((sc.split3d_ref(g, 1, "cross", T, 2) != g).sum()) for T in sorted({1, K - 1, K, K + 1, 2 * K + 3, 64})]
        assert cut == sorted(cut) and len(set(cut)) == len(cut), (axis, cut)        # every reach the GPU test runs cuts more
    # the elbows need more than 2 K + 3 steps
    e = sc.elbows(TILE)
    assert np.array_equal(sc.split3d_ref(e, 1, "cube", 2 * K + 3, 2), e) and (sc.split3d_ref(e, 1, "cube", 64, 2) != e).sum() == 2
    # nothing leaks between slices, rows or volumes: the blobs at the seams of the linear order stay whole
    s = sc.slices_stacked()
    out = sc.split3d_ref(s, 1, "cross", None, 2)
    assert np.array_equal(out[0, :10, :, :22], s[0, :10, :, :22]) and (out != s).sum() == 1
    s = sc.row_ends()
    out = sc.split3d_ref(s, 1, "plane_square", None, 2)
    assert np.array_equal(out[0, :, :10], s[0, :, :10]) and (out != s).sum() == 1
    s = sc.volumes_stacked()
    out = sc.split3d_ref(s, 1, "cube", None, 2)
    assert np.array_equal(out[..., :14], s[..., :14]) and (out != s).sum() == 3
    # classes in contact: a cut inside each class, none along the plane where they touch
    c = sc.contact()
    out = sc.split3d_ref(c, 2, "cube", None, 3)
    assert np.array_equal(out[0, :, :12], c[0, :, :12]) and (out != c)[0, :, :, :12].any() and (out != c)[0, :, :, 12:].any()
    # the wall of unknown bytes: the bar it cuts through is unchanged, the whole bar beside it is cut
    u = sc.unknown_wall()
    out = sc.split3d_ref(u, 2, "cross", 16, 3)
    assert np.array_equal(out[0, :, :11], u[0, :, :11]) and (out != u)[0, :, 11:].any()


def test_python_constants_are_the_headers():
    src = open(os.path.join(ROOT, "include", "sequitr_hip.h")).read()
    val = {k: int(v) for k, v in re.findall(r"#define (SQ_[A-Z0-9_]+) (\d+)", src)}
    assert volumeops.SPLIT3D_TILE == (val["SQ_SPLIT3D_TILE_D"], val["SQ_SPLIT3D_TILE_H"], val["SQ_SPLIT3D_TILE_W"])
    assert volumeops.SPLIT3D_STEPS == val["SQ_SPLIT3D_STEPS"]
    assert volumeops.SPLIT3D_LDS_DEFAULT == val["SQ_SPLIT3D_LDS_DEFAULT"] in (0, 1)
    assert volumeops.SPLIT3D_MAX_REACH == val["SQ_SPLIT3D_MAX_REACH"] == 64
    assert volumeops.SPLIT3D_MAX_EROSIONS == val["SQ_SPLIT3D_MAX_EROSIONS"] == 16
    assert volumeops.SPLIT3D_STRUCTURES == {"cross": val["SQ_MORPH3D_CROSS"], "cube": val["SQ_MORPH3D_CUBE"],
                                            "plane_cross": val["SQ_SPLIT3D_PLANE_CROSS"],
                                            "plane_square": val["SQ_SPLIT3D_PLANE_SQUARE"]}
    assert volumeops.SPLIT3D_STRUCTURES == {"cross": 0, "cube": 1, "plane_cross": 2, "plane_square": 3}
    assert tuple(sorted(volumeops.SPLIT3D_STRUCTURES, key=volumeops.SPLIT3D_STRUCTURES.get)) == sc.STRUCTURES
    assert "Volume clean-up: splitting" in src and "Not built: a 3-D split" not in src
    for r in (1, 4, 16):
        for st in sc.STRUCTURES:
            assert volumeops.default_reach3d(r, st) == sc.default_reach(r, st) == (3 * r if st == "cube" else 2 * r)


def test_volume_cleanup_validation_of_split3d():
    steps = [{"op": "open", "iterations": 2, "structure": "cross"},
             {"op": "split3d", "erosions": 8, "structure": "plane_square", "reach": 12}, {"op": "clear_border", "faces": "all"}]
    vcl = volumeops.VolumeCleanup(steps)
    assert vcl.record() == steps and json.loads(json.dumps(vcl.record())) == steps
    assert volumeops.VolumeCleanup([{"op": "split3d", "erosions": 4}]).record() == [
        {"op": "split3d", "erosions": 4, "structure": "cross", "reach": None}]         # None stays None
    assert volumeops.VolumeCleanup(vcl).record() == steps
    for st in sc.STRUCTURES:
        volumeops.VolumeCleanup([{"op": "split3d", "erosions": 16, "structure": st, "reach": 64}])
    for bad, match in (([{"op": "split3d"}], "step 0 \\(split3d\\): erosions must be an integer 1 .. 16, got None"),
                       ([{"op": "open"}, {"op": "split3d", "erosions": 0}], "step 1 \\(split3d\\): erosions .* got 0"),
                       ([{"op": "split3d", "erosions": 17}], "got 17"),
                       ([{"op": "split3d", "erosions": True}], "got True"),
                       ([{"op": "split3d", "erosions": 2.0}], "got 2.0"),
                       ([{"op": "split3d", "erosions": 2, "structure": "square"}], "structure must be one of .* got 'square'"),
                       ([{"op": "split3d", "erosions": 2, "reach": 0}], "reach must be an integer 1 .. 64 or null, got 0"),
                       ([{"op": "split3d", "erosions": 2, "reach": 65}], "got 65"),
                       ([{"op": "split3d", "erosions": 2, "reach": 4.0}], "got 4.0"),
                       ([{"op": "split3d", "erosions": 2, "iterations": 2}], "unknown key\\(s\\) 'iterations'"),
                       ([{"op": "split", "erosions": 2}], "'split' is not a step for volumes: a 3-D split is not built.*split3d")):
        with pytest.raises(ValueError, match=match):
            volumeops.VolumeCleanup(bad)


def test_device_functions_refuse_host_and_planar_masks():
    import torch
    m = torch.zeros((1, 3, 4, 4), dtype=torch.uint8)
    for call in (lambda: volumeops.split3d(m, 2), lambda: volumeops.split3d(m, 2, "plane_cross"),
                 lambda: volumeops.VolumeCleanup([{"op": "split3d", "erosions": 2}]).apply(m, 2)):
        with pytest.raises(_lib.SequitrHipError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="one of"):
        volumeops.split3d(m, 2, "square")
    with pytest.raises(ValueError, match="erosions must be 1 .. 16"):
        volumeops.split3d(m, 17)
    with pytest.raises(ValueError, match="reach must be 1 .. 64"):
        volumeops.split3d(m, 2, reach=65)
    with pytest.raises(ValueError, match="reach must be 1 .. 64"):
        volumeops.split3d(m, 2, reach=0)
    if torch.cuda.is_available():                               # the shape check comes after the device check
        with pytest.raises(ValueError, match="use sequitr_amd.maskops"):
            volumeops.split3d(m[0].cuda(), 2)


def test_entry_point_checks_its_arguments_before_any_launch():
    lib = _lib.load()
    buf = np.zeros(8192 + 64, np.uint8)
    base = (buf.ctypes.data + 15) // 16 * 16                    # host memory will do: every call below is refused first
    a, b, ws = base, base + 1024, base + 2048
    CROSS = 0

    def refused(rc, word):
        assert rc == -1 and word.encode() in lib.sq_last_error(), (rc, lib.sq_last_error())

    fn = lib.sq_volume_split_u8
    refused(fn(None, b, 1, 2, 8, 8, 2, 1, CROSS, 2, ws, None), "null")
    refused(fn(a, None, 1, 2, 8, 8, 2, 1, CROSS, 2, ws, None), "null")
    refused(fn(a, b, 1, 2, 8, 8, 2, 1, CROSS, 2, None, None), "null")
    refused(fn(a, b, 1, 2, 8, 8, 1, 1, CROSS, 2, ws, None), "C must be")
    refused(fn(a, b, 1, 2, 8, 8, 257, 1, CROSS, 2, ws, None), "C must be")
    refused(fn(a, b, 1, 2, 8, 8, 2, 1, 4, 2, ws, None), "structure must be")
    refused(fn(a, b, 1, 2, 8, 8, 2, 1, -1, 2, ws, None), "structure must be")
    refused(fn(a, b, 1, 2, 8, 8, 2, 0, CROSS, 2, ws, None), "erosions must be 1 .. 16")
    refused(fn(a, b, 1, 2, 8, 8, 2, 17, CROSS, 2, ws, None), "erosions must be 1 .. 16")
    refused(fn(a, b, 1, 2, 8, 8, 2, 1, CROSS, 0, ws, None), "reach must be 1 .. 64")
    refused(fn(a, b, 1, 2, 8, 8, 2, 1, CROSS, 65, ws, None), "reach must be 1 .. 64")
    refused(fn(a, b, 1, 0, 8, 8, 2, 1, CROSS, 2, ws, None), "2^31")
    refused(fn(a, b, 0, 2, 8, 8, 2, 1, CROSS, 2, ws, None), "2^31")
    refused(fn(a, b, 1, 2, 8, -1, 2, 1, CROSS, 2, ws, None), "2^31")
    refused(fn(a, b, 2, 64, 4096, 4096, 2, 1, CROSS, 2, ws, None), "2^31")
    refused(fn(a, b, 65536, 65536, 65536, 65536, 2, 1, CROSS, 2, ws, None), "2^31")
    refused(fn(a, b, 1, 2, 8, 8, 2, 1, CROSS, 2, ws + 8, None), "16-byte aligned")
    refused(fn(a, a + 127, 1, 2, 8, 8, 2, 1, CROSS, 2, ws, None), "out must not overlap mask")
    refused(fn(a, a, 1, 2, 8, 8, 2, 1, CROSS, 2, ws, None), "out must not overlap mask")
    refused(fn(a, b, 1, 2, 8, 8, 2, 1, CROSS, 2, a + 112, None), "workspace must not overlap")
    refused(fn(a, b, 1, 2, 8, 8, 2, 1, CROSS, 2, b - 1024, None), "workspace must not overlap")
    for st in (1, 2, 3):                                        # every structure is checked the same way
        refused(fn(a, b, 1, 2, 8, 8, 2, 1, st, 2, ws + 8, None), "16-byte aligned")
    assert not buf.any()                                        # `out` and the workspace are untouched
    # the workspace: two int32 label planes and the seed bytes, 9 B per voxel, rounded up to 16
    wsf = lib.sq_volume_split_workspace
    assert wsf(3, 2, 5, 11) == (330 * 9 + 15) // 16 * 16
    assert wsf(1, 1, 1, 1) == 16 and wsf(1, 64, 1024, 1024) == 64 * 1024 * 1024 * 9
    assert wsf(2, 64, 4096, 4096) == -1 and wsf(0, 4, 4, 4) == -1 and wsf(1, 4, 4, -1) == -1 and wsf(1, 0, 4, 4) == -1
    assert wsf(65536, 65536, 65536, 65536) == -1 and wsf(1, 1, 32768, 65535) > 0


class _Untouchable(np.ndarray):
    """an array whose voxels must not be touched: the jobs under test raise before they read one"""

    def __getitem__(self, key):
        raise AssertionError("the job read the input")


def test_volume_jobs_refuse_a_bad_split3d_step_before_any_input_is_opened(tmp_path):
    vols = np.zeros((2, 4, 8, 8), np.uint16).view(_Untouchable)
    base = {"input": str(tmp_path / "missing.npy"), "labels": str(tmp_path / "missing_labels.npy"), "output": str(tmp_path)}
    path = str(tmp_path / "steps.json")
    json.dump([{"op": "split3d", "erosions": 4, "structure": "ring"}], open(path, "w"))
    for run, more in ((jobs.SERVER_segment_volume, {}), (jobs.SERVER_segment_volume, {"brick": (8, 8, 4)}),
                      (jobs.SERVER_evaluate, {"brick": (8, 8, 4)})):
        for bad, match in (([{"op": "split3d"}], "erosions"),
                           ([{"op": "split3d", "erosions": 99}], "erosions must be an integer 1 .. 16, got 99"),
                           ([{"op": "open"}, {"op": "split3d", "erosions": 4, "reach": 100}], "step 1 \\(split3d\\): reach"),
                           ([{"op": "split3d", "erosions": 4, "radius": 2}], "unknown key"),
                           ([{"op": "split", "erosions": 4}], "a 3-D split is not built"),
                           (path, "structure")):
            with pytest.raises(ValueError, match=match):
                run(dict(base, volume_postprocess=bad, **more), {})     # the input does not even exist
            with pytest.raises(ValueError, match=match):
                run(dict(base, input=vols, labels=vols, volume_postprocess=bad, **more), {})
    assert os.listdir(str(tmp_path)) == ["steps.json"]
