"""GPU: options['shape'] of SERVER_segment_frames and of SERVER_segment_volume with ``brick``.  The shape columns of
``objects.npz`` must equal the scipy restatement (tests/objects_shape_cases.py) applied to the ``mask.npy`` the same job
writes -- also behind a split step and a size filter, and under spacing 2.5 for volumes -- the record must carry the option,
and without the option every file must be what a run with the key absent writes."""
import json
import os

import numpy as np
import pytest

from sequitr_amd import jobs
from sequitr_amd.objects import ObjectTable
from tests import objects_shape_cases as sc
from tests import volume_cleanup_cases as vc
from tests.test_gpu_jobs_objects import frames_u16, run_job
from tests.test_gpu_jobs_volume_postprocess import BRICK, read, run

pytestmark = pytest.mark.gpu

INTEGER = {'coord_sums': slice(0, 3), 'moments2': slice(3, 9), 'faces': slice(9, 12), 'boundary': 12,
           'perimeter_counts': slice(13, 16)}
DERIVED = ('covariance', 'axis_lengths', 'equivalent_diameter', 'extent')
PLANAR = ('eccentricity', 'orientation', 'perimeter', 'crack_perimeter', 'circularity')
VOLUME = ('surface_area', 'sphericity')


def check_npz(out, spacing=1.0, volumetric=False):
    """objects.npz of a job against the restatement of the job's own mask.npy; returns the number of rows"""
    mask = np.load(os.path.join(out, "mask.npy"))
    ref = sc.shape_ref(mask)
    z = np.load(os.path.join(out, "objects.npz"))
    for name in ('frame', 'cls', 'key', 'area'):
        assert np.array_equal(z[name], ref[name]), name
    for name, cols in INTEGER.items():
        assert z[name].dtype == np.int64 and np.array_equal(z[name], ref['shape'][:, cols]), name
    k = len(ref['key'])
    ri, rf = np.zeros((k, 12), np.int64), np.zeros((k, 7))
    ri[:, 0], ri[:, 1], ri[:, 2], ri[:, 3], ri[:, 4:10] = z['frame'], z['cls'], z['key'], z['area'], z['bbox']
    rf[:, :3] = z['centroid']
    want = ObjectTable(ri, rf, mask.shape[0], volumetric, shape_i=ref['shape']).columns(spacing=spacing)
    for name in DERIVED + (VOLUME if volumetric else PLANAR):
        assert z[name].dtype == np.float64 and np.array_equal(z[name].view(np.uint64), want[name].view(np.uint64)), name
    assert not any(name in z.files for name in (PLANAR if volumetric else VOLUME))
    return k


def test_segment_frames_shape(tmp_path):
    frames = frames_u16()
    out, info = run_job(tmp_path, "shape", frames, {"shape": True})             # implies measure
    k = check_npz(out)
    rec = json.load(open(os.path.join(out, "segment.json")))
    assert rec["objects"]["shape"] is True and info["objects"]["shape"] is True and rec["objects"]["count"] == k > 3
    assert rec["shape"] == [96, 160]                            # the record's own 'shape' stays the frames' shape
    # behind a split step and a size filter: the columns describe the mask the job writes
    steps = [{"op": "split", "erosions": 1}]
    cut, cinfo = run_job(tmp_path, "cut", frames, {"shape": True, "measure": True, "save_labels": True}, postprocess=steps,
                         min_area=4)
    kc = check_npz(cut)
    plain_cut, _ = run_job(tmp_path, "plaincut", frames, {"measure": True, "save_labels": True}, postprocess=steps, min_area=4)
    assert cinfo["objects"]["count"] == kc and cinfo["objects"]["found"] > kc, "the frames must exercise the filter"
    assert not np.array_equal(np.load(os.path.join(cut, "mask.npy")), np.load(os.path.join(out, "mask.npy")))
    # the old columns and files do not move with the option
    for fn in ("mask.npy", "labels.npy", "tracks.npz"):
        assert read(cut, fn) == read(plain_cut, fn), fn
    za, zb = np.load(os.path.join(plain_cut, "objects.npz")), np.load(os.path.join(cut, "objects.npz"))
    assert set(za.files) < set(zb.files) and all(np.array_equal(za[f], zb[f]) and za[f].dtype == zb[f].dtype for f in za.files)
    # without the option: byte-identical to a run with the key absent
    a, ia = run_job(tmp_path, "absent", frames, {"measure": True, "save_labels": True})
    b, ib = run_job(tmp_path, "false", frames, {"measure": True, "save_labels": True, "shape": False})
    for fn in ("mask.npy", "labels.npy", "tracks.npz", "objects.npz"):
        assert read(a, fn) == read(b, fn), fn
    assert ia["objects"] == ib["objects"] == json.load(open(os.path.join(b, "segment.json")))["objects"] and "shape" not in ia["objects"]
    assert list(np.load(os.path.join(a, "objects.npz")).files) == list(za.files)


def test_segment_volume_shape(tmp_path):
    vols = vc.volumes_u16()
    seg = jobs.SERVER_segment_volume
    out, info = run(seg, tmp_path, "shape", input=vols, spacing=2.5, options={"shape": True}, **BRICK)
    k = check_npz(out, spacing=2.5, volumetric=True)
    rec = json.load(open(os.path.join(out, "segment_volume.json")))
    assert rec["objects"]["shape"] is True and info["objects"]["shape"] is True and rec["objects"]["count"] == k > 3
    assert rec["objects"]["spacing"] == 2.5 and rec["shape"] == [16, 48, 48]
    z = np.load(os.path.join(out, "objects.npz"))
    assert z["covariance"].shape == (k, 3, 3) and np.all(z["perimeter_counts"] == 0) and z["faces"][:, 0].min() >= 2
    unit, _ = run(seg, tmp_path, "unit", input=vols, options={"shape": True}, **BRICK)
    check_npz(unit, volumetric=True)
    assert not np.array_equal(np.load(os.path.join(unit, "objects.npz"))["surface_area"], z["surface_area"])
    # behind split3d and a size filter
    steps = [{"op": "split3d", "erosions": 1}]
    opts = {"measure": True, "save_labels": True}
    cut, cinfo = run(seg, tmp_path, "cut", input=vols, spacing=2.5, volume_postprocess=steps, min_area=4,
                     options=dict(opts, shape=True), **BRICK)
    kc = check_npz(cut, spacing=2.5, volumetric=True)
    assert cinfo["objects"]["count"] == kc and cinfo["objects"]["found"] > kc, "the volumes must exercise the filter"
    plain_cut, _ = run(seg, tmp_path, "plaincut", input=vols, volume_postprocess=steps, min_area=4, options=opts, **BRICK)
    for fn in ("mask.npy", "labels.npy"):
        assert read(cut, fn) == read(plain_cut, fn), fn
    za, zb = np.load(os.path.join(plain_cut, "objects.npz")), np.load(os.path.join(cut, "objects.npz"))
    assert set(za.files) < set(zb.files) and all(np.array_equal(za[f], zb[f]) and za[f].dtype == zb[f].dtype for f in za.files)
    # without the option: byte-identical to a run with the key absent
    a, ia = run(seg, tmp_path, "absent", input=vols, options=opts, **BRICK)
    b, ib = run(seg, tmp_path, "false", input=vols, options=dict(opts, shape=False), **BRICK)
    for fn in ("mask.npy", "labels.npy", "objects.npz"):
        assert read(a, fn) == read(b, fn), fn
    assert ia["objects"] == ib["objects"] and "shape" not in ia["objects"] and "spacing" not in ib["objects"]
    # refused without brick, like its siblings, and a bad spacing before anything is opened
    with pytest.raises(ValueError, match="brick"):
        seg({"input": str(tmp_path / "missing.npy"), "output": str(tmp_path)}, {"shape": True})
    with pytest.raises(ValueError, match="spacing"):
        seg(dict({"input": str(tmp_path / "missing.npy"), "output": str(tmp_path), "spacing": 0}, **BRICK), {"shape": True})
