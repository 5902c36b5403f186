"""GPU: options['neighbors'] of SERVER_segment_frames.  ``neighbors.npz`` and ``zones.npy`` must equal the restatement
(tests/neighbors_cases.py) applied to the ``labels.npy`` and ``objects.npz`` the same job writes -- also behind a `split`
step and a size filter -- the recorded parameters carry the defaults, and without the option the job writes what a run
that never heard of it writes."""
import json
import os

import numpy as np
import pytest

from sequitr_amd import jobs
from tests import mask_cleanup_cases as mc
from tests import neighbors_cases as nc

pytestmark = pytest.mark.gpu
NET = {"shape": (64, 64), "filters": (16, 32), "seed": 2, "margin": 16, "frames_per_batch": 2}
FILES = ("mask.npy", "objects.npz", "labels.npy", "tracks.npz")


def run(tmp_path, name, options=None, **params):
    out = str(tmp_path / name)
    os.makedirs(out)
    info = jobs.SERVER_segment_frames(dict(NET, output=out, **params), dict({"gpu": 0}, **(options or {})))
    return out, info


def read(out, fn):
    return open(os.path.join(out, fn), "rb").read()


def check_against_own_labels(out, info, C=2, d_thresh=100.0, reach=None, seeds="objects"):
    labels = np.load(os.path.join(out, "labels.npy"))
    obj = np.load(os.path.join(out, "objects.npz"))
    assert np.array_equal(labels > 0, np.load(os.path.join(out, "mask.npy")) > 0)     # dropped objects are not seeds
    want = nc.neighbors_ref(labels, obj["cls"], obj["centroid"], obj["frame"], C, d_thresh, reach, seeds)
    got = np.load(os.path.join(out, "neighbors.npz"))
    assert sorted(got.files) == sorted(nc.TABLE_COLUMNS)
    nc.assert_table(got, want, out)
    assert np.array_equal(got["label"], obj["label"])
    zones = np.load(os.path.join(out, "zones.npy"))
    assert zones.dtype == np.int32 and np.array_equal(zones, want["zones"])
    rec = json.load(open(os.path.join(out, "segment.json")))["neighbors"]
    assert rec == info["neighbors"] == {"objects": len(obj["frame"]), "pairs": want["n_pairs"],
                                        "pairs_removed": want["n_pairs_removed"], "num_classes": C, "d_thresh": d_thresh,
                                        "zone_reach": reach, "neighbor_seeds": seeds}
    return want


def test_segment_frames_job_writes_the_neighbours_of_its_own_labels(tmp_path):
    frames = mc.frames_u16()                                    # 3 frames of 96 x 130: an odd last batch
    opts = {"measure": True, "save_labels": True}
    plain, pinfo = run(tmp_path, "plain", input=frames, options=opts)
    out, info = run(tmp_path, "nb", input=frames, options=dict(opts, neighbors=True, save_zones=True))
    for fn in FILES:                                            # the option changes no other file
        assert read(plain, fn) == read(out, fn), fn
    assert "neighbors" not in pinfo and not {"neighbors.npz", "zones.npy"} & set(os.listdir(plain))
    want = check_against_own_labels(out, info)                  # the defaults, written out
    assert want["n_pairs"] > 3 and len(set(want["frame"])) == 3
    assert want["indices"].max() >= (want["frame"] == 0).sum()  # rows of the whole stack's table

    # neighbors implies measure; no zones.npy unless asked for; a threshold that removes pairs; centroid seeds and a reach
    d = float(np.sort(want["distance"])[len(want["distance"]) // 2])
    out2, info2 = run(tmp_path, "nb2", input=frames, d_thresh=d, zone_reach=7, neighbor_seeds="centroids",
                      options={"neighbors": True, "save_labels": True})
    assert not os.path.exists(os.path.join(out2, "zones.npy")) and read(out2, "objects.npz") == read(plain, "objects.npz")
    obj = np.load(os.path.join(out2, "objects.npz"))
    want2 = nc.neighbors_ref(np.load(os.path.join(out2, "labels.npy")), obj["cls"], obj["centroid"], obj["frame"], 2, d, 7,
                             "centroids")
    nc.assert_table(np.load(os.path.join(out2, "neighbors.npz")), want2, "centroid seeds")
    assert info2["neighbors"]["zone_reach"] == 7 and info2["neighbors"]["pairs"] == want2["n_pairs"]

    # behind a split step and a size filter: the table describes the mask the job leaves
    steps = [{"op": "split", "erosions": 1, "structure": "cross"}]
    areas = np.unique(obj["area"])                              # from the plain run's table: a bound that drops its smallest
    assert len(areas) > 1                                       # objects (too small to be split) and keeps its largest
    min_area = int(areas[len(areas) // 2])
    print("min_area %d of areas %d .. %d" % (min_area, areas[0], areas[-1]))
    out3, info3 = run(tmp_path, "nb3", input=frames, postprocess=steps, min_area=min_area, d_thresh=d,
                      options=dict(opts, neighbors=True, save_zones=True))
    want3 = check_against_own_labels(out3, info3, d_thresh=d)
    print("found %d, kept %d, pairs %d, removed %d" % (info3["objects"]["found"], info3["objects"]["count"],
                                                       want3["n_pairs"], want3["n_pairs_removed"]))
    assert info3["objects"]["found"] > info3["objects"]["count"] == len(want3["frame"])
    assert want3["n_pairs_removed"] > 0
