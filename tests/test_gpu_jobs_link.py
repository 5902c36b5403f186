"""GPU: options['link'] of SERVER_segment_frames.  ``lineage.npz`` and ``track_labels.npy`` must equal the restatement
(tests/link_cases.py) applied to the ``labels.npy`` and ``objects.npz`` the same job writes -- also behind a `split` step and
a size filter -- they must not depend on frames_per_batch, the recorded parameters carry the defaults, and without the
option the job writes what a run that never heard of it writes."""
import json
import os

import numpy as np
import pytest

from sequitr_amd import jobs
from tests import link_cases as lc
from tests import mask_cleanup_cases as mc

pytestmark = pytest.mark.gpu
NET = {"shape": (64, 64), "filters": (16, 32), "seed": 2, "margin": 16, "frames_per_batch": 2}
FILES = ("mask.npy", "objects.npz", "labels.npy", "tracks.npz")
LINK_FILES = ("lineage.npz", "track_labels.npy")


def run(tmp_path, name, options=None, **params):
    out = str(tmp_path / name)
    os.makedirs(out)
    info = jobs.SERVER_segment_frames(dict(NET, output=out, **params), dict({"gpu": 0}, **(options or {})))
    return out, info


def read(out, fn):
    return open(os.path.join(out, fn), "rb").read()


def check_against_own_labels(out, info, **opts):
    labels = np.load(os.path.join(out, "labels.npy"))
    obj = np.load(os.path.join(out, "objects.npz"))
    F = labels.shape[0]
    bounds = np.searchsorted(obj["frame"], np.arange(F + 1))
    assert np.diff(bounds).tolist() == lc.counts_of(labels)
    cls = [obj["cls"][bounds[t]:bounds[t + 1]] for t in range(F)]
    want = lc.link_ref_labels(labels, cls, **opts)
    got = np.load(os.path.join(out, "lineage.npz"))
    assert sorted(got.files) == sorted(lc.TRACK_COLUMNS)
    lc.assert_tracks(got, want, out)
    lc.check_consequences(want, lc.counts_of(labels))
    video = np.load(os.path.join(out, "track_labels.npy"))
    offsets = np.concatenate([[0], np.cumsum(lc.counts_of(labels))])
    assert video.dtype == np.int32 and np.array_equal(video, lc.relabel_ref(labels, offsets, want["track"].astype(np.int32)))
    assert np.array_equal(video > 0, np.load(os.path.join(out, "mask.npy")) > 0)
    rec = json.load(open(os.path.join(out, "segment.json")))["link"]
    assert rec == info["link"] == dict(lc.DEFAULTS, objects=len(obj["frame"]), tracks=len(want["ID"]),
                                       links=len(want["links"]), divisions=int((want["children"][:, 0] > 0).sum()),
                                       roots=int((want["parent"] == want["ID"]).sum()), **opts)
    return want


def test_segment_frames_job_links_its_own_labels(tmp_path):
    frames = mc.frames_u16()                                    # 3 frames of 96 x 130: an odd last batch
    opts = {"measure": True, "save_labels": True}
    plain, pinfo = run(tmp_path, "plain", input=frames, options=opts)
    out, info = run(tmp_path, "link", input=frames, options=dict(opts, link=True, save_track_labels=True))
    for fn in FILES:                                            # the option changes no other file
        assert read(plain, fn) == read(out, fn), fn
    assert "link" not in pinfo and not set(LINK_FILES) & set(os.listdir(plain))
    assert set(pinfo) == set(info) - {"link"}
    want = check_against_own_labels(out, info)                  # the defaults, written out
    print("objects %d, tracks %d, links %d, divisions %d" % (len(want["track"]), len(want["ID"]), len(want["links"]),
                                                             info["link"]["divisions"]))
    assert len(want["links"]) > 0 and len(want["ID"]) < len(want["track"])   # something was followed

    # link implies measure; no track_labels.npy unless asked for; identical at every batch size
    for fpb in (1, 3):
        o, _ = run(tmp_path, "fpb%d" % fpb, input=frames, frames_per_batch=fpb,
                   options={"link": True, "save_labels": True, "save_track_labels": fpb == 1})
        assert os.path.exists(os.path.join(o, "track_labels.npy")) == (fpb == 1)
        assert read(o, "objects.npz") == read(plain, "objects.npz")
        got = np.load(os.path.join(o, "lineage.npz"))
        lc.assert_tracks(got, want, "frames_per_batch %d" % fpb)
        if fpb == 1:
            assert read(o, "track_labels.npy") == read(out, "track_labels.npy")

    # behind a split step and a size filter, with a reach and other thresholds: the tracks describe the mask the job leaves
    obj = np.load(os.path.join(plain, "objects.npz"))
    areas = np.unique(obj["area"])
    assert len(areas) > 1
    min_area = int(areas[len(areas) // 2])
    steps = [{"op": "split", "erosions": 1, "structure": "cross"}]
    out3, info3 = run(tmp_path, "link3", input=frames, postprocess=steps, min_area=min_area, link_reach=4, link_min_iou=0.05,
                      link_min_overlap=2, link_same_class=False, link_min_child_fraction=0.25,
                      options=dict(opts, link=True, save_track_labels=True))
    check_against_own_labels(out3, info3, reach=4, min_iou=0.05, min_overlap=2, same_class=False, min_child_fraction=0.25)
    assert info3["objects"]["found"] > info3["objects"]["count"]


def test_bad_link_parameters_raise_before_a_frame_is_opened(tmp_path):
    for bad in ({"link_reach": -1}, {"link_min_iou": 2.0}, {"link_min_overlap": 0}, {"link_divisions": "yes"},
                {"link_min_child_fraction": -1}, {"link_same_class": 3}):
        with pytest.raises(ValueError, match=list(bad)[0][5:]):
            jobs.SERVER_segment_frames(dict(NET, output=str(tmp_path), input="/nonexistent/frames.npy", **bad),
                                       {"gpu": 0, "link": True})
