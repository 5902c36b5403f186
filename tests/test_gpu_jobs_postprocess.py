"""GPU: the mask clean-up wired through the frame jobs (params['postprocess'] of SERVER_segment_frames and SERVER_evaluate)
and the ``postprocess=`` keyword of frontend.segment_frames they ride on.  What a job writes with the key must equal the
scipy restatement (tests/mask_cleanup_cases.py) applied to the mask the same job writes without it, and everything
measured must describe that cleaned mask; without the key the jobs write what they wrote before."""
import json
import os

import numpy as np
import pytest

from sequitr_amd import jobs
from sequitr_amd.frontend import segment_frames
from sequitr_amd.networks.unet import UNet2D
from tests import confusion_cases as cc
from tests import mask_cleanup_cases as mc
from tests import objects_cases as oc

pytestmark = pytest.mark.gpu
STEPS = [{"op": "open", "iterations": 1, "structure": "cross"}, {"op": "fill_holes", "max_area": 30}, {"op": "clear_border"}]
NET = {"shape": (64, 64), "filters": (16, 32), "seed": 2, "margin": 16, "frames_per_batch": 2}


def run(job, tmp_path, name, options=None, **params):
    out = str(tmp_path / name)
    os.makedirs(out)
    info = job(dict(NET, output=out, **params), dict({"gpu": 0}, **(options or {})))
    return out, info


def read(out, fn):
    return open(os.path.join(out, fn), "rb").read()


def test_segment_frames_job_measures_the_cleaned_mask(tmp_path):
    frames = mc.frames_u16()                                    # 3 frames of 96 x 130: an odd last batch
    seg = jobs.SERVER_segment_frames
    opts = {"measure": True, "save_labels": True}
    plain, pinfo = run(seg, tmp_path, "plain", input=frames, options=opts)
    raw = np.load(os.path.join(plain, "mask.npy"))
    want = mc.steps_ref(raw, STEPS, 2)
    print("foreground: raw %.3f, cleaned %.3f; %d pixels changed" % (raw.mean(), want.mean(), int((want != raw).sum())))
    assert (want != raw).any() and want.any(), "the synthetic frames must exercise the clean-up"

    out, info = run(seg, tmp_path, "cleaned", input=frames, postprocess=STEPS, options=opts)
    assert np.array_equal(np.load(os.path.join(out, "mask.npy")), want)
    ref = oc.objects_ref(want, frames)
    z = np.load(os.path.join(out, "objects.npz"))
    for name in ("frame", "cls", "key", "area", "bbox", "label"):
        assert np.array_equal(z[name], ref[name]), name
    assert np.array_equal(z["centroid"].view(np.uint64), ref["centroid"].view(np.uint64))
    for name in ("sum", "sumsq", "min", "max"):
        assert np.array_equal(z["intensity_" + name], ref[name]), name
    assert np.array_equal(np.load(os.path.join(out, "labels.npy")), ref["labels"])
    t = np.load(os.path.join(out, "tracks.npz"))
    for f in range(3):
        sel = ref["frame"] == f
        coords = t["frames/frame_%d/coords" % f]
        assert np.array_equal(t["frames/frame_%d/area" % f], ref["area"][sel])
        assert np.array_equal(coords[:, 1:3], ref["centroid"][sel][:, 1:3].astype(np.float32)) and np.all(coords[:, 0] == f)
    rec = json.load(open(os.path.join(out, "segment.json")))
    assert rec["postprocess"] == STEPS == info["postprocess"] and rec["objects"]["count"] == len(ref["area"])
    assert "postprocess" not in pinfo and "postprocess" not in json.load(open(os.path.join(plain, "segment.json")))

    # with the size filter on top: the filter sees the cleaned mask; and the step list from a JSON file
    path = str(tmp_path / "steps.json")
    json.dump(STEPS, open(path, "w"))
    out2, _ = run(seg, tmp_path, "bounded", input=frames, postprocess=path, min_area=12, options=opts)
    ref2 = oc.objects_ref(want, frames, min_area=12)
    assert len(ref2["area"]) < len(ref["area"]), "the filter must drop something"
    assert np.array_equal(np.load(os.path.join(out2, "mask.npy")), ref2["mask"])
    assert np.array_equal(np.load(os.path.join(out2, "objects.npz"))["area"], ref2["area"])

    # the other two routes of the job: centroids alone (on_masks) and the double-buffered download
    out3, _ = run(seg, tmp_path, "centroids", input=frames, postprocess=STEPS, options={"centroids": True})
    out4, _ = run(seg, tmp_path, "download", input=frames, postprocess=STEPS)
    assert np.array_equal(np.load(os.path.join(out3, "mask.npy")), want) and np.array_equal(np.load(os.path.join(out4, "mask.npy")), want)
    t3 = np.load(os.path.join(out3, "tracks.npz"))
    for f in range(3):
        assert np.array_equal(t3["frames/frame_%d/coords" % f], t["frames/frame_%d/coords" % f])


def test_jobs_without_the_key_write_what_they_wrote(tmp_path):
    frames = mc.frames_u16(seed=6)
    net = UNet2D({"shape": (64, 64), "filters": (16, 32), "device": "cuda:0", "seed": 2}, "infer").initialize()
    direct = segment_frames(net, frames, tile=64, margin=16, frames_per_batch=2)
    a, ia = run(jobs.SERVER_segment_frames, tmp_path, "a", input=frames, options={"measure": True, "save_labels": True})
    b, _ = run(jobs.SERVER_segment_frames, tmp_path, "b", input=frames, options={"measure": True, "save_labels": True})
    assert np.array_equal(np.load(os.path.join(a, "mask.npy")), direct)      # the mask the front end makes, untouched
    ref = oc.objects_ref(direct, frames)                        # and what the existing job tests pin for it
    z = np.load(os.path.join(a, "objects.npz"))
    assert np.array_equal(z["area"], ref["area"]) and np.array_equal(z["key"], ref["key"])
    assert np.array_equal(np.load(os.path.join(a, "labels.npy")), ref["labels"])
    for fn in ("mask.npy", "objects.npz", "labels.npy", "tracks.npz"):
        assert read(a, fn) == read(b, fn), fn
    assert sorted(os.listdir(a)) == ["labels.npy", "mask.npy", "objects.npz", "segment.json", "tracks.npz"]
    assert "postprocess" not in ia
    # the keyword of the front end: a step list or a MaskCleanup, every sink sees the cleaned batch
    want = mc.steps_ref(direct, STEPS, 2)
    assert np.array_equal(segment_frames(net, frames, tile=64, margin=16, frames_per_batch=2, postprocess=STEPS), want)
    seen = {}
    segment_frames(net, frames, tile=64, margin=16, frames_per_batch=2, postprocess=STEPS,
                   on_batch=lambda first, raw, m: seen.__setitem__(first, m.cpu().numpy()))
    assert sorted(seen) == [0, 2] and np.array_equal(np.concatenate([seen[0], seen[2]]), want)
    with pytest.raises(ValueError, match="unknown op"):
        segment_frames(net, frames, tile=64, margin=16, postprocess=[{"op": "thin"}])


def test_evaluate_scores_the_cleaned_masks(tmp_path):
    frames = mc.frames_u16(seed=8)
    labels = (np.random.default_rng(3).random(frames.shape) < 0.4).astype(np.uint8)
    labels[:, 3:9] = 255
    p = {"input": frames, "labels": labels, "num_outputs": 2}
    plain, pinfo = run(jobs.SERVER_evaluate, tmp_path, "plain", options={"masks": True}, **p)
    raw = np.load(os.path.join(plain, "mask.npy"))
    want = mc.steps_ref(raw, STEPS, 2)
    assert (want != raw).any()
    out, info = run(jobs.SERVER_evaluate, tmp_path, "cleaned", postprocess=STEPS, options={"masks": True}, **p)
    assert np.array_equal(np.load(os.path.join(out, "mask.npy")), want)
    counts, ignored = cc.confusion_ref(want.reshape(3, -1), labels.reshape(3, -1), 2)
    assert np.array_equal(np.load(os.path.join(out, "confusion.npy")), counts)
    assert info["confusion"] == counts.sum(0).tolist() and info["ignored"] == int(ignored.sum())
    rec = json.load(open(os.path.join(out, "evaluate.json")))
    assert rec["postprocess"] == STEPS and "postprocess" not in pinfo
    # without the key: the counts of the raw masks, as before, and the same bytes on a second run
    c0, i0 = cc.confusion_ref(raw.reshape(3, -1), labels.reshape(3, -1), 2)
    assert np.array_equal(np.load(os.path.join(plain, "confusion.npy")), c0) and pinfo["ignored"] == int(i0.sum())
    again, _ = run(jobs.SERVER_evaluate, tmp_path, "again", options={"masks": True}, **p)
    for fn in ("confusion.npy", "mask.npy"):
        assert read(plain, fn) == read(again, fn), fn
