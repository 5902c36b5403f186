"""GPU: SERVER_evaluate and SERVER_train's held-out validation against the segment jobs.  What a job counted on the device
must equal, integer for integer, the numpy confusion (tests/confusion_cases.py) of the masks the matching segment job
writes for the same model on the same data; validation must leave the training step's losses bit-identical."""
import json
import os

import numpy as np
import pytest

from sequitr_amd import confusion, jobs
from sequitr_amd.pipeline import ImageNorm, ImageOutliers, ImagePipeline
from tests import confusion_cases as cc

pytestmark = pytest.mark.gpu
NET = {"shape": (64, 64), "filters": (16, 32), "num_outputs": 2}


def _labels(shape, seed):
    """class indices 0 / 1 with a band of 255 (unlabelled) and a few 7s (a class the two-class net does not have)"""
    rng = np.random.default_rng(seed)
    lab = (rng.random(shape) < 0.4).astype(np.uint8)
    lab[..., 3:9, :] = 255
    lab[rng.random(shape) < 0.01] = 7
    return lab


def _out(tmp_path, name):
    d = str(tmp_path / name)
    os.mkdir(d)
    return d


def _want(masks, labels, C=2):
    F = masks.shape[0]
    return cc.confusion_ref(masks.reshape(F, -1), labels.reshape(F, -1), C)


def _check_record(info, counts, ignored, n_items):
    assert info["confusion"] == counts.sum(0).tolist() and info["ignored"] == int(ignored.sum()) > 0
    total = confusion.json_ready(confusion.scores(counts.sum(0)))
    assert info["scores"] == total and len(info["per_frame"]) == n_items
    for k in range(n_items):
        assert info["per_frame"][k] == dict(confusion.json_ready(confusion.scores(counts[k])), ignored=int(ignored[k]))
    assert info["seconds"] > 0 and info["mpixels_per_s"] > 0 and info["num_classes"] == 2


@pytest.mark.parametrize("pipeline", [False, True], ids=["norm", "outliers+norm"])
def test_evaluate_frames_equals_segment_frames_masks(tmp_path, pipeline):
    rng = np.random.default_rng(5)
    frames = rng.integers(100, 4000, (3, 80, 104)).astype(np.uint16)    # a little larger than a tile, no multiple of it
    labels = _labels(frames.shape, 6)
    np.save(str(tmp_path / "frames.npy"), frames)
    np.save(str(tmp_path / "labels.npy"), labels)
    params = dict(NET, input=str(tmp_path / "frames.npy"), seed=2, margin=8, frames_per_batch=2)
    if pipeline:
        ImagePipeline([ImageOutliers(2, 50.), ImageNorm()]).save(str(tmp_path / "pipe.json"))
        params["pipeline"] = str(tmp_path / "pipe.json")
    seg = jobs.SERVER_segment_frames(dict(params, output=_out(tmp_path, "seg")), {"gpu": 0})
    masks = np.load(str(tmp_path / "seg" / "mask.npy"))
    want_c, want_i = _want(masks, labels)

    ev = dict(params, labels=str(tmp_path / "labels.npy"))
    info = jobs.SERVER_evaluate(dict(ev, output=_out(tmp_path, "ev")), {"gpu": 0})
    got = np.load(str(tmp_path / "ev" / "confusion.npy"))
    assert got.dtype == np.int64 and got.shape == (3, 2, 2) and np.array_equal(got, want_c)
    assert [p["ignored"] for p in info["per_frame"]] == want_i.tolist()
    assert np.array_equal(got.sum((1, 2)) + want_i, np.full(3, 80 * 104))
    on_disk = json.load(open(str(tmp_path / "ev" / "evaluate.json")))
    assert on_disk == json.loads(json.dumps(info))
    _check_record(on_disk, want_c, want_i, 3)
    assert on_disk["frames"] == 3 and on_disk["shape"] == [80, 104] and on_disk["tile"] == 64
    assert on_disk.get("pipeline") == seg.get("pipeline") and ("pipeline" in on_disk) == pipeline
    assert not os.path.exists(str(tmp_path / "ev" / "mask.npy"))
    if not pipeline:
        # labels that follow the frames batch by batch instead of staying resident, as an ndarray, and with the masks kept
        info2 = jobs.SERVER_evaluate(dict(ev, labels=labels, output=_out(tmp_path, "ev2")),
                                     {"gpu": 0, "resident_label_gib": 0, "masks": True})
        assert np.array_equal(np.load(str(tmp_path / "ev2" / "confusion.npy")), want_c) and info2["ignored"] == info["ignored"]
        assert np.array_equal(np.load(str(tmp_path / "ev2" / "mask.npy")), masks)


def test_evaluate_volume_bricks_equals_segment_volume_masks(tmp_path):
    vols = np.random.default_rng(8).integers(100, 4000, (2, 11, 26, 37)).astype(np.uint16)
    labels = _labels(vols.shape, 9)
    np.save(str(tmp_path / "vols.npy"), vols)
    np.save(str(tmp_path / "labels.npy"), labels)
    params = {"input": str(tmp_path / "vols.npy"), "filters": (16, 32), "num_outputs": 2, "seed": 6, "brick": (16, 16, 8),
              "margin": (4, 4, 2), "bricks_per_batch": 5}
    jobs.SERVER_segment_volume(dict(params, output=_out(tmp_path, "seg")), {"gpu": 0})
    masks = np.load(str(tmp_path / "seg" / "mask.npy"))
    want_c, want_i = _want(masks, labels)
    for name, options in (("ev", {"gpu": 0}), ("ev2", {"gpu": 0, "resident_label_gib": 0, "masks": True})):
        info = jobs.SERVER_evaluate(dict(params, labels=str(tmp_path / "labels.npy"), output=_out(tmp_path, name)), options)
        assert np.array_equal(np.load(str(tmp_path / name / "confusion.npy")), want_c), name
        _check_record(json.load(open(str(tmp_path / name / "evaluate.json"))), want_c, want_i, 2)
        assert info["volumes"] == 2 and info["shape"] == [11, 26, 37] and info["brick"] == [16, 16, 8]
        assert os.path.exists(str(tmp_path / name / "mask.npy")) == (name == "ev2")
    assert np.array_equal(np.load(str(tmp_path / "ev2" / "mask.npy")), masks)


def _check_validation(tj, steps_per_epoch, want_c, want_i):
    val = tj["validation"]
    assert [v["step"] for v in val] == [steps_per_epoch, 2 * steps_per_epoch] and [v["epoch"] for v in val] == [1, 2]
    last = val[-1]
    assert last["confusion"] == want_c.sum(0).tolist() and last["ignored"] == int(want_i.sum()) > 0
    s = confusion.json_ready(confusion.scores(want_c.sum(0)))
    assert all(last[k] == s[k] for k in ("iou", "dice", "accuracy", "mean_iou")) and last["seconds"] > 0
    assert set(last) == {"step", "epoch", "confusion", "ignored", "iou", "dice", "accuracy", "mean_iou", "seconds"}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_train_with_validation_leaves_the_losses_and_scores_the_saved_model(dtype, tmp_path, monkeypatch):
    from sequitr_amd import core
    monkeypatch.setattr(core.TensorflowConfiguration, "MODELDIR", _out(tmp_path, "models"))
    rng = np.random.default_rng(4)
    lab = (rng.random((12, 64, 64)) < 0.3).astype(np.uint8)
    np.save(str(tmp_path / "im.npy"), (lab * 1.5 + rng.standard_normal(lab.shape) * 0.5).astype(np.float32))
    np.save(str(tmp_path / "lab.npy"), lab)
    vlab = _labels((5, 64, 64), 3)
    vim = ((vlab == 1) * 1.5 + rng.standard_normal(vlab.shape) * 0.5).astype(np.float32)
    np.save(str(tmp_path / "vim.npy"), vim)
    np.save(str(tmp_path / "vlab.npy"), vlab)
    params = dict(NET, images=str(tmp_path / "im.npy"), labels=str(tmp_path / "lab.npy"), num_epochs=2, batch_size=4,
                  dropout=0.4, seed=1, dtype=dtype)             # dropout on: its salt must not move either
    plain = jobs.SERVER_train(dict(params, output=_out(tmp_path, "plain")), {"gpu": 0})
    info = jobs.SERVER_train(dict(params, output=_out(tmp_path, "val"), val_images=str(tmp_path / "vim.npy"),
                                  val_labels=str(tmp_path / "vlab.npy"), validate_every=1, val_batch=2), {"gpu": 0})
    tj_plain = json.load(open(str(tmp_path / "plain" / "train.json")))
    tj = json.load(open(str(tmp_path / "val" / "train.json")))
    print("losses (%s): %r" % (dtype, tj["losses"]))
    assert info["steps"] == plain["steps"] == 6 and tj["dtype"] == dtype and "validation" not in tj_plain
    assert tj["losses"] == tj_plain["losses"] and np.isfinite(tj["losses"]).all()      # bit for bit: the same floats

    jobs.SERVER_segment(dict(NET, input=str(tmp_path / "vim.npy"), model=info["model_dir"], batch=3,
                             output=_out(tmp_path, "seg")), {"gpu": 0})
    want_c, want_i = _want(np.load(str(tmp_path / "seg" / "mask.npy")), vlab)
    _check_validation(tj, 3, want_c, want_i)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_train_on_whole_frames_with_validation(dtype, tmp_path, monkeypatch):
    from sequitr_amd import core
    monkeypatch.setattr(core.TensorflowConfiguration, "MODELDIR", _out(tmp_path, "models"))
    rng = np.random.default_rng(7)
    lab = (rng.random((3, 80, 96)) < 0.3).astype(np.uint8)
    np.save(str(tmp_path / "im.npy"), ((lab == 1) * 900 + rng.integers(100, 1000, lab.shape)).astype(np.uint16))
    np.save(str(tmp_path / "lab.npy"), lab)
    vlab = _labels((3, 80, 96), 11)
    np.save(str(tmp_path / "vim.npy"), ((vlab == 1) * 900 + rng.integers(100, 1000, vlab.shape)).astype(np.uint16))
    np.save(str(tmp_path / "vlab.npy"), vlab)
    params = {"images": str(tmp_path / "im.npy"), "labels": str(tmp_path / "lab.npy"), "tile": (64, 64), "filters": (16, 32),
              "num_outputs": 2, "batch_size": 4, "samples_per_epoch": 8, "num_epochs": 2, "dropout": 0.4, "seed": 5,
              "dtype": dtype, "margin": 8, "frames_per_batch": 2}
    plain = jobs.SERVER_train(dict(params, output=_out(tmp_path, "plain")), {"gpu": 0})
    info = jobs.SERVER_train(dict(params, output=_out(tmp_path, "val"), val_images=str(tmp_path / "vim.npy"),
                                  val_labels=str(tmp_path / "vlab.npy"), validate_every=1), {"gpu": 0})
    tj_plain = json.load(open(str(tmp_path / "plain" / "train.json")))
    tj = json.load(open(str(tmp_path / "val" / "train.json")))
    print("losses (%s): %r" % (dtype, tj["losses"]))
    assert info["steps"] == plain["steps"] == 4 and "validation" not in tj_plain
    assert tj["losses"] == tj_plain["losses"] and np.isfinite(tj["losses"]).all()

    jobs.SERVER_segment_frames(dict(NET, input=str(tmp_path / "vim.npy"), model=info["model_dir"], margin=8, frames_per_batch=2,
                                    output=_out(tmp_path, "seg")), {"gpu": 0})
    want_c, want_i = _want(np.load(str(tmp_path / "seg" / "mask.npy")), vlab)
    _check_validation(tj, 2, want_c, want_i)
