"""GPU: params['volume_tta'] and options['save_volume_probabilities'] of the brick jobs.  The files equal what
segment_volumes returns for the same model, the sinks (centroids, confusion counts) describe the merged mask the job itself
writes, the refusals come before anything is opened, and without the new keys both jobs write what they always wrote."""
import json
import os

import numpy as np
import pytest

from sequitr_amd import jobs
from sequitr_amd.frontend import segment_volumes
from sequitr_amd.networks.unet import UNet3D
from tests import confusion_cases as cc
from tests import volume_cleanup_cases as vcc

pytestmark = pytest.mark.gpu
NET = {"filters": (16, 32), "num_outputs": 2, "seed": 1}
BRICK = {"brick": (32, 32, 8), "margin": (4, 4, 2), "bricks_per_batch": 3}     # 2 x 2 x 2 bricks and more, an odd last batch
KW = dict(brick=(8, 32, 32), margin=(2, 4, 4), bricks_per_batch=3)             # the same, as segment_volumes takes it


def run(tmp_path, name, job=jobs.SERVER_segment_volume, options=None, **params):
    out = str(tmp_path / name)
    os.makedirs(out)
    info = job(dict(NET, output=out, **dict(BRICK, **params)), dict({"gpu": 0}, **(options or {})))
    return out, info


def read(out, fn):
    return open(os.path.join(out, fn), "rb").read()


def load(out, fn):
    return np.load(os.path.join(out, fn))


def the_jobs_net():
    return UNet3D(dict(NET, shape=(32, 32, 8), num_inputs=1, device="cuda:0"), "infer").initialize()


def test_job_writes_what_segment_volumes_returns(tmp_path):
    vols = vcc.volumes_u16()                                    # (2, 16, 48, 48)
    net = the_jobs_net()
    for tta, save, kind in (("dihedral", True, "uint8"), ("flips", "float32", "float32"), (None, "uint8", "uint8")):
        out, info = run(tmp_path, "job_%s_%s" % (tta, kind), input=vols, volume_tta=tta,
                        options={"save_volume_probabilities": save, "save_logits": True})
        want_m, want_l, want_p = segment_volumes(net, vols, want_logits=True, tta=tta, probabilities=kind, **KW)
        p = load(out, "probability.npy")
        assert np.array_equal(load(out, "mask.npy"), want_m)
        assert p.dtype == np.dtype(kind) and p.shape == (2, 2, 16, 48, 48) and np.array_equal(p, want_p)
        assert np.array_equal(load(out, "logits.npy").view(np.uint32), want_l.view(np.uint32))     # the mean logits
        rec = json.load(open(os.path.join(out, "segment_volume.json")))
        assert rec["volume_tta"] == tta and rec["probabilities"] == kind and info["volume_tta"] == tta
    plain, _ = run(tmp_path, "plain", input=vols)
    assert not np.array_equal(load(str(tmp_path / "job_flips_float32"), "mask.npy"), load(plain, "mask.npy"))
    # the keys are recorded with their defaults when present, and only then
    out, info = run(tmp_path, "defaults", input=vols, volume_tta=None, options={"save_volume_probabilities": False})
    assert info["volume_tta"] is None and info["probabilities"] is None
    assert not os.path.exists(os.path.join(out, "probability.npy")) and read(out, "mask.npy") == read(plain, "mask.npy")
    # with a sink in the way (centroids) the files are the same
    a, _ = run(tmp_path, "sunk", input=vols, volume_tta="flips",
               options={"save_volume_probabilities": "float32", "centroids": True})
    assert read(a, "probability.npy") == read(str(tmp_path / "job_flips_float32"), "probability.npy")
    assert read(a, "mask.npy") == read(str(tmp_path / "job_flips_float32"), "mask.npy")


def test_evaluate_counts_the_merged_mask(tmp_path):
    vols = vcc.volumes_u16()
    rng = np.random.default_rng(9)
    labels = (rng.random(vols.shape) < 0.4).astype(np.uint8)
    labels[..., 3:9, :] = 255
    out, info = run(tmp_path, "ev", job=jobs.SERVER_evaluate, input=vols, labels=labels, volume_tta="flips",
                    options={"masks": True})
    mask = load(out, "mask.npy")
    seg, _ = run(tmp_path, "seg", input=vols, volume_tta="flips")
    assert np.array_equal(mask, load(seg, "mask.npy"))
    plain, pinfo = run(tmp_path, "plain", job=jobs.SERVER_evaluate, input=vols, labels=labels, options={"masks": True})
    assert not np.array_equal(mask, load(plain, "mask.npy")) and "volume_tta" not in pinfo
    want_c, want_i = cc.confusion_ref(mask.reshape(2, -1), labels.reshape(2, -1), 2)
    assert np.array_equal(load(out, "confusion.npy"), want_c) and info["ignored"] == int(want_i.sum()) > 0
    assert json.load(open(os.path.join(out, "evaluate.json")))["volume_tta"] == "flips"


def test_refusals_come_before_anything_is_opened(tmp_path):
    missing = "/nonexistent/volumes.npy"
    base = dict(NET, output=str(tmp_path), input=missing)
    brick = dict(base, **BRICK)
    seg, ev = jobs.SERVER_segment_volume, jobs.SERVER_evaluate
    for bad in ("rot90", 8, True, ["flips"]):
        with pytest.raises(ValueError, match="volume_tta"):
            seg(dict(brick, volume_tta=bad), {"gpu": 0})
        with pytest.raises(ValueError, match="volume_tta"):
            ev(dict(brick, volume_tta=bad, labels=missing), {"gpu": 0})
    for bad in ("float16", 8, "yes"):
        with pytest.raises(ValueError, match="save_volume_probabilities"):
            seg(brick, {"gpu": 0, "save_volume_probabilities": bad})
    with pytest.raises(ValueError, match="brick"):              # without brick
        seg(dict(base, volume_tta="flips"), {"gpu": 0})
    with pytest.raises(ValueError, match="brick"):
        seg(base, {"gpu": 0, "save_volume_probabilities": True})
    with pytest.raises(ValueError, match="square"):             # 'dihedral' transposes x and y
        seg(dict(brick, brick=(32, 16, 8), volume_tta="dihedral"), {"gpu": 0})
    with pytest.raises(ValueError, match="square"):
        ev(dict(brick, brick=(32, 16, 8), volume_tta="dihedral", labels=missing), {"gpu": 0})
    with pytest.raises(ValueError, match="save_volume_probabilities"):
        ev(dict(brick, labels=missing), {"gpu": 0, "save_volume_probabilities": True})
    with pytest.raises(ValueError, match="volume_tta"):         # evaluate on frames
        ev(dict(base, volume_tta="flips", labels=missing), {"gpu": 0})
    for job in (jobs.SERVER_segment, jobs.SERVER_segment_frames, jobs.SERVER_train, jobs.SERVER_train_volume,
                jobs.SERVER_train_gan):                         # every other job refuses the keys by name
        with pytest.raises(ValueError, match="volume_tta"):
            job(dict(base, volume_tta="flips"), {"gpu": 0})
        with pytest.raises(ValueError, match="save_volume_probabilities"):
            job(dict(base), {"gpu": 0, "save_volume_probabilities": True})
    # the planar keys keep their refusals on volumes
    with pytest.raises(ValueError, match="SERVER_segment_volume"):
        seg(dict(brick, tta="flips"), {"gpu": 0})
    with pytest.raises(ValueError, match="SERVER_segment_volume"):
        seg(dict(brick), {"gpu": 0, "save_probabilities": True})
    with pytest.raises(ValueError, match="brick"):
        ev(dict(brick, tta="flips", labels=missing), {"gpu": 0})


def test_jobs_without_the_new_keys_write_what_they_wrote(tmp_path):
    """the unchanged code path is segment_volumes without the keywords: net.predict and scatter"""
    vols = vcc.volumes_u16()
    net = the_jobs_net()
    want, want_l = segment_volumes(net, vols, want_logits=True, **KW)
    a, ia = run(tmp_path, "a", input=vols, options={"save_logits": True})
    assert np.array_equal(load(a, "mask.npy"), want) and "probability.npy" not in os.listdir(a)
    assert np.array_equal(load(a, "logits.npy").view(np.uint32), want_l.view(np.uint32))
    assert "volume_tta" not in ia and "probabilities" not in ia
    b, ib = run(tmp_path, "b", input=vols, volume_tta=None, options={"save_logits": True})     # the default, spelled out
    assert read(a, "mask.npy") == read(b, "mask.npy") and read(a, "logits.npy") == read(b, "logits.npy")
    assert set(ib) == set(ia) | {"volume_tta"} and sorted(os.listdir(a)) == sorted(os.listdir(b))
    rng = np.random.default_rng(6)
    labels = (rng.random(vols.shape) < 0.4).astype(np.uint8)
    e, ie = run(tmp_path, "e", job=jobs.SERVER_evaluate, input=vols, labels=labels)
    f, jf = run(tmp_path, "f", job=jobs.SERVER_evaluate, input=vols, labels=labels, volume_tta=None)
    assert read(e, "confusion.npy") == read(f, "confusion.npy") and "volume_tta" not in ie and jf["volume_tta"] is None
    want_c, _ = cc.confusion_ref(want.reshape(2, -1), labels.reshape(2, -1), 2)
    assert np.array_equal(load(e, "confusion.npy"), want_c)
