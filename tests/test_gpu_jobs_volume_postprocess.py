"""GPU: the volume clean-up wired through the volume jobs (params['volume_postprocess'] of SERVER_segment_volume, with and
without ``brick``, and of SERVER_evaluate with ``brick``) and the ``postprocess=`` keyword of frontend.segment_volumes they
ride on.  What a job writes with the key must equal the scipy restatement (tests/volume_cleanup_cases.py) applied to the
mask the same job writes without it, and the centroids and the confusion counts must describe that cleaned mask; without
the key the jobs write what they wrote before."""
import json
import os

import numpy as np
import pytest
import torch

from sequitr_amd import jobs
from sequitr_amd.centroids import mask_centroids
from tests import confusion_cases as cc
from tests import volume_cleanup_cases as vc

pytestmark = pytest.mark.gpu
STEPS = [{"op": "open", "structure": "cross"}, {"op": "fill_holes", "max_voxels": 30}, {"op": "clear_border", "faces": "lateral"}]
FULL = [{"op": "open", "iterations": 1, "structure": "cross"}, {"op": "fill_holes", "max_voxels": 30, "planar": False},
        {"op": "clear_border", "faces": "lateral"}]
NET = {"filters": (16, 32), "num_outputs": 2, "seed": 1}         # this seed's mask is 44 % foreground in many objects
BRICK = {"brick": (32, 32, 8), "margin": (4, 4, 2), "bricks_per_batch": 3}     # 2 x 2 x 2 bricks and more, an odd last batch


def run(job, tmp_path, name, options=None, **params):
    out = str(tmp_path / name)
    os.makedirs(out)
    info = job(dict(NET, output=out, **params), dict({"gpu": 0}, **(options or {})))
    return out, info


def read(out, fn):
    return open(os.path.join(out, fn), "rb").read()


def tracks(out, info, n):
    """the centroid file's coords per volume, whichever container it is"""
    path = os.path.join(out, info["centroids"]["file"])
    if path.endswith(".npz"):
        z = np.load(path)
        return [z["frames/frame_%d/coords" % i] for i in range(n)]
    import h5py
    with h5py.File(path, "r") as f:
        return [f["frames/frame_%d/coords" % i][...] for i in range(n)]


def centroids_of(masks):
    out = []
    for i in range(masks.shape[0]):
        m = torch.from_numpy(masks[i:i + 1]).cuda()
        coords = mask_centroids(m.transpose(1, 3).contiguous())[0]      # the axes as CentroidWriter.write swaps them
        coords[:, 0] = i
        out.append(coords)
    return out


def check_cleaned(plain, out, info, pinfo, name):
    raw = np.load(os.path.join(plain, "mask.npy"))
    want = vc.steps_ref(raw, STEPS, 2)
    print("%s: foreground raw %.3f, cleaned %.3f; %d voxels changed" % (name, raw.mean(), want.mean(), int((want != raw).sum())))
    assert raw.shape == (2, 16, 48, 48) and (want != raw).any() and want.any(), "the volumes must exercise the clean-up"
    got = np.load(os.path.join(out, "mask.npy"))
    assert np.array_equal(got, want)
    got_t, want_t = tracks(out, info, 2), centroids_of(want)
    for i in range(2):
        assert np.array_equal(np.asarray(got_t[i]), want_t[i]), i
    assert info["centroids"]["objects"] == sum(len(t) for t in want_t)
    rec = json.load(open(os.path.join(out, "segment_volume.json")))
    assert rec["volume_postprocess"] == FULL == info["volume_postprocess"]
    assert "volume_postprocess" not in pinfo and "volume_postprocess" not in json.load(open(os.path.join(plain, "segment_volume.json")))
    return want


def test_segment_volume_bricks_writes_the_cleaned_mask(tmp_path):
    vols = vc.volumes_u16()
    seg = jobs.SERVER_segment_volume
    cen = {"centroids": True}
    plain, pinfo = run(seg, tmp_path, "plain", input=vols, options=cen, **BRICK)
    assert pinfo["bricks_per_volume"] > 1
    out, info = run(seg, tmp_path, "cleaned", input=vols, volume_postprocess=STEPS, options=cen, **BRICK)
    want = check_cleaned(plain, out, info, pinfo, "bricks")
    # the download route (no centroids), with the step list from a JSON file
    path = str(tmp_path / "steps.json")
    json.dump(STEPS, open(path, "w"))
    out2, info2 = run(seg, tmp_path, "download", input=vols, volume_postprocess=path, options={"save_logits": True}, **BRICK)
    assert np.array_equal(np.load(os.path.join(out2, "mask.npy")), want) and info2["volume_postprocess"] == FULL
    # logits are not touched; without the key the files are what the untouched path writes
    plain2, _ = run(seg, tmp_path, "plain2", input=vols, options={"centroids": True, "save_logits": True}, **BRICK)
    assert read(plain2, "logits.npy") == read(out2, "logits.npy")
    assert read(plain2, "mask.npy") == read(plain, "mask.npy")
    assert [np.asarray(t).tobytes() for t in tracks(plain2, pinfo, 2)] == [np.asarray(t).tobytes() for t in tracks(plain, pinfo, 2)]
    # the planar key is still refused for volumes
    with pytest.raises(ValueError, match="volumes"):
        seg(dict(NET, input=vols, output=out, postprocess=[{"op": "open"}], **BRICK), {"gpu": 0})


def test_segment_volumes_keyword_matches_the_job(tmp_path):
    from sequitr_amd.frontend import segment_volumes
    from sequitr_amd.networks.unet import UNet3D
    from sequitr_amd.volumeops import VolumeCleanup
    vols = vc.volumes_u16()
    plain, _ = run(jobs.SERVER_segment_volume, tmp_path, "plain", input=vols, **BRICK)
    raw = np.load(os.path.join(plain, "mask.npy"))
    net = UNet3D(dict(NET, shape=(32, 32, 8), num_inputs=1, device="cuda:0"), "infer")
    net.initialize()
    untouched, _ = segment_volumes(net, vols, (8, 32, 32), (2, 4, 4), bricks_per_batch=3)
    assert np.array_equal(untouched, raw)                       # the job without the key is the untouched code path
    seen = {}
    got, logits = segment_volumes(net, vols, (8, 32, 32), (2, 4, 4), bricks_per_batch=3, postprocess=VolumeCleanup(STEPS),
                                  want_logits=True, on_masks=lambda i, m: seen.__setitem__(i, m[0].cpu().numpy()))
    want = vc.steps_ref(raw, STEPS, 2)
    assert got is None and np.array_equal(np.stack([seen[0], seen[1]]), want)
    assert np.array_equal(logits.argmax(-1).astype(np.uint8), raw)      # the logits still describe the raw mask
    got2, _ = segment_volumes(net, vols, (8, 32, 32), (2, 4, 4), bricks_per_batch=3, postprocess=STEPS)
    assert np.array_equal(got2, want)


def test_segment_volume_whole_writes_the_cleaned_mask(tmp_path):
    v = vc.volumes_u16().astype(np.float32)
    v = (v - v.mean()) / v.std()
    seg = jobs.SERVER_segment_volume
    plain, pinfo = run(seg, tmp_path, "plain", input=v, options={"centroids": True})
    out, info = run(seg, tmp_path, "cleaned", input=v, volume_postprocess=STEPS, options={"centroids": True})
    assert "brick" not in info
    check_cleaned(plain, out, info, pinfo, "whole volumes")
    plain2, _ = run(seg, tmp_path, "plain2", input=v, options={"centroids": True})
    assert read(plain2, "mask.npy") == read(plain, "mask.npy")


def test_evaluate_volume_bricks_counts_the_cleaned_masks(tmp_path):
    vols = vc.volumes_u16()
    rng = np.random.default_rng(9)
    labels = (rng.random(vols.shape) < 0.4).astype(np.uint8)
    labels[..., 3:9, :] = 255
    plain, pinfo = run(jobs.SERVER_evaluate, tmp_path, "plain", input=vols, labels=labels, options={"masks": True}, **BRICK)
    raw = np.load(os.path.join(plain, "mask.npy"))
    want = vc.steps_ref(raw, STEPS, 2)
    assert (want != raw).any() and want.any()
    out, info = run(jobs.SERVER_evaluate, tmp_path, "cleaned", input=vols, labels=labels, volume_postprocess=STEPS,
                    options={"masks": True}, **BRICK)
    assert np.array_equal(np.load(os.path.join(out, "mask.npy")), want)
    want_c, want_i = cc.confusion_ref(want.reshape(2, -1), labels.reshape(2, -1), 2)
    assert np.array_equal(np.load(os.path.join(out, "confusion.npy")), want_c)
    rec = json.load(open(os.path.join(out, "evaluate.json")))
    assert rec["volume_postprocess"] == FULL and rec["confusion"] == want_c.sum(0).tolist() and rec["ignored"] == int(want_i.sum())
    assert "volume_postprocess" not in pinfo and rec["confusion"] != pinfo["confusion"]
    again, _ = run(jobs.SERVER_evaluate, tmp_path, "again", input=vols, labels=labels, options={"masks": True}, **BRICK)
    assert read(again, "mask.npy") == read(plain, "mask.npy") and read(again, "confusion.npy") == read(plain, "confusion.npy")
