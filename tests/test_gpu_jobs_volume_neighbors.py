"""GPU: options['measure'] / ['save_labels'] / ['neighbors'] / ['save_zones'] of SERVER_segment_volume with ``brick`` and the
``on_volume=`` sink of frontend.segment_volumes they ride on.  ``objects.npz`` and ``labels.npy`` must equal the scipy
restatement (tests/objects_cases.py) of the ``mask.npy`` the same job writes against the raw volumes, ``neighbors.npz`` and
``zones.npy`` the restatement of tests/neighbors3d_cases.py applied to those -- also behind a ``volume_postprocess`` list
and a size filter -- the records carry the defaults, and the options change no file the job wrote before."""
import json
import os

import numpy as np
import pytest

from sequitr_amd import jobs
from tests import neighbors3d_cases as n3
from tests import objects_cases as oc
from tests import volume_cleanup_cases as vc
from tests.test_gpu_jobs_volume_postprocess import BRICK, NET, STEPS, read, run, tracks

pytestmark = pytest.mark.gpu
SEG = jobs.SERVER_segment_volume
ALL = {"measure": True, "save_labels": True, "neighbors": True, "save_zones": True}


def check_against_own_mask(out, info, vols, C=2, d_thresh=100.0, reach=None, seeds="objects", spacing=1.0, min_area=1):
    mask = np.load(os.path.join(out, "mask.npy"))
    ref = oc.objects_ref(mask, vols)                            # 6-connected, (plane, row, column) = (Z, X, Y) as they lie
    obj = np.load(os.path.join(out, "objects.npz"))
    for name in ("frame", "cls", "key", "area", "bbox", "label"):
        assert obj[name].dtype == np.int64 and np.array_equal(obj[name], ref[name]), name
    assert np.array_equal(obj["centroid"].view(np.uint64), ref["centroid"].view(np.uint64))
    assert np.array_equal(obj["intensity_sum"], ref["sum"]) and np.array_equal(obj["intensity_max"], ref["max"])
    assert len(obj["frame"]) and obj["area"].min() >= min_area
    labels = np.load(os.path.join(out, "labels.npy"))
    assert labels.dtype == np.int32 and labels.shape == vols.shape and np.array_equal(labels, ref["labels"])
    assert np.array_equal(labels > 0, mask > 0)                 # dropped objects are in neither
    rec = json.load(open(os.path.join(out, "segment_volume.json")))
    assert rec["objects"] == info["objects"] and rec["objects"]["count"] == len(obj["frame"])
    assert rec["objects"]["min_area"] == min_area and rec["objects"]["max_area"] is None and rec["objects"]["with_intensity"]
    want = n3.neighbors3d_ref(labels, obj["cls"], obj["centroid"], obj["frame"], C, d_thresh, reach, seeds, spacing)
    got = np.load(os.path.join(out, "neighbors.npz"))
    assert sorted(got.files) == sorted(n3.TABLE_COLUMNS)
    n3.assert_table(got, want, out)
    if os.path.exists(os.path.join(out, "zones.npy")):
        zones = np.load(os.path.join(out, "zones.npy"))
        assert zones.dtype == np.int32 and np.array_equal(zones, want["zones"])
    assert rec["neighbors"] == info["neighbors"] == {
        "objects": len(obj["frame"]), "pairs": want["n_pairs"], "pairs_removed": want["n_pairs_removed"], "num_classes": C,
        "d_thresh": d_thresh, "zone_reach": reach, "neighbor_seeds": seeds, "spacing": spacing}
    return want, rec


def test_segment_volume_job_writes_objects_and_neighbours_of_its_own_mask(tmp_path):
    vols = vc.volumes_u16()
    plain, pinfo = run(SEG, tmp_path, "plain", input=vols, options={"centroids": True}, **BRICK)
    out, info = run(SEG, tmp_path, "nb", input=vols, options=dict(ALL, centroids=True), **BRICK)
    # the options change no file the job wrote before
    assert read(plain, "mask.npy") == read(out, "mask.npy")
    assert [np.asarray(t).tobytes() for t in tracks(plain, pinfo, 2)] == [np.asarray(t).tobytes() for t in tracks(out, info, 2)]
    assert not {"objects", "neighbors"} & set(pinfo) and set(info) - set(pinfo) == {"objects", "neighbors"}
    assert not {"objects.npz", "labels.npy", "neighbors.npz", "zones.npy"} & set(os.listdir(plain))
    want, rec = check_against_own_mask(out, info, vols)         # the defaults, written out
    print("objects %d, pairs %d, lateral %d, axial %d" % (len(want["frame"]), want["n_pairs"], want["border_lateral"].sum(),
                                                           want["border_axial"].sum()))
    assert want["n_pairs"] > 3 and set(want["frame"]) == {0, 1}
    assert want["border_axial"].any() and want["border_lateral"].any()
    assert want["indices"].max() >= (want["frame"] == 0).sum()  # rows of the whole stack's table

    # neighbors implies measure; the download route (no centroids); no labels.npy / zones.npy unless asked for
    out2, info2 = run(SEG, tmp_path, "nb2", input=vols, options={"neighbors": True}, **BRICK)
    assert read(out2, "mask.npy") == read(plain, "mask.npy") and read(out2, "objects.npz") == read(out, "objects.npz")
    assert read(out2, "neighbors.npz") == read(out, "neighbors.npz") and "centroids" not in info2
    assert not {"labels.npy", "zones.npy"} & set(os.listdir(out2))
    # measure alone
    out3, info3 = run(SEG, tmp_path, "measure", input=vols, options={"measure": True}, **BRICK)
    assert read(out3, "objects.npz") == read(out, "objects.npz") and "neighbors" not in info3
    assert not {"labels.npy", "neighbors.npz", "zones.npy"} & set(os.listdir(out3))


def test_behind_a_clean_up_list_and_a_size_filter_with_every_parameter_set(tmp_path):
    vols = vc.volumes_u16()
    first, finfo = run(SEG, tmp_path, "first", input=vols, volume_postprocess=STEPS, options=ALL, **BRICK)
    areas = np.unique(np.load(os.path.join(first, "objects.npz"))["area"])
    assert len(areas) > 1
    min_area = int(areas[len(areas) // 2])                      # a bound that drops the smaller objects and keeps the largest
    free = np.load(os.path.join(first, "neighbors.npz"))
    d = float(np.sort(free["distance"])[len(free["distance"]) // 2])
    out, info = run(SEG, tmp_path, "all", input=vols, volume_postprocess=STEPS, min_area=min_area, d_thresh=d, zone_reach=6,
                    neighbor_seeds="centroids", spacing=2.5, options=dict(ALL, centroids=True), **BRICK)
    want, rec = check_against_own_mask(out, info, vols, d_thresh=d, reach=6, seeds="centroids", spacing=2.5,
                                       min_area=min_area)
    print("min_area %d: found %d, kept %d, pairs %d, removed %d" % (min_area, info["objects"]["found"],
                                                                    info["objects"]["count"], want["n_pairs"],
                                                                    want["n_pairs_removed"]))
    assert info["objects"]["found"] > info["objects"]["count"] == len(want["frame"])
    assert rec["volume_postprocess"] == finfo["volume_postprocess"]
    # mask.npy is the cleaned mask without the dropped objects, and the centroid file describes it
    cleaned = np.load(os.path.join(first, "mask.npy"))
    kept = np.load(os.path.join(out, "mask.npy"))
    assert np.array_equal(kept, oc.objects_ref(cleaned, min_area=min_area)["mask"]) and (kept != cleaned).any()
    assert info["centroids"]["objects"] == info["objects"]["count"]


def test_on_volume_receives_the_raw_volume_it_uploaded(tmp_path):
    from sequitr_amd.frontend import segment_volumes
    from sequitr_amd.networks.unet import UNet3D
    vols = vc.volumes_u16()
    net = UNet3D(dict(NET, shape=(32, 32, 8), num_inputs=1, device="cuda:0"), "infer")
    net.initialize()
    want, _ = segment_volumes(net, vols, (8, 32, 32), (2, 4, 4), bricks_per_batch=3)
    seen = {}

    def sink(i, raw, mask):
        assert raw.is_cuda and mask.is_cuda and tuple(raw.shape) == tuple(mask.shape) == (1,) + vols.shape[1:]
        seen[i] = (raw.cpu().numpy()[0], mask.cpu().numpy()[0])

    got, logits = segment_volumes(net, vols, (8, 32, 32), (2, 4, 4), bricks_per_batch=3, on_volume=sink)
    assert got is None and logits is None and sorted(seen) == [0, 1]
    for i in range(2):
        assert seen[i][0].dtype == vols.dtype and np.array_equal(seen[i][0], vols[i]) and np.array_equal(seen[i][1], want[i])
    with pytest.raises(ValueError, match="one of them"):
        segment_volumes(net, vols, (8, 32, 32), (2, 4, 4), on_masks=lambda i, m: None, on_volume=sink)
