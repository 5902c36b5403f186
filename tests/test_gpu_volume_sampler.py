"""GPU volume sampler vs the numpy restatement of its definition (tests/volume_sampler_cases.py), BIT-EXACT throughout:
images under all 16 ops in three voxel types with and without ImageNorm, the verbatim copy at every supported voxel size,
the one-hot expansion, the LDS and the direct path of the transposed ops against each other, plans that point outside
the volumes, the tie to VolumeTiler, and SERVER_train_volume's brick mode closed into SERVER_segment_volume."""
import json
import os

import numpy as np
import pytest
import torch

from sequitr_amd import _lib
from sequitr_amd.frontend import VolumeSampler, VolumeTiler, sample_plan, segment_volumes, volume_bricks, volume_stats
from tests import volume_frontend_cases as vc
from tests import volume_sampler_cases as sc
from tests.util import assert_bit_exact

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_cache = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def volumes(shape, dtype):
    """(raw volumes, {normalise: what ImageNorm makes of them}) -- computed once per shape and type"""
    key = (shape, np.dtype(dtype).name)
    if key not in _cache:
        vols = vc.random_volume(shape, dtype, seed=3)
        _cache[key] = (vols, {n: sc.np_normalised(vols, n) for n in (True, False)})
    return _cache[key]


def both_paths(monkeypatch, fn):
    """fn() with the LDS tiles (default) and with SQ_SAMPLE_LDS=0, the direct gather; the switch is read per launch"""
    monkeypatch.delenv('SQ_SAMPLE_LDS', raising=False)
    a = fn()
    monkeypatch.setenv('SQ_SAMPLE_LDS', '0')
    b = fn()
    monkeypatch.delenv('SQ_SAMPLE_LDS', raising=False)
    return a, b


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
@pytest.mark.parametrize("brick,ops", sc.IMAGE_CASES, ids=lambda v: 'x'.join(map(str, v)) if len(v) == 3 else 'ops%d-%d' % (v[0], v[-1]))
def test_images_bit_exact(brick, ops, dtype, monkeypatch):
    vols, normed = volumes(sc.VOL_SHAPE, dtype)
    plan = sc.case_plan(sc.VOL_SHAPE, brick, ops, seed=brick[2])
    L = sc.VOL_SHAPE[1:]
    for a in range(3):                                          # the handcrafted rows hold both extreme origins
        assert 0 in plan[:, 1 + a] and max(L[a] - brick[a], 0) in plan[:, 1 + a]
    sm = VolumeSampler(L, brick, DEV)
    d, dplan = dev(vols), dev(plan)
    stats = volume_stats(d)
    for normalise in (True, False):
        ref = sc.np_images(vols, plan, brick, normalised=normed[normalise])
        lds, direct = both_paths(monkeypatch, lambda: sm.images(d, dplan, normalise=normalise).cpu().numpy())
        assert lds.shape == (len(plan),) + brick + (1,) and lds.dtype == np.float32
        assert_bit_exact(lds, ref, "%s %s normalise=%s" % (brick, np.dtype(dtype).name, normalise))
        assert_bit_exact(direct, ref, "%s %s normalise=%s, SQ_SAMPLE_LDS=0" % (brick, np.dtype(dtype).name, normalise))
    out = torch.full((len(plan),) + brick + (1,), float('nan'), device=DEV)
    assert sm.images(d, dplan, stats=stats, out=out) is out     # into a fixed buffer, with the caller's statistics
    assert_bit_exact(out.cpu().numpy(), sc.np_images(vols, plan, brick, normalised=normed[True]), "out=")


def test_more_than_one_lds_tile(monkeypatch):
    """bricks of 70 x 70 in the plane: four LDS tiles per plane, three of them partial; images, 3-byte voxels, one-hot"""
    shape, (brick, ops) = (1, 3, 80, 75), sc.BIG_TILE_CASE
    vols, normed = volumes(shape, np.uint16)
    plan = sc.case_plan(shape, brick, ops, seed=1)
    sm = VolumeSampler(shape[1:], brick, DEV)
    dplan = dev(plan)
    for got in both_paths(monkeypatch, lambda: sm.images(dev(vols), dplan).cpu().numpy()):
        assert_bit_exact(got, sc.np_images(vols, plan, brick, normalised=normed[True]), "images 70x70")
    rgb = np.random.default_rng(4).integers(0, 256, shape + (3,)).astype(np.uint8)
    for got in both_paths(monkeypatch, lambda: sm.copy(dev(rgb), dplan).cpu().numpy()):
        assert_bit_exact(got, sc.np_copy(rgb, plan, brick), "3-byte voxels 70x70")
    lab = np.random.default_rng(5).integers(0, 3, shape).astype(np.uint8)
    for got in both_paths(monkeypatch, lambda: sm.onehot(dev(lab), 2, dplan).cpu().numpy()):
        assert_bit_exact(got, sc.np_onehot(lab, 2, plan, brick), "one-hot 70x70")


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
def test_short_axis_fill_follows_the_flip(dtype):
    """Z = 5 under a brick of 8: the crop holds the volume in z 0 .. 4 and fill in 5 .. 7; after a z flip the fill is in
    0 .. 2.  Exactly 0.0 in both modes."""
    brick = (8, 16, 16)
    vols, normed = volumes(sc.SHORT_SHAPE, dtype)
    plan = sc.case_plan(sc.SHORT_SHAPE, brick, sc.ALL_OPS, seed=2)
    assert not plan[:, 1].any()
    sm = VolumeSampler(sc.SHORT_SHAPE[1:], brick, DEV)
    for normalise in (True, False):
        got = sm.images(dev(vols), dev(plan), normalise=normalise).cpu().numpy()
        assert_bit_exact(got, sc.np_images(vols, plan, brick, normalised=normed[normalise]), "short axis")
        flipped = (plan[:, 4] & 1).astype(bool)
        bits = got.view(np.uint32)
        assert not bits[flipped, :3].any() and not bits[~flipped, 5:].any()
        if normalise:
            assert np.all((got[flipped, 3:] != 0).mean((1, 2, 3, 4)) > 0.99)


@pytest.mark.parametrize("shape", [sc.VOL_SHAPE, sc.SHORT_SHAPE])
def test_op0_at_a_tilers_origins_is_the_tilers_brick(shape):
    brick = (8, 16, 16)
    tl = VolumeTiler(shape[1:], brick, (2, 4, 4), device=DEV)
    per = tl.bricks_per_volume
    plan = np.asarray([[k // per] + list(tl.geometry.box(k % per)[0]) + [0] for k in range(shape[0] * per)], np.int32)
    sm = VolumeSampler(shape[1:], brick, DEV)
    for dtype in (np.uint8, np.uint16, np.float32):
        d = dev(volumes(shape, dtype)[0])
        for normalise in (True, False):
            a, b = sm.images(d, dev(plan), normalise=normalise), tl.bricks(d, normalise=normalise)
            assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


COPY_SOURCES = {                                                # voxel bytes: dtype, trailing axis
    1: (np.uint8, ()), 2: (np.uint16, ()), 3: (np.uint8, (3,)), 4: (np.float32, (1,)), 8: (np.uint8, (8,))}


@pytest.mark.parametrize("nbytes", sorted(COPY_SOURCES))
@pytest.mark.parametrize("brick,ops", [sc.IMAGE_CASES[0], sc.IMAGE_CASES[1], sc.IMAGE_CASES[4]],
                         ids=['8x16x16-all', '8x16x18-flips', '3x17x17-transposed'])
def test_copy_is_verbatim(brick, ops, nbytes, monkeypatch):
    """voxels of 1, 2, 3, 4 and 8 bytes; 3 bytes with BY = 18 are 54-byte rows, no row but the first 16-byte aligned"""
    dtype, tail = COPY_SOURCES[nbytes]
    rng = np.random.default_rng(nbytes)
    shape = sc.VOL_SHAPE + tail
    src = rng.standard_normal(shape).astype(np.float32) if dtype == np.float32 else \
        rng.integers(1, np.iinfo(dtype).max, shape, endpoint=True).astype(dtype)
    plan = sc.case_plan(sc.VOL_SHAPE, brick, ops, seed=nbytes)
    sm = VolumeSampler(sc.VOL_SHAPE[1:], brick, DEV)
    ref = sc.np_copy(src, plan, brick)
    for got in both_paths(monkeypatch, lambda: sm.copy(dev(src), dev(plan)).cpu().numpy()):
        assert_bit_exact(got, ref, "%d-byte voxels, brick %s" % (nbytes, brick))
    out = dev(np.full(ref.shape, 7, ref.dtype))
    assert sm.copy(dev(src), dev(plan), out=out) is out
    assert_bit_exact(out.cpu().numpy(), ref, "out=")
    if nbytes == 4:                                             # other 4- and 8-byte types ride the same path
        for other in (src[..., 0], src.astype(np.float64)):
            assert_bit_exact(sm.copy(dev(other), dev(plan)).cpu().numpy(), sc.np_copy(other, plan, brick), str(other.dtype))


@pytest.mark.parametrize("C", [1, 2, 3])
@pytest.mark.parametrize("brick,ops", [sc.IMAGE_CASES[0], sc.IMAGE_CASES[1], sc.IMAGE_CASES[4]],
                         ids=['8x16x16-all', '8x16x18-flips', '3x17x17-transposed'])
def test_onehot_bit_exact(brick, ops, C, monkeypatch):
    """labels 0 .. 3 with C <= 3 classes: a label >= C is present and gives an all-zero voxel"""
    lab = np.random.default_rng(11).integers(0, 4, sc.VOL_SHAPE).astype(np.uint8)
    plan = sc.case_plan(sc.VOL_SHAPE, brick, ops, seed=C)
    sm = VolumeSampler(sc.VOL_SHAPE[1:], brick, DEV)
    ref = sc.np_onehot(lab, C, plan, brick)
    assert ref.shape == (len(plan),) + brick + (C,) and (ref.sum(-1) == 0).any() and set(np.unique(ref)) == {0, 1}
    for got in both_paths(monkeypatch, lambda: sm.onehot(dev(lab), C, dev(plan)).cpu().numpy()):
        assert_bit_exact(got, ref, "one-hot C=%d, brick %s" % (C, brick))
    out = torch.full(ref.shape, 9, dtype=torch.uint8, device=DEV)
    assert sm.onehot(dev(lab), C, dev(plan), out=out) is out
    assert_bit_exact(out.cpu().numpy(), ref, "out=")


def test_a_plan_that_points_outside_the_volumes_reads_fill(monkeypatch):
    """Negative origins, origins beyond the volume, v = V, v < 0 and coordinates at the ends of int32: the kernels form every
    coordinate in wrap-around arithmetic and compare it with the axis length before any load, so such rows are arithmetic
    on the guarded path: pure fill where the box lies outside, the restatement's padding where it straddles a face."""
    brick = (8, 16, 16)
    outside, straddle = sc.hostile_plan(sc.VOL_SHAPE, brick)
    plan = np.concatenate([outside, straddle])
    n = len(outside)
    vols, normed = volumes(sc.VOL_SHAPE, np.uint16)
    w = np.random.default_rng(1).standard_normal(sc.VOL_SHAPE + (1,)).astype(np.float32) + 3
    lab = np.random.default_rng(2).integers(0, 2, sc.VOL_SHAPE).astype(np.uint8)
    sm = VolumeSampler(sc.VOL_SHAPE[1:], brick, DEV)
    runs = [("images", lambda: sm.images(dev(vols), dev(plan)), sc.np_images(vols, plan, brick, normalised=normed[True])),
            ("raw images", lambda: sm.images(dev(vols), dev(plan), normalise=False),
             sc.np_images(vols, plan, brick, normalised=normed[False])),
            ("weights", lambda: sm.copy(dev(w), dev(plan)), sc.np_copy(w, plan, brick)),
            ("one-hot", lambda: sm.onehot(dev(lab), 2, dev(plan)), sc.np_onehot(lab, 2, plan, brick))]
    for what, fn, ref in runs:
        assert not ref[:n].any() and all(r.any() for r in ref[n:])
        for got in both_paths(monkeypatch, lambda: fn().cpu().numpy()):
            assert not got[:n].view(np.uint32 if got.dtype == np.float32 else got.dtype).any(), what
            assert_bit_exact(got, ref, what)
    torch.cuda.synchronize()


def test_errors_are_loud():
    shape, brick = (19, 37, 45), (8, 16, 16)
    sm = VolumeSampler(shape, brick, DEV)
    vols = torch.zeros((1,) + shape, dtype=torch.uint16, device=DEV)
    lab = torch.zeros((1,) + shape, dtype=torch.uint8, device=DEV)
    plan = torch.zeros((2, 5), dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.SequitrHipError):
        VolumeSampler(shape, brick, 'cpu')
    with pytest.raises(ValueError):
        VolumeSampler(shape, (8, 16), DEV)
    for call in (lambda: sm.images(vols.cpu(), plan), lambda: sm.images(vols, plan.cpu()), lambda: sm.copy(lab.cpu(), plan),
                 lambda: sm.onehot(lab.cpu(), 2, plan), lambda: sm.onehot(lab, 2, plan.cpu()),
                 lambda: sm.images(vols, plan, out=torch.zeros((2,) + brick + (1,)))):
        with pytest.raises(_lib.SequitrHipError, match='no CPU fallback'):
            call()
    bad = [lambda: sm.images(vols.to(torch.float64), plan),                             # wrong voxel type
           lambda: sm.images(lab.to(torch.int16), plan),
           lambda: sm.onehot(vols, 2, plan),                                             # labels are uint8
           lambda: sm.images(torch.zeros((1, 19, 45, 37), dtype=torch.uint8, device=DEV).transpose(2, 3), plan),   # non-contiguous
           lambda: sm.copy(torch.zeros((1, 19, 45, 37), device=DEV).transpose(2, 3), plan),
           lambda: sm.images(torch.zeros((1, 19, 37, 46), dtype=torch.uint8, device=DEV), plan),                   # not the sampler's shape
           lambda: sm.onehot(lab[0], 2, plan),
           lambda: sm.images(vols, torch.zeros((2, 4), dtype=torch.int32, device=DEV)),                            # plan of the wrong shape
           lambda: sm.images(vols, torch.zeros(10, dtype=torch.int32, device=DEV)),
           lambda: sm.images(vols, torch.zeros((2, 5), dtype=torch.int64, device=DEV)),
           lambda: sm.images(vols, torch.zeros((2, 10), dtype=torch.int32, device=DEV)[:, ::2]),
           lambda: sm.images(vols, torch.zeros((0, 5), dtype=torch.int32, device=DEV)),
           lambda: sm.images(vols, torch.zeros((65536, 5), dtype=torch.int32, device=DEV)),                        # more than one launch
           lambda: sm.copy(lab, torch.zeros((65536, 5), dtype=torch.int32, device=DEV)),
           lambda: sm.onehot(lab, 2, torch.zeros((65536, 5), dtype=torch.int32, device=DEV)),
           lambda: sm.onehot(lab, 0, plan), lambda: sm.onehot(lab, 17, plan),
           lambda: sm.copy(torch.zeros((1,) + shape + (5,), dtype=torch.uint8, device=DEV), plan),                 # 5-byte voxels
           lambda: sm.copy(torch.zeros((1,) + shape + (3,), device=DEV), plan),                                    # 12-byte voxels
           lambda: sm.images(vols, plan, out=torch.zeros((2,) + brick, device=DEV)),                               # out of the wrong shape
           lambda: sm.onehot(lab, 2, plan, out=torch.zeros((2,) + brick + (2,), device=DEV)),                      # ... and type
           lambda: sm.images(vols, plan, stats=(torch.zeros(2, device=DEV), torch.ones(2, device=DEV)))]           # stats of 2 volumes
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("call %d was accepted" % i)
    # the Python layer never sends bit 3 for a brick that is not square: the transpose bit of such a row is ignored
    rect = VolumeSampler(shape, (8, 16, 18), DEV)
    v = dev(vc.random_volume((1,) + shape, np.uint8, seed=1))
    p8 = dev(np.asarray([[0, 3, 4, 5, 8 | 5]], np.int32))
    p0 = dev(np.asarray([[0, 3, 4, 5, 5]], np.int32))
    assert torch.equal(rect.images(v, p8, normalise=False), rect.images(v, p0, normalise=False))


def test_train_volume_job_with_bricks_then_segment(tmp_path, monkeypatch):
    """SERVER_train_volume in brick mode on a (2, 20, 40, 48) uint16 stack, then SERVER_segment_volume with the saved model
    and the same brick.

    The job's first loss is compared BIT FOR BIT with the loss of one step of a fresh UNetTrainer (the job's network
    parameters and seed) on the first batch restated in numpy: the plan's first two rows from the seeded generator, the
    images normalised and cut by tests/volume_sampler_cases, the labels expanded there, and the weight map the job is
    specified to use -- device_weightmaps3d of the whole volumes -- cropped there.  The first loss involves the forward pass
    and the loss kernel only.  Whether bit-for-bit is the right demand is established first: two fresh trainers on that
    batch must reproduce each other bit for bit."""
    from sequitr_amd import core, jobs, utils
    from sequitr_amd.networks.unet import UNet3D, UNet3DTrain
    from sequitr_amd.train import UNetTrainer
    from sequitr_amd.weightmap import device_weightmaps3d
    monkeypatch.setattr(core.TensorflowConfiguration, "MODELDIR", str(tmp_path / "models"))
    for d in ("models", "out_t", "out_s"):
        os.mkdir(str(tmp_path / d))
    shape, brick_xyz, brick = (2, 20, 40, 48), (32, 32, 16), (16, 32, 32)
    rng = np.random.default_rng(0)
    zz, xx, yy = np.mgrid[0:20, 0:40, 0:48]
    lab = np.zeros(shape, np.uint8)
    lab[0][(zz - 8) ** 2 * 4 + (xx - 15) ** 2 + (yy - 17) ** 2 < 90] = 1
    lab[0][(zz - 12) ** 2 * 4 + (xx - 30) ** 2 + (yy - 36) ** 2 < 60] = 1
    lab[1][(zz - 10) ** 2 * 4 + (xx - 22) ** 2 + (yy - 28) ** 2 < 120] = 1
    imgs = (400 + lab * 900.0 + rng.standard_normal(shape) * 150).clip(0, 65535).astype(np.uint16)
    np.save(str(tmp_path / "im.npy"), imgs)
    np.save(str(tmp_path / "lab.npy"), lab)
    net_keys = {"filters": (16, 32, 64), "dropout": 0.0, "num_outputs": 2, "seed": 5}
    params = dict(net_keys, images=str(tmp_path / "im.npy"), labels=str(tmp_path / "lab.npy"), brick=brick_xyz, batch_size=2,
                  weightmap="edt", num_epochs=2, output=str(tmp_path / "out_t"))
    info = jobs.SERVER_train_volume(params, {"gpu": 0, "max_steps": 3})
    tj = json.load(open(str(tmp_path / "out_t" / "train.json")))
    per = volume_bricks(shape[1:], brick, 0).per_volume
    assert per == 8
    assert info["steps"] == 3 and len(tj["losses"]) == 3 and np.isfinite(tj["losses"]).all()
    assert tj["brick"] == [32, 32, 16] and tj["augment"] == ["flip", "rot90"] and tj["samples_per_epoch"] == 2 * per
    assert tj["seed"] == 5 and tj["batch_size"] == 2 and tj["volumes"] == 2 and tj["shape"] == [20, 40, 48]
    assert tj["weightmap"] == "edt"
    cfg = json.load(open(os.path.join(info["model_dir"], "net.config")))["NetConfiguration"]
    assert tuple(cfg["shape"]) == brick_xyz and cfg["num_inputs"] == 1
    weights = utils.load_model_weights(info["model_dir"])
    net = UNet3D(dict(net_keys, shape=brick_xyz, device=DEV), "infer")
    net.load_state_dict(weights, strict=True)

    seg = {"input": str(tmp_path / "im.npy"), "model": info["model_dir"], "brick": brick_xyz, "filters": (16, 32, 64),
           "num_outputs": 2, "output": str(tmp_path / "out_s")}
    sinfo = jobs.SERVER_segment_volume(seg, {"gpu": 0})
    assert sinfo["volumes"] == 2 and sinfo["bricks_per_volume"] == per
    mask = np.load(str(tmp_path / "out_s" / "mask.npy"))
    assert mask.shape == shape and mask.dtype == np.uint8
    ref_mask, _ = segment_volumes(net, imgs, brick, 0)
    assert np.array_equal(mask, ref_mask)

    # the first batch, restated
    plan = sample_plan(shape[1:], brick, 2, 2 * per, np.random.default_rng(5), ("flip", "rot90"))[:2]
    wmap = device_weightmaps3d(lab, 10., 5., 1., device=DEV).cpu().numpy()
    assert wmap.shape == shape + (1,)
    batch = [dev(sc.np_images(imgs, plan, brick)), dev(sc.np_onehot(lab, 2, plan, brick)), dev(sc.np_copy(wmap, plan, brick))]
    net_p = dict(net_keys, shape=brick_xyz, num_inputs=1, device=DEV)
    fresh = [float(UNetTrainer(net_p, net_cls=UNet3DTrain).step(*batch).cpu()) for _ in range(2)]
    print("first loss: job %r, fresh trainers %r" % (tj["losses"][0], fresh))
    assert np.float32(fresh[0]).tobytes() == np.float32(fresh[1]).tobytes(), fresh
    assert np.float32(tj["losses"][0]).tobytes() == np.float32(fresh[0]).tobytes(), (tj["losses"][0], fresh)
