"""GPU volume front end vs numpy (tests/volume_frontend_cases.py): per-volume ImageNorm statistics and bricks BIT-EXACT,
the scatter of masks and logits, the streamed whole-volume path against the per-brick CPU oracle, its tie to
UNet3D.predict, and SERVER_segment_volume's brick mode through worker()."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

from sequitr_amd import worker
from sequitr_amd.frontend import VolumeTiler, segment_volumes, volume_bricks, volume_stats
from sequitr_amd.networks.unet import UNet3D, init_unet3d_weights
from tests import test_gpu_unet3d as t3
from tests import volume_frontend_cases as vc
from tests.test_jobs_config import write_job
from tests.util import assert_bit_exact

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BRICK, MARGIN = (8, 16, 16), (2, 4, 4)
E2E_FILTERS = (16, 32)
E2E_PARAMS = {'shape': (16, 16, 8), 'filters': E2E_FILTERS, 'num_outputs': 2, 'seed': 6}
_cache = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def batches(total, n=7):
    return [(first, min(n, total - first)) for first in range(0, total, n)]


@pytest.mark.parametrize("shape,dtype", vc.STATS_SHAPES + [((2, 9, 33, 130), np.uint8)])
def test_volume_stats_bit_exact(shape, dtype):
    """the five shapes of the CPU test, which ties the helper to np.mean / np.std, and two volumes kept apart; the
    17 039 295-voxel case is the one where only the double division equals numpy"""
    vols = vc.random_volume(shape if len(shape) == 4 else (1,) + shape, dtype, seed=shape[-2])
    tl = VolumeTiler(vols.shape[1:], vols.shape[1:], 0, device=DEV)
    mean, std = tl.stats(dev(vols))
    assert mean.dtype == torch.float32 and tuple(mean.shape) == tuple(std.shape) == (len(vols),)
    mean, std = mean.cpu().numpy(), std.cpu().numpy()
    for v in range(len(vols)):
        ref_mean, ref_std = vc.np_stats(vols[v])
        assert_bit_exact(mean[v], ref_mean, "mean of volume %d" % v)
        assert_bit_exact(std[v], ref_std, "std of volume %d" % v)


def test_volume_stats_past_2_31_voxels():
    """A uint8 volume of 2^31 + 16390 voxels, 1 in its first half and 3 in its second, made on the device: an element
    offset that wrapped at 32 bits would sum the wrong half.  The reference is the stated definition evaluated chunk by
    chunk: a chunk of the volume is all 1, all 3, the one mixed chunk or the ragged tail, each summed by the helper."""
    n = (1 << 31) + 2 * vc.CHUNK + 6
    half, nchunks = n // 2, (n + vc.CHUNK - 1) // vc.CHUNK
    vol = torch.ones(n, dtype=torch.uint8, device=DEV)
    vol[half:] = 3
    mean, std = volume_stats(vol.view(1, n))
    mixed = np.where(np.arange(vc.CHUNK) < half % vc.CHUNK, 1, 3).astype(np.float32)
    kinds = {1: np.full(vc.CHUNK, 1, np.float32), 3: np.full(vc.CHUNK, 3, np.float32), 'mixed': mixed,
             'tail': np.full(n % vc.CHUNK, 3, np.float32)}
    which = [1] * (half // vc.CHUNK) + ['mixed'] + [3] * (nchunks - half // vc.CHUNK - 2) + ['tail']
    assert len(which) == nchunks

    def total(f):
        sums = {k: vc.chunked_sum(f(a)) for k, a in kinds.items()}
        res = np.float32(0)
        for k in which:
            res = np.float32(res + sums[k])
        return np.float32(np.float64(res) / np.float64(n))

    ref_mean = total(lambda a: a)
    ref_std = np.sqrt(total(lambda a: (a - ref_mean) * (a - ref_mean)))
    assert_bit_exact(mean.cpu().numpy()[0], ref_mean, "mean")
    assert_bit_exact(std.cpu().numpy()[0], ref_std, "std")
    assert abs(float(ref_mean) - 2) < 1e-3 and abs(float(ref_std) - 1) < 1e-3


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
@pytest.mark.parametrize("shape", [(2, 19, 37, 45), (1, 5, 37, 16)])
def test_bricks_bit_exact(shape, dtype):
    vols = vc.random_volume(shape, dtype, seed=3)
    tl = VolumeTiler(shape[1:], BRICK, MARGIN, device=DEV)
    assert tl.geometry.counts == ((4, 4, 5) if shape[1] == 19 else (1, 4, 1))
    total = shape[0] * tl.bricks_per_volume
    d = dev(vols)
    for normalise in (True, False):
        ref = vc.np_bricks(vols, tl.geometry, normalise)
        got = tl.bricks(d, normalise=normalise)
        assert tuple(got.shape) == (total,) + BRICK + (1,) and got.dtype == torch.float32
        assert_bit_exact(got.cpu().numpy(), ref, "all bricks, normalise=%s" % normalise)
        stats = tl.stats(d) if normalise else None
        for first, count in batches(total):                     # first / count, ragged last batch
            got = tl.bricks(d, first, count, normalise=normalise, stats=stats)
            assert_bit_exact(got.cpu().numpy(), ref[first:first + count], "bricks %d..+%d" % (first, count))
        if shape[1] < BRICK[0]:                                 # padded: the fill is exactly 0.0 in both modes
            assert np.all(got.cpu().numpy().view(np.uint32)[:, shape[1]:] == 0)


@pytest.mark.parametrize("shape", [(2, 19, 37, 45), (1, 5, 37, 16)])
def test_scatter_masks_and_logits(shape):
    """Y = 45 with C = 3 (and C = 1, 2): owned y runs and destination offsets that are no multiples of 4 or 16 elements,
    so rows start with a scalar head, run through 16-byte stores and end in a scalar tail"""
    tl = VolumeTiler(shape[1:], BRICK, MARGIN, device=DEV)
    g = tl.geometry
    total = shape[0] * tl.bricks_per_volume
    rng = np.random.default_rng(5)
    masks = rng.integers(0, 200, (total,) + BRICK).astype(np.uint8)
    out = torch.full(shape, 255, dtype=torch.uint8, device=DEV)
    for first, count in reversed(batches(total)):               # batches in any order
        assert tl.scatter(dev(masks[first:first + count]), out, first) is out
    ref = vc.np_scatter(masks, np.full(shape, 255, np.uint8), g)
    assert not np.any(ref == 255) and np.array_equal(out.cpu().numpy(), ref)
    for C in (2, 3):
        logits = rng.standard_normal((total,) + BRICK + (C,)).astype(np.float32)
        out = torch.full(shape + (C,), float('nan'), dtype=torch.float32, device=DEV)
        for first, count in batches(total):
            tl.scatter(dev(logits[first:first + count]), out, first)
        got = out.cpu().numpy()
        assert not np.isnan(got).any()                          # no sentinel survives
        assert_bit_exact(got, vc.np_scatter(logits, np.empty(shape + (C,), np.float32), g), "logits, C=%d" % C)


@pytest.mark.parametrize("shape", [(2, 19, 37, 45), (1, 5, 37, 16)])
def test_raw_bricks_scattered_back_are_the_volume(shape):
    idx = np.arange(int(np.prod(shape)), dtype=np.float32).reshape(shape) % 65521
    tl = VolumeTiler(shape[1:], BRICK, MARGIN, device=DEV)
    bricks = tl.bricks(dev(idx), normalise=False)
    out = torch.full(shape + (1,), -1.0, dtype=torch.float32, device=DEV)
    tl.scatter(bricks, out)
    assert np.array_equal(out.cpu().numpy()[..., 0], idx)
    as_u8 = dev((idx % 251).astype(np.uint8))
    masks = tl.bricks(as_u8, normalise=False).to(torch.uint8).reshape((-1,) + BRICK).contiguous()
    assert torch.equal(tl.scatter(masks, torch.full(shape, 255, dtype=torch.uint8, device=DEV)), as_u8)


def e2e():
    """two uint16 volumes, the network, and the reference: numpy cutter -> CPU oracle per brick -> numpy scatter"""
    if not _cache:
        vols = np.random.default_rng(8).integers(100, 4000, (2, 11, 26, 37)).astype(np.uint16)
        params = dict(E2E_PARAMS, device=DEV)
        w = init_unet3d_weights(params, 4)
        net = UNet3D(params, 'infer')
        net.load_state_dict(w)
        g = volume_bricks(vols.shape[1:], BRICK, MARGIN)
        assert g.counts == (2, 3, 4)
        filters, t3.FILTERS = t3.FILTERS, E2E_FILTERS            # unet3d_ref reads its module's FILTERS
        try:
            logits, masks = t3.unet3d_ref(vc.np_bricks(vols, g), w)
        finally:
            t3.FILTERS = filters
        ref_masks = vc.np_scatter(masks, np.full(vols.shape, 255, np.uint8), g)
        ref_logits = vc.np_scatter(logits, np.full(vols.shape + (2,), np.nan, np.float32), g)
        _cache.update(vols=vols, net=net, ref_masks=ref_masks, ref_logits=ref_logits)
    return _cache


def test_segment_volumes_matches_per_brick_oracle():
    c = e2e()
    masks, logits = segment_volumes(c['net'], c['vols'], BRICK, MARGIN, bricks_per_batch=5, want_logits=True)
    assert_bit_exact(logits, c['ref_logits'], "streamed logits")
    assert_bit_exact(masks, c['ref_masks'], "streamed masks")
    seen = []
    none, logits = segment_volumes(c['net'], c['vols'], BRICK, MARGIN, bricks_per_batch=5,
                                   on_masks=lambda i, m: seen.append((i, tuple(m.shape), m.cpu().numpy()[0])))
    assert none is None and logits is None
    assert [s[0] for s in seen] == [0, 1] and all(s[1] == (1, 11, 26, 37) for s in seen)
    assert np.array_equal(np.stack([s[2] for s in seen]), c['ref_masks'])


def test_one_brick_is_predict():
    """brick = the volume, margin 0, no normalisation: the front end adds nothing to net.predict / net.logits()"""
    params = {'shape': (32, 32, 16), 'num_outputs': 2, 'seed': 3, 'device': DEV}
    net = UNet3D(params).initialize()
    x = np.random.default_rng(2).standard_normal((2, 16, 32, 32)).astype(np.float32)
    masks, logits = segment_volumes(net, x, (16, 32, 32), 0, normalise=False, want_logits=True)
    for i in range(2):
        assert_bit_exact(masks[i], net.predict(x[i:i + 1])[0].cpu().numpy(), "mask %d" % i)
        assert_bit_exact(logits[i], net.logits()[0].cpu().numpy(), "logits %d" % i)


def test_segment_volume_job_with_bricks(tmp_path):
    from sequitr_amd.centroids import mask_centroids
    c = e2e()
    src = str(tmp_path / "vols.npy")
    np.save(src, c['vols'])
    params = dict(E2E_PARAMS, input=src, brick=(16, 16, 8), margin=(4, 4, 2), bricks_per_batch=5)
    del params['shape']
    fn = write_job(tmp_path, func="SERVER_segment_volume", params=repr(params),
                   options="{'gpu': 0, 'save_logits': True, 'centroids': True}")
    out = str(tmp_path / "out")
    worker.worker(argparse.Namespace(job=fn, out=out))
    logs = open(os.path.join(out, [f for f in os.listdir(out) if f.startswith("LOG_")][0])).read()
    assert "exception" not in logs, logs
    net = UNet3D(dict(E2E_PARAMS, device=DEV)).initialize()     # the job's network: seeded initial weights
    ref_masks, ref_logits = segment_volumes(net, c['vols'], BRICK, MARGIN, bricks_per_batch=5, want_logits=True)
    mask, logits = np.load(os.path.join(out, "mask.npy")), np.load(os.path.join(out, "logits.npy"))
    assert_bit_exact(mask, ref_masks, "job mask")
    assert_bit_exact(logits, ref_logits, "job logits")
    info = json.load(open(os.path.join(out, "segment_volume.json")))
    assert info['volumes'] == 2 and info['shape'] == [11, 26, 37] and info['mvoxels_per_s'] > 0
    assert info['brick'] == [16, 16, 8] and info['margin'] == [4, 4, 2] and info['bricks_per_volume'] == 24
    ref = mask_centroids(torch.from_numpy(mask).to(DEV).transpose(1, 3).contiguous())
    for i, r in enumerate(ref):
        r[:, 0] = i
    assert info['centroids']['objects'] == sum(len(r) for r in ref)
    f = os.path.join(out, info['centroids']['file'])
    if f.endswith('.npz'):
        z = np.load(f)
        got = [z['frames/frame_%d/coords' % i] for i in range(2)]
    else:
        import h5py
        with h5py.File(f, 'r') as h:
            got = [h['frames/frame_%d/coords' % i][()] for i in range(2)]
    for g, r in zip(got, ref):
        assert np.array_equal(g, r)


def test_errors_are_loud():
    tl = VolumeTiler((19, 37, 45), BRICK, MARGIN, device=DEV)
    ok = torch.zeros((1, 19, 37, 45), dtype=torch.uint8, device=DEV)
    with pytest.raises(Exception):
        tl.bricks(torch.zeros((1, 19, 37, 45), dtype=torch.uint8))                       # CPU tensor
    with pytest.raises(ValueError):
        tl.stats(torch.zeros((1, 19, 37, 45), dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        tl.bricks(torch.zeros((1, 19, 37, 46), dtype=torch.uint8, device=DEV))           # not the tiler's shape
    with pytest.raises(ValueError):
        tl.bricks(torch.zeros((1, 19, 45, 37), dtype=torch.uint8, device=DEV).transpose(2, 3))   # non-contiguous
    with pytest.raises(ValueError):
        tl.bricks(ok, first=75, count=7)                                                 # past the last brick
    with pytest.raises(ValueError):
        tl.scatter(torch.zeros((3,) + BRICK, dtype=torch.uint8, device=DEV), torch.zeros((1, 19, 37, 45, 1), device=DEV))
    with pytest.raises(ValueError):
        VolumeTiler((19, 37, 45), BRICK, (2, 8, 4), device=DEV)                          # margin too large
    with pytest.raises(TypeError):
        segment_volumes(None, np.zeros((1, 8, 16, 16), np.float64), BRICK)
