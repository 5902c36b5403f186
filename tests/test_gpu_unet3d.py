"""GPU: the whole UNet3D against an oracle composed here from the planar C oracle (stacked conv2d, numpy 2x2x2 max,
per-parity transpose conv, the 1x1 head and argmax), bit for bit, for every bridge type and with batch norm; model I/O;
and jobs.SERVER_segment_volume through worker()."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

from oracle import c_oracle
from sequitr_amd import worker
from sequitr_amd.networks.unet import UNet3D, init_unet3d_weights, init_unet_weights
from tests import conv3d_cases as cc
from tests.test_jobs_config import write_job
from tests.util import assert_bit_exact

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FILTERS = (16, 32, 64, 128, 256)


def unet3d_ref(x, w, bridge='eltwise_mul', batch_norm=False, eps=1e-3):
    """x (N, D, H, W, C) -> (logits, mask) of the reference wiring (unet.py:224-262) on the oracle ops"""
    def conv(t, s):
        y = cc.conv3d_ref(t, w[s + '/kernel'], w[s + '/bias'], act=None if batch_norm else 'relu')
        if batch_norm:
            sc, sh = c_oracle.bn_fold(w[s + '/gamma'], w[s + '/beta'], w[s + '/moving_mean'], w[s + '/moving_variance'], eps)
            y = c_oracle.bn_apply(y, sc, sh, act='relu')
        return y

    net = []
    t = x
    for i in range(len(FILTERS)):
        if i:
            t = cc.maxpool3d_ref(net[-1])
        t = conv(conv(t, 'UNet/down%d/conv1' % i), 'UNet/down%d/conv2' % i)
        net.append(t)
    for i in reversed(range(len(FILTERS) - 1)):
        s = 'UNet/up%d' % i
        eltwise = bridge in ('eltwise_add', 'eltwise_mul', 'eltwise_sub')
        up = cc.convT3d_ref(net[-1], w[s + '/upscale/kernel'], w[s + '/upscale/bias'], net[i] if eltwise else None,
                            bridge if eltwise else None)
        if bridge == 'concat':
            up = np.ascontiguousarray(np.concatenate([up, net[i]], -1))
        net.append(conv(conv(up, s + '/conv1'), s + '/conv2'))
    N, D, H, W, C = net[-1].shape
    wh = w['UNet/to_image/kernel']
    logits = c_oracle.conv2d(net[-1].reshape(N * D, H, W, C), wh.reshape(1, 1, C, wh.shape[-1]), w['UNet/to_image/bias'])
    logits = logits.reshape(N, D, H, W, -1)
    return logits, c_oracle.argmax_u8(logits)


def _weights(params, seed, batch_norm=False):
    w = init_unet3d_weights(params, seed)
    rng = np.random.default_rng(seed + 100)
    for k in list(w):
        if k.endswith('/bias'):                                 # non-zero biases: the bias path is part of the check
            w[k] = (0.05 * rng.standard_normal(w[k].shape)).astype(np.float32)
        if batch_norm and k.endswith('/gamma'):
            sc, n = k.rsplit('/', 1)[0], w[k].shape[0]
            w[k] = (1 + 0.1 * rng.standard_normal(n)).astype(np.float32)
            w[sc + '/beta'] = (0.1 * rng.standard_normal(n)).astype(np.float32)
            w[sc + '/moving_mean'] = (0.1 * rng.standard_normal(n)).astype(np.float32)
            w[sc + '/moving_variance'] = (0.5 + rng.random(n)).astype(np.float32)
    return w


@pytest.mark.parametrize("bridge,batch_norm,vol", [
    ('eltwise_mul', False, (2, 16, 64, 64)), ('eltwise_add', False, (2, 16, 32, 32)), ('eltwise_sub', False, (2, 16, 32, 32)),
    ('concat', False, (2, 16, 32, 32)), (None, False, (1, 16, 32, 32)), ('eltwise_mul', True, (1, 16, 32, 32))])
def test_unet3d_bit_exact(bridge, batch_norm, vol):
    N, D, H, W = vol
    params = {'shape': (H, W, D), 'num_outputs': 2, 'bridge': bridge, 'batch_norm': batch_norm, 'device': DEV}
    w = _weights(params, seed=len(str(bridge)) + batch_norm, batch_norm=batch_norm)
    x = np.random.default_rng(N + H).standard_normal((N, D, H, W, 1)).astype(np.float32)
    net = UNet3D(params, 'infer')
    net.load_state_dict(w)
    mask = net.predict(x)
    logits = net.logits()
    assert tuple(mask.shape) == (N, D, H, W) and mask.dtype == torch.uint8
    ref_logits, ref_mask = unet3d_ref(x, w, bridge, batch_norm)
    assert_bit_exact(logits.cpu().numpy(), ref_logits, "UNet3D logits (%s, bn=%s)" % (bridge, batch_norm))
    assert_bit_exact(mask.cpu().numpy(), ref_mask, "UNet3D mask")


def test_save_and_strict_load_and_2d_checkpoint_refused():
    params = {'shape': (32, 32, 16), 'num_outputs': 2, 'seed': 5, 'device': DEV}
    x = np.random.default_rng(2).standard_normal((1, 16, 32, 32)).astype(np.float32)    # (N, slices, width, height)
    a = UNet3D(params).initialize()
    m1 = a.predict(x).cpu().numpy()
    sd = a.state_dict()
    b = UNet3D(dict(params, seed=99))
    b.load_state_dict(sd)
    assert np.array_equal(b.predict(x).cpu().numpy(), m1)
    with pytest.raises(ValueError, match='shape mismatches'):
        UNet3D(params).load_state_dict(init_unet_weights({'shape': (32, 32)}, 0))


def test_segment_volume_job(tmp_path):
    from sequitr_amd import jobs
    from sequitr_amd.centroids import mask_centroids
    params = {'input': {'synthetic': True, 'volumes': 2, 'seed': 4}, 'shape': (32, 32, 16), 'num_outputs': 2, 'seed': 3}
    fn = write_job(tmp_path, func="SERVER_segment_volume", params=repr(params),
                   options="{'gpu': 0, 'save_logits': True, 'centroids': True}")
    out = str(tmp_path / "out")
    worker.worker(argparse.Namespace(job=fn, out=out))
    logs = open(os.path.join(out, [f for f in os.listdir(out) if f.startswith("LOG_")][0])).read()
    assert "exception" not in logs, logs
    mask, logits = np.load(os.path.join(out, "mask.npy")), np.load(os.path.join(out, "logits.npy"))
    assert mask.shape == (2, 16, 32, 32) and mask.dtype == np.uint8 and logits.shape == (2, 16, 32, 32, 2)
    x = jobs._load_volumes(params)
    net = UNet3D({'shape': (32, 32, 16), 'num_outputs': 2, 'seed': 3, 'device': DEV}).initialize()
    for i in range(2):
        assert_bit_exact(mask[i], net.predict(x[i:i + 1])[0].cpu().numpy(), "job mask %d" % i)
        assert_bit_exact(logits[i], net.logits()[0].cpu().numpy(), "job logits %d" % i)
    info = json.load(open(os.path.join(out, "segment_volume.json")))
    assert info['volumes'] == 2 and info['mvoxels_per_s'] > 0 and info['setup_seconds'] >= 0
    # centroids: mask_centroids of the (N, Z, X, Y) mask as CentroidWriter.write sees it (axes 1 and 3 swapped)
    ref = mask_centroids(torch.from_numpy(mask).to(DEV).transpose(1, 3).contiguous())
    assert info['centroids']['objects'] == sum(len(r) for r in ref) > 0
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
