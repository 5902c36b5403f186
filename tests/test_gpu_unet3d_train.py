"""GPU: f32 training of the volumetric U-Net (functional.conv3d / maxpool2x2x2 / convT2x2x2s2, networks.unet.UNet3DTrain,
train.UNetTrainer, jobs.SERVER_train_volume) against a torch-CPU fp64 restatement of the same graph
(tests/unet3d_torch_ref.py).  Tolerances: a short functional chain within 1e-5 of max |ref| (the tolerance of
test_gpu_train.py::test_functional_conv_chain_backward); the whole net's loss within 1e-5 relative and every gradient
within max(1e-3, 4 * err32) of max |ref|, err32 being the torch-CPU f32 vs fp64 difference on the same graph (the rule of
test_unet_training_forward_backward_vs_fp64: measured on the reference, never on the kernels)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from sequitr_amd import functional as F
from sequitr_amd.networks.unet import UNet3D, UNet3DTrain, init_unet3d_weights
from sequitr_amd.train import UNetTrainer
from tests import unet3d_torch_ref as r3
from tests.test_gpu_train import close, dev
from tests.util import rand_weights

pytestmark = pytest.mark.gpu


def vol(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def test_functional_volume_chain_backward():
    """autograd through conv3d(relu) -> pool -> conv3d(relu) -> convT -> bridge(mul) -> conv3d vs fp64"""
    x, skip = vol(1, 2, 4, 12, 20, 16), vol(2, 2, 4, 12, 20, 16)
    p = {"w1": rand_weights(3, (3, 3, 3, 16, 32)), "b1": rand_weights(4, (32,), 0.1),
         "w2": rand_weights(5, (3, 3, 3, 32, 32)), "b2": rand_weights(6, (32,), 0.1),
         "wt": rand_weights(7, (2, 2, 2, 16, 32), 0.2), "bt": rand_weights(8, (16,), 0.1),
         "w3": rand_weights(9, (3, 3, 3, 16, 16)), "b3": rand_weights(10, (16,), 0.1)}
    cot = vol(11, 2, 4, 12, 20, 16)
    g = {k: dev(v).requires_grad_(True) for k, v in p.items()}
    xs, sk = dev(x).requires_grad_(True), dev(skip).requires_grad_(True)
    h = F.conv3d(xs, g["w1"], g["b1"], act="relu")
    h = F.maxpool2x2x2(h)
    h = F.conv3d(h, g["w2"], g["b2"], act="relu")
    h = F.convT2x2x2s2(h, g["wt"], g["bt"])
    h = F.bridge(h, sk, "eltwise_mul")
    z = F.conv3d(h, g["w3"], g["b3"], act=None)
    (z * dev(cot)).sum().backward()

    q = {k: torch.as_tensor(v, dtype=torch.float64).requires_grad_(True) for k, v in p.items()}
    xr, sr = r3.to_ncdhw(x).requires_grad_(True), r3.to_ncdhw(skip).requires_grad_(True)
    hr = TF.relu(TF.conv3d(xr, q["w1"].permute(4, 3, 0, 1, 2), q["b1"], padding=1))
    hr = TF.max_pool3d(hr, 2, 2)
    hr = TF.relu(TF.conv3d(hr, q["w2"].permute(4, 3, 0, 1, 2), q["b2"], padding=1))
    hr = TF.conv_transpose3d(hr, q["wt"].permute(4, 3, 0, 1, 2), q["bt"], stride=2)
    hr = hr * sr
    zr = TF.conv3d(hr, q["w3"].permute(4, 3, 0, 1, 2), q["b3"], padding=1)
    (zr * r3.to_ncdhw(cot)).sum().backward()
    close(z.detach().cpu().numpy(), r3.to_ndhwc_np(zr.detach()), 1e-5, "fwd")
    for k in p:
        close(g[k].grad.cpu().numpy(), q[k].grad.numpy(), 1e-5, k)
    close(xs.grad.cpu().numpy(), r3.to_ndhwc_np(xr.grad), 1e-5, "dx")
    close(sk.grad.cpu().numpy(), r3.to_ndhwc_np(sr.grad), 1e-5, "dskip")


def _batch(seed, n, shape=(32, 32, 16)):
    X, Y, Z = shape
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, Z, X, Y, 1)).astype(np.float32)
    lab = rng.random((n, Z, X, Y)) < 0.3
    onehot = np.stack([~lab, lab], -1).astype(np.uint8)
    wmap = (1 + 9 * rng.random((n, Z, X, Y, 1))).astype(np.float32)
    return x, onehot, wmap


@pytest.mark.parametrize("cfg", [{"bridge": "eltwise_mul"}, {"bridge": "eltwise_add"}, {"bridge": "concat"},
                                 {"bridge": "eltwise_mul", "batch_norm": True}],
                         ids=["mul", "add", "concat", "mul-batch_norm"])
def test_unet3d_training_forward_backward_vs_fp64(cfg):
    params = dict({"shape": (32, 32, 16), "dropout": 0.0, "device": "cuda:0", "seed": 2}, **cfg)
    x, onehot, wmap = _batch(0, 2)
    t = UNetTrainer(params, net_cls=UNet3DTrain)
    w0 = t.state_dict()
    init = init_unet3d_weights(params, 2)
    assert all(np.array_equal(w0[k], v) for k, v in init.items())
    loss = t.forward_backward(dev(x), dev(onehot), dev(wmap))
    train_w = {k: w0[k] for k in init}
    rloss, rgrads, _ = r3.unet3d_loss_and_grads(x, onehot, wmap, train_w, params)
    print("loss %.9g vs fp64 %.9g" % (loss.item(), rloss))
    assert abs(loss.item() - rloss) <= 1e-5 * abs(rloss)
    g = t.grads()
    _, fgrads, _ = r3.unet3d_loss_and_grads(x, onehot, wmap, train_w, params, dtype=torch.float32)
    assert set(g) == set(rgrads)
    for k in rgrads:
        scale = max(float(np.max(np.abs(rgrads[k]))), 1e-30)
        err32 = float(np.max(np.abs(fgrads[k].astype(np.float64) - rgrads[k]))) / scale
        got = float(np.max(np.abs(g[k].astype(np.float64) - rgrads[k]))) / scale
        print("%-28s err %.3g  torch-f32 err %.3g" % (k, got, err32))
        if params.get("batch_norm") and k.endswith("/bias") and "to_image" not in k and "upscale" not in k:
            # the batch mean removes a conv's bias: its exact gradient is 0 (fp64 leaves ~1e-18), so "of max |ref|" has
            # no meaning for it; the absolute floor of test_gpu_batchnorm.py::test_unet_training_with_batchnorm_vs_fp64
            assert float(np.max(np.abs(rgrads[k]))) < 1e-12 and float(np.max(np.abs(g[k]))) <= 2e-6, k
            continue
        close(g[k], rgrads[k], max(1e-3, 4 * err32), k)


def test_unet3d_pinned_dropout_masks_and_adam_step():
    params = {"shape": (32, 32, 16), "dropout": 0.4, "device": "cuda:0", "seed": 1, "filters": (16, 32, 64)}
    x, onehot, wmap = _batch(1, 2)
    rng = np.random.default_rng(5)
    shapes = [(2, 16, 32, 32, 16), (2, 8, 16, 16, 32), (2, 4, 8, 8, 64), (2, 8, 16, 16, 32), (2, 16, 32, 32, 16)]
    masks = [(rng.random(s) >= 0.4).astype(np.uint8) for s in shapes]
    t = UNetTrainer(params, learning_rate=0.01, warmup_steps=0, net_cls=UNet3DTrain)   # the plain Adam formula, no ramp
    w0 = t.state_dict()
    t.net.dropout_masks = [dev(m) for m in masks]
    loss = t.step(dev(x), dev(onehot), dev(wmap))
    rloss, rgrads, _ = r3.unet3d_loss_and_grads(x, onehot, wmap, w0, params, dropout_masks=masks)
    assert abs(loss.item() - rloss) <= 1e-5 * abs(rloss)
    w1 = t.state_dict()
    for k, g in rgrads.items():                                    # first Adam step: p -= lr * g/(|g| + eps')
        ref = w0[k] - 0.01 * g / (np.abs(g) + 1e-8 / np.sqrt(1 - 0.999) * 1.0)
        big = np.abs(g) > 1e-3 * np.abs(g).max()                   # sign(g) is ill-conditioned at g ~ 0
        assert np.allclose(w1[k][big], ref[big], atol=2e-4), k
    loss2 = t.step(dev(x), dev(onehot), dev(wmap))                 # generated masks
    assert np.isfinite(loss2.item()) and t.step_count == 2


@pytest.mark.parametrize("bridge", ["eltwise_mul", "concat"])
def test_direct_gradient_sinks_equal_autograd_accumulation(bridge):
    params = {"shape": (32, 32, 16), "dropout": 0.0, "device": "cuda:0", "seed": 3, "filters": (16, 32, 64),
              "bridge": bridge}
    x, onehot, wmap = _batch(2, 2)
    grads = []
    for direct in (True, False):
        t = UNetTrainer(params, net_cls=UNet3DTrain, direct_grads=direct)
        t.forward_backward(dev(x), dev(onehot), dev(wmap))
        grads.append(t.grads())
    for k in grads[0]:
        close(grads[0][k], grads[1][k], 1e-5, k)


def test_volume_training_reduces_loss_and_the_model_loads_into_unet3d():
    params = {"shape": (32, 32, 16), "dropout": 0.0, "device": "cuda:0", "seed": 0, "filters": (16, 32, 64)}
    rng = np.random.default_rng(3)
    zz, yy, xx = np.mgrid[0:16, 0:32, 0:32]
    lab = ((zz - 8) ** 2 * 4 + (yy - 16) ** 2 + (xx - 15) ** 2 < 90)
    x = (lab[None, ..., None] * 2.0 + rng.standard_normal((1, 16, 32, 32, 1)) * 0.5).astype(np.float32)
    onehot = np.stack([~lab, lab], -1)[None].astype(np.uint8)
    wmap = np.ones((1, 16, 32, 32, 1), np.float32)
    t = UNetTrainer(params, learning_rate=0.003, warmup_steps=0, net_cls=UNet3DTrain)
    xd, od, wd = dev(x), dev(onehot), dev(wmap)
    losses = [t.step(xd, od, wd).item() for _ in range(30)]
    print("losses", losses[0], losses[-1])
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    sd = t.state_dict()
    net = UNet3D(params, "infer")
    net.load_state_dict(sd, strict=True)
    ev = UNet3DTrain(params, "eval")
    ev.load_state_dict(sd, strict=True)
    a, b = net.build(x), ev.build(x)
    assert a.shape == (1, 16, 32, 32, 2)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))   # same kernels, same bits
    mask = net.predict(x)
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == (1, 16, 32, 32)
    assert torch.equal(mask, a.argmax(-1).to(torch.uint8))
    assert torch.equal(ev.predict(x), mask)
    with pytest.raises(NotImplementedError, match='dgrad'):
        UNet3D(params, "train")


def test_train_volume_job_then_segment_with_the_saved_model(tmp_path, monkeypatch):
    from sequitr_amd import core, jobs
    monkeypatch.setattr(core.TensorflowConfiguration, "MODELDIR", str(tmp_path / "models"))
    os.mkdir(str(tmp_path / "models"))
    os.mkdir(str(tmp_path / "out_t")), os.mkdir(str(tmp_path / "out_s"))
    rng = np.random.default_rng(0)
    zz, yy, xx = np.mgrid[0:16, 0:32, 0:32]
    lab = ((zz - 8) ** 2 * 4 + (yy - 15) ** 2 + (xx - 17) ** 2 < 90).astype(np.uint8)
    imgs = (lab[None] * 2.0 + rng.standard_normal((2, 16, 32, 32)) * 0.4).astype(np.float32)
    np.save(str(tmp_path / "im.npy"), imgs)
    np.save(str(tmp_path / "lab.npy"), np.broadcast_to(lab, (2, 16, 32, 32)).copy())
    params = {"images": str(tmp_path / "im.npy"), "labels": str(tmp_path / "lab.npy"), "num_outputs": 2, "num_epochs": 5,
              "dropout": 0.0, "seed": 0, "output": str(tmp_path / "out_t")}
    info = jobs.SERVER_train_volume(params, {"gpu": 0, "max_steps": 3})
    assert info["steps"] == 3 and info["batch_size"] == 1 and info["volumes"] == 2 and info["shape"] == [16, 32, 32]
    assert info["model_dir"].endswith(os.path.join("UNet2D_test", "0001"))
    assert os.path.exists(os.path.join(info["model_dir"], "weights.npz"))
    cfg = json.load(open(os.path.join(info["model_dir"], "net.config")))["NetConfiguration"]
    assert tuple(cfg["shape"]) == (32, 32, 16) and cfg["learning_rate"] == info["learning_rate"]
    tj = json.load(open(str(tmp_path / "out_t" / "train.json")))
    assert len(tj["losses"]) == 3 and np.isfinite(tj["losses"]).all()
    seg = {"input": str(tmp_path / "im.npy"), "model": "UNet2D_test", "output": str(tmp_path / "out_s")}
    sinfo = jobs.SERVER_segment_volume(seg, {"gpu": 0})
    assert sinfo["volumes"] == 2
    mask = np.load(str(tmp_path / "out_s" / "mask.npy"))
    assert mask.shape == (2, 16, 32, 32) and mask.dtype == np.uint8
    # the segmentation ran with the trained weights, not a fresh draw
    from sequitr_amd import utils
    w = utils.load_model_weights(info["model_dir"])
    net = UNet3D({"shape": (32, 32, 16), "device": "cuda:0"}, "infer")
    net.load_state_dict(w, strict=True)
    assert np.array_equal(net.predict(imgs[:1, ..., None])[0].cpu().numpy(), mask[0])
