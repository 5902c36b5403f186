"""Torch-CPU restatement of the volumetric U-Net training graph -- TEST INFRASTRUCTURE ONLY (tests/test_gpu_unet3d_train.py).
It shares nothing with the code under test but the weights: ATen conv3d / max_pool3d / conv_transpose3d on NCDHW tensors,
autograd for every gradient, in fp64 (the reference) or fp32 (the yardstick of what an f32 evaluation of this graph costs).

Wiring: UNet.build (down blocks, 2x2x2 max pool, transpose conv + bridge + block, 1x1x1 head); loss: the weighted softmax
cross-entropy, sum over voxels of w * CE divided by the number of voxels."""
import numpy as np
import torch
import torch.nn.functional as TF

DEFAULT_FILTERS = (16, 32, 64, 128, 256)


def to_ncdhw(a, dtype=torch.float64):
    return torch.as_tensor(np.asarray(a)).to(dtype).permute(0, 4, 1, 2, 3).contiguous()


def to_ndhwc_np(t):
    return t.permute(0, 2, 3, 4, 1).contiguous().numpy()


def _bridge(up, skip, kind):
    if kind == 'eltwise_add':
        return up + skip
    if kind == 'eltwise_mul':
        return up * skip
    if kind == 'eltwise_sub':
        return up - skip
    if kind == 'concat':
        return torch.cat([up, skip], 1)                         # the up-scaled tensor first
    return up


def unet3d_loss_and_grads(x, onehot, wmap, weights, params, dropout_masks=None, dtype=torch.float64):
    """x (N,D,H,W,C), onehot (N,D,H,W,K) uint8, wmap one value per voxel, weights {name: ndarray} in the project's layouts
    (conv (3,3,3,Cin,Cout), transpose conv (2,2,2,Cout,Cin), head (1,1,1,C,K)).  Returns (loss, {name: gradient},
    logits NDHWC).  Dropout multiplies by the SUPPLIED masks (NDHWC uint8, call order) / (1 - rate)."""
    filters = tuple(params.get('filters', DEFAULT_FILTERS))
    kind = params.get('bridge', 'eltwise_mul')
    bn, eps = bool(params.get('batch_norm', False)), float(params.get('bn_epsilon', 1e-3))
    rate = float(params.get('dropout', 0.0)) if dropout_masks is not None else 0.0
    masks = list(dropout_masks) if dropout_masks is not None else None
    W = {k: torch.as_tensor(np.asarray(v)).to(dtype).requires_grad_(True) for k, v in weights.items()
         if not k.endswith(('moving_mean', 'moving_variance'))}

    def conv(t, s):
        return TF.conv3d(t, W[s + '/kernel'].permute(4, 3, 0, 1, 2), W[s + '/bias'], padding=1)

    def block(t, s):
        for k in ('conv1', 'conv2'):
            z = conv(t, s + '/' + k)
            if bn:                                              # training form: batch statistics over every voxel
                mu = z.mean((0, 2, 3, 4), keepdim=True)
                var = ((z - mu) ** 2).mean((0, 2, 3, 4), keepdim=True)
                g, b = W[s + '/' + k + '/gamma'].view(1, -1, 1, 1, 1), W[s + '/' + k + '/beta'].view(1, -1, 1, 1, 1)
                z = g * (z - mu) / torch.sqrt(var + eps) + b
            t = TF.relu(z)
        if masks is not None and rate > 0:
            t = t * to_ncdhw(masks.pop(0), dtype) / (1.0 - rate)
        return t

    net = [block(to_ncdhw(x, dtype), 'UNet/down0')]
    for i in range(1, len(filters)):
        net.append(block(TF.max_pool3d(net[-1], 2, 2), 'UNet/down%d' % i))
    for i in reversed(range(len(filters) - 1)):
        s = 'UNet/up%d' % i
        up = TF.conv_transpose3d(net[-1], W[s + '/upscale/kernel'].permute(4, 3, 0, 1, 2), W[s + '/upscale/bias'], stride=2)
        net.append(block(_bridge(up, net[i], kind), s))
    logits = TF.conv3d(net[-1], W['UNet/to_image/kernel'].permute(4, 3, 0, 1, 2), W['UNet/to_image/bias'])
    logits = logits.permute(0, 2, 3, 4, 1)
    y = torch.as_tensor(np.asarray(onehot)).to(dtype)
    wm = torch.as_tensor(np.asarray(wmap)).to(dtype).reshape(logits.shape[:-1])
    loss = (wm * -(y * TF.log_softmax(logits, -1)).sum(-1)).sum() / wm.numel()
    loss.backward()
    return float(loss.detach()), {k: v.grad.numpy() for k, v in W.items()}, logits.detach().numpy()
