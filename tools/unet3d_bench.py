"""UNet3D inference benchmark: one JSON line.

Default workload: UNet3D, filters (16,32,64,128,256), one 1 x 64 x 256 x 256 single-channel volume.  Reports
  * ms per volume (HIP events around predict(), after warm-up) and Mvoxels/s;
  * per 3x3x3 conv layer: the conv3d kernel time, its FLOPs from shapes (2 * voxels * 27 * Cin * Cout) and fraction of the
    157.3 TF f32 MFMA peak; and the obvious alternative, timed alternately in the same run: the depth-stacked input
    materialised with torch.cat + the planar ops.conv2d on 3*Cin channels (same bits by the contract), with the planar
    conv alone (stacking excluded) and the stack + conv sum.
Usage: python tools/unet3d_bench.py [--depth 64] [--size 256] [--warmup 3] [--iters 10]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK_TF = 157.3


def _time(fn, iters):
    """median ms of fn() by HIP events"""
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def stack_depth(x):
    """(N,D,H,W,C) -> (N*D, H, W, 3C): the stacked planar input of the conv3d definition (torch.cat, on the GPU)"""
    N, D, H, W, C = x.shape
    z = torch.zeros((N, 1, H, W, C), dtype=x.dtype, device=x.device)
    p = torch.cat([z, x, z], 1)
    return torch.cat([p[:, 0:D], p[:, 1:D + 1], p[:, 2:D + 2]], -1).reshape(N * D, H, W, 3 * C)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--depth', type=int, default=64)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('unet3d_bench needs the GPU')
    from sequitr_amd import ops
    from sequitr_amd.networks.unet import UNet3D

    dev = 'cuda:0'
    torch.cuda.set_device(0)
    D, S = args.depth, args.size
    filters = (16, 32, 64, 128, 256)
    net = UNet3D({'shape': (S, S, D), 'num_outputs': 2, 'filters': filters, 'device': dev, 'seed': 0}).initialize()
    x = torch.randn((1, D, S, S, 1), device=dev)
    for _ in range(args.warmup):
        net.predict(x)
    torch.cuda.synchronize()
    ms = _time(lambda: net.predict(x), args.iters)

    # per-layer conv3d vs stacked planar conv, alternately in the same run
    layers, cin = [], 1
    for i, fo in enumerate(filters):
        layers += [('down%d/conv1' % i, i, cin, fo), ('down%d/conv2' % i, i, fo, fo)]
        cin = fo
    for i in reversed(range(len(filters) - 1)):
        layers += [('up%d/conv1' % i, i, filters[i], filters[i]), ('up%d/conv2' % i, i, filters[i], filters[i])]
    g = torch.Generator(device=dev).manual_seed(1)
    rows = []
    tot3 = tot2 = totst = 0.0
    flops_all = 0.0
    for name, lvl, ci, co in layers:
        d, h = D >> lvl, S >> lvl
        xl = torch.randn((1, d, h, h, ci), generator=g, device=dev)
        w = torch.randn((3, 3, 3, ci, co), generator=g, device=dev) / np.sqrt(27 * ci)
        b = torch.zeros((co,), device=dev)
        ws = w.permute(1, 2, 0, 3, 4).reshape(3, 3, 3 * ci, co).contiguous()
        xs = stack_depth(xl).contiguous()
        y3 = ops.conv3d(xl, w, b, act='relu')
        y2 = ops.conv2d(xs, ws, b, act='relu')
        same = bool(torch.equal(y3.view(-1), y2.view(-1)))
        for _ in range(2):
            ops.conv3d(xl, w, b, act='relu', out=y3)
            ops.conv2d(xs, ws, b, act='relu', out=y2)
        t3, t2, tst = [], [], []
        for _ in range(args.iters):                       # alternate the three so drift hits all of them alike
            t3.append(_time(lambda: ops.conv3d(xl, w, b, act='relu', out=y3), 1))
            t2.append(_time(lambda: ops.conv2d(xs, ws, b, act='relu', out=y2), 1))
            tst.append(_time(lambda: stack_depth(xl).contiguous(), 1))
        t3, t2, tst = float(np.median(t3)), float(np.median(t2)), float(np.median(tst))
        flops = 2.0 * d * h * h * 27 * ci * co
        flops_all += flops
        tot3, tot2, totst = tot3 + t3, tot2 + t2, totst + tst
        plan = ops.conv3d_plan(1, d, h, h, ci, co)
        rows.append({'layer': name, 'shape': [1, d, h, h, ci, co], 'plan': [plan['kind'], plan['bn'], plan['kc']],
                     'conv3d_ms': round(t3, 4), 'stacked_conv2d_ms': round(t2, 4), 'stack_ms': round(tst, 4),
                     'ratio_vs_stacked_conv': round(t3 / t2, 3), 'ratio_vs_stack_plus_conv': round(t3 / (t2 + tst), 3),
                     'gflop': round(flops / 1e9, 3), 'peak_fraction': round(flops / (t3 * 1e-3) / (PEAK_TF * 1e12), 3),
                     'bit_identical': same})
        del xl, xs, y3, y2
    vox = D * S * S
    print(json.dumps({'workload': 'UNet3D 1x%dx%dx%d, filters %s' % (D, S, S, list(filters)), 'ms_per_volume': round(ms, 3),
                      'mvoxels_per_s': round(vox / (ms * 1e-3) / 1e6, 1), 'conv3d_ms_total': round(tot3, 3),
                      'stacked_conv2d_ms_total': round(tot2, 3), 'stack_ms_total': round(totst, 3),
                      'conv_peak_fraction': round(flops_all / (tot3 * 1e-3) / (PEAK_TF * 1e12), 3), 'layers': rows}))


if __name__ == '__main__':
    main()
