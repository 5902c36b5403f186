"""UNet3D f32 training benchmark: one JSON line, also written to profiles/unet3d_train_bench.json.

Default workload: UNet3DTrain, filters (16,32,64,128,256), one 1 x 32 x 128 x 128 single-channel volume.  Reports
  * ms per training step (forward, loss, backward, Adam; eager), HIP events around UNetTrainer.step after warm-up;
  * per 3x3x3 conv layer: the 3-D weight gradient (ops.conv3d_wgrad, both launches) next to the composition that was
    available before it existed -- three planar ops.conv2d_wgrad launches on the depth-shifted contiguous views of the
    single volume (tap kd pairs input slices d + kd - 1 with output-gradient slices d), bias gradient from the centre
    tap, each writing its slice of a preallocated (3,3,3,Cin,Cout) buffer -- timed alternately in the same run, 8 calls
    per event pair, with the largest difference between the two results relative to max |dW|.
    speedup = composition / 3-D op; layers below 0.9 are listed under "below_0p9".
Usage: python tools/unet3d_train_bench.py [--depth 32] [--size 128] [--warmup 3] [--iters 10] [--out PATH]
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


REPS = 8                                                        # calls per event pair: a window of several launches, not one


def _time(fn, reps=1):
    """ms per call of fn(), HIP events round `reps` back-to-back calls"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def planar_composition(ops, x, dy, dw, db):
    """dW (3,3,3,Cin,Cout), db of ONE volume x (1,D,H,W,Cin), dy (1,D,H,W,Cout) from three planar weight gradients, each
    written straight into its slice of the preallocated dw (a depth tap with no slice pair keeps the zeros dw holds): the
    timed work is the three weight-gradient calls and nothing else"""
    D = x.shape[1]
    for kd in range(3):
        lo, hi = max(0, 1 - kd), D - max(0, kd - 1)             # output slices d with 0 <= d + kd - 1 < D
        if hi > lo:
            ops.conv2d_wgrad(x[0, lo + kd - 1:hi + kd - 1], dy[0, lo:hi], 3, want_bias=(kd == 1), dw_out=dw[kd],
                             db_out=db if kd == 1 else None)
    return dw, db


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--depth', type=int, default=32)
    ap.add_argument('--size', type=int, default=128)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'unet3d_train_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('unet3d_train_bench needs the GPU')
    from sequitr_amd import ops
    from sequitr_amd.networks.unet import UNet3DTrain
    from sequitr_amd.train import UNetTrainer

    dev = 'cuda:0'
    torch.cuda.set_device(0)
    D, S = args.depth, args.size
    filters = (16, 32, 64, 128, 256)
    g = torch.Generator(device=dev).manual_seed(1)
    trainer = UNetTrainer({'shape': (S, S, D), 'num_outputs': 2, 'filters': filters, 'device': dev, 'seed': 0},
                          net_cls=UNet3DTrain)
    x = torch.randn((1, D, S, S, 1), generator=g, device=dev)
    lab = torch.rand((1, D, S, S), generator=g, device=dev) < 0.3
    onehot = torch.stack([~lab, lab], -1).to(torch.uint8).contiguous()
    wmap = torch.ones((1, D, S, S, 1), device=dev)
    for _ in range(args.warmup):
        trainer.step(x, onehot, wmap)
    torch.cuda.synchronize()
    steps = [_time(lambda: trainer.step(x, onehot, wmap)) for _ in range(args.iters)]
    loss = float(trainer.last_loss)

    layers, cin = [], 1
    for i, fo in enumerate(filters):
        layers += [('down%d/conv1' % i, i, cin, fo), ('down%d/conv2' % i, i, fo, fo)]
        cin = fo
    for i in reversed(range(len(filters) - 1)):
        layers += [('up%d/conv1' % i, i, filters[i], filters[i]), ('up%d/conv2' % i, i, filters[i], filters[i])]
    rows, tot3, tot2 = [], 0.0, 0.0
    for name, lvl, ci, co in layers:
        d, h = D >> lvl, S >> lvl
        xl = torch.randn((1, d, h, h, ci), generator=g, device=dev)
        dy = torch.randn((1, d, h, h, co), generator=g, device=dev)
        dw3, db3 = ops.conv3d_wgrad(xl, dy)
        dw2, db2 = torch.zeros_like(dw3), torch.zeros_like(db3)
        planar_composition(ops, xl, dy, dw2, db2)
        diff = float((dw3 - dw2).abs().max() / dw2.abs().max())
        for _ in range(2):
            ops.conv3d_wgrad(xl, dy, dw_out=dw3, db_out=db3)
            planar_composition(ops, xl, dy, dw2, db2)
        t3, t2 = [], []
        for _ in range(args.iters):                             # alternate the two so drift hits both alike
            t3.append(_time(lambda: ops.conv3d_wgrad(xl, dy, dw_out=dw3, db_out=db3), REPS))
            t2.append(_time(lambda: planar_composition(ops, xl, dy, dw2, db2), REPS))
        m3, m2 = float(np.median(t3)), float(np.median(t2))
        tot3, tot2 = tot3 + m3, tot2 + m2
        plan = ops.conv3d_wgrad_plan(1, d, h, h, ci, co)
        rows.append({'layer': name, 'shape': [1, d, h, h, ci, co],
                     'plan': [plan['kind'], plan['no'], plan['npairs'], plan['gx'], plan['tpb']],
                     'wgrad3d_ms': round(m3, 4), 'planar_x3_ms': round(m2, 4), 'speedup_vs_planar_x3': round(m2 / m3, 3),
                     'wgrad3d_ms_min_max': [round(min(t3), 4), round(max(t3), 4)],
                     'planar_x3_ms_min_max': [round(min(t2), 4), round(max(t2), 4)],
                     'gflop': round(2.0 * d * h * h * 27 * ci * co / 1e9, 3), 'max_rel_diff': diff})
        del xl, dy
    line = {'workload': 'UNet3DTrain f32 1x%dx%dx%d, filters %s, eager step' % (D, S, S, list(filters)),
            'ms_per_step': round(float(np.median(steps)), 3), 'ms_per_step_min_max': [round(min(steps), 3), round(max(steps), 3)],
            'warmup': args.warmup, 'iters': args.iters, 'calls_per_window': REPS, 'loss_after': loss,
            'wgrad3d_ms_total': round(tot3, 3), 'planar_x3_ms_total': round(tot2, 3),
            'below_0p9': [r['layer'] for r in rows if r['speedup_vs_planar_x3'] < 0.9], 'layers': rows}
    text = json.dumps(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
