"""Volume sampler benchmark: one JSON line, also written to profiles/volume_sampler_bench.json.

Workload: one 64 x 1024 x 1024 uint16 volume with uint8 class-index labels (2 classes) and a float32 weight map, all
resident in HBM; a step's batch is 8 bricks of 32 x 128 x 128 (Z, X, Y) at random origins.  HIP events round each call
after warm-up, the variants alternated call by call, 8 calls per event pair:
  * images / weights / onehot : VolumeSampler.images (ImageNorm applied), .copy of the weight map, .onehot of the labels,
    each into a fixed buffer, for three op classes -- every row the identity (op 0), every row a y flip (op 4), every
    row transposed (op 8) with the LDS tiles (default) and with SQ_SAMPLE_LDS=0, the direct gather;
  * torch : the same batch composed from torch ops, brick by brick -- slice, flip, transpose, contiguous, normalise (the
    one-hot as a comparison with the class indices) -- into the same buffers.
Bytes are what a call has to move (reads + writes, from the shapes); GB/s stands next to the 6.3 TB/s an HBM-bound kernel
can reach on the MI355X -- a batch is 4 .. 8 MiB a side, so these calls are launch- and latency-sized, not
bandwidth-sized.  `step` is one UNet3DTrain step (default filters, eager, batch of 8 bricks) timed as
tools/unet3d_train_bench.py times it, `sampling_ms` the three kernels of a mixed plan (sample_plan's own ops) in front of
it, and `sampling_share` their ratio.
Usage: python tools/volume_sampler_bench.py [--warmup 2] [--iters 7] [--step-iters 3] [--out PATH]
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

SHAPE, BRICK, BATCH, CLASSES = (64, 1024, 1024), (32, 128, 128), 8, 2
HBM_ACHIEVABLE_GBS = 6300.
REPS = 8                                                        # calls per event pair


def _time(fn, reps=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--iters', type=int, default=7)
    ap.add_argument('--step-iters', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'volume_sampler_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('volume_sampler_bench needs the GPU')
    from sequitr_amd.frontend import VolumeSampler, sample_plan, volume_stats
    from sequitr_amd.networks.unet import UNet3DTrain
    from sequitr_amd.train import UNetTrainer
    torch.cuda.set_device(0)
    dev = 'cuda:0'
    rng = np.random.default_rng(0)
    vol = torch.from_numpy(rng.integers(100, 4000, (1,) + SHAPE).astype(np.uint16)).to(dev)
    lab = torch.from_numpy(rng.integers(0, CLASSES, (1,) + SHAPE).astype(np.uint8)).to(dev)
    wmap = torch.rand((1,) + SHAPE + (1,), device=dev) + 0.5
    sampler = VolumeSampler(SHAPE, BRICK, dev)
    stats = volume_stats(vol)
    mean, std = stats[0][0], stats[1][0]
    base = sample_plan(SHAPE, BRICK, 1, BATCH, rng, augment=())
    plans_host = {'identity': base.copy(), 'flip_y': base.copy(), 'transpose': base.copy()}
    plans_host['flip_y'][:, 4] = 4
    plans_host['transpose'][:, 4] = 8
    plans = {k: torch.from_numpy(v).to(dev) for k, v in plans_host.items()}
    mixed = torch.from_numpy(sample_plan(SHAPE, BRICK, 1, BATCH, rng)).to(dev)
    bx = torch.empty((BATCH,) + BRICK + (1,), dtype=torch.float32, device=dev)
    by = torch.empty((BATCH,) + BRICK + (CLASSES,), dtype=torch.uint8, device=dev)
    bw = torch.empty((BATCH,) + BRICK + (1,), dtype=torch.float32, device=dev)
    classes = torch.arange(CLASSES, dtype=torch.uint8, device=dev)

    hip = {'images': lambda p: sampler.images(vol, p, stats=stats, out=bx),
           'weights': lambda p: sampler.copy(wmap, p, out=bw),
           'onehot': lambda p: sampler.onehot(lab, CLASSES, p, out=by)}

    def crop(t, row, to_float=False):
        _, oz, ox, oy, op = (int(v) for v in row)
        box = t[0, oz:oz + BRICK[0], ox:ox + BRICK[1], oy:oy + BRICK[2]]
        if to_float:                                            # torch flips no uint16: the cast comes first
            box = box.float()
        if op & 8:
            box = box.transpose(1, 2)
        dims = [d for d, bit in ((0, 1), (1, 2), (2, 4)) if op & bit]
        return box.flip(dims) if dims else box

    def torch_images(rows):
        for j, row in enumerate(rows):
            bx[j, ..., 0] = (crop(vol, row, True).contiguous() - mean) / std

    def torch_weights(rows):
        for j, row in enumerate(rows):
            bw[j] = crop(wmap, row).contiguous()

    def torch_onehot(rows):
        for j, row in enumerate(rows):
            by[j] = crop(lab, row).contiguous()[..., None] == classes

    ref = {'images': torch_images, 'weights': torch_weights, 'onehot': torch_onehot}
    vox = BATCH * BRICK[0] * BRICK[1] * BRICK[2]
    nbytes = {'images': vox * (2 + 4), 'weights': vox * (4 + 4), 'onehot': vox * (1 + CLASSES)}

    # variants: (kernel, op class, path); the LDS switch is read per launch, so it is flipped round the call
    def with_lds(on, fn):
        def run():
            if on:
                os.environ.pop('SQ_SAMPLE_LDS', None)
            else:
                os.environ['SQ_SAMPLE_LDS'] = '0'
            fn()
            os.environ.pop('SQ_SAMPLE_LDS', None)
        return run

    variants = {}
    for kern in hip:
        for cls in plans:
            variants[(kern, cls, 'hip')] = with_lds(True, lambda k=kern, c=cls: hip[k](plans[c]))
            variants[(kern, cls, 'torch')] = (lambda k=kern, c=cls: ref[k](plans_host[c]))
        variants[(kern, 'transpose', 'hip_direct')] = with_lds(False, lambda k=kern: hip[k](plans['transpose']))
    # both paths of the transposed ops and the torch composition agree before anything is timed
    for kern, buf in (('images', bx), ('weights', bw), ('onehot', by)):
        variants[(kern, 'transpose', 'hip')]()
        a = buf.clone()
        variants[(kern, 'transpose', 'hip_direct')]()
        assert torch.equal(a.view(torch.uint8), buf.view(torch.uint8)), kern
        ref[kern](plans_host['transpose'])
        if kern == 'images':
            assert float((a - buf).abs().max()) < 1e-5, kern
        else:
            assert torch.equal(a.view(torch.uint8), buf.view(torch.uint8)), kern
    for _ in range(args.warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(args.iters):                                 # interleaved rounds: drift hits all variants alike
        for k, fn in variants.items():
            t[k].append(_time(fn, REPS))
    kernels = {}
    for kern in hip:
        rows = {}
        for cls in plans:
            h, r = t[(kern, cls, 'hip')], t[(kern, cls, 'torch')]
            hm, rm = float(np.median(h)), float(np.median(r))
            rows[cls] = {'hip_ms': round(hm, 4), 'hip_ms_min_max': [round(min(h), 4), round(max(h), 4)],
                         'hip_gb_per_s': round(nbytes[kern] / hm / 1e6, 1),
                         'fraction_of_hbm_achievable': round(nbytes[kern] / hm / 1e6 / HBM_ACHIEVABLE_GBS, 4),
                         'torch_ms': round(rm, 4), 'torch_ms_min_max': [round(min(r), 4), round(max(r), 4)],
                         'torch_over_hip': round(rm / hm, 3)}
        d = t[(kern, 'transpose', 'hip_direct')]
        dm = float(np.median(d))
        rows['transpose'].update({'lds': 'default', 'direct_ms': round(dm, 4), 'direct_ms_min_max': [round(min(d), 4), round(max(d), 4)],
                                  'direct_gb_per_s': round(nbytes[kern] / dm / 1e6, 1),
                                  'direct_over_lds': round(dm / rows['transpose']['hip_ms'], 3)})
        kernels[kern] = dict(rows, bytes=int(nbytes[kern]))

    def sample_mixed():
        hip['images'](mixed), hip['onehot'](mixed), hip['weights'](mixed)

    sample_mixed()
    samp = [_time(sample_mixed, REPS) for _ in range(args.iters)]
    trainer = UNetTrainer({'shape': (BRICK[1], BRICK[2], BRICK[0]), 'num_outputs': CLASSES, 'device': dev, 'seed': 0},
                          net_cls=UNet3DTrain)
    for _ in range(2):
        trainer.step(bx, by, bw)
    torch.cuda.synchronize()
    steps = [_time(lambda: trainer.step(bx, by, bw)) for _ in range(args.step_iters)]
    samp_ms, step_ms = float(np.median(samp)), float(np.median(steps))
    line = {'workload': 'volume sampler: 1 x %d x %d x %d uint16 + uint8 labels (%d classes) + f32 weights resident, batches of '
                        '%d bricks of %s (Z, X, Y)' % (SHAPE + (CLASSES, BATCH, list(BRICK))),
            'warmup': args.warmup, 'iters': args.iters, 'calls_per_window': REPS, 'device': torch.cuda.get_device_name(0),
            'hbm_achievable_gb_per_s': HBM_ACHIEVABLE_GBS, 'kernels': kernels,
            'sampling_ms': round(samp_ms, 4), 'sampling_ms_min_max': [round(min(samp), 4), round(max(samp), 4)],
            'step': {'what': 'UNet3DTrain f32, default filters, eager, batch %d' % BATCH, 'ms': round(step_ms, 3),
                     'ms_min_max': [round(min(steps), 3), round(max(steps), 3)], 'iters': args.step_iters},
            'sampling_share': round(samp_ms / step_ms, 6)}
    text = json.dumps(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
