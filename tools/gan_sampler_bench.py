"""GAN sampler benchmark: one JSON line, also written to profiles/gan_sampler_bench.json.

Workload: 256 uint8 images of 512 x 512 x 2 resident in HBM; a step's batch is 32 samples of a 512 x 512 crop under random
mirrors, resized to the level's size (frontend.gan_sample_plan, GanSampler.sample: one launch into a fixed buffer), at every
level 0 .. 7 (4 x 4 up to 512 x 512).  HIP events round each call after warm-up, the variants alternated call by call, 8
calls per event pair:
  * hip   : GanSampler.sample with the statistics computed once;
  * host  : the path taken without params['crop'], GenerativeAdverserialNetwork._next_real_batch on the same stack as a
            .npy memmap -- fancy indexing on the host, the cast to float32, a synchronous upload, ops.resize_nearest;
  * torch : the same batch composed from torch ops on the resident stack -- index, cast, normalise with the same
            statistics, flip, F.interpolate(bilinear, align_corners=True) -- into the same buffer.
`stats_ms` is the one-off statistics call over the whole stack.  `iteration` is GenerativeAdverserialNetwork.iteration at
level 6 (256 x 256, batch 32, bf16, graph replay), `sampling_share` the level-6 sampler call over it.
Usage: python tools/gan_sampler_bench.py [--warmup 2] [--iters 5] [--step-iters 5] [--out PATH]
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

STACK, CROP, BATCH, LEVELS = (256, 512, 512, 2), (512, 512), 32, 8
REPS = 8                                                        # calls per event pair
WORKLOAD = 'GAN sampler: %d x %d x %d x %d uint8 images resident, batches of %d crops of %d x %d at levels 0 .. %d' % (
    STACK + (BATCH,) + CROP + (LEVELS - 1,))


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
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--step-iters', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gan_sampler_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('gan_sampler_bench needs the GPU')
    import torch.nn.functional as F
    from sequitr_amd.frontend import GanSampler, gan_sample_plan
    from sequitr_amd.networks.gan import TRAIN, GenerativeAdverserialNetwork
    torch.cuda.set_device(0)
    dev = 'cuda:0'
    N, H, W, C = STACK
    rng = np.random.default_rng(0)
    host_images = rng.integers(0, 256, STACK, dtype=np.uint8)
    images = torch.from_numpy(host_images).to(dev)
    sampler = GanSampler((H, W), C, CROP, dev)
    stats = sampler.stats(images)
    torch.cuda.synchronize()
    stats_t = [_time(lambda: sampler.stats(images)) for _ in range(args.iters + args.warmup)][args.warmup:]
    plan_host = gan_sample_plan((H, W), CROP, N, BATCH, np.random.default_rng(1))
    plan = torch.from_numpy(plan_host).to(dev)
    idx = plan[:, 0].long()
    fx, fy = (plan[:, 3] & 1).bool()[:, None, None, None], (plan[:, 3] & 2).bool()[:, None, None, None]
    mean, inv = stats

    tmp = tempfile.mkdtemp(prefix='gan_sampler_bench_')
    fn = os.path.join(tmp, 'stack.npy')
    np.save(fn, host_images)
    net = GenerativeAdverserialNetwork({'num_levels': LEVELS, 'batch_size': BATCH, 'device': dev, 'training_data': fn}, TRAIN)
    step = [0]

    result = {}
    try:
        for level in range(LEVELS):
            size = (4 << level, 4 << level)
            net.set_level(level)
            out = torch.empty((BATCH,) + size + (C,), dtype=torch.float32, device=dev)

            def hip():
                sampler.sample(images, plan, size, stats=stats, out=out)

            def host():
                step[0] += 1
                net._next_real_batch(step[0])

            def composed():
                x = (images[idx].float() - mean[idx][:, None, None]) * inv[idx][:, None, None]   # crop = the whole image here
                x = torch.where(fy, x.flip(1), x)
                x = torch.where(fx, x.flip(2), x)
                out.copy_(F.interpolate(x.permute(0, 3, 1, 2), size=size, mode='bilinear', align_corners=True).permute(0, 2, 3, 1))

            hip()
            a = out.clone()
            composed()
            agree = float((a - out).abs().max())
            variants = {'hip': hip, 'host': host, 'torch': composed}
            for _ in range(args.warmup):
                for f in variants.values():
                    f()
            torch.cuda.synchronize()
            t = {k: [] for k in variants}
            for _ in range(args.iters):                         # interleaved rounds: drift hits all variants alike
                for k, f in variants.items():
                    t[k].append(_time(f, REPS))
            med = {k: float(np.median(v)) for k, v in t.items()}
            result[str(level)] = {'size': list(size), 'hip_ms': round(med['hip'], 4), 'host_ms': round(med['host'], 3),
                                  'torch_ms': round(med['torch'], 4),
                                  'hip_ms_min_max': [round(min(t['hip']), 4), round(max(t['hip']), 4)],
                                  'host_over_hip': round(med['host'] / med['hip'], 1),
                                  'torch_over_hip': round(med['torch'] / med['hip'], 2), 'torch_max_abs': agree}
    finally:
        del net
        os.remove(fn)
        os.rmdir(tmp)

    g = GenerativeAdverserialNetwork({'num_levels': 7, 'batch_size': BATCH, 'repeat_batch': 1, 'learning_rate': 1e-3,
                                      'device': dev, 'seed': 0, 'dtype': 'bf16', 'graph': True}, mode=None)
    g.build()
    g.set_level(6)
    X = torch.empty((BATCH, 256, 256, C), dtype=torch.float32, device=dev)
    Z = torch.randn((BATCH, 1, 1, 512), device=dev)

    def sample6():
        sampler.sample(images, plan, (256, 256), stats=stats, out=X)

    sample6()
    for _ in range(3):                                          # eager, capture, replay
        g.iteration(X, Z, 1.0)
    torch.cuda.synchronize()
    it = [_time(lambda: g.iteration(X, Z, 1.0)) for _ in range(args.step_iters)]
    sm = [_time(sample6, REPS) for _ in range(args.step_iters)]
    line = {'workload': WORKLOAD, 'device': torch.cuda.get_device_name(0), 'warmup': args.warmup, 'iters': args.iters,
            'calls_per_window': REPS, 'stats_ms': round(float(np.median(stats_t)), 4), 'levels': result,
            'iteration': {'what': 'GenerativeAdverserialNetwork.iteration, level 6, batch %d, bf16, graph replay' % BATCH,
                          'ms': round(float(np.median(it)), 3), 'ms_min_max': [round(min(it), 3), round(max(it), 3)],
                          'iters': args.step_iters},
            'sampling_ms': round(float(np.median(sm)), 4),
            'sampling_share': round(float(np.median(sm)) / float(np.median(it)), 5)}
    text = json.dumps(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
