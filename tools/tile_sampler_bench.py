"""Tile sampler benchmark: one JSON line, also written to profiles/tile_sampler_bench.json.

Workload: 8 uint16 frames of 2048 x 2048 with uint8 class-index labels (2 classes) and float32 weight maps, all resident in
HBM; a step's batch is 16 tiles of 512 x 512 at random origins (frontend.tile_sample_plan, TileSampler.sample: one launch
for image, one-hot labels and weights, into fixed buffers).  HIP events round each call after warm-up, the variants
alternated call by call, 8 calls per event pair:
  * theta = 0, theta = pi/4 and random theta, each with SQ_ROTATE_LDS=1, the LDS form, and with SQ_ROTATE_LDS=0, the
    direct gather (the default of an unset switch, chosen from this tool's figures);
  * torch : the same batch composed from torch ops -- the frames gathered and cast, F.grid_sample (bilinear, zeros,
    align_corners) for image and weights, indexing with the rounded coordinates for the labels -- into the same buffers.
Bytes are the compulsory ones of a call (every output pixel written once, and one source pixel of each array read per output
pixel); GB/s stands next to the 6.3 TB/s an HBM-bound kernel can reach on the MI355X.  `step` is SERVER_train's captured
step (UNetTrainer.capture, default filters, batch 16 of 512 x 512) in f32 and in bf16, `sampling_share` the random-theta
sampler call over it.
Usage: python tools/tile_sampler_bench.py [--warmup 2] [--iters 7] [--step-iters 5] [--out PATH]
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

FRAMES, TILE, BATCH, CLASSES = (8, 2048, 2048), (512, 512), 16, 2
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
    ap.add_argument('--step-iters', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tile_sampler_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tile_sampler_bench needs the GPU')
    import torch.nn.functional as F
    from sequitr_amd.frontend import TileSampler, tile_sample_plan
    from sequitr_amd.train import UNetTrainer
    torch.cuda.set_device(0)
    dev = 'cuda:0'
    rng = np.random.default_rng(0)
    nF, H, W = FRAMES
    frames = torch.from_numpy(rng.integers(100, 4000, FRAMES).astype(np.uint16)).to(dev)
    lab = torch.from_numpy(rng.integers(0, CLASSES, FRAMES).astype(np.uint8)).to(dev)
    wmap = torch.rand(FRAMES, device=dev) + 0.5
    sampler = TileSampler((H, W), TILE, dev)
    stats = sampler.stats(frames)
    thetas = {'theta_0': np.zeros(BATCH), 'theta_pi_4': np.full(BATCH, np.pi / 4), 'theta_random': rng.uniform(0, 2 * np.pi, BATCH)}
    rows_host = {k: tile_sample_plan((H, W), TILE, nF, BATCH, np.random.default_rng(1), theta=v) for k, v in thetas.items()}
    rows = {k: tuple(torch.from_numpy(a).to(dev) for a in v) for k, v in rows_host.items()}
    bufs = (torch.empty((BATCH,) + TILE + (1,), dtype=torch.float32, device=dev),
            torch.empty((BATCH,) + TILE + (CLASSES,), dtype=torch.uint8, device=dev),
            torch.empty((BATCH,) + TILE + (1,), dtype=torch.float32, device=dev))
    classes = torch.arange(CLASSES, dtype=torch.uint8, device=dev)
    jj = torch.arange(TILE[1], dtype=torch.float32, device=dev)[None, None, :]
    ii = torch.arange(TILE[0], dtype=torch.float32, device=dev)[None, :, None]

    def hip(name):
        plan, coef = rows[name]
        sampler.sample(frames, lab, wmap, plan, coef, CLASSES, stats=stats, out=bufs)

    def composed(name):
        plan, coef = rows[name]
        f = plan[:, 0].long()
        x, y = plan[:, 2, None, None].float() + jj, plan[:, 1, None, None].float() + ii
        c = coef[:, :, None, None]
        sx, sy = c[:, 0] * x + c[:, 1] * y + c[:, 2], c[:, 3] * x + c[:, 4] * y + c[:, 5]
        grid = torch.stack([sx * (2. / (W - 1)) - 1., sy * (2. / (H - 1)) - 1.], -1)
        img = (frames.view(torch.int16)[f].float() - stats[0][f, None, None]) / stats[1][f, None, None]   # counts < 2^15
        bufs[0][..., 0] = F.grid_sample(img[:, None], grid, mode='bilinear', padding_mode='zeros', align_corners=True)[:, 0]
        r, q = torch.round(sy).long(), torch.round(sx).long()
        inside = (r >= 0) & (r < H) & (q >= 0) & (q < W)
        picked = lab[f[:, None, None], r.clamp(0, H - 1), q.clamp(0, W - 1)] * inside
        bufs[1][...] = picked[..., None] == classes
        bufs[2][..., 0] = F.grid_sample(wmap[f][:, None], grid, mode='bilinear', padding_mode='zeros',
                                        align_corners=True)[:, 0] + (~inside).float()

    def with_lds(on, fn):                                       # the switch is read per launch: flipped round the call
        def run():
            os.environ['SQ_ROTATE_LDS'] = '1' if on else '0'
            fn()
            os.environ.pop('SQ_ROTATE_LDS', None)
        return run

    variants, agreement = {}, {}
    for name in thetas:
        variants[(name, 'lds')] = with_lds(True, lambda n=name: hip(n))
        variants[(name, 'direct')] = with_lds(False, lambda n=name: hip(n))
        variants[(name, 'torch')] = (lambda n=name: composed(n))
    for name in thetas:                                         # both forms agree bit for bit, torch to its own rounding
        variants[(name, 'lds')]()
        a = [b.clone() for b in bufs]
        variants[(name, 'direct')]()
        assert all(torch.equal(u.view(torch.uint8), v.view(torch.uint8)) for u, v in zip(a, bufs)), name
        composed(name)
        agreement[name] = {'image_max_abs': float((a[0] - bufs[0]).abs().max()), 'weights_max_abs': float((a[2] - bufs[2]).abs().max()),
                           'onehot_differing': int((a[1] != bufs[1]).sum())}
    for _ in range(args.warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(args.iters):                                 # interleaved rounds: drift hits all variants alike
        for k, fn in variants.items():
            t[k].append(_time(fn, REPS))
    px = BATCH * TILE[0] * TILE[1]
    nbytes = px * ((2 + 1 + 4) + (4 + CLASSES + 4))
    result = {}
    for name in thetas:
        row = {}
        for form in ('lds', 'direct', 'torch'):
            v = t[(name, form)]
            m = float(np.median(v))
            row[form] = {'ms': round(m, 4), 'ms_min_max': [round(min(v), 4), round(max(v), 4)],
                         'gb_per_s': round(nbytes / m / 1e6, 1),
                         'fraction_of_hbm_achievable': round(nbytes / m / 1e6 / HBM_ACHIEVABLE_GBS, 4)}
        row['direct_over_lds'] = round(row['direct']['ms'] / row['lds']['ms'], 3)
        row['torch_over_lds'] = round(row['torch']['ms'] / row['lds']['ms'], 3)
        row['torch_over_direct'] = round(row['torch']['ms'] / row['direct']['ms'], 3)
        row['torch_agreement'] = agreement[name]
        result[name] = row

    steps = {}
    for dtype in ('f32', 'bf16'):
        trainer = UNetTrainer({'shape': TILE, 'num_outputs': CLASSES, 'device': dev, 'seed': 0, 'dtype': dtype})
        hip('theta_random')
        trainer.capture(*bufs, warmup=1)
        static = trainer.static_inputs
        plan, coef = rows['theta_random']

        def sample_static():
            sampler.sample(frames, lab, wmap, plan, coef, CLASSES, stats=stats, out=static)

        for _ in range(2):
            sample_static()
            trainer.step(*static)
        torch.cuda.synchronize()
        st = [_time(lambda: trainer.step(*static)) for _ in range(args.step_iters)]
        sm = [_time(sample_static, REPS) for _ in range(args.step_iters)]
        steps[dtype] = {'step_ms': round(float(np.median(st)), 3), 'step_ms_min_max': [round(min(st), 3), round(max(st), 3)],
                        'sampling_ms': round(float(np.median(sm)), 4),
                        'sampling_share': round(float(np.median(sm)) / float(np.median(st)), 5)}
        del trainer
        torch.cuda.empty_cache()
    line = {'workload': 'tile sampler: %d x %d x %d uint16 frames + uint8 labels (%d classes) + f32 weights resident, batches of %d '
                        'tiles of %d x %d' % (FRAMES + (CLASSES, BATCH) + TILE),
            'warmup': args.warmup, 'iters': args.iters, 'calls_per_window': REPS, 'device': torch.cuda.get_device_name(0),
            'hbm_achievable_gb_per_s': HBM_ACHIEVABLE_GBS, 'compulsory_bytes': int(nbytes), 'angles': result,
            'step': dict(steps, what='UNetTrainer.capture, default filters, batch %d of %d x %d' % ((BATCH,) + TILE),
                         iters=args.step_iters)}
    text = json.dumps(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
