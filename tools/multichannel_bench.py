"""Multi-channel front end benchmark: one JSON line, also written to profiles/multichannel_bench.json.

Tile cutter: 8 uint16 frames of 2048 x 2048 per channel at C = 2 and 3, resident in HBM as channel-major planes, cut into
512 x 512 tiles with margin 32 (25 tiles a frame).
  * mc          : one sq_frames_to_tiles_mc launch in mode SQ_CH_NORM, statistics precomputed (FrameTiler's own call)
  * composed    : what the library had before -- C sq_frames_to_tiles launches, one per channel, and torch.stack(..., -1)
  * mc_clean / composed_clean : FrameTiler.tiles(clean=ImageOutliers(3) -> ImageBGSubtract -> ImageNorm), the whole chain
                  with its statistics, against C single-channel chains and the stack
  * host        : numpy ImageNorm per channel, slicing, stacking and the upload of the float32 tiles
  * segment_share : the multi-channel tiles() call (statistics included) over tiles() + net.predict + stitch of one batch
                  of 4 frames, default UNet2D with num_inputs = C
Sampler: 16 tiles of 512 x 512 at CI = 2 and 3 out of the same planes, theta = 0, pi/4 and random.
  * mc          : one sq_tile_sample_affine_mc launch (image, one-hot labels, weights)
  * composed    : CI sq_tile_sample_affine launches (the first with labels and weights) and torch.stack(..., -1)
  * step        : UNetTrainer.capture's step with num_inputs = CI in f32 and bf16, and the sampler's share of it
HIP events round REPS calls after warm-up, the variants alternated window by window, at least 20 windows; minimum, median
and maximum are reported, and `spread` is (max - min) / median of the same run.  Bytes are the compulsory ones (every input
pixel a tile covers read once, every output written once); GB/s stands next to the 6.3 TB/s an HBM-bound kernel can reach.
Without a GPU every field says "not measured".
Usage: python tools/multichannel_bench.py [--warmup 3] [--iters 20] [--out PATH]
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

FRAMES, TILE, MARGIN, BATCH, CLASSES = (8, 2048, 2048), 512, 32, 16, 2
CHANNELS = (2, 3)
HBM_ACHIEVABLE_GBS = 6300.
REPS = 4                                                        # calls per event pair
NOT_MEASURED = 'not measured'


def _time(fn, reps=REPS):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def _row(v, nbytes=None):
    m = float(np.median(v))
    row = {'ms_min': round(min(v), 4), 'ms_median': round(m, 4), 'ms_max': round(max(v), 4),
           'spread': round((max(v) - min(v)) / m, 3)}
    if nbytes:
        row['gb_per_s'] = round(nbytes / m / 1e6, 1)
        row['fraction_of_hbm_achievable'] = round(nbytes / m / 1e6 / HBM_ACHIEVABLE_GBS, 4)
    return row


def _race(variants, warmup, iters):
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(iters):                                      # interleaved windows: drift hits all variants alike
        for k, fn in variants.items():
            t[k].append(_time(fn))
    return t


def _verdict(mc, composed):
    """no slower than the composition, within the spread of the same run"""
    slack = max(mc['spread'], composed['spread']) * composed['ms_median']
    return {'mc_over_composed': round(mc['ms_median'] / composed['ms_median'], 3),
            'no_slower_within_spread': bool(mc['ms_median'] <= composed['ms_median'] + slack)}


def not_measured():
    cut = {'mc': NOT_MEASURED, 'composed': NOT_MEASURED, 'mc_clean': NOT_MEASURED, 'composed_clean': NOT_MEASURED,
           'host': NOT_MEASURED, 'segment_share': NOT_MEASURED}
    smp = {'theta_0': NOT_MEASURED, 'theta_pi_4': NOT_MEASURED, 'theta_random': NOT_MEASURED, 'step': NOT_MEASURED}
    return {'workload': NOT_MEASURED, 'device': NOT_MEASURED, 'tile_cutter': {'C=%d' % c: dict(cut) for c in CHANNELS},
            'sampler': {'CI=%d' % c: dict(smp) for c in CHANNELS}}


def bench_cutter(C, planes, args, dev):
    from sequitr_amd import _lib
    from sequitr_amd.frontend import CH_NORM, PIX, FrameClean, FrameTiler
    from sequitr_amd.networks.unet import UNet2D
    F, H, W = FRAMES
    x = planes[:C]
    one = FrameTiler((H, W), TILE, MARGIN, device=dev)
    many = FrameTiler((H, W), TILE, MARGIN, device=dev, channels=C)
    mean, std = many.stats(x)
    N = F * one.TR * one.TC
    out = torch.empty((N, TILE, TILE, C), dtype=torch.float32, device=dev)
    singles = [torch.empty((N, TILE, TILE, 1), dtype=torch.float32, device=dev) for _ in range(C)]
    lib, modes = _lib.load(), np.full(C, CH_NORM, np.int32)
    st = lambda: torch.cuda.current_stream().cuda_stream

    def mc():
        _lib.check(lib.sq_frames_to_tiles_mc(x.data_ptr(), PIX[x.dtype], x.stride(0), modes.ctypes.data, mean.data_ptr(),
                                             std.data_ptr(), None, None, None, one._oy.data_ptr(), one._ox.data_ptr(),
                                             out.data_ptr(), F, H, W, C, one.TR, one.TC, TILE, st()), 'sq_frames_to_tiles_mc')

    def composed():
        for c in range(C):
            _lib.check(lib.sq_frames_to_tiles(x[c].data_ptr(), PIX[x.dtype], mean[c].data_ptr(), std[c].data_ptr(),
                                              one._oy.data_ptr(), one._ox.data_ptr(), singles[c].data_ptr(), F, H, W, one.TR,
                                              one.TC, TILE, st()), 'sq_frames_to_tiles')
        torch.stack([s[..., 0] for s in singles], -1, out=out)

    mc()
    a = out.clone()
    composed()
    assert torch.equal(a.view(torch.int32), out.view(torch.int32)), 'mc and the composition differ'
    clean = FrameClean(outliers=(3, 500.), bgsubtract=True)
    scratch_mc = many.clean_scratch(F, clean)
    scratch_one = one.clean_scratch(F, clean)
    variants = {'mc': mc, 'composed': composed,
                'mc_clean': lambda: many.tiles(x, clean=clean, scratch=scratch_mc),
                'composed_clean': lambda: torch.stack([one.tiles(x[c], clean=clean, scratch=scratch_one)[..., 0]
                                                       for c in range(C)], -1)}
    t = _race(variants, args.warmup, args.iters)
    covered = F * one.TR * one.TC * TILE * TILE
    nbytes = covered * C * (2 + 4)
    res = {k: _row(v, nbytes if k in ('mc', 'composed') else None) for k, v in t.items()}
    res['mc_vs_composed'] = _verdict(res['mc'], res['composed'])
    res['mc_clean_vs_composed_clean'] = _verdict(res['mc_clean'], res['composed_clean'])
    res['compulsory_bytes'] = int(nbytes)

    import time
    host_frames = x.cpu().numpy()
    ht = []
    for _ in range(2):
        t0 = time.perf_counter()
        tiles = np.empty((N, TILE, TILE, C), np.float32)
        for c in range(C):
            k = 0
            for f in range(F):
                g = host_frames[c, f].astype(np.float32)
                g = (g - np.mean(g)) / (1e-99 + np.std(g))
                for y in one.oy:
                    for xx in one.ox:
                        tiles[k, :, :, c] = g[y:y + TILE, xx:xx + TILE]
                        k += 1
        torch.from_numpy(tiles).to(dev)
        torch.cuda.synchronize()
        ht.append((time.perf_counter() - t0) * 1e3)
    res['host'] = {'ms_min': round(min(ht), 1), 'ms_median': round(float(np.median(ht)), 1), 'runs': len(ht)}
    del tiles, out, singles, a

    B = 4                                                       # one segment_frames batch
    net = UNet2D({'shape': (TILE, TILE), 'num_inputs': C, 'num_outputs': CLASSES, 'device': dev, 'seed': 0}, 'infer')
    net.initialize()
    xb = x[:, :B]
    batch = lambda: many.stitch(net.predict(many.tiles(xb)))
    for _ in range(2):
        batch()
    torch.cuda.synchronize()
    tb = [_time(batch, 1) for _ in range(5)]
    tt = [_time(lambda: many.tiles(xb), 1) for _ in range(args.iters)]
    res['segment_share'] = {'batch_frames': B, 'batch_ms': round(float(np.median(tb)), 3), 'tiles_ms': round(float(np.median(tt)), 4),
                            'share': round(float(np.median(tt)) / float(np.median(tb)), 5)}
    del net
    torch.cuda.empty_cache()
    return res


def bench_sampler(CI, planes, lab, wmap, args, dev):
    from sequitr_amd.frontend import TileSampler, tile_sample_plan
    from sequitr_amd.train import UNetTrainer
    F, H, W = FRAMES
    x = planes[:CI]
    tile = (TILE, TILE)
    old = TileSampler((H, W), tile, dev)
    new = TileSampler((H, W), tile, dev, channels=CI)
    stats = new.stats(x)
    rng = np.random.default_rng(0)
    thetas = {'theta_0': np.zeros(BATCH), 'theta_pi_4': np.full(BATCH, np.pi / 4), 'theta_random': rng.uniform(0, 2 * np.pi, BATCH)}
    rows = {k: tuple(torch.from_numpy(a).to(dev) for a in tile_sample_plan((H, W), tile, F, BATCH, np.random.default_rng(1), theta=v))
            for k, v in thetas.items()}
    bufs = [torch.empty((BATCH,) + tile + (CI,), dtype=torch.float32, device=dev),
            torch.empty((BATCH,) + tile + (CLASSES,), dtype=torch.uint8, device=dev),
            torch.empty((BATCH,) + tile + (1,), dtype=torch.float32, device=dev)]
    parts = [torch.empty((BATCH,) + tile + (1,), dtype=torch.float32, device=dev) for _ in range(CI)]

    def mc(name):
        new.sample(x, lab, wmap, rows[name][0], rows[name][1], CLASSES, stats=stats, out=bufs)

    def composed(name):
        plan, coef = rows[name]
        old.sample(x[0], lab, wmap, plan, coef, CLASSES, stats=(stats[0][0], stats[1][0]), out=(parts[0], bufs[1], bufs[2]))
        for c in range(1, CI):
            old.sample(x[c], None, None, plan, coef, CLASSES, stats=(stats[0][c], stats[1][c]), out=(parts[c], None, None))
        torch.stack([p[..., 0] for p in parts], -1, out=bufs[0])

    variants = {}
    for name in thetas:
        mc(name)
        a = [b.clone() for b in bufs]
        composed(name)
        assert all(torch.equal(u.view(torch.uint8), v.view(torch.uint8)) for u, v in zip(a, bufs)), name
        variants[(name, 'mc')] = (lambda n=name: mc(n))
        variants[(name, 'composed')] = (lambda n=name: composed(n))
    t = _race(variants, args.warmup, args.iters)
    px = BATCH * TILE * TILE
    nbytes = px * ((2 * CI + 1 + 4) + (4 * CI + CLASSES + 4))
    res = {}
    for name in thetas:
        row = {form: _row(t[(name, form)], nbytes) for form in ('mc', 'composed')}
        row['mc_vs_composed'] = _verdict(row['mc'], row['composed'])
        res[name] = row
    res['compulsory_bytes'] = int(nbytes)
    steps = {}
    for dtype in ('f32', 'bf16'):
        trainer = UNetTrainer({'shape': tile, 'num_inputs': CI, 'num_outputs': CLASSES, 'device': dev, 'seed': 0, 'dtype': dtype})
        mc('theta_random')
        trainer.capture(*bufs, warmup=1)
        static = trainer.static_inputs
        plan, coef = rows['theta_random']
        sample_static = lambda: new.sample(x, lab, wmap, plan, coef, CLASSES, stats=stats, out=static)
        for _ in range(2):
            sample_static()
            trainer.step(*static)
        torch.cuda.synchronize()
        stp = [_time(lambda: trainer.step(*static), 1) for _ in range(5)]
        sm = [_time(sample_static) for _ in range(args.iters)]
        steps[dtype] = {'step_ms': round(float(np.median(stp)), 3), 'sampling_ms': round(float(np.median(sm)), 4),
                        'sampling_share': round(float(np.median(sm)) / float(np.median(stp)), 5)}
        del trainer
        torch.cuda.empty_cache()
    res['step'] = steps
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'multichannel_bench.json'))
    args = ap.parse_args()
    if args.iters < 20:
        raise SystemExit('at least 20 timed windows')
    if not torch.cuda.is_available():
        line = not_measured()
    else:
        torch.cuda.set_device(0)
        dev = 'cuda:0'
        rng = np.random.default_rng(0)
        planes = torch.from_numpy(rng.integers(100, 4000, (max(CHANNELS),) + FRAMES).astype(np.uint16)).to(dev)
        lab = torch.from_numpy(rng.integers(0, CLASSES, FRAMES).astype(np.uint8)).to(dev)
        wmap = torch.rand(FRAMES, device=dev) + 0.5
        line = {'workload': '%d x %d x %d uint16 frames per channel, channel-major planes; tiles of %d, margin %d; sampler '
                            'batches of %d tiles' % (FRAMES + (TILE, MARGIN, BATCH)),
                'device': torch.cuda.get_device_name(0), 'warmup': args.warmup, 'windows': args.iters, 'calls_per_window': REPS,
                'hbm_achievable_gb_per_s': HBM_ACHIEVABLE_GBS,
                'tile_cutter': {'C=%d' % c: bench_cutter(c, planes, args, dev) for c in CHANNELS},
                'sampler': {'CI=%d' % c: bench_sampler(c, planes, lab, wmap, args, dev) for c in CHANNELS}}
    text = json.dumps(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
