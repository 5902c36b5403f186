"""Volume front end benchmark: one JSON line, also written to profiles/volume_frontend_bench.json.

Workload: one 64 x 1024 x 1024 uint16 volume generated here from a seed, UNet3D with the default filters, brick
(32, 128, 128), margin (4, 16, 16) in (Z, X, Y) order, 8 bricks per network launch.  HIP events round each step over the
whole volume after warm-up, the HIP kernels and a torch composition of the same step alternated call by call:
  * stats      : VolumeTiler.stats                          | x.float().mean(), x.float().std(unbiased=False)
  * cut        : VolumeTiler.bricks, batch by batch          | out[j] = (vol[box].float() - mean) / std, brick by brick
  * scatter_u8 : VolumeTiler.scatter of uint8 masks          | out[owned box] = masks[j][owned box], brick by brick
  * scatter_f32: VolumeTiler.scatter of float32 logits, C=2  | the same on logits
Bytes are what the step has to move (reads + writes, computed from the shapes); GB/s stands next to the 6.3 TB/s an
HBM-bound kernel can reach on the MI355X.  `volume` is one whole pass in HBM (stats, then per batch cut -> net.predict ->
scatter of the masks), `frontend_share` the three kernels' event time over it; `job` is SERVER_segment_volume with
params['brick'] on the same volume from host memory (Mvoxel/s of its own timed region).
Usage: python tools/volume_frontend_bench.py [--warmup 2] [--iters 5] [--out PATH]
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

SHAPE, BRICK, MARGIN, BATCH = (64, 1024, 1024), (32, 128, 128), (4, 16, 16), 8
HBM_ACHIEVABLE_GBS = 6300.


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'volume_frontend_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('volume_frontend_bench needs the GPU')
    from sequitr_amd import jobs
    from sequitr_amd.frontend import VolumeTiler
    from sequitr_amd.networks.unet import UNet3D
    torch.cuda.set_device(0)
    dev = 'cuda:0'
    Z, X, Y = SHAPE
    host = np.random.default_rng(0).integers(100, 4000, (1,) + SHAPE).astype(np.uint16)
    vol = torch.from_numpy(host).to(dev)
    tiler = VolumeTiler(SHAPE, BRICK, MARGIN, device=dev)
    g, nb = tiler.geometry, tiler.bricks_per_volume
    boxes = [g.box(k) for k in range(nb)]
    batches = [(first, min(BATCH, nb - first)) for first in range(0, nb, BATCH)]
    net = UNet3D({'shape': (BRICK[1], BRICK[2], BRICK[0]), 'num_outputs': 2, 'device': dev}, 'infer').initialize()
    C = int(net.n_outputs)
    masks = torch.randint(0, 2, (BATCH,) + BRICK, dtype=torch.uint8, device=dev)
    logits = torch.randn((BATCH,) + BRICK + (C,), device=dev)
    out_u8 = torch.empty((1,) + SHAPE, dtype=torch.uint8, device=dev)
    out_f32 = torch.empty((1,) + SHAPE + (C,), dtype=torch.float32, device=dev)
    t_bricks = torch.empty((BATCH,) + BRICK + (1,), dtype=torch.float32, device=dev)
    stats = tiler.stats(vol)

    def hip_cut():
        for first, n in batches:
            tiler.bricks(vol, first, n, stats=stats)

    def hip_scatter(values, out):
        for first, n in batches:
            tiler.scatter(values[:n], out, first)

    def torch_stats():
        x = vol[0].float()
        return x.mean(), x.std(unbiased=False)

    def torch_cut():
        mean, std = stats[0][0], stats[1][0]
        for first, n in batches:
            for j in range(n):
                (oz, ox, oy), _, _ = boxes[first + j]
                t_bricks[j, ..., 0] = (vol[0, oz:oz + BRICK[0], ox:ox + BRICK[1], oy:oy + BRICK[2]].float() - mean) / std

    def torch_scatter(values, out):
        for first, n in batches:
            for j in range(n):
                (oz, ox, oy), (lz, lx, ly), (hz, hx, hy) = boxes[first + j]
                out[0, lz:hz, lx:hx, ly:hy] = values[j, lz - oz:hz - oz, lx - ox:hx - ox, ly - oy:hy - oy]

    def volume_pass():
        st = tiler.stats(vol)
        for first, n in batches:
            tiler.scatter(net.predict(tiler.bricks(vol, first, n, stats=st)), out_u8, first)

    steps = {'stats': (lambda: tiler.stats(vol), torch_stats),
             'cut': (hip_cut, torch_cut),
             'scatter_u8': (lambda: hip_scatter(masks, out_u8), lambda: torch_scatter(masks, out_u8)),
             'scatter_f32': (lambda: hip_scatter(logits, out_f32), lambda: torch_scatter(logits, out_f32))}
    brick_vox, owned = nb * BRICK[0] * BRICK[1] * BRICK[2], Z * X * Y
    nbytes = {'stats': 2 * owned * 2,                           # the volume read twice (mean, variance)
              'cut': brick_vox * (2 + 4),                       # every brick voxel read as uint16, written as float32
              'scatter_u8': 2 * owned,                          # every voxel of the volume read from its brick, written once
              'scatter_f32': 2 * owned * C * 4}
    for _ in range(args.warmup):
        for hip, ref in steps.values():
            hip()
            ref()
        volume_pass()
    torch.cuda.synchronize()
    t = {name: ([], []) for name in steps}
    t_vol = []
    for _ in range(args.iters):                                 # alternate the variants so drift hits all alike
        for name, (hip, ref) in steps.items():
            t[name][0].append(_time(hip))
            t[name][1].append(_time(ref))
        t_vol.append(_time(volume_pass))
    rows = {}
    for name in steps:
        hip_ms, torch_ms = float(np.median(t[name][0])), float(np.median(t[name][1]))
        gbs = nbytes[name] / hip_ms / 1e6
        rows[name] = {'hip_ms': round(hip_ms, 4), 'hip_ms_min_max': [round(min(t[name][0]), 4), round(max(t[name][0]), 4)],
                      'bytes': int(nbytes[name]), 'hip_gb_per_s': round(gbs, 1),
                      'fraction_of_hbm_achievable': round(gbs / HBM_ACHIEVABLE_GBS, 4),
                      'torch_ms': round(torch_ms, 4), 'torch_ms_min_max': [round(min(t[name][1]), 4), round(max(t[name][1]), 4)],
                      'torch_over_hip': round(torch_ms / hip_ms, 3), 'hip_slower_than_torch': bool(hip_ms > torch_ms)}
    vol_ms = float(np.median(t_vol))
    front_ms = rows['stats']['hip_ms'] + rows['cut']['hip_ms'] + rows['scatter_u8']['hip_ms']
    with tempfile.TemporaryDirectory() as out_dir:              # the job, from host memory, its own warm-up and timing
        info = jobs.SERVER_segment_volume({'input': host, 'output': out_dir, 'num_outputs': 2, 'bricks_per_batch': BATCH,
                                           'brick': (BRICK[1], BRICK[2], BRICK[0]),
                                           'margin': (MARGIN[1], MARGIN[2], MARGIN[0])}, {'gpu': 0})
    line = {'workload': 'volume front end: 1 x %d x %d x %d uint16, UNet3D default filters, brick %s margin %s (Z, X, Y), '
                        '%d bricks, %d per launch' % (SHAPE + (list(BRICK), list(MARGIN), nb, BATCH)),
            'warmup': args.warmup, 'iters': args.iters, 'device': torch.cuda.get_device_name(0),
            'hbm_achievable_gb_per_s': HBM_ACHIEVABLE_GBS, 'steps': rows,
            'volume': {'ms': round(vol_ms, 3), 'ms_min_max': [round(min(t_vol), 3), round(max(t_vol), 3)],
                       'mvoxels_per_s': round(owned / vol_ms / 1e3, 1),
                       'brick_voxels_over_volume_voxels': round(brick_vox / owned, 3)},
            'frontend_ms': round(front_ms, 4), 'frontend_share': round(front_ms / vol_ms, 5),
            'job': {'mvoxels_per_s': round(info['mvoxels_per_s'], 1), 'seconds': round(info['seconds'], 4),
                    'setup_seconds': round(info['setup_seconds'], 3), 'bricks_per_volume': info['bricks_per_volume']}}
    text = json.dumps(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
