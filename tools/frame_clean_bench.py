"""Frame cleaning benchmark: one JSON line, also written to profiles/frame_clean_bench.json.

Workload: 8 uint16 frames of 2048 x 2048 generated here from a seed (a quadratic ramp, noise, 1 % hot pixels), resident in
HBM.  HIP events round each kernel after warm-up, the steps alternated call by call so that drift hits all alike:
  * outliers_size2 / outliers_size3 : sq_frame_outliers_f32 (uint16 in, float32 out)
  * fit                             : sq_frame_bgfit_f64 (moments + solve)
  * residual_stats                  : sq_frame_bg_stats_f64
  * tile_kernel                     : sq_frames_to_tiles_bg at tile 512, margin 32
  * norm_only                       : the existing ImageNorm-only front end on the raw frames (sq_frame_stats +
                                      sq_frames_to_tiles), the comparison of record
Bytes are what the step has to move (reads + writes, from the shapes); GB/s stands next to the 6.3 TB/s an HBM-bound
kernel can reach on the MI355X.  `batch` is tiles -> net.predict -> stitch for the 8 frames with the default U-Net, once
with the three-pipe chain and once with ImageNorm alone; `chain_share` / `norm_only_share` are the front-end kernels' event
time over it.  `host_one_frame_ms` is the same chain through sequitr_amd.pipeline on the host for one frame.
Usage: python tools/frame_clean_bench.py [--warmup 2] [--iters 7] [--out PATH]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

F, H, W, TILE, MARGIN = 8, 2048, 2048, 512, 32
HBM_ACHIEVABLE_GBS = 6300.


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _frames():
    rng = np.random.default_rng(0)
    v, u = np.mgrid[0:H, 0:W].astype(np.float32)
    s, t = u / (W - 1) - 0.5, v / (H - 1) - 0.5
    out = np.empty((F, H, W), np.uint16)
    for f in range(F):
        img = 1500 * (1 + 0.3 * s - 0.2 * t - 0.4 * s * s + 0.1 * s * t - 0.3 * t * t) + 12 * rng.standard_normal((H, W), np.float32)
        img[rng.random((H, W)) < 0.01] += 4000
        out[f] = np.rint(img)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--iters', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'frame_clean_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('frame_clean_bench needs the GPU')
    from sequitr_amd import _lib, pipeline
    from sequitr_amd.frontend import FrameClean, FrameTiler
    from sequitr_amd.networks.unet import UNet2D
    torch.cuda.set_device(0)
    dev = 'cuda:0'
    host = _frames()
    raw = torch.from_numpy(host).to(dev)
    tl = FrameTiler((H, W), TILE, MARGIN, device=dev)
    clean = FrameClean(outliers=(2, 50.), bgsubtract=True)
    scratch = tl.clean_scratch(F, clean)
    f32 = tl.outliers(raw, 2, 50.)
    coef = tl.background(f32, scratch=scratch)
    tl.background_stats(f32, coef, scratch=scratch)
    net = UNet2D({'shape': (TILE, TILE), 'device': dev}, 'infer').initialize()
    npix, tile_px = F * H * W, F * tl.tiles_per_frame * TILE * TILE
    mean, std = scratch['mean64'], scratch['std64']
    tiles_out = torch.empty((F * tl.tiles_per_frame, TILE, TILE, 1), dtype=torch.float32, device=dev)
    lib = _lib.load()

    def tile_kernel():
        _lib.check(lib.sq_frames_to_tiles_bg(f32.data_ptr(), coef.data_ptr(), mean.data_ptr(), std.data_ptr(), tl._oy.data_ptr(),
                                             tl._ox.data_ptr(), tiles_out.data_ptr(), F, H, W, tl.TR, tl.TC, TILE,
                                             torch.cuda.current_stream().cuda_stream), 'sq_frames_to_tiles_bg')

    steps = {'outliers_size2': lambda: tl.outliers(raw, 2, 50., out=scratch['f32'][0]),   # the one channel's planes
             'outliers_size3': lambda: tl.outliers(raw, 3, 50., out=scratch['f32'][0]),
             'fit': lambda: tl.background(f32, scratch=scratch),
             'residual_stats': lambda: tl.background_stats(f32, coef, scratch=scratch),
             'tile_kernel': tile_kernel,
             'norm_only': lambda: tl.tiles(raw)}
    nbytes = {'outliers_size2': npix * (2 + 4), 'outliers_size3': npix * (2 + 4), 'fit': npix * 4, 'residual_stats': npix * 4,
              'tile_kernel': tile_px * (4 + 4),                 # every tile pixel read as float32, written as float32
              'norm_only': npix * 2 * 2 + tile_px * (2 + 4)}    # the raw frame read twice for the statistics, then cut

    def batch(with_chain):
        tiles = tl.tiles(raw, clean=clean, scratch=scratch) if with_chain else tl.tiles(raw)
        per = 2 * tl.tiles_per_frame                            # the network takes two frames' tiles per launch
        return [tl.stitch(net.predict(tiles[k:k + per])) for k in range(0, tiles.shape[0], per)]

    for _ in range(args.warmup):
        for fn in steps.values():
            fn()
        batch(True)
        batch(False)
    torch.cuda.synchronize()
    t = {name: [] for name in steps}
    t_batch = {True: [], False: []}
    for _ in range(args.iters):
        for name, fn in steps.items():
            t[name].append(_time(fn))
        for with_chain in (True, False):
            t_batch[with_chain].append(_time(lambda: batch(with_chain)))
    med = {name: float(np.median(v)) for name, v in t.items()}
    rows = {}
    for name in steps:
        gbs = nbytes[name] / max(med[name], 1e-9) / 1e6
        rows[name] = {'ms': round(med[name], 4), 'ms_min_max': [round(min(t[name]), 4), round(max(t[name]), 4)],
                      'bytes': int(nbytes[name]), 'gb_per_s': round(gbs, 1),
                      'fraction_of_hbm_achievable': round(gbs / HBM_ACHIEVABLE_GBS, 4)}
    chain_ms = med['outliers_size2'] + med['fit'] + med['residual_stats'] + med['tile_kernel']
    b_chain, b_norm = float(np.median(t_batch[True])), float(np.median(t_batch[False]))
    chain_host = pipeline.ImagePipeline([pipeline.ImageOutliers(2, 50.), pipeline.ImageBGSubtract(), pipeline.ImageNorm()])
    t0 = time.perf_counter()
    chain_host(np.array(host[0]))
    host_ms = (time.perf_counter() - t0) * 1e3
    line = {'workload': 'frame cleaning: %d x %d x %d uint16 in HBM, ImageOutliers(2, 50.) -> ImageBGSubtract -> ImageNorm, tile %d '
                        'margin %d, UNet2D default filters' % (F, H, W, TILE, MARGIN),
            'warmup': args.warmup, 'iters': args.iters, 'device': torch.cuda.get_device_name(0),
            'hbm_achievable_gb_per_s': HBM_ACHIEVABLE_GBS, 'steps': rows,
            'chain_ms': round(chain_ms, 4), 'chain_mpixels_per_s': round(npix / chain_ms / 1e3, 1),
            'batch': {'with_chain_ms': round(b_chain, 3), 'with_chain_ms_min_max': [round(min(t_batch[True]), 3), round(max(t_batch[True]), 3)],
                      'norm_only_ms': round(b_norm, 3), 'norm_only_ms_min_max': [round(min(t_batch[False]), 3), round(max(t_batch[False]), 3)]},
            'chain_share': round(chain_ms / b_chain, 5), 'norm_only_share': round(med['norm_only'] / b_norm, 5),
            'host_one_frame_ms': round(host_ms, 1), 'host_over_device_per_frame': round(host_ms / (chain_ms / F), 1)}
    text = json.dumps(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
