"""ImageBlur benchmark: one JSON line, also written to profiles/frame_blur_bench.json.

Workload: the 8 uint16 frames of 2048 x 2048 of tools/frame_clean_bench.py (same generator, same seed), resident in HBM.
Per sigma 0.5 / 1.5 / 4 / 8 (radius 2 / 6 / 16 / 32), HIP events round every call after warm-up, the steps alternated call by
call so that drift hits all alike:
  * blur     : sq_frame_blur_f32 (uint16 in, float32 out), one launch; ms (median, minimum and maximum of the windows) and
               GB/s of the 6 B per pixel a call must move, next to the 6.3 TB/s an HBM-bound kernel can reach
  * outliers : sq_frame_outliers_f32 at size 3 -- the same traffic shape, the nearest yardstick in the tree
  * torch    : a composition -- the reflected border gathered by index, then two float64 conv2d passes (axis 0, axis 1) with
               the rounding to float32 in between and after -- with its largest difference from the kernel
  * host     : pipeline.ImageBlur on one frame (scipy), host clock
`stream` is the per-frame host-clock time of frontend.segment_frames over the same frames (tile 512, margin 32, 4 frames per
batch, UNet2D default filters) with clean=FrameClean(blur=1.5) and without, alternated.
A field that could not be measured says "not measured" (with the reason where there is one).
Usage: python tools/frame_blur_bench.py [--warmup 2] [--iters 7] [--stream-iters 3] [--out PATH]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from frame_clean_bench import F, H, W, HBM_ACHIEVABLE_GBS, _frames, _time  # noqa: E402

SIGMAS = (0.5, 1.5, 4.0, 8.0)
NOT_MEASURED = 'not measured'


def _reflect_index(L, R):
    """scipy's mode='reflect' indices for positions -R .. L-1+R"""
    i = np.arange(-R, L + R)
    m = np.mod(i, 2 * L)
    return np.where(m < L, m, 2 * L - 1 - m)


def torch_blur(raw, sigma, blur_weights):
    """the composition: per frame (a float64 conv2d over all eight would unfold 2R + 1 copies of them at once)"""
    R, w = blur_weights(sigma)
    dev = raw.device
    k = torch.from_numpy(np.concatenate([w[:0:-1], w])).to(dev)
    iy, ix = (torch.from_numpy(_reflect_index(L, R)).to(dev) for L in (H, W))
    out = torch.empty((F, H, W), dtype=torch.float32, device=dev)
    for f in range(F):
        x = raw[f].to(torch.float32).to(torch.float64)
        x = x.index_select(0, iy).index_select(1, ix)[None, None]
        x = torch.nn.functional.conv2d(x, k.view(1, 1, -1, 1)).to(torch.float32).to(torch.float64)
        out[f] = torch.nn.functional.conv2d(x, k.view(1, 1, 1, -1))[0, 0].to(torch.float32)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--iters', type=int, default=7)
    ap.add_argument('--stream-iters', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'frame_blur_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('frame_blur_bench needs the GPU')
    from sequitr_amd import pipeline
    from sequitr_amd.frontend import FrameClean, FrameTiler, blur_weights, segment_frames
    from sequitr_amd.networks.unet import UNet2D
    torch.cuda.set_device(0)
    dev = 'cuda:0'
    host = _frames()
    raw = torch.from_numpy(host).to(dev)
    tl = FrameTiler((H, W), 512, 32, device=dev)
    out = torch.empty((F, H, W), dtype=torch.float32, device=dev)
    out2 = torch.empty_like(out)
    npix = F * H * W
    nbytes = npix * (2 + 4)

    def row(times):
        med = float(np.median(times))
        gbs = nbytes / max(med, 1e-9) / 1e6
        return {'ms': round(med, 4), 'ms_min_max': [round(min(times), 4), round(max(times), 4)], 'gb_per_s': round(gbs, 1),
                'fraction_of_hbm_achievable': round(gbs / HBM_ACHIEVABLE_GBS, 4)}

    rows, notes = {}, []
    for sigma in SIGMAS:
        R = blur_weights(sigma)[0]
        steps = {'blur': lambda: tl.blur(raw, sigma, out=out), 'outliers_size3': lambda: tl.outliers(raw, 3, 50., out=out2)}
        torch_ok = True
        try:
            composed = torch_blur(raw, sigma, blur_weights)
            diff = float((composed.double() - tl.blur(raw, sigma).double()).abs().max())
            steps['torch'] = lambda: torch_blur(raw, sigma, blur_weights)
        except Exception as e:                                  # e.g. no float64 convolution in this torch build
            torch_ok, diff = False, '%s: %s' % (NOT_MEASURED, str(e).splitlines()[0][:160])
        for _ in range(args.warmup):
            for fn in steps.values():
                fn()
        torch.cuda.synchronize()
        t = {name: [] for name in steps}
        for _ in range(args.iters):
            for name, fn in steps.items():
                t[name].append(_time(fn))
        t0 = time.perf_counter()
        pipeline.ImageBlur(sigma)(np.array(host[0]))
        host_ms = (time.perf_counter() - t0) * 1e3
        r = {'radius': R, 'blur': row(t['blur']), 'outliers_size3': row(t['outliers_size3']),
             'blur_over_outliers': round(float(np.median(t['blur']) / np.median(t['outliers_size3'])), 3),
             'torch': ({'ms': round(float(np.median(t['torch'])), 3),
                        'ms_min_max': [round(min(t['torch']), 3), round(max(t['torch']), 3)],
                        'over_blur': round(float(np.median(t['torch']) / np.median(t['blur'])), 1)} if torch_ok else NOT_MEASURED),
             'torch_max_abs_difference': diff,
             'host_one_frame_ms': round(host_ms, 1),
             'host_over_device_per_frame': round(host_ms / (float(np.median(t['blur'])) / F), 1)}
        if torch_ok and np.median(t['blur']) > np.median(t['torch']):
            notes.append('sigma %g loses to the torch composition' % sigma)
        if np.median(t['blur']) > 2 * np.median(t['outliers_size3']):
            notes.append('sigma %g takes more than twice the outliers kernel' % sigma)
        rows['sigma_%g' % sigma] = r

    net = UNet2D({'shape': (512, 512), 'device': dev}, 'infer').initialize()
    cleans = {'with_blur': FrameClean(blur=1.5), 'without': None}

    def stream(clean):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        segment_frames(net, host, tile=512, margin=32, frames_per_batch=4, clean=clean, on_masks=lambda first, m: None)
        return (time.perf_counter() - t0) * 1e3 / F             # segment_frames ends in a synchronise

    for clean in cleans.values():
        stream(clean)
    ts = {k: [] for k in cleans}
    for _ in range(args.stream_iters):
        for k, clean in cleans.items():
            ts[k].append(stream(clean))
    line = {'workload': 'ImageBlur: %d x %d x %d uint16 in HBM -> float32, one launch of sq_frame_blur_f32 per call' % (F, H, W),
            'warmup': args.warmup, 'iters': args.iters, 'device': torch.cuda.get_device_name(0),
            'hbm_achievable_gb_per_s': HBM_ACHIEVABLE_GBS, 'bytes_per_call': int(nbytes), 'sigmas': rows,
            'stream': {'what': 'segment_frames over the same frames, tile 512, margin 32, 4 frames per batch, UNet2D default '
                               'filters: clean=FrameClean(blur=1.5) against no clean, host clock per frame',
                       'with_blur_ms_per_frame': round(float(np.median(ts['with_blur'])), 3),
                       'without_ms_per_frame': round(float(np.median(ts['without'])), 3),
                       'ms_min_max': {k: [round(min(v), 3), round(max(v), 3)] for k, v in ts.items()}},
            'notes': notes}
    text = json.dumps(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
