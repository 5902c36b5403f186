"""Seam-blending benchmark: one JSON line, also written to profiles/blend_bench.json.

Workload: 8 frames of 2048 x 2048, tile 512 and margin 32 (25 tiles a frame), K = 2 classes; blend 8 and 32.  HIP events
round REPS calls after warm-up, all variants alternated window by window in one run, the median of `--iters` windows:
  * probs  : sq_stitch_probs on the 200 x 512 x 512 x 2 logits, one owner per pixel -- the yardstick;
  * blend  : sq_stitch_blend on the same logits at each blend width;
  * torch  : the composition a user would write: every tile's logits times its outer-product tent weights accumulated into
    its frame slice (25 slice-adds a frame stack, ky then kx ascending: the header's order), the divide, softmax, argmax.
Each with mask + float32 probabilities; `mask_only` repeats probs and blend for the mask alone.  Bytes are what a call has
to move (the logits of every contributing tile of every pixel, the mask, the planes; the slot tables stay in cache); GB/s
stands next to the 6.3 TB/s an HBM-bound kernel can reach on the MI355X.  `band_share` is the share of the pixels with more
than one contributor, `blend_over_probs` the yardstick ratio, `torch_over_blend` the composition's.  `agree`: the kernel's
mask equals the composition's and the probabilities differ by at most the header's bound, at every blend, and blend 0
equals sq_stitch_probs bit for bit.  `segment_frames` is the whole path, host frames in and host masks out, ms per frame at
blend None / 8 / 32 with the default network, and `stitch_share` the stitch launch's part of a batch.
Without a GPU the tool refuses to run; --placeholder writes the file with "not measured" in every field.
Usage: python tools/blend_bench.py [--warmup 2] [--iters 7] [--frames-iters 5] [--out PATH] [--placeholder]
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

FRAMES, SIDE, TILE, MARGIN, K, BATCH = 8, 2048, 512, 32, 2, 4
BLENDS = (8, 32)
HBM_ACHIEVABLE_GBS = 6300.
REPS = 20                                                       # calls per event pair
NM = 'not measured'
WORKLOAD = ('seam blending: %d frames of %d x %d, tile %d margin %d, K = %d; blend %s; batches of %d frames'
            % (FRAMES, SIDE, SIDE, TILE, MARGIN, K, ' and '.join(str(b) for b in BLENDS), BATCH))
ROW = ('ms', 'ms_min_max', 'gb_per_s', 'fraction_of_hbm_achievable')
BLEND_FIELDS = ('band_share', 'bytes', 'blend', 'torch', 'blend_over_probs', 'torch_over_blend', 'mask_only',
                'mask_only_over_probs')
STREAM_FIELDS = ('ms_per_frame', 'ms_per_frame_min_max', 'stitch_ms_per_batch', 'stitch_share', 'over_plain')


def placeholder():
    return {'workload': WORKLOAD, 'device': NM, 'hbm_achievable_gb_per_s': HBM_ACHIEVABLE_GBS,
            'probs': {f: NM for f in ROW + ('bytes',)}, 'probs_mask_only': {f: NM for f in ROW + ('bytes',)},
            'blend': {str(b): {f: NM for f in BLEND_FIELDS} for b in BLENDS},
            'segment_frames': {str(b): {f: NM for f in STREAM_FIELDS} for b in (None,) + BLENDS},
            'agree': NM, 'max_abs_probability_difference': NM, 'probability_bound': (K + 4) * 2.0 ** -23}


def measure(args):
    import torch
    from sequitr_amd.frontend import FrameTiler, axis_blend, segment_frames
    from sequitr_amd.networks.unet import UNet2D
    torch.cuda.set_device(0)
    dev = 'cuda:0'

    def timed(fn, reps=1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    def row(ts, nbytes):
        m = float(np.median(ts))
        return {'ms': round(m, 4), 'ms_min_max': [round(min(ts), 4), round(max(ts), 4)], 'gb_per_s': round(nbytes / m / 1e6, 1),
                'fraction_of_hbm_achievable': round(nbytes / m / 1e6 / HBM_ACHIEVABLE_GBS, 4)}

    tiler = FrameTiler((SIDE, SIDE), TILE, MARGIN, device=dev)
    nt = FRAMES * tiler.tiles_per_frame
    logits = torch.randn((nt, TILE, TILE, K), device=dev) * 4
    npix = FRAMES * SIDE * SIDE

    # the torch composition: per tile (weights (T, T, 1), the frame slice it lands on, the tile's part with positive weight)
    plans = {}
    for B in BLENDS:
        per_axis = []
        for L, origins in ((SIDE, tiler.oy), (SIDE, tiler.ox)):
            slots = axis_blend(L, TILE, MARGIN, B)[1].astype(np.int64)
            w = np.zeros((len(origins), L), np.int64)
            live = slots[:, :, 1] > 0
            w[(slots[:, :, 0] >> 16)[live], np.nonzero(live)[0]] = slots[:, :, 1][live]
            per_axis.append(w)
        wy, wx = per_axis
        tiles = []
        for ky in range(tiler.TR):
            ys = np.flatnonzero(wy[ky])
            for kx in range(tiler.TC):
                xs = np.flatnonzero(wx[kx])
                w2 = torch.from_numpy((wy[ky, ys][:, None] * wx[kx, xs][None, :]).astype(np.float32)).to(dev)[:, :, None]
                tiles.append((ky * tiler.TC + kx, int(ys[0]), int(ys[-1]) + 1, int(xs[0]), int(xs[-1]) + 1,
                              int(ys[0] - tiler.oy[ky]), int(xs[0] - tiler.ox[kx]), w2))
        wt = torch.from_numpy((wy.sum(0)[:, None] * wx.sum(0)[None, :]).astype(np.float32)).to(dev)[None, :, :, None]
        contributors = int(((wy > 0).sum(0)[:, None] * (wx > 0).sum(0)[None, :]).sum())
        band = float((((wy > 0).sum(0)[:, None] * (wx > 0).sum(0)[None, :]) > 1).mean())
        plans[B] = (tiles, wt, contributors, band)
    by_frame = logits.view(FRAMES, tiler.tiles_per_frame, TILE, TILE, K)
    S = torch.empty((FRAMES, SIDE, SIDE, K), device=dev)

    def torch_blend(B):
        tiles, wt, _, _ = plans[B]
        S.zero_()
        for t, y0, y1, x0, x1, ly, lx, w2 in tiles:
            S[:, y0:y1, x0:x1] += w2 * by_frame[:, t, ly:ly + y1 - y0, lx:lx + x1 - x0]
        b = S / wt
        return b.argmax(-1).to(torch.uint8), torch.softmax(b * 0.125, -1).permute(0, 3, 1, 2).contiguous()

    variants, nbytes = {}, {}
    variants[('probs', 'both')] = lambda: tiler.stitch_probs(logits, n=8, probabilities='float32')
    variants[('probs', 'mask')] = lambda: tiler.stitch_probs(logits, n=8)
    nbytes[('probs', 'both')], nbytes[('probs', 'mask')] = npix * (K * 4 + 1 + K * 4), npix * (K * 4 + 1)
    for B in BLENDS:
        reads = FRAMES * plans[B][2] * K * 4
        variants[('blend', B, 'both')] = lambda B=B: tiler.stitch_blend(logits, B, n=8, probabilities='float32')
        variants[('blend', B, 'mask')] = lambda B=B: tiler.stitch_blend(logits, B, n=8)
        variants[('torch', B, 'both')] = lambda B=B: torch_blend(B)
        nbytes[(B, 'both')], nbytes[(B, 'mask')] = reads + npix * (1 + K * 4), reads + npix

    # the variants agree before anything is timed
    bound, agree, worst = (K + 4) * 2.0 ** -23, True, 0.0
    m0, p0 = tiler.stitch_blend(logits, 0, n=8, probabilities='float32')
    m1, p1 = variants[('probs', 'both')]()
    agree &= bool(torch.equal(m0, m1) and torch.equal(p0.view(torch.int32), p1.view(torch.int32)))
    for B in BLENDS:
        m_hip, p_hip = variants[('blend', B, 'both')]()
        m_ref, p_ref = torch_blend(B)
        worst = max(worst, float((p_hip - p_ref).abs().max()))
        agree &= bool(torch.equal(m_hip, m_ref)) and worst <= 2 * bound
    del m0, p0, m1, p1, m_hip, p_hip, m_ref, p_ref

    for _ in range(args.warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(args.iters):                                 # interleaved rounds: drift hits all variants alike
        for k, fn in variants.items():
            t[k].append(timed(fn, REPS))
    probs = dict(row(t[('probs', 'both')], nbytes[('probs', 'both')]), bytes=int(nbytes[('probs', 'both')]))
    probs_mask = dict(row(t[('probs', 'mask')], nbytes[('probs', 'mask')]), bytes=int(nbytes[('probs', 'mask')]))
    blend = {}
    for B in BLENDS:
        h, r = row(t[('blend', B, 'both')], nbytes[(B, 'both')]), row(t[('torch', B, 'both')], nbytes[(B, 'both')])
        mo = row(t[('blend', B, 'mask')], nbytes[(B, 'mask')])
        blend[str(B)] = {'band_share': round(plans[B][3], 4), 'bytes': int(nbytes[(B, 'both')]), 'blend': h, 'torch': r,
                         'blend_over_probs': round(h['ms'] / probs['ms'], 3), 'torch_over_blend': round(r['ms'] / h['ms'], 3),
                         'mask_only': mo, 'mask_only_over_probs': round(mo['ms'] / probs_mask['ms'], 3)}
    del logits, by_frame, S, plans
    torch.cuda.empty_cache()

    # the whole path, and the stitch launch's part of one batch of BATCH frames
    rng = np.random.default_rng(0)
    frames = rng.integers(100, 4000, (FRAMES, SIDE, SIDE)).astype(np.uint16)
    net = UNet2D({'shape': (TILE, TILE), 'num_outputs': K, 'device': dev, 'seed': 0}, 'infer').initialize()
    bl = torch.randn((BATCH * tiler.tiles_per_frame, TILE, TILE, K), device=dev)
    whole = {}
    for B in (None,) + BLENDS:
        run = lambda: segment_frames(net, frames, tile=TILE, margin=MARGIN, frames_per_batch=BATCH, blend=B)
        run()
        ts = []
        for _ in range(args.frames_iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            ts.append((time.perf_counter() - t0) * 1e3 / FRAMES)
        whole[str(B)] = {'ms_per_frame': round(float(np.median(ts)), 3), 'ms_per_frame_min_max': [round(min(ts), 3), round(max(ts), 3)]}
        if B is None:                                           # today's path stitches uint8 tile masks: no logits survive
            whole[str(B)].update({'stitch_ms_per_batch': NM, 'stitch_share': NM, 'over_plain': 1.0})
            continue
        launch = lambda: tiler.stitch_blend(bl, B)
        launch()
        ls = [timed(launch, REPS) for _ in range(args.iters)]
        whole[str(B)].update({'stitch_ms_per_batch': round(float(np.median(ls)), 4),
                              'stitch_share': round(float(np.median(ls)) / (whole[str(B)]['ms_per_frame'] * BATCH), 5),
                              'over_plain': round(whole[str(B)]['ms_per_frame'] / whole['None']['ms_per_frame'], 3)})
    return dict(placeholder(), device=torch.cuda.get_device_name(0), warmup=args.warmup, iters=args.iters, calls_per_window=REPS,
                probs=probs, probs_mask_only=probs_mask, blend=blend, segment_frames=whole, agree=bool(agree),
                max_abs_probability_difference=worst)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--iters', type=int, default=7)
    ap.add_argument('--frames-iters', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'blend_bench.json'))
    ap.add_argument('--placeholder', action='store_true', help='write "not measured" in every field (no GPU needed)')
    args = ap.parse_args()
    if args.placeholder:
        line = placeholder()
    else:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit('blend_bench needs the GPU (--placeholder writes the file without one)')
        line = measure(args)
    text = json.dumps(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
