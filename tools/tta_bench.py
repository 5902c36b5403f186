"""Test-time augmentation benchmark: one JSON line, also written to profiles/tta_bench.json.

Workload: 8 uint16 frames of 2048 x 2048, tile 512 and margin 32 (25 tiles a frame), K = 2 classes.  HIP events round each
call after warm-up, the variants alternated call by call:
  * view   : sq_tiles_view_f32 on the 200 x 512 x 512 x 2 logits of the stack, accumulating (the merge step) and plain,
    per op class -- identity (op 0), mirrored (op 3), transposed (op 5) with the LDS block (default) and with
    SQ_TTA_LDS=0, the direct gather -- and on the 200 x 512 x 512 x 1 input tiles, plain (the view step);
    next to the torch composition flip / transpose(...).contiguous() (+ add_);
  * stitch : sq_stitch_probs, mask + float32 and mask + uint8 probabilities, next to torch's softmax + argmax + index gather.
Bytes are what a call has to move (reads + writes, from the shapes); GB/s stands next to the 6.3 TB/s an HBM-bound kernel
can reach on the MI355X.  `segment_frames` is the whole path, host frames in and host masks out, ms per frame at tta None /
flips / dihedral with the default network; `tta_launches_ms` the view, merge and stitch launches of one batch timed on
their own and `tta_share` their part of the batch.  `max_abs_probability_error` is the largest |p - p64| of the float32
probabilities against torch's float64 softmax on the same logits, next to the bound (K + 4) * 2^-23.
Usage: python tools/tta_bench.py [--warmup 2] [--iters 7] [--frames-iters 3] [--out PATH]
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

FRAMES, SIDE, TILE, MARGIN, K, BATCH = 8, 2048, 512, 32, 2, 4
HBM_ACHIEVABLE_GBS = 6300.
REPS = 20                                                       # calls per event pair
OP_CLASSES = {'identity': 0, 'mirrored': 3, 'transposed': 5}


def _time(fn, reps=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def _row(ts, nbytes):
    m = float(np.median(ts))
    return {'ms': round(m, 4), 'ms_min_max': [round(min(ts), 4), round(max(ts), 4)], 'gb_per_s': round(nbytes / m / 1e6, 1),
            'fraction_of_hbm_achievable': round(nbytes / m / 1e6 / HBM_ACHIEVABLE_GBS, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--iters', type=int, default=7)
    ap.add_argument('--frames-iters', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tta_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tta_bench needs the GPU')
    from sequitr_amd.frontend import FrameTiler, segment_frames
    from sequitr_amd.networks.unet import UNet2D
    torch.cuda.set_device(0)
    dev = 'cuda:0'
    rng = np.random.default_rng(0)
    frames = rng.integers(100, 4000, (FRAMES, SIDE, SIDE)).astype(np.uint16)
    tiler = FrameTiler((SIDE, SIDE), TILE, MARGIN, device=dev)
    nt = FRAMES * tiler.tiles_per_frame
    logits = torch.randn((nt, TILE, TILE, K), device=dev) * 4
    tiles = torch.randn((nt, TILE, TILE, 1), device=dev)
    acc, out_tiles = torch.zeros_like(logits), torch.empty_like(tiles)

    def with_lds(on, fn):                                       # the switch is read per call
        def run():
            if on:
                os.environ.pop('SQ_TTA_LDS', None)
            else:
                os.environ['SQ_TTA_LDS'] = '0'
            fn()
            os.environ.pop('SQ_TTA_LDS', None)
        return run

    def torch_view(x, op):
        dims = [d for d, bit in ((1, 1), (2, 2)) if op & bit]
        x = x.flip(dims) if dims else x                         # view_op(x)[i, j] = x[f1(j), f2(i)]: mirror, then transpose
        return x.transpose(1, 2) if op & 4 else x

    variants, nbytes = {}, {}
    for cls, op in OP_CLASSES.items():
        forms = (('lds', True), ('direct', False)) if op & 4 else (('hip', True),)
        for form, on in forms:
            variants[('merge', cls, form)] = with_lds(on, lambda op=op: tiler.view(logits, op, inverse=True, out=acc, accumulate=True))
            variants[('copy', cls, form)] = with_lds(on, lambda op=op: tiler.view(logits, op, inverse=True, out=acc))
            variants[('input', cls, form)] = with_lds(on, lambda op=op: tiler.view(tiles, op, out=out_tiles))
        variants[('merge', cls, 'torch')] = lambda op=op: acc.add_(torch_view(logits, op).contiguous())
        variants[('copy', cls, 'torch')] = lambda op=op: acc.copy_(torch_view(logits, op))
        variants[('input', cls, 'torch')] = lambda op=op: out_tiles.copy_(torch_view(tiles, op))
    nbytes.update({'merge': logits.numel() * 4 * 3, 'copy': logits.numel() * 4 * 2, 'input': tiles.numel() * 4 * 2})
    # the two forms and the torch composition agree before anything is timed (op 5 inverse is op 6)
    for cls, op in OP_CLASSES.items():
        want = torch_view(logits, {5: 6}.get(op, op)).contiguous()
        for form in ('lds', 'direct') if op & 4 else ('hip',):
            variants[('copy', cls, form)]()
            assert torch.equal(acc.view(torch.int32), want.view(torch.int32)), (cls, form)

    ymap, xmap = tiler._ymap.long(), tiler._xmap.long()
    ty, ly, tx, lx = (ymap >> 16)[:, None], (ymap & 0xffff)[:, None], (xmap >> 16)[None, :], (xmap & 0xffff)[None, :]

    def torch_stitch(u8):
        p = torch.softmax(logits * 0.125, -1)
        m = logits.argmax(-1).to(torch.uint8)
        p = p.view(FRAMES, tiler.TR, tiler.TC, TILE, TILE, K)[:, ty, tx, ly, lx].permute(0, 3, 1, 2).contiguous()
        if u8:
            p = (p * 255 + 0.5).floor().to(torch.uint8)
        return m.view(FRAMES, tiler.TR, tiler.TC, TILE, TILE)[:, ty, tx, ly, lx], p

    npix = FRAMES * SIDE * SIDE
    for kind, size in (('float32', 4), ('uint8', 1)):
        variants[('stitch', kind, 'hip')] = lambda kind=kind: tiler.stitch_probs(logits, n=8, probabilities=kind)
        variants[('stitch', kind, 'torch')] = lambda kind=kind: torch_stitch(kind == 'uint8')
        nbytes[('stitch', kind)] = npix * (K * 4 + 1 + K * size)        # logits, mask, planes (the maps stay in cache)
    m_hip, p_hip = tiler.stitch_probs(logits, n=8, probabilities='float32')
    m_ref, _ = torch_stitch(False)
    assert torch.equal(m_hip, m_ref)
    rows64 = logits.view(FRAMES, tiler.TR, tiler.TC, TILE, TILE, K)[:, ty, tx, ly, lx].double() * 0.125
    p64 = torch.softmax(rows64, -1).permute(0, 3, 1, 2)
    prob_err = float((p_hip.double() - p64).abs().max())
    del rows64, p64, m_hip, p_hip, m_ref

    for _ in range(args.warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(args.iters):                                 # interleaved rounds: drift hits all variants alike
        for k, fn in variants.items():
            t[k].append(_time(fn, REPS))
    view = {}
    for step in ('merge', 'copy', 'input'):
        view[step] = {'bytes': int(nbytes[step])}
        for cls, op in OP_CLASSES.items():
            forms = ('lds', 'direct') if op & 4 else ('hip',)
            row = {form: _row(t[(step, cls, form)], nbytes[step]) for form in forms}
            row['torch'] = _row(t[(step, cls, 'torch')], nbytes[step])
            best = row[forms[0]]['ms']
            row['torch_over_hip'] = round(row['torch']['ms'] / best, 3)
            if op & 4:
                row['direct_over_lds'] = round(row['direct']['ms'] / row['lds']['ms'], 3)
            view[step][cls] = row
    stitch = {}
    for kind in ('float32', 'uint8'):
        h, r = _row(t[('stitch', kind, 'hip')], nbytes[('stitch', kind)]), _row(t[('stitch', kind, 'torch')], nbytes[('stitch', kind)])
        stitch[kind] = {'bytes': int(nbytes[('stitch', kind)]), 'hip': h, 'torch': r, 'torch_over_hip': round(r['ms'] / h['ms'], 3)}
    del logits, tiles, acc, out_tiles
    torch.cuda.empty_cache()

    # the whole path, and the launches test-time augmentation adds to one batch of BATCH frames
    net = UNet2D({'shape': (TILE, TILE), 'num_outputs': K, 'device': dev, 'seed': 0}, 'infer').initialize()
    whole = {}
    for tta in (None, 'flips', 'dihedral'):
        run = lambda: segment_frames(net, frames, tile=TILE, margin=MARGIN, frames_per_batch=BATCH, tta=tta)
        run()
        ts = []
        for _ in range(args.frames_iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            ts.append((time.perf_counter() - t0) * 1e3 / FRAMES)
        whole[str(tta)] = {'ms_per_frame': round(float(np.median(ts)), 3), 'ms_per_frame_min_max': [round(min(ts), 3), round(max(ts), 3)]}
    nb = BATCH * tiler.tiles_per_frame
    bl, bt = torch.randn((nb, TILE, TILE, K), device=dev), torch.randn((nb, TILE, TILE, 1), device=dev)
    ba, bo = torch.empty_like(bl), torch.empty_like(bt)
    for tta, ops in (('flips', (0, 1, 2, 3)), ('dihedral', tuple(range(8)))):
        def launches(ops=ops):
            for op in ops:
                if op:
                    tiler.view(bt, op, out=bo)
                tiler.view(bl, op, inverse=True, out=ba, accumulate=op != 0)
            tiler.stitch_probs(ba, n=len(ops))
        launches()
        ls = [_time(launches, REPS) for _ in range(args.iters)]
        batch_ms = whole[tta]['ms_per_frame'] * BATCH
        whole[tta].update({'tta_launches_ms_per_batch': round(float(np.median(ls)), 4),
                           'tta_launches_ms_min_max': [round(min(ls), 4), round(max(ls), 4)],
                           'tta_share': round(float(np.median(ls)) / batch_ms, 5),
                           'over_plain': round(whole[tta]['ms_per_frame'] / whole['None']['ms_per_frame'], 3)})
    lds_faster = all(view[s]['transposed']['direct_over_lds'] >= 1.0 for s in ('merge', 'copy', 'input'))
    line = {'workload': 'tta: %d uint16 frames of %d x %d, tile %d margin %d (%d tiles), K = %d; batches of %d frames'
                        % (FRAMES, SIDE, SIDE, TILE, MARGIN, nt, K, BATCH),
            'warmup': args.warmup, 'iters': args.iters, 'calls_per_window': REPS, 'device': torch.cuda.get_device_name(0),
            'hbm_achievable_gb_per_s': HBM_ACHIEVABLE_GBS, 'view': view, 'stitch': stitch, 'segment_frames': whole,
            'sq_tta_lds': {'default': 'lds', 'lds_no_slower_in_every_step': bool(lds_faster)},
            'max_abs_probability_error': prob_err, 'probability_bound': (K + 4) * 2.0 ** -23}
    text = json.dumps(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
