"""Scoring benchmark: one JSON line, also written to profiles/score_bench.json.

Workload: confusion counts (ops.confusion_, one row of counts per item) of data resident in HBM --
  * tiles  : 32 x 512 x 512 at C = 2;
  * frames : 8 x 2048 x 2048 at C = 2, 4 and 16;
each from uint8 masks and from float32 logits, against uint8 class-index labels.  HIP events round each call after warm-up,
the variants alternated round by round, REPS calls per event pair:
  * hip   : sq_confusion.  `bytes` is what a call must read (2 bytes per pixel from masks, 4 C + 1 from logits), `gb_per_s`
            those bytes over the call, `fraction_of_hbm_achievable` that over 6.3 TB/s;
  * torch : the same counts composed from torch ops -- (arg-max for logits,) widen to int64, t * C + p with an item offset,
            torch.bincount(minlength=items * C * C);
  * host  : the path this replaces -- download the masks (and labels) and sklearn.metrics.confusion_matrix per item; timed
            with the host clock, `--host-iters` times.
`agree` says that the three give the same integers.  `evaluate` is the share of scoring in SERVER_evaluate's stream:
frontend.segment_frames over 8 uint16 frames of 2048 x 2048 (tile 512, margin 32, UNet2D default filters) with a sink that
scores each batch against resident labels, over the same call with a sink that does nothing, alternated.
Without a GPU the tool refuses to run; --placeholder writes the file with "not measured" in every field.
Usage: python tools/score_bench.py [--warmup 2] [--iters 5] [--host-iters 2] [--stream-iters 3] [--out PATH] [--placeholder]
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

HBM_ACHIEVABLE = 6.3e12                                         # bytes/s, the figure the README uses
CASES = [('tiles', 32, 512 * 512, 2), ('frames', 8, 2048 * 2048, 2), ('frames', 8, 2048 * 2048, 4),
         ('frames', 8, 2048 * 2048, 16)]
REPS = 8                                                        # calls per event pair
NM = 'not measured'
WORKLOAD = ('scoring: confusion counts of 32 x 512^2 (C = 2) and 8 x 2048^2 (C = 2, 4, 16) resident masks / float32 logits '
            'against uint8 labels, one row of counts per item')
CASE_FIELDS = ('hip_ms', 'hip_ms_min_max', 'bytes', 'gb_per_s', 'fraction_of_hbm_achievable', 'torch_ms', 'torch_over_hip',
               'host_ms', 'host_over_hip', 'agree')
EVAL_FIELDS = ('what', 'segment_ms_per_frame', 'evaluate_ms_per_frame', 'ms_min_max', 'scoring_share')


def case_name(kind, items, n, C, src):
    return '%s_%dx%d_C%d_%s' % (kind, items, n, C, src)


def placeholder():
    cases = {case_name(k, i, n, C, src): {f: NM for f in CASE_FIELDS} for k, i, n, C in CASES for src in ('masks', 'logits')}
    return {'workload': WORKLOAD, 'device': NM, 'hbm_achievable_gb_per_s': HBM_ACHIEVABLE / 1e9, 'cases': cases,
            'evaluate': {f: NM for f in EVAL_FIELDS}}


def _time(fn, reps=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def run_case(dev, items, n, C, src, args):
    from sklearn.metrics import confusion_matrix
    from sequitr_amd import ops
    g = torch.Generator(device=dev).manual_seed(C)
    truth = torch.randint(0, C, (items, n), dtype=torch.uint8, device=dev, generator=g)
    if src == 'masks':
        pred = torch.randint(0, C, (items, n), dtype=torch.uint8, device=dev, generator=g)
        nbytes = 2 * items * n
    else:
        pred = torch.randn((items, n, C), dtype=torch.float32, device=dev, generator=g)
        nbytes = (4 * C + 1) * items * n
    counts = torch.zeros((items, C, C), dtype=torch.int64, device=dev)
    ignored = torch.zeros((items,), dtype=torch.int64, device=dev)
    offs = (torch.arange(items, device=dev, dtype=torch.int64) * (C * C))[:, None]
    box = {}

    def hip():
        ops.confusion_(counts, ignored, pred, truth, C)

    def composed():
        p = pred if src == 'masks' else pred.argmax(-1)
        box['torch'] = torch.bincount((truth.to(torch.int64) * C + p.to(torch.int64) + offs).view(-1), minlength=items * C * C)

    def host():
        p = (pred if src == 'masks' else ops.argmax_u8(pred)).cpu().numpy()
        t = truth.cpu().numpy()
        box['host'] = np.stack([confusion_matrix(t[i], p[i], labels=list(range(C))) for i in range(items)])

    hip()
    composed()
    first = counts.cpu().numpy()
    agree = bool(np.array_equal(first.reshape(-1), box['torch'].cpu().numpy()))
    t_host = []
    for _ in range(args.host_iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host()
        t_host.append((time.perf_counter() - t0) * 1e3)
    agree = agree and bool(np.array_equal(first, box['host'])) and int(ignored.sum()) == 0
    variants = {'hip': hip, 'torch': composed}
    for _ in range(args.warmup):
        for f in variants.values():
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(args.iters):                                 # interleaved rounds: drift hits both variants alike
        for k, f in variants.items():
            t[k].append(_time(f, REPS))
    hip_ms, torch_ms, host_ms = (float(np.median(v)) for v in (t['hip'], t['torch'], t_host))
    rate = nbytes / (hip_ms * 1e-3)
    return {'hip_ms': round(hip_ms, 4), 'hip_ms_min_max': [round(min(t['hip']), 4), round(max(t['hip']), 4)], 'bytes': nbytes,
            'gb_per_s': round(rate / 1e9, 1), 'fraction_of_hbm_achievable': round(rate / HBM_ACHIEVABLE, 3),
            'torch_ms': round(torch_ms, 4), 'torch_over_hip': round(torch_ms / hip_ms, 1), 'host_ms': round(host_ms, 1),
            'host_over_hip': round(host_ms / hip_ms, 0), 'agree': agree}


def run_evaluate(dev, args):
    from sequitr_amd import ops
    from sequitr_amd.frontend import segment_frames
    from sequitr_amd.networks.unet import UNet2D
    F, H, W, C = 8, 2048, 2048, 2
    frames = np.random.default_rng(0).integers(100, 4000, (F, H, W)).astype(np.uint16)
    labels = torch.randint(0, C, (F, H, W), dtype=torch.uint8, device=dev)
    net = UNet2D({'shape': (512, 512), 'num_outputs': C, 'device': dev}, 'infer').initialize()
    counts = torch.zeros((F, C, C), dtype=torch.int64, device=dev)
    ignored = torch.zeros((F,), dtype=torch.int64, device=dev)

    def score(first, m):
        k = m.shape[0]
        ops.confusion_(counts[first:first + k], ignored[first:first + k], m, labels[first:first + k], C)

    def stream(sink):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        segment_frames(net, frames, tile=512, margin=32, frames_per_batch=4, on_masks=sink)   # ends in a synchronise
        return (time.perf_counter() - t0) * 1e3 / F

    sinks = {'segment': lambda first, m: None, 'evaluate': score}
    for sink in sinks.values():
        stream(sink)
    t = {k: [] for k in sinks}
    for _ in range(args.stream_iters):
        for k, sink in sinks.items():
            t[k].append(stream(sink))
    seg, ev = float(np.median(t['segment'])), float(np.median(t['evaluate']))
    return {'what': 'segment_frames over %d uint16 frames of %d x %d, tile 512, margin 32, 4 frames per batch: a scoring sink '
                    'against an empty one, host clock per frame' % (F, H, W),
            'segment_ms_per_frame': round(seg, 3), 'evaluate_ms_per_frame': round(ev, 3),
            'ms_min_max': {k: [round(min(v), 3), round(max(v), 3)] for k, v in t.items()},
            'scoring_share': round((ev - seg) / seg, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--host-iters', type=int, default=2)
    ap.add_argument('--stream-iters', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'score_bench.json'))
    ap.add_argument('--placeholder', action='store_true', help='write "not measured" in every field (no GPU needed)')
    args = ap.parse_args()
    if args.placeholder:
        line = placeholder()
    else:
        if not torch.cuda.is_available():
            raise SystemExit('score_bench needs the GPU')
        torch.cuda.set_device(0)
        dev = 'cuda:0'
        line = {'workload': WORKLOAD, 'device': torch.cuda.get_device_name(0), 'hbm_achievable_gb_per_s': HBM_ACHIEVABLE / 1e9,
                'warmup': args.warmup, 'iters': args.iters, 'calls_per_window': REPS, 'cases': {}}
        for kind, items, n, C in CASES:
            for src in ('masks', 'logits'):
                line['cases'][case_name(kind, items, n, C, src)] = run_case(dev, items, n, C, src, args)
                torch.cuda.empty_cache()
        line['evaluate'] = run_evaluate(dev, args)
    text = json.dumps(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
