"""Mask splitting benchmark: one JSON line, also written to profiles/mask_split_bench.json.

Workload: 8 uint8 masks of 2048 x 2048 at C = 2 resident in HBM, generated once: ~2000 touching disk pairs per frame
(radius 9 .. 13, joined by a neck about 5 pixels wide, so that an erosion by 4 or 8 tells the two cores apart).
HIP events round each call after warm-up, outputs and workspaces allocated before, the variants alternated round by round.
Per erosions r = 4, 8 (reach 2 r) and structure cross, square:
  * ms             : sq_mask_split_u8 (maskops.split), the whole call -- erosion, labelling, regrowth, cut -- with the
                     regrowth in LDS tiles (the default form);
  * step_form_ms   : the same call under SQ_SPLIT_LDS=0, one synchronous step per launch on the global planes, same run;
  * regrowth_ms / step_form_regrowth_ms : the regrowth launches alone, and erosion_ms / labelling_ms / cut_ms beside them:
                     kernel times from a run of their own under `rocprofv3 --kernel-trace` (`--trace-run`: every variant in
                     both forms, one call to warm up and three that count), folded into the JSON afterwards with
                     `--fold-trace DIR` (the median call's sum per kernel group); "not measured" until then;
  * torch_ms       : a torch composition of the same definition -- max-pool erosion, labels by propagating the smallest
                     pixel index through each seed until nothing changes (torch has no labelling; the loop reads a flag
                     back every 8 rounds), reach padded-minimum steps, the cut;
  * host_ms        : download + the scipy restatement (tests/mask_split_cases.py: binary_erosion, label, padded minimum
                     steps) by the host clock, `--host-iters` times, at r = 8 cross only (the others: "not measured");
  * gb_per_s       : against the 2 B per pixel a split must move (one read, one write), next to the 6.3 TB/s of HBM; and
                     model_bytes, what the chain of launches moves by its own count (every plane a launch reads or writes
                     once, the staged halo included), with the rate that gives.
`agree` says the variants computed the same masks; `objects` the 4-connected objects before and after.  `stream` is the share
of a split step (erosions 8) in frontend.segment_frames' stream over 8 uint16 frames of 2048 x 2048 (tile 512, margin 32,
UNet2D default filters) against the stream without it, alternated, host clock per frame.
Without a GPU the tool refuses to run; --placeholder writes the file with "not measured" in every field.
Usage: python tools/mask_split_bench.py [--warmup 2] [--iters 7] [--host-iters 1] [--stream-iters 3] [--out PATH] [--placeholder]
       rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/mask_split_bench.py --trace-run
       python tools/mask_split_bench.py --fold-trace DIR [--out PATH]
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

NM = 'not measured'
N, H, W, C = 8, 2048, 2048, 2
HBM_TBS = 6.3
WORKLOAD = ('mask splitting: %d x %d x %d uint8 masks at C = %d, ~2000 touching disk pairs per frame; erosions 4 and 8 with '
            'reach twice that, cross and square' % (N, H, W, C))
VARIANTS = tuple((r, st) for r in (4, 8) for st in ('cross', 'square'))
MOVED = 2 * N * H * W                                          # bytes a call must move: the mask in, the mask out
TRACED = ('regrowth_ms', 'regrowth_launches', 'step_form_regrowth_ms', 'step_form_regrowth_launches',
          'regrowth_lds_over_step_form', 'erosion_ms', 'labelling_ms', 'cut_ms')
FIELDS = ('ms', 'ms_min_max', 'step_form_ms', 'step_form_ms_min_max', 'lds_over_step_form') + TRACED + ('torch_ms', 'torch_over_kernel', 'host_ms', 'host_over_kernel',
          'gb_per_s', 'share_of_hbm', 'model_bytes', 'model_gb_per_s', 'model_share_of_hbm', 'pixels_cut', 'objects')
STREAM_FIELDS = ('what', 'plain_ms_per_frame', 'split_ms_per_frame', 'ms_min_max', 'split_share')


def placeholder():
    return {'workload': WORKLOAD, 'device': NM, 'hbm_tb_per_s': HBM_TBS, 'bytes_moved_per_call': MOVED, 'default_form': NM,
            'variants': {'r%d_%s' % v: {f: NM for f in FIELDS} for v in VARIANTS}, 'agree': NM,
            'stream': {f: NM for f in STREAM_FIELDS}}


def pair_masks(seed=0, per_frame=2000):
    rng = np.random.default_rng(seed)
    m = np.zeros((N, H, W), np.uint8)
    for i in range(N):
        for _ in range(per_frame):
            cy, cx, rad = int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(9, 14))
            half = (rad * rad - 6.0) ** 0.5                    # a neck of about 5 pixels
            dy, dx = (0.0, half) if rng.random() < 0.5 else (half, 0.0)
            for sy, sx in ((int(round(cy - dy)), int(round(cx - dx))), (int(round(cy + dy)), int(round(cx + dx)))):
                y0, y1, x0, x1 = max(sy - rad, 0), min(sy + rad + 1, H), max(sx - rad, 0), min(sx + rad + 1, W)
                yy, xx = np.mgrid[y0:y1, x0:x1]
                m[i, y0:y1, x0:x1][(yy - sy) ** 2 + (xx - sx) ** 2 <= rad * rad] = 1
    return m


def model_bytes(reach, lds):
    """what the chain of launches reads and writes, every plane once per launch that touches it"""
    from sequitr_amd import maskops
    px = N * H * W
    total = 2 * px                                              # erosion: mask in, seed plane out
    total += (1 + 4) * px + (1 + 4) * px + (4 + 4) * px         # row scan, merge (seed bytes, parents), compress
    if lds:
        R, Cc = maskops.SPLIT_TILE
        left = reach
        first = True
        while left > 0:
            s = min(left, maskops.SPLIT_STEPS)
            staged = (R + 2 * s) * (Cc + 2 * s) / float(R * Cc)
            total += int(((1 + 4 + (1 if first else 0)) * staged + 4) * px)
            left -= s
            first = False
    else:
        total += reach * (1 + 4 + 4) * px + px                  # per step: mask, labels in, labels out; the seed bytes once
    return total + (1 + 4 + 1) * px                             # cut: mask, labels, out


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _min4(L, big):
    import torch.nn.functional as F
    p = F.pad(torch.where(L > 0, L, big), (1, 1, 1, 1), value=int(big))
    return torch.minimum(torch.minimum(p[:, :-2, 1:-1], p[:, 2:, 1:-1]), torch.minimum(p[:, 1:-1, :-2], p[:, 1:-1, 2:]))


def torch_split(mask_d, r, st, reach):
    """the composition a torch user writes at C = 2"""
    import torch.nn.functional as F
    P = mask_d == 1
    x = P.to(torch.float16)[:, None]
    for _ in range(r):
        xp = -F.pad(x, (1, 1, 1, 1), value=0.0)                 # a zero border, not max_pool2d's -inf
        if st == 'square':
            x = -F.max_pool2d(xp, 3, 1, 0)
        else:
            x = -torch.maximum(F.max_pool2d(xp[:, :, 1:-1], (1, 3), 1, 0), F.max_pool2d(xp[:, :, :, 1:-1], (3, 1), 1, 0))
    S = x[:, 0] > 0
    big = torch.tensor(H * W + 1, dtype=torch.int32, device=mask_d.device)
    idx = torch.arange(1, H * W + 1, dtype=torch.int32, device=mask_d.device).view(1, H, W)
    L = torch.where(S, idx, torch.zeros_like(idx)).expand(N, H, W).contiguous()
    while True:                                                 # a seed's label: the smallest index in its component
        prev = L
        for _ in range(8):
            L = torch.where(S, torch.minimum(L, _min4(L, big)), L)
        if torch.equal(prev, L):
            break
    for _ in range(reach):
        nb = _min4(L, big)
        L = torch.where(P & (L == 0) & (nb < big), nb, L)
    cut = (L > 0) & (_min4(L, big) < L)
    return torch.where(cut, torch.zeros_like(mask_d), mask_d)


def _host_ms(fn, iters):
    t, res = [], None
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return (round(float(np.median(t)), 1) if t else NM), res


def _set_form(lds):
    if lds:
        os.environ.pop('SQ_SPLIT_LDS', None)
    else:
        os.environ['SQ_SPLIT_LDS'] = '0'


def run_variants(dev, mask, args):
    from scipy import ndimage
    from sequitr_amd import _lib, maskops
    from tests import mask_split_cases as sc
    lib = _lib.load()
    mask_d = torch.from_numpy(mask).to(dev)
    out = torch.empty_like(mask_d)
    ws = torch.empty(int(lib.sq_mask_split_workspace(N, H, W)) // 4, dtype=torch.int32, device=dev)

    def kernel(r, st, reach, lds):
        def call():
            _set_form(lds)                                      # the switch is read per call
            maskops.split(mask_d, r, st, reach, classes=C, out=out, workspace=ws)
            _set_form(True)
        return call

    variants, agree, extra = {}, True, {}
    for r, st in VARIANTS:
        variants[('lds', r, st)] = kernel(r, st, 2 * r, True)
        variants[('step', r, st)] = kernel(r, st, 2 * r, False)
        variants[('torch', r, st)] = lambda r=r, st=st: torch_split(mask_d, r, st, 2 * r)
        variants[('lds', r, st)]()
        a = out.clone()
        variants[('step', r, st)]()
        agree = agree and torch.equal(a, out) and torch.equal(a, variants[('torch', r, st)]())
        objects = [int(sum(ndimage.label(m == 1)[1] for m in t.cpu().numpy())) for t in (mask_d, a)]
        extra[(r, st)] = {'pixels_cut': int((a != mask_d).sum()), 'objects': {'before': objects[0], 'after': objects[1]}}
    host_ms, res = _host_ms(lambda: sc.split_ref(mask_d.cpu().numpy(), 8, 'cross', None, C), args.host_iters)
    if res is not None:
        variants[('lds', 8, 'cross')]()
        agree = agree and np.array_equal(out.cpu().numpy(), res)

    for _ in range(args.warmup):
        for f in variants.values():
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(args.iters):                                 # interleaved rounds: drift hits all variants alike
        for k, f in variants.items():
            t[k].append(_time(f))
    med = {k: float(np.median(v)) for k, v in t.items()}
    span = {k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()}
    res, wins = {}, []
    for r, st in VARIANTS:
        lds, step, tt = med[('lds', r, st)], med[('step', r, st)], med[('torch', r, st)]
        gbs, mb = MOVED / (lds * 1e-3) / 1e9, model_bytes(2 * r, True)
        hm = host_ms if (r, st) == (8, 'cross') else NM
        res['r%d_%s' % (r, st)] = dict(
            ms=round(lds, 4), ms_min_max=span[('lds', r, st)], step_form_ms=round(step, 4),
            step_form_ms_min_max=span[('step', r, st)], lds_over_step_form=round(lds / step, 3), **{f: NM for f in TRACED},
            torch_ms=round(tt, 3), torch_over_kernel=round(tt / lds, 1), host_ms=hm,
            host_over_kernel=round(hm / lds, 1) if hm != NM else NM, gb_per_s=round(gbs, 1),
            share_of_hbm=round(gbs / (HBM_TBS * 1e3), 4), model_bytes=mb, model_gb_per_s=round(mb / (lds * 1e-3) / 1e9, 1),
            model_share_of_hbm=round(mb / (lds * 1e-3) / 1e9 / (HBM_TBS * 1e3), 4), **extra[(r, st)])
        wins.append(lds < step)
    form = 'LDS tiles' if all(wins) else ('one step per launch' if not any(wins) else 'mixed: see lds_over_step_form')
    return res, bool(agree), form


TRACE_CALLS = 4                                                 # per variant and form under the profiler: the first warms up


def trace_run(dev):
    """every variant in both forms, TRACE_CALLS calls each, in the order fold_trace() expects; for rocprofv3 --kernel-trace"""
    from sequitr_amd import _lib, maskops
    mask_d = torch.from_numpy(pair_masks()).to(dev)
    out = torch.empty_like(mask_d)
    ws = torch.empty(int(_lib.load().sq_mask_split_workspace(N, H, W)) // 4, dtype=torch.int32, device=dev)
    for r, st in VARIANTS:
        for lds in (True, False):
            _set_form(lds)
            for _ in range(TRACE_CALLS):
                maskops.split(mask_d, r, st, 2 * r, classes=C, out=out, workspace=ws)
            torch.cuda.synchronize()
    _set_form(True)


def fold_trace(trace_dir, line):
    """kernel times of a --trace-run into the JSON line: a call begins at its erosion launch (morph_kernel)"""
    import csv
    import glob
    files = glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True)
    if len(files) != 1:
        raise SystemExit('expected one kernel_trace.csv under %s, found %d' % (trace_dir, len(files)))
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r['Start_Timestamp']))
    groups = (('erosion', 'morph_kernel'), ('labelling', 'cc_'), ('lds', 'split_grow_lds_kernel'),
              ('step', 'split_grow_step_kernel'), ('cut', 'split_cut_kernel'))
    calls = []
    for r in rows:
        name = r['Kernel_Name']
        kind = next((g for g, pat in groups if pat in name), None)
        if kind == 'erosion':
            calls.append({g: [] for g, _ in groups})
        if kind is not None and calls:
            calls[-1][kind].append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e6)
    if len(calls) != len(VARIANTS) * 2 * TRACE_CALLS:
        raise SystemExit('expected %d calls in the trace, found %d' % (len(VARIANTS) * 2 * TRACE_CALLS, len(calls)))
    k = 0
    for r, st in VARIANTS:
        v = line['variants']['r%d_%s' % (r, st)]
        for form in ('lds', 'step'):
            timed = calls[k + 1:k + TRACE_CALLS]
            k += TRACE_CALLS
            assert all(len(c[form]) == len(timed[0][form]) > 0 and not c['step' if form == 'lds' else 'lds'] for c in timed), (r, st, form)
            med = {g: round(float(np.median([sum(c[g]) for c in timed])), 4) for g, _ in groups}
            pre = '' if form == 'lds' else 'step_form_'
            v[pre + 'regrowth_ms'], v[pre + 'regrowth_launches'] = med[form], len(timed[0][form])
            if form == 'lds':
                v['erosion_ms'], v['labelling_ms'], v['cut_ms'] = med['erosion'], med['labelling'], med['cut']
        v['regrowth_lds_over_step_form'] = round(v['regrowth_ms'] / v['step_form_regrowth_ms'], 3)
    line['kernel_times'] = 'rocprofv3 --kernel-trace, a run of its own: the median of %d calls per variant and form' % (TRACE_CALLS - 1)
    return line


def run_stream(dev, args):
    from sequitr_amd.frontend import segment_frames
    from sequitr_amd.maskops import MaskCleanup
    from sequitr_amd.networks.unet import UNet2D
    frames = np.random.default_rng(0).integers(100, 4000, (N, H, W)).astype(np.uint16)
    net = UNet2D({'shape': (512, 512), 'num_outputs': C, 'device': dev}, 'infer').initialize()
    cleanup = MaskCleanup([{'op': 'split', 'erosions': 8}])

    def stream(**kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        segment_frames(net, frames, tile=512, margin=32, frames_per_batch=4, **kw)   # ends in a synchronise
        return (time.perf_counter() - t0) * 1e3 / N

    kinds = {'plain': {}, 'split': {'postprocess': cleanup}}
    for kw in kinds.values():
        stream(**kw)
    t = {k: [] for k in kinds}
    for _ in range(args.stream_iters):
        for k, kw in kinds.items():
            t[k].append(stream(**kw))
    plain, split = float(np.median(t['plain'])), float(np.median(t['split']))
    return {'what': 'segment_frames over %d uint16 frames of %d x %d, tile 512, margin 32, 4 frames per batch, masks downloaded: '
                    'with postprocess = split erosions 8 (cross, reach 16) against without, host clock per frame' % (N, H, W),
            'plain_ms_per_frame': round(plain, 3), 'split_ms_per_frame': round(split, 3),
            'ms_min_max': {k: [round(min(v), 3), round(max(v), 3)] for k, v in t.items()},
            'split_share': round((split - plain) / plain, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--iters', type=int, default=7)
    ap.add_argument('--host-iters', type=int, default=1)
    ap.add_argument('--stream-iters', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mask_split_bench.json'))
    ap.add_argument('--placeholder', action='store_true', help='write "not measured" in every field (no GPU needed)')
    ap.add_argument('--trace-run', action='store_true', help='only launch every variant in both forms, for rocprofv3 --kernel-trace')
    ap.add_argument('--fold-trace', metavar='DIR', help="fold a --trace-run's kernel_trace.csv into the JSON at --out (no GPU needed)")
    args = ap.parse_args()
    if args.trace_run:
        if not torch.cuda.is_available():
            raise SystemExit('mask_split_bench needs the GPU')
        torch.cuda.set_device(0)
        trace_run('cuda:0')
        return
    if args.fold_trace:
        line = fold_trace(args.fold_trace, json.loads(open(args.out).read()))
    elif args.placeholder:
        line = placeholder()
    else:
        if not torch.cuda.is_available():
            raise SystemExit('mask_split_bench needs the GPU')
        torch.cuda.set_device(0)
        dev = 'cuda:0'
        line = {'workload': WORKLOAD, 'device': torch.cuda.get_device_name(0), 'warmup': args.warmup, 'iters': args.iters,
                'hbm_tb_per_s': HBM_TBS, 'bytes_moved_per_call': MOVED}
        line['variants'], line['agree'], line['default_form'] = run_variants(dev, pair_masks(), args)
        print('mask_split_bench: variants done', file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
        line['stream'] = run_stream(dev, args)
    text = json.dumps(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
