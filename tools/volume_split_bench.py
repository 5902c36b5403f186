"""Volume splitting benchmark: one JSON line, also written to profiles/volume_split_bench.json.

Workload: one uint8 mask of 64 x 1024 x 1024 at C = 2 resident in HBM, generated here from a seed: ~2000 touching ball pairs
(radius 9 .. 13, joined along a random axis by a neck about 5 voxels wide, so that an erosion tells the two cores apart).
HIP events round each call after warm-up, output and workspace allocated before, the variants alternated round by round.
Per variant -- r = 4 cross at reach 8, r = 4 cube at reach 12, r = 8 plane_cross at reach 16:
  * lds_form_ms    : sq_volume_split_u8 (volumeops.split3d), the whole call -- erosion, labelling, regrowth, cut -- under
                     SQ_SPLIT3D_LDS=1, the regrowth in LDS bricks, median with minimum and maximum;
  * step_form_ms   : the same call under SQ_SPLIT3D_LDS=0, one synchronous step per launch on the global planes, same run;
                     lds_over_step_form is the ratio, `default_form` the form the library runs when the variable is unset;
  * regrowth_ms / step_form_regrowth_ms : the regrowth launches alone, and erosion_ms / labelling_ms / cut_ms beside them:
                     kernel times from a run of their own under `rocprofv3 --kernel-trace` (`--trace-run`: every variant in
                     both forms, one call to warm up and three that count), folded into the JSON afterwards with
                     `--fold-trace DIR` (the median call's sum per kernel group); "not measured" until then;
  * torch_ms       : a torch composition of the same definition -- max-pool erosion on the float16 plane, labels by
                     propagating the smallest voxel index through each seed until nothing changes (torch has no labelling;
                     the loop reads a flag back every 8 rounds), reach padded-minimum steps, the cut;
  * host_ms        : download + the scipy restatement (tests/volume_split_cases.py) by the host clock, `--host-iters` times,
                     at r = 4 cross only (the others: "not measured");
  * gb_per_s       : of the faster form, against the 2 B per voxel a split must move (one read, one write), next to the
                     6.3 TB/s of HBM; and model_bytes, what each form's chain of launches moves by its own count (every plane
                     a launch reads or writes once, the staged halo included), with the rate that gives;
  * objects        : the 6-connected objects before and after; voxels_cut; workspace_bytes.
`agree` says the variants computed the same masks.  `stream` is the share of a split3d step (erosions 4, cross) in
frontend.segment_volumes' stream over 2 uint16 volumes of 64 x 1024 x 1024 (bricks 32 x 128 x 128, margin 0, UNet3D default
filters, masks kept in HBM) against the stream without it, alternated, host clock per volume.
Without a GPU the tool refuses to run; --placeholder writes the file with "not measured" in every field.
Usage: python tools/volume_split_bench.py [--warmup 2] [--iters 7] [--host-iters 1] [--stream-iters 3] [--out PATH] [--placeholder]
       rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/volume_split_bench.py --trace-run
       python tools/volume_split_bench.py --fold-trace DIR [--out PATH]
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
SHAPE = (1, 64, 1024, 1024)
C = 2
BRICK = (32, 128, 128)
HBM_TBS = 6.3
VOX = SHAPE[0] * SHAPE[1] * SHAPE[2] * SHAPE[3]
MOVED = 2 * VOX                                                 # bytes a call must move: the mask in, the mask out
WORKLOAD = ('volume splitting: one %d x %d x %d x %d uint8 mask at C = 2, ~2000 touching ball pairs; r = 4 cross at reach 8, '
            'r = 4 cube at reach 12, r = 8 plane_cross at reach 16' % SHAPE)
VARIANTS = ((4, 'cross', 8), (4, 'cube', 12), (8, 'plane_cross', 16))
TRACED = ('regrowth_ms', 'regrowth_launches', 'step_form_regrowth_ms', 'step_form_regrowth_launches',
          'regrowth_lds_over_step_form', 'erosion_ms', 'labelling_ms', 'cut_ms')
FIELDS = ('lds_form_ms', 'lds_form_ms_min_max', 'step_form_ms', 'step_form_ms_min_max', 'lds_over_step_form') + TRACED + (
    'torch_ms', 'torch_over_kernel', 'host_ms', 'host_over_kernel', 'gb_per_s', 'share_of_hbm', 'model_bytes_lds_form',
    'model_bytes_step_form', 'model_gb_per_s', 'model_share_of_hbm', 'voxels_cut', 'objects', 'workspace_bytes')
STREAM_FIELDS = ('what', 'plain_ms_per_volume', 'split_ms_per_volume', 'ms_min_max', 'split_share')


def name_of(v):
    return 'r%d_%s_reach%d' % v


def placeholder():
    return {'workload': WORKLOAD, 'device': NM, 'hbm_tb_per_s': HBM_TBS, 'bytes_moved_per_call': MOVED, 'default_form': NM,
            'faster_form': NM, 'geometry': NM, 'variants': {name_of(v): {f: NM for f in FIELDS} for v in VARIANTS}, 'agree': NM,
            'stream': {f: NM for f in STREAM_FIELDS}}


def pair_mask(seed=0, pairs=2000):
    rng = np.random.default_rng(seed)
    _, D, H, W = SHAPE
    m = np.zeros(SHAPE, np.uint8)
    for _ in range(pairs):
        c = np.array([rng.integers(0, D), rng.integers(0, H), rng.integers(0, W)], float)
        rad = int(rng.integers(9, 14))
        off = np.zeros(3)
        off[int(rng.integers(0, 3))] = (rad * rad - 6.0) ** 0.5   # a neck of about 5 voxels
        for s in (c - off, c + off):
            sz, sy, sx = (int(round(v)) for v in s)
            z0, z1, y0, y1, x0, x1 = max(sz - rad, 0), min(sz + rad + 1, D), max(sy - rad, 0), min(sy + rad + 1, H), \
                max(sx - rad, 0), min(sx + rad + 1, W)
            if z0 >= z1 or y0 >= y1 or x0 >= x1:
                continue
            zz, yy, xx = np.mgrid[z0:z1, y0:y1, x0:x1]
            m[0, z0:z1, y0:y1, x0:x1][(zz - sz) ** 2 + (yy - sy) ** 2 + (xx - sx) ** 2 <= rad * rad] = 1
    return m


def erosion_launches(r, st):
    from sequitr_amd import volumeops
    return 1 if st.startswith('plane') else -(-r // volumeops.MORPH3D_MAX_ITER)


def model_bytes(r, st, reach, lds):
    """what the chain of launches reads and writes, every plane once per launch that touches it"""
    from sequitr_amd import volumeops
    total = 2 * VOX * erosion_launches(r, st)                   # erosion: bytes in, bytes out
    total += (1 + 4) * VOX + (1 + 4) * VOX + (4 + 4) * VOX      # row scan, merge (seed bytes, parents), compress
    if lds:
        TD, TH, TW = volumeops.SPLIT3D_TILE
        left, first = reach, True
        while left > 0:
            s = min(left, volumeops.SPLIT3D_STEPS)
            staged = (TD + 2 * s) * (TH + 2 * s) * (TW + 2 * s) / float(TD * TH * TW)
            total += int(((1 + 4 + (1 if first else 0)) * staged + 4) * VOX)
            left -= s
            first = False
    else:
        total += reach * (1 + 4 + 4) * VOX + VOX                # per step: mask, labels in, labels out; the seed bytes once
    return total + (1 + 4 + 1) * VOX                            # cut: mask, labels, out


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _min6(L, big):
    import torch.nn.functional as F
    p = F.pad(torch.where(L > 0, L, big), (1, 1, 1, 1, 1, 1), value=int(big))
    m = torch.minimum(p[:, :-2, 1:-1, 1:-1], p[:, 2:, 1:-1, 1:-1])
    m = torch.minimum(m, torch.minimum(p[:, 1:-1, :-2, 1:-1], p[:, 1:-1, 2:, 1:-1]))
    return torch.minimum(m, torch.minimum(p[:, 1:-1, 1:-1, :-2], p[:, 1:-1, 1:-1, 2:]))


def torch_split(mask_d, r, st, reach):
    """the composition a torch user writes at C = 2"""
    import torch.nn.functional as F
    P = mask_d == 1
    x = P.to(torch.float16)[:, None]
    for _ in range(r):
        if st == 'cube':
            x = -F.max_pool3d(-F.pad(x, (1, 1, 1, 1, 1, 1), value=0.0), 3, 1, 0)    # a zero border, not max_pool3d's -inf
            continue
        xp = -F.pad(x, (1, 1, 1, 1, 1, 1), value=0.0)
        y = torch.maximum(F.max_pool3d(xp[:, :, 1:-1, 1:-1], (1, 1, 3), 1, 0), F.max_pool3d(xp[:, :, 1:-1, :, 1:-1], (1, 3, 1), 1, 0))
        if st == 'cross':
            y = torch.maximum(y, F.max_pool3d(xp[:, :, :, 1:-1, 1:-1], (3, 1, 1), 1, 0))
        x = -y
    S = x[:, 0] > 0
    big = torch.tensor(VOX + 1, dtype=torch.int32, device=mask_d.device)
    idx = torch.arange(1, VOX + 1, dtype=torch.int32, device=mask_d.device).view(SHAPE)
    L = torch.where(S, idx, torch.zeros_like(idx))
    while True:                                                 # a seed's label: the smallest index in its component
        prev = L
        for _ in range(8):
            L = torch.where(S, torch.minimum(L, _min6(L, big)), L)
        if torch.equal(prev, L):
            break
    for _ in range(reach):
        nb = _min6(L, big)
        L = torch.where(P & (L == 0) & (nb < big), nb, L)
    cut = (L > 0) & (_min6(L, big) < L)
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
    if lds is None:
        os.environ.pop('SQ_SPLIT3D_LDS', None)
    else:
        os.environ['SQ_SPLIT3D_LDS'] = '1' if lds else '0'


def run_variants(dev, mask, args):
    from scipy import ndimage
    from sequitr_amd import _lib, volumeops
    from tests import volume_split_cases as sc
    lib = _lib.load()
    mask_d = torch.from_numpy(mask).to(dev)
    out = torch.empty_like(mask_d)
    nws = int(lib.sq_volume_split_workspace(*SHAPE))
    ws = torch.empty(nws // 4, dtype=torch.int32, device=dev)

    def kernel(r, st, reach, lds):
        def call():
            _set_form(lds)                                      # the switch is read per call
            volumeops.split3d(mask_d, r, st, reach, classes=C, out=out, workspace=ws)
            _set_form(None)
        return call

    variants, agree, extra = {}, True, {}
    before = int(ndimage.label(mask[0] == 1)[1])
    for v in VARIANTS:
        r, st, reach = v
        variants[('lds',) + v] = kernel(r, st, reach, True)
        variants[('step',) + v] = kernel(r, st, reach, False)
        variants[('torch',) + v] = lambda r=r, st=st, reach=reach: torch_split(mask_d, r, st, reach)
        variants[('lds',) + v]()
        a = out.clone()
        variants[('step',) + v]()
        agree = agree and torch.equal(a, out) and torch.equal(a, variants[('torch',) + v]())
        torch.cuda.empty_cache()
        extra[v] = {'voxels_cut': int((a != mask_d).sum()),
                    'objects': {'before': before, 'after': int(ndimage.label(a.cpu().numpy()[0] == 1)[1])},
                    'workspace_bytes': nws}
        print('volume_split_bench: %s agrees %s, %s' % (name_of(v), agree, extra[v]), file=sys.stderr, flush=True)
    r, st, reach = VARIANTS[0]
    host_ms, res = _host_ms(lambda: sc.split3d_ref(mask_d.cpu().numpy(), r, st, reach, C), args.host_iters)
    if res is not None:
        variants[('lds',) + VARIANTS[0]]()
        agree = agree and np.array_equal(out.cpu().numpy(), res)
        del res
    print('volume_split_bench: host path %s ms' % host_ms, file=sys.stderr, flush=True)

    for _ in range(args.warmup):
        for f in variants.values():
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(args.iters):                                 # interleaved rounds: drift hits all variants alike
        for k, f in variants.items():
            t[k].append(_time(f))
    med = {k: float(np.median(x)) for k, x in t.items()}
    span = {k: [round(min(x), 4), round(max(x), 4)] for k, x in t.items()}
    res, wins = {}, []
    for v in VARIANTS:
        r, st, reach = v
        lds, step, tt = med[('lds',) + v], med[('step',) + v], med[('torch',) + v]
        best, best_lds = min(lds, step), lds < step
        gbs, mb = MOVED / (best * 1e-3) / 1e9, model_bytes(r, st, reach, best_lds)
        hm = host_ms if v == VARIANTS[0] else NM
        res[name_of(v)] = dict(
            lds_form_ms=round(lds, 4), lds_form_ms_min_max=span[('lds',) + v], step_form_ms=round(step, 4),
            step_form_ms_min_max=span[('step',) + v], lds_over_step_form=round(lds / step, 3), **{f: NM for f in TRACED},
            torch_ms=round(tt, 3), torch_over_kernel=round(tt / best, 1), host_ms=hm,
            host_over_kernel=round(hm / best, 1) if hm != NM else NM, gb_per_s=round(gbs, 1),
            share_of_hbm=round(gbs / (HBM_TBS * 1e3), 4), model_bytes_lds_form=model_bytes(r, st, reach, True),
            model_bytes_step_form=model_bytes(r, st, reach, False), model_gb_per_s=round(mb / (best * 1e-3) / 1e9, 1),
            model_share_of_hbm=round(mb / (best * 1e-3) / 1e9 / (HBM_TBS * 1e3), 4), **extra[v])
        wins.append(best_lds)
    faster = 'LDS bricks' if all(wins) else ('one step per launch' if not any(wins) else 'mixed: see lds_over_step_form')
    return res, bool(agree), faster, 'LDS bricks' if volumeops.SPLIT3D_LDS_DEFAULT else 'one step per launch'


TRACE_CALLS = 4                                                 # per variant and form under the profiler: the first warms up


def trace_run(dev):
    """every variant in both forms, TRACE_CALLS calls each, in the order fold_trace() expects; for rocprofv3 --kernel-trace"""
    from sequitr_amd import _lib, volumeops
    mask_d = torch.from_numpy(pair_mask()).to(dev)
    out = torch.empty_like(mask_d)
    ws = torch.empty(int(_lib.load().sq_volume_split_workspace(*SHAPE)) // 4, dtype=torch.int32, device=dev)
    for r, st, reach in VARIANTS:
        for lds in (True, False):
            _set_form(lds)
            for _ in range(TRACE_CALLS):
                volumeops.split3d(mask_d, r, st, reach, classes=C, out=out, workspace=ws)
            torch.cuda.synchronize()
    _set_form(None)


def fold_trace(trace_dir, line):
    """kernel times of a --trace-run into the JSON line: a call begins at the first erosion launch (morph_kernel) after
    another kind of kernel"""
    import csv
    import glob
    files = glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True)
    if len(files) != 1:
        raise SystemExit('expected one kernel_trace.csv under %s, found %d' % (trace_dir, len(files)))
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r['Start_Timestamp']))
    groups = (('erosion', 'morph_kernel'), ('labelling', 'cc_'), ('lds', 'split_grow_lds_kernel'),
              ('step', 'split_grow_step_kernel'), ('cut', 'split_cut_kernel'))
    calls, last = [], None
    for r in rows:
        name = r['Kernel_Name']
        kind = next((g for g, pat in groups if pat in name), None)
        if kind == 'erosion' and last != 'erosion':
            calls.append({g: [] for g, _ in groups})
        if kind is not None and calls:
            calls[-1][kind].append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e6)
            last = kind
    if len(calls) != len(VARIANTS) * 2 * TRACE_CALLS:
        raise SystemExit('expected %d calls in the trace, found %d' % (len(VARIANTS) * 2 * TRACE_CALLS, len(calls)))
    k = 0
    for v in VARIANTS:
        row = line['variants'][name_of(v)]
        for form in ('lds', 'step'):
            timed = calls[k + 1:k + TRACE_CALLS]
            k += TRACE_CALLS
            assert all(len(c[form]) == len(timed[0][form]) > 0 and not c['step' if form == 'lds' else 'lds'] for c in timed), (v, form)
            med = {g: round(float(np.median([sum(c[g]) for c in timed])), 4) for g, _ in groups}
            pre = '' if form == 'lds' else 'step_form_'
            row[pre + 'regrowth_ms'], row[pre + 'regrowth_launches'] = med[form], len(timed[0][form])
            if form == 'lds':
                row['erosion_ms'], row['labelling_ms'], row['cut_ms'] = med['erosion'], med['labelling'], med['cut']
        row['regrowth_lds_over_step_form'] = round(row['regrowth_ms'] / row['step_form_regrowth_ms'], 3)
    line['kernel_times'] = 'rocprofv3 --kernel-trace, a run of its own: the median of %d calls per variant and form' % (TRACE_CALLS - 1)
    return line


def run_stream(dev, args):
    from sequitr_amd.frontend import segment_volumes
    from sequitr_amd.networks.unet import UNet3D
    from sequitr_amd.volumeops import VolumeCleanup
    host = np.random.default_rng(0).integers(100, 4000, (2,) + SHAPE[1:]).astype(np.uint16)
    net = UNet3D({'shape': (BRICK[1], BRICK[2], BRICK[0]), 'num_outputs': C, 'device': dev}, 'infer').initialize()
    cleaner = VolumeCleanup([{'op': 'split3d', 'erosions': 4}])

    def stream(post):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        segment_volumes(net, host, BRICK, 0, bricks_per_batch=8, on_masks=lambda i, m: None, postprocess=post)
        return (time.perf_counter() - t0) * 1e3 / host.shape[0]

    stream(None), stream(cleaner)
    t = {'plain': [], 'split': []}
    for _ in range(args.stream_iters):
        t['plain'].append(stream(None))
        t['split'].append(stream(cleaner))
    plain, split = float(np.median(t['plain'])), float(np.median(t['split']))
    return {'what': 'segment_volumes over 2 uint16 volumes of 64 x 1024 x 1024, bricks 32 x 128 x 128, margin 0, masks kept in '
                    'HBM: with postprocess = split3d erosions 4 (cross, reach 8, the default form) against without, host clock '
                    'per volume', 'plain_ms_per_volume': round(plain, 3), 'split_ms_per_volume': round(split, 3),
            'ms_min_max': {k: [round(min(v), 3), round(max(v), 3)] for k, v in t.items()},
            'split_share': round((split - plain) / split, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--iters', type=int, default=7)
    ap.add_argument('--host-iters', type=int, default=1)
    ap.add_argument('--stream-iters', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'volume_split_bench.json'))
    ap.add_argument('--placeholder', action='store_true', help='write "not measured" in every field (no GPU needed)')
    ap.add_argument('--trace-run', action='store_true', help='only launch every variant in both forms, for rocprofv3 --kernel-trace')
    ap.add_argument('--fold-trace', metavar='DIR', help="fold a --trace-run's kernel_trace.csv into the JSON at --out (no GPU needed)")
    args = ap.parse_args()
    if args.trace_run:
        if not torch.cuda.is_available():
            raise SystemExit('volume_split_bench needs the GPU')
        torch.cuda.set_device(0)
        trace_run('cuda:0')
        return
    if args.fold_trace:
        line = fold_trace(args.fold_trace, json.loads(open(args.out).read()))
    elif args.placeholder:
        line = placeholder()
    else:
        if not torch.cuda.is_available():
            raise SystemExit('volume_split_bench needs the GPU (--placeholder writes the file without one)')
        from sequitr_amd import volumeops
        torch.cuda.set_device(0)
        dev = 'cuda:0'
        line = {'workload': WORKLOAD, 'device': torch.cuda.get_device_name(0), 'warmup': args.warmup, 'iters': args.iters,
                'hbm_tb_per_s': HBM_TBS, 'bytes_moved_per_call': MOVED,
                'geometry': {'brick': list(volumeops.SPLIT3D_TILE), 'steps_per_launch': volumeops.SPLIT3D_STEPS}}
        line['variants'], line['agree'], line['faster_form'], line['default_form'] = run_variants(dev, pair_mask(), args)
        print('volume_split_bench: variants done', file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
        line['stream'] = run_stream(dev, args)
    text = json.dumps(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
