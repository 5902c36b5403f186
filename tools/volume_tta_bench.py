"""Volume test-time augmentation benchmark: one JSON line, also written to profiles/volume_tta_bench.json.

Workload: one uint16 volume of 64 x 1024 x 1024, bricks of 32 x 128 x 128 (Z, X, Y), K = 2 classes, 8 bricks per network
launch.  HIP events round each call after warm-up, the variants alternated call by call:
  * view    : sq_bricks_view_f32 on all bricks of the volume at once (HBM-sized, not cache-sized): `input`, the forward
    view of the E = 1 bricks, plain, and `merge`, the inverse view of the E = K logits, accumulating; per op class -- a
    flip (op 7: z, x and y mirrored) and a transposed op (op 11: transposed, z and x mirrored) with the LDS block (default)
    and with SQ_TTA_LDS=0, the direct gather -- next to the torch composition flip / transpose(...).contiguous() (+ add_),
    whose largest difference from the kernel is recorded (0: the same bits);
  * scatter : sq_bricks_scatter_probs -- the mask only, mask + uint8 and mask + float32 probabilities -- next to torch's
    argmax + softmax + one slice assignment per owned box; the largest difference of the float32 probabilities is recorded.
Bytes are what a call has to move (reads + writes, from the shapes); GB/s stands next to the 6.3 TB/s an HBM-bound kernel
can reach on the MI355X.  `segment_volumes` is the whole path, host volume in and host mask out, ms per volume at tta None /
flips / dihedral; `tta_launches_ms_per_batch` the view, merge and scatter launches of one batch of 8 bricks timed on their own
and `tta_share` their part of the batch.  `planar` holds what tools/tta_bench.py measured for the planar merge on the parent
commit and on this one (--planar-parent / --planar-this: the two JSON files), since sq_tiles_view_f32 now instantiates the
shared templates; --planar-shared / --planar-shared-parent record the run-time general form that was
measured and not kept, next to the parent commit in that same session.  Without a GPU the tool refuses to run; --placeholder writes the file with "not measured" in every field.
Usage: python tools/volume_tta_bench.py [--warmup 2] [--iters 7] [--volume-iters 3] [--planar-parent F --planar-this F]
                                        [--planar-shared F --planar-shared-parent F]
                                        [--out PATH] [--placeholder]
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

NM = 'not measured'
VOLUME, BRICK, MARGIN, K, BATCH = (64, 1024, 1024), (32, 128, 128), (4, 16, 16), 2, 8
HBM_ACHIEVABLE_GBS = 6300.
REPS = 10                                                       # calls per event pair
OP_CLASSES = {'flip': 7, 'transposed': 11}
WORKLOAD = ('volume tta: one uint16 volume of %d x %d x %d, bricks of %d x %d x %d, margin %d x %d x %d, K = %d; %d bricks '
            'per launch' % (VOLUME + BRICK + MARGIN + (K, BATCH)))
ROW_FIELDS = ('ms', 'ms_min_max', 'gb_per_s', 'fraction_of_hbm_achievable')


def placeholder():
    row = {f: NM for f in ROW_FIELDS}
    view = {step: dict({'bytes': NM}, flip={'hip': dict(row), 'torch': dict(row), 'torch_over_hip': NM, 'max_abs_difference': NM},
                       transposed={'lds': dict(row), 'direct': dict(row), 'torch': dict(row), 'torch_over_hip': NM,
                                   'direct_over_lds': NM, 'max_abs_difference': NM}) for step in ('input', 'merge')}
    scatter = {kind: {'bytes': NM, 'hip': dict(row), 'torch': dict(row), 'torch_over_hip': NM, 'max_abs_difference': NM}
               for kind in ('mask', 'uint8', 'float32')}
    whole = {str(t): {'ms_per_volume': NM, 'ms_per_volume_min_max': NM} for t in (None, 'flips', 'dihedral')}
    for t in ('flips', 'dihedral'):
        whole[t].update({'tta_launches_ms_per_batch': NM, 'tta_launches_ms_min_max': NM, 'tta_share': NM, 'over_plain': NM})
    return {'workload': WORKLOAD, 'device': NM, 'hbm_achievable_gb_per_s': HBM_ACHIEVABLE_GBS, 'view': view, 'scatter': scatter,
            'segment_volumes': whole, 'planar': {'parent': NM, 'this': NM, 'shared_form': NM, 'shared_form_parent': NM}}


def planar_record(path):
    """what tools/tta_bench.py wrote, cut down to the merge step and the whole path"""
    if not path:
        return NM
    rec = json.loads(open(path).read())
    return {'view': {step: {cls: {form: row['ms'] if isinstance(row, dict) else row for form, row in rec['view'][step][cls].items()}
                            for cls in ('identity', 'mirrored', 'transposed')} for step in ('merge', 'copy', 'input')},
            'view_ms_min_max': {step: {cls: {form: row['ms_min_max'] for form, row in rec['view'][step][cls].items()
                                             if isinstance(row, dict)} for cls in ('identity', 'mirrored', 'transposed')}
                                for step in ('merge', 'copy', 'input')},
            'stitch_ms': {kind: rec['stitch'][kind]['hip']['ms'] for kind in ('float32', 'uint8')},
            'segment_frames_ms_per_frame': {t: rec['segment_frames'][t]['ms_per_frame'] for t in ('None', 'flips', 'dihedral')}}


def measure(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('volume_tta_bench needs the GPU')
    from sequitr_amd.frontend import VOLUME_TTA_OPS, VolumeTiler, segment_volumes
    from sequitr_amd.networks.unet import UNet3D
    torch.cuda.set_device(0)
    dev = 'cuda:0'

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

    rng = np.random.default_rng(0)
    volume = rng.integers(100, 4000, (1,) + VOLUME).astype(np.uint16)
    tiler = VolumeTiler(VOLUME, BRICK, MARGIN, device=dev)
    nb = tiler.bricks_per_volume
    logits = torch.randn((nb,) + BRICK + (K,), device=dev) * 4
    bricks = torch.randn((nb,) + BRICK + (1,), device=dev)
    acc, out_bricks = torch.zeros_like(logits), torch.empty_like(bricks)

    def with_lds(on, fn):                                       # the switch is read per call
        def run():
            if on:
                os.environ.pop('SQ_TTA_LDS', None)
            else:
                os.environ['SQ_TTA_LDS'] = '0'
            fn()
            os.environ.pop('SQ_TTA_LDS', None)
        return run

    def torch_view(x, op):                                      # the header's numpy text
        x = x.transpose(2, 3) if op & 8 else x
        dims = [d for d, bit in ((1, 1), (2, 2), (3, 4)) if op & bit]
        return x.flip(dims) if dims else x

    inverse = {10: 12, 11: 13, 12: 10, 13: 11}
    variants, nbytes, diff = {}, {}, {}
    for cls, op in OP_CLASSES.items():
        forms = (('lds', True), ('direct', False)) if op & 8 else (('hip', True),)
        for form, on in forms:
            variants[('merge', cls, form)] = with_lds(on, lambda op=op: tiler.view(logits, op, inverse=True, out=acc, accumulate=True))
            variants[('input', cls, form)] = with_lds(on, lambda op=op: tiler.view(bricks, op, out=out_bricks))
        variants[('merge', cls, 'torch')] = lambda op=op: acc.add_(torch_view(logits, inverse.get(op, op)).contiguous())
        variants[('input', cls, 'torch')] = lambda op=op: out_bricks.copy_(torch_view(bricks, op))
    nbytes.update({'merge': logits.numel() * 4 * 3, 'input': bricks.numel() * 4 * 2})
    for cls, op in OP_CLASSES.items():                          # the forms and the torch composition, before anything is timed
        for step, buf in (('merge', acc), ('input', out_bricks)):
            buf.zero_()
            variants[(step, cls, 'torch')]()
            want = buf.clone()
            worst = 0.0
            for form in ('lds', 'direct') if op & 8 else ('hip',):
                buf.zero_()
                variants[(step, cls, form)]()
                worst = max(worst, float((buf - want).abs().max()))
            diff[(step, cls)] = worst
            del want

    boxes = []                                                  # (brick, origin, low, high) of every owned box, from the table
    table = tiler.geometry.table()
    KZ, KX, KY = tiler.geometry.counts
    n = KZ + KX + KY
    for b, (kz, kx, ky) in enumerate(np.ndindex(KZ, KX, KY)):
        idx = (kz, KZ + kx, KZ + KX + ky)
        boxes.append((b, [int(table[i]) for i in idx], [int(table[n + i]) for i in idx], [int(table[2 * n + i]) for i in idx]))
    mask_out = torch.empty((1,) + VOLUME, dtype=torch.uint8, device=dev)
    prob_out = {'uint8': torch.empty((1, K) + VOLUME, dtype=torch.uint8, device=dev),
                'float32': torch.empty((1, K) + VOLUME, dtype=torch.float32, device=dev)}
    t_mask, t_prob = torch.empty_like(mask_out), {k: torch.empty_like(v) for k, v in prob_out.items()}

    def torch_scatter(kind):
        m = logits.argmax(-1).to(torch.uint8)
        p = None
        if kind != 'mask':
            p = torch.softmax(logits * 0.125, -1)
            if kind == 'uint8':
                p = (p * 255 + 0.5).floor().to(torch.uint8)
        for b, o, lo, hi in boxes:
            sl = tuple(slice(lo[d] - o[d], hi[d] - o[d]) for d in range(3))
            dl = tuple(slice(lo[d], hi[d]) for d in range(3))
            t_mask[(0,) + dl] = m[(b,) + sl]
            if p is not None:
                t_prob[kind][(0, slice(None)) + dl] = p[(b,) + sl].permute(3, 0, 1, 2)

    nvox = int(np.prod(VOLUME))
    for kind, size in (('mask', 0), ('uint8', 1), ('float32', 4)):
        variants[('scatter', kind, 'hip')] = lambda kind=kind: tiler.scatter_probs(logits, mask_out, prob_out.get(kind), n=8)
        variants[('scatter', kind, 'torch')] = lambda kind=kind: torch_scatter(kind)
        nbytes[('scatter', kind)] = nvox * (K * 4 + 1 + K * size)      # the owned logits, the mask, the planes
        variants[('scatter', kind, 'hip')]()
        variants[('scatter', kind, 'torch')]()
        assert torch.equal(mask_out, t_mask), kind
        diff[('scatter', kind)] = 0.0 if kind == 'mask' else float((prob_out[kind].float() - t_prob[kind].float()).abs().max())

    for _ in range(args.warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(args.iters):                                 # interleaved rounds: drift hits all variants alike
        for k, fn in variants.items():
            t[k].append(_time(fn, REPS if k[2] != 'torch' or k[0] != 'scatter' else 1))
    view = {}
    for step in ('input', 'merge'):
        view[step] = {'bytes': int(nbytes[step])}
        for cls, op in OP_CLASSES.items():
            forms = ('lds', 'direct') if op & 8 else ('hip',)
            row = {form: _row(t[(step, cls, form)], nbytes[step]) for form in forms}
            row['torch'] = _row(t[(step, cls, 'torch')], nbytes[step])
            row['torch_over_hip'] = round(row['torch']['ms'] / row[forms[0]]['ms'], 3)
            if op & 8:
                row['direct_over_lds'] = round(row['direct']['ms'] / row['lds']['ms'], 3)
            row['max_abs_difference'] = diff[(step, cls)]
            view[step][cls] = row
    scatter = {}
    for kind in ('mask', 'uint8', 'float32'):
        nby = nbytes[('scatter', kind)]
        h, r = _row(t[('scatter', kind, 'hip')], nby), _row(t[('scatter', kind, 'torch')], nby)
        scatter[kind] = {'bytes': int(nby), 'hip': h, 'torch': r, 'torch_over_hip': round(r['ms'] / h['ms'], 3),
                         'max_abs_difference': diff[('scatter', kind)]}
    del logits, bricks, acc, out_bricks, prob_out, t_prob
    torch.cuda.empty_cache()

    # the whole path, and the launches test-time augmentation adds to one batch of BATCH bricks
    net = UNet3D({'shape': (BRICK[1], BRICK[2], BRICK[0]), 'num_outputs': K, 'device': dev, 'seed': 0}, 'infer').initialize()
    whole = {}
    for tta in (None, 'flips', 'dihedral'):
        run = lambda: segment_volumes(net, volume, BRICK, MARGIN, bricks_per_batch=BATCH, tta=tta)
        run()
        ts = []
        for _ in range(args.volume_iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            ts.append((time.perf_counter() - t0) * 1e3)
        whole[str(tta)] = {'ms_per_volume': round(float(np.median(ts)), 2), 'ms_per_volume_min_max': [round(min(ts), 2), round(max(ts), 2)]}
    bl, bt = torch.randn((BATCH,) + BRICK + (K,), device=dev), torch.randn((BATCH,) + BRICK + (1,), device=dev)
    ba, bo = torch.empty_like(bl), torch.empty_like(bt)
    for tta in ('flips', 'dihedral'):
        ops = VOLUME_TTA_OPS[tta]

        def launches(ops=ops):
            for op in ops:
                if op:
                    tiler.view(bt, op, out=bo)
                tiler.view(bl, op, inverse=True, out=ba, accumulate=op != 0)
            tiler.scatter_probs(ba, mask_out, None, n=len(ops))
        launches()
        ls = [_time(launches, REPS) for _ in range(args.iters)]
        batch_ms = whole[tta]['ms_per_volume'] / ((nb + BATCH - 1) // BATCH)
        whole[tta].update({'tta_launches_ms_per_batch': round(float(np.median(ls)), 4),
                           'tta_launches_ms_min_max': [round(min(ls), 4), round(max(ls), 4)],
                           'tta_share': round(float(np.median(ls)) / batch_ms, 5),
                           'over_plain': round(whole[tta]['ms_per_volume'] / whole['None']['ms_per_volume'], 3)})
    return {'workload': WORKLOAD, 'bricks_per_volume': int(nb), 'warmup': args.warmup, 'iters': args.iters, 'calls_per_window': REPS,
            'device': torch.cuda.get_device_name(0), 'hbm_achievable_gb_per_s': HBM_ACHIEVABLE_GBS, 'view': view,
            'scatter': scatter, 'segment_volumes': whole,
            'planar': {'parent': planar_record(args.planar_parent), 'this': planar_record(args.planar_this),
                       'shared_form': planar_record(args.planar_shared),
                       'shared_form_parent': planar_record(args.planar_shared_parent)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--iters', type=int, default=7)
    ap.add_argument('--volume-iters', type=int, default=3)
    ap.add_argument('--planar-parent', default=None, help="tools/tta_bench.py's JSON measured on the parent commit")
    ap.add_argument('--planar-this', default=None, help="tools/tta_bench.py's JSON measured on this commit")
    ap.add_argument('--planar-shared', default=None,
                    help="the same, measured with sq_tiles_view_f32 on the run-time general kernels (the form not kept)")
    ap.add_argument('--planar-shared-parent', default=None, help="the parent commit measured in that same session")
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'volume_tta_bench.json'))
    ap.add_argument('--placeholder', action='store_true', help='write "not measured" in every field (no GPU needed)')
    args = ap.parse_args()
    line = placeholder() if args.placeholder else measure(args)
    text = json.dumps(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
