"""Volume clean-up benchmark: one JSON line, also written to profiles/volume_cleanup_bench.json.

Workload: one resident (1, 64, 1024, 1024) uint8 mask generated here from a seed -- about 2000 random balls with a small
cavity each -- at C = 2, the same mask with every other ball in class 2 (C = 3: the morphology kernel reads its region once
per class), and the 3-D checkerboard, the labelling's worst case.
  * morph      : ms per morph3d launch (HIP events, median of --iters) for erode and open, 'cross' and 'cube', r = 1, 2, 4,
                 and GB/s of the 2 B per voxel a call must move next to the 6.3 TB/s an HBM-bound kernel reaches.  In the same
                 run, alternated round by round, with minimum and maximum: `plane_cross` at the same r through the planar
                 kernel on the same bytes (a different operation -- slice by slice -- shown as the cost of the third axis),
                 and the composition a torch user writes: iterated max_pool3d on the float16 plane, conversion and merge
                 included.  `host_ms`: download + scipy.ndimage + nothing else, once per variant at r = 1 and 4 (--host-iters 0
                 leaves them "not measured").
  * components : fill_cavities and clear_border3d in ms with their workspace bytes, against the host path, on the balls
                 and on the checkerboard.
  * stream     : frontend.segment_volumes over the 64 x 1024 x 1024 uint16 volume of tools/volume_frontend_bench.py
                 (bricks 32 x 128 x 128, margin 0) with and without a three-step list (open 1 cross, fill_holes, clear_border
                 lateral), alternated, by the host clock: the list's share of the stream.
`agree` says that every variant gave the same masks as the others that compute the same thing (kernel, torch composition,
host path); `loses_to_torch` lists every variant whose kernel is slower than its composition.
Without a GPU the tool refuses to run; --placeholder writes the file with "not measured" in every field.  Reads nothing
outside the repository.
Usage: python tools/volume_cleanup_bench.py [--warmup 1] [--iters 5] [--host-iters 1] [--stream-iters 2] [--out PATH] [--placeholder]
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
BRICK = (32, 128, 128)
HBM_TBS = 6.3
MOVED = 2 * SHAPE[1] * SHAPE[2] * SHAPE[3]                      # bytes a call must move: the mask in, the mask out
WORKLOAD = ('volume clean-up: one %d x %d x %d x %d uint8 mask, ~2000 balls with a cavity each, C = 2 and C = 3; '
            'the 3-D checkerboard for the component operations' % SHAPE)
VARIANTS = tuple((op, st, r) for op in ('erode', 'open') for st in ('cross', 'cube') for r in (1, 2, 4))
FIELDS = ('ms', 'ms_min_max', 'gb_per_s', 'share_of_hbm', 'c3_ms', 'c3_over_c2', 'plane_cross_ms', 'plane_cross_ms_min_max',
          'torch_ms', 'torch_ms_min_max', 'torch_over_kernel', 'host_ms', 'host_over_kernel')
COMPONENTS = ('fill_cavities', 'clear_border3d_all', 'clear_border3d_lateral', 'fill_cavities_checkerboard',
              'clear_border3d_checkerboard')
COMPONENT_FIELDS = ('ms', 'ms_min_max', 'workspace_bytes', 'host_ms', 'host_over_kernel')
STREAM_FIELDS = ('what', 'plain_ms_per_volume', 'cleaned_ms_per_volume', 'ms_min_max', 'cleanup_share')
STEPS = [{'op': 'open', 'iterations': 1, 'structure': 'cross'}, {'op': 'fill_holes'}, {'op': 'clear_border', 'faces': 'lateral'}]


def name_of(v):
    return '%s_%s_r%d' % v


def placeholder():
    return {'workload': WORKLOAD, 'device': NM, 'hbm_tb_per_s': HBM_TBS, 'bytes_moved_per_call': MOVED,
            'morph': {name_of(v): {f: NM for f in FIELDS} for v in VARIANTS},
            'components': {c: {f: NM for f in COMPONENT_FIELDS} for c in COMPONENTS},
            'launch_time_flat_in_r': NM, 'agree': NM, 'loses_to_torch': NM, 'stream': {f: NM for f in STREAM_FIELDS}}


def ball_mask(seed=0, balls=2000, classes=2):
    rng = np.random.default_rng(seed)
    _, D, H, W = SHAPE
    m = np.zeros(SHAPE, np.uint8)
    for k in range(balls):
        cz, cy, cx, rad = int(rng.integers(0, D)), int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(6, 14))
        z0, z1, y0, y1, x0, x1 = max(cz - rad, 0), min(cz + rad + 1, D), max(cy - rad, 0), min(cy + rad + 1, H), \
            max(cx - rad, 0), min(cx + rad + 1, W)
        zz, yy, xx = np.mgrid[z0:z1, y0:y1, x0:x1]
        d2 = (zz - cz) ** 2 + (yy - cy) ** 2 + (xx - cx) ** 2
        box = m[0, z0:z1, y0:y1, x0:x1]
        box[d2 <= rad * rad] = 1 + (k % (classes - 1))
        box[d2 <= 2] = 0                                        # the cavity
    return m


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def torch_morph(mask_d, op, st, r):
    """the composition a torch user writes at C = 2: iterated max_pool3d on the float16 plane, zeros outside the volume"""
    import torch.nn.functional as F
    x = (mask_d == 1).to(torch.float16)[:, None]

    def step(x, dilate):
        x = x if dilate else 1.0 - x                            # erosion: dilate the complement, ones outside the volume
        xp = F.pad(x, (1, 1, 1, 1, 1, 1), value=0.0 if dilate else 1.0)
        if st == 'cube':
            y = F.max_pool3d(xp, 3, 1, 0)
        else:
            c = xp[:, :, 1:-1, 1:-1, 1:-1]
            y = torch.maximum(torch.maximum(F.max_pool3d(xp[:, :, :, 1:-1, 1:-1], (3, 1, 1), 1, 0),
                                            F.max_pool3d(xp[:, :, 1:-1, :, 1:-1], (1, 3, 1), 1, 0)),
                              torch.maximum(F.max_pool3d(xp[:, :, 1:-1, 1:-1, :], (1, 1, 3), 1, 0), c))
        return y if dilate else 1.0 - y
    for dilate in {'erode': [False] * r, 'open': [False] * r + [True] * r}[op]:
        x = step(x, dilate)
    return torch.where((x[:, 0] > 0) & (mask_d == 1), mask_d, torch.zeros_like(mask_d))    # the anti-extensive merge


def host_morph(mask_d, op, st, r):
    from scipy import ndimage
    m = mask_d.cpu().numpy()
    fn = ndimage.binary_erosion if op == 'erode' else ndimage.binary_opening
    q = fn(m[0] == 1, ndimage.generate_binary_structure(3, 1 if st == 'cross' else 3), iterations=r)
    return np.where(q & (m[0] == 1), 1, 0).astype(np.uint8)[None]


def host_fill(mask_d):
    from scipy import ndimage
    m = mask_d.cpu().numpy()
    return np.where(m > 0, m, ndimage.binary_fill_holes(m[0] == 1)[None].astype(np.uint8))


def host_clear(mask_d, faces):
    from scipy import ndimage
    m = mask_d.cpu().numpy()
    lab, n = ndimage.label(m[0] == 1)
    hit = np.zeros(n + 1, bool)
    for side in [lab[:, 0], lab[:, -1], lab[:, :, 0], lab[:, :, -1]] + ([lab[0], lab[-1]] if faces == 'all' else []):
        hit[side] = True
    hit[0] = True
    return (~hit[lab]).astype(np.uint8)[None]


def _host_ms(fn, iters):
    t, res = [], None
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return (float(np.median(t)) if t else None), res


def _r(x, n=4):
    return round(float(x), n)


def measure(args):
    from sequitr_amd import _lib, volumeops
    from sequitr_amd.frontend import segment_volumes
    from sequitr_amd.networks.unet import UNet3D
    torch.cuda.set_device(0)
    dev = 'cuda:0'
    lib = _lib.load()
    d2 = torch.from_numpy(ball_mask(0, classes=2)).to(dev)
    d3 = torch.from_numpy(ball_mask(0, classes=3)).to(dev)
    out, out_p = torch.empty_like(d2), torch.empty_like(d2)
    agree, loses, morph = True, [], {}
    for v in VARIANTS:
        op, st, r = v
        kern = lambda: volumeops.morph3d(d2, op, r, st, classes=2, out=out)             # noqa: E731
        kern3 = lambda: volumeops.morph3d(d3, op, r, st, classes=3, out=out_p)          # noqa: E731
        plane = lambda: volumeops.morph3d(d2, op, r, 'plane_cross', classes=2, out=out_p)   # noqa: E731
        comp = lambda: torch_morph(d2, op, st, r)                                         # noqa: E731
        for _ in range(args.warmup):
            kern(), kern3(), plane(), comp()
        torch.cuda.synchronize()
        t = {'k': [], 'k3': [], 'p': [], 't': []}
        for _ in range(args.iters):                             # alternate the variants so drift hits all alike
            t['k'].append(_time(kern))
            t['k3'].append(_time(kern3))
            t['p'].append(_time(plane))
            t['t'].append(_time(comp))
        kern()
        same = torch.equal(out, comp())
        host_ms = None
        if r in (1, 4) and args.host_iters > 0:
            host_ms, ref = _host_ms(lambda: host_morph(d2, op, st, r), args.host_iters)
            same = same and np.array_equal(out.cpu().numpy(), ref)
        agree = agree and same
        ms, tms = float(np.median(t['k'])), float(np.median(t['t']))
        if ms > tms:
            loses.append(name_of(v))
        morph[name_of(v)] = {
            'ms': _r(ms), 'ms_min_max': [_r(min(t['k'])), _r(max(t['k']))], 'gb_per_s': _r(MOVED / ms / 1e6, 1),
            'share_of_hbm': _r(MOVED / ms / 1e6 / (HBM_TBS * 1e3)), 'c3_ms': _r(np.median(t['k3'])),
            'c3_over_c2': _r(np.median(t['k3']) / ms, 3), 'plane_cross_ms': _r(np.median(t['p'])),
            'plane_cross_ms_min_max': [_r(min(t['p'])), _r(max(t['p']))], 'torch_ms': _r(tms),
            'torch_ms_min_max': [_r(min(t['t'])), _r(max(t['t']))], 'torch_over_kernel': _r(tms / ms, 2),
            'host_ms': NM if host_ms is None else _r(host_ms, 1),
            'host_over_kernel': NM if host_ms is None else _r(host_ms / ms, 1)}
        print(name_of(v), morph[name_of(v)], file=sys.stderr, flush=True)
    flat = {}
    for op in ('erode', 'open'):
        for st in ('cross', 'cube'):
            a, b = morph[name_of((op, st, 1))]['ms'], morph[name_of((op, st, 4))]['ms']
            flat['%s_%s_r4_over_r1' % (op, st)] = _r(b / a, 2)

    # the component operations
    _, D, H, W = SHAPE
    zz, yy, xx = np.ogrid[0:D, 0:H, 0:W]
    board = torch.from_numpy(((zz + yy + xx) % 2).astype(np.uint8)[None]).to(dev)
    ws_fill, ws_clear = int(lib.sq_volume_fill_holes_workspace(*SHAPE)), int(lib.sq_volume_clear_border_workspace(*SHAPE))
    ws = torch.empty(ws_fill // 4, dtype=torch.int32, device=dev)
    comps = {'fill_cavities': (lambda: volumeops.fill_cavities(d2, None, classes=2, out=out, workspace=ws), ws_fill,
                               lambda: host_fill(d2)),
             'clear_border3d_all': (lambda: volumeops.clear_border3d(d2, 'all', classes=2, out=out, workspace=ws), ws_clear,
                                    lambda: host_clear(d2, 'all')),
             'clear_border3d_lateral': (lambda: volumeops.clear_border3d(d2, 'lateral', classes=2, out=out, workspace=ws),
                                        ws_clear, lambda: host_clear(d2, 'lateral')),
             'fill_cavities_checkerboard': (lambda: volumeops.fill_cavities(board, None, classes=2, out=out, workspace=ws),
                                            ws_fill, None),
             'clear_border3d_checkerboard': (lambda: volumeops.clear_border3d(board, 'all', classes=2, out=out, workspace=ws),
                                             ws_clear, None)}
    rows = {}
    for name, (fn, nbytes, host) in comps.items():
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t = [_time(fn) for _ in range(args.iters)]
        ms, host_ms = float(np.median(t)), None
        if host is not None and args.host_iters > 0:
            host_ms, ref = _host_ms(host, args.host_iters)
            agree = agree and np.array_equal(out.cpu().numpy(), ref)
        rows[name] = {'ms': _r(ms), 'ms_min_max': [_r(min(t)), _r(max(t))], 'workspace_bytes': nbytes,
                      'host_ms': NM if host_ms is None else _r(host_ms, 1),
                      'host_over_kernel': NM if host_ms is None else _r(host_ms / ms, 1)}
        print(name, rows[name], file=sys.stderr, flush=True)
    del ws, board, d3, out_p
    torch.cuda.empty_cache()

    # the three-step list in segment_volumes' stream
    host = np.random.default_rng(0).integers(100, 4000, (2,) + SHAPE[1:]).astype(np.uint16)
    net = UNet3D({'shape': (BRICK[1], BRICK[2], BRICK[0]), 'num_outputs': 2, 'device': dev}, 'infer').initialize()
    cleaner = volumeops.VolumeCleanup(STEPS)

    def stream(post):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        segment_volumes(net, host, BRICK, 0, bricks_per_batch=8, on_masks=lambda i, m: None, postprocess=post)
        return (time.perf_counter() - t0) * 1e3 / host.shape[0]
    stream(None), stream(cleaner)
    plain, cleaned = [], []
    for _ in range(args.stream_iters):
        plain.append(stream(None))
        cleaned.append(stream(cleaner))
    p, c = float(np.median(plain)), float(np.median(cleaned))
    return {'workload': WORKLOAD, 'device': torch.cuda.get_device_name(0), 'hbm_tb_per_s': HBM_TBS,
            'bytes_moved_per_call': MOVED, 'warmup': args.warmup, 'iters': args.iters, 'morph': morph, 'components': rows,
            'launch_time_flat_in_r': flat, 'agree': bool(agree), 'loses_to_torch': loses,
            'stream': {'what': 'segment_volumes, 2 x 64 x 1024 x 1024 uint16, bricks 32 x 128 x 128, margin 0, masks kept in '
                               'HBM; steps: open 1 cross, fill_holes, clear_border lateral', 'plain_ms_per_volume': _r(p, 2),
                       'cleaned_ms_per_volume': _r(c, 2), 'ms_min_max': [_r(min(plain + cleaned), 2), _r(max(plain + cleaned), 2)],
                       'cleanup_share': _r((c - p) / c, 4)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--host-iters', type=int, default=1)
    ap.add_argument('--stream-iters', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'volume_cleanup_bench.json'))
    ap.add_argument('--placeholder', action='store_true', help='write "not measured" in every field (no GPU needed)')
    args = ap.parse_args()
    if args.placeholder:
        line = placeholder()
    elif not torch.cuda.is_available():
        raise SystemExit('volume_cleanup_bench needs the GPU (--placeholder writes the file without one)')
    else:
        line = measure(args)
    text = json.dumps(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
