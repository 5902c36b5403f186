"""Mask clean-up benchmark: one JSON line, also written to profiles/mask_cleanup_bench.json.

Workload: 8 uint8 masks of 2048 x 2048 at C = 2 resident in HBM, generated once --
  * disks        : ~2000 random disks per frame, each with a small hole (cell-like objects);
  * checkerboard : every other pixel its own object and its own hole, the worst case for the labelling.
HIP events round each call after warm-up, outputs and workspaces allocated before, the variants alternated round by round:
  * morph        : sq_mask_morph_u8 (maskops.morph) for open and erode, cross and square, r = 1, 2, 4, 8, 16: ms per launch
                   and GB/s against the 2 B per pixel a call must move (one read, one write), next to the 6.3 TB/s of HBM;
                   `r16_over_r1` says how flat the launch time is in r.
  * fill_holes / clear_border : the same for the two component operations (several kernels per call).
  * torch        : the torch composition in the same run -- max_pool2d on the Boolean plane (float16), iterated, the
                   plane's conversion and the merge included; the two component operations have none (torch has no
                   labelling) and are compared with the host path.
  * host         : download + scipy.ndimage (binary_opening / binary_erosion at r = 1 and 16, binary_fill_holes, label) by the
                   host clock, `--host-iters` times.
`agree` says the variants computed the same masks.  `loses_to_torch` lists every morph variant whose launch is slower than
its torch composition.  `stream` is the share of a three-step clean-up (open 2 cross, fill_holes 400, clear_border) in
frontend.segment_frames' stream over 8 uint16 frames of 2048 x 2048 (tile 512, margin 32, UNet2D default filters) against the
stream without it, alternated, host clock per frame.
Without a GPU the tool refuses to run; --placeholder writes the file with "not measured" in every field.
Usage: python tools/mask_cleanup_bench.py [--warmup 2] [--iters 5] [--host-iters 1] [--stream-iters 3] [--out PATH] [--placeholder]
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
WORKLOAD = ('mask clean-up: %d x %d x %d uint8 masks at C = %d, ~2000 random disks per frame with a small hole each and the '
            'checkerboard worst case' % (N, H, W, C))
RADII = (1, 2, 4, 8, 16)
MORPHS = tuple((op, st) for op in ('open', 'erode') for st in ('cross', 'square'))
MOVED = 2 * N * H * W                                          # bytes a call must move: the mask in, the mask out
STEPS = [{'op': 'open', 'iterations': 2, 'structure': 'cross'}, {'op': 'fill_holes', 'max_area': 400}, {'op': 'clear_border'}]
MORPH_FIELDS = ('ms', 'gb_per_s', 'share_of_hbm', 'torch_ms', 'torch_over_kernel', 'r16_over_r1', 'ms_min_max')
COMP_FIELDS = ('ms', 'gb_per_s', 'share_of_hbm', 'host_ms', 'host_over_kernel', 'workspace_bytes', 'ms_min_max')
STREAM_FIELDS = ('what', 'plain_ms_per_frame', 'cleanup_ms_per_frame', 'ms_min_max', 'cleanup_share')


def placeholder():
    case = {'morph': {'%s_%s' % m: {f: NM for f in MORPH_FIELDS} for m in MORPHS},
            'fill_holes': {f: NM for f in COMP_FIELDS}, 'clear_border': {f: NM for f in COMP_FIELDS},
            'host_morph_ms': NM, 'loses_to_torch': NM, 'agree': NM}
    return {'workload': WORKLOAD, 'device': NM, 'hbm_tb_per_s': HBM_TBS, 'bytes_moved_per_call': MOVED,
            'cases': {'disks': case, 'checkerboard': case}, 'stream': {f: NM for f in STREAM_FIELDS}}


def disk_masks(seed=0, per_frame=2000):
    """N masks with ~per_frame disks of radius 4 .. 14, each with a hole of radius 1 .. 2 somewhere inside"""
    rng = np.random.default_rng(seed)
    m = np.zeros((N, H, W), np.uint8)
    for i in range(N):
        holes = []
        for _ in range(per_frame):
            cy, cx, r = int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(4, 15))
            y0, y1, x0, x1 = max(cy - r, 0), min(cy + r + 1, H), max(cx - r, 0), min(cx + r + 1, W)
            yy, xx = np.mgrid[y0:y1, x0:x1]
            m[i, y0:y1, x0:x1][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 1
            holes.append((cy + int(rng.integers(-1, 2)), cx + int(rng.integers(-1, 2)), int(rng.integers(1, 3))))
        for cy, cx, r in holes:
            y0, y1, x0, x1 = max(cy - r, 0), min(cy + r + 1, H), max(cx - r, 0), min(cx + r + 1, W)
            yy, xx = np.mgrid[y0:y1, x0:x1]
            m[i, y0:y1, x0:x1][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 0
    return m


def checkerboard():
    yy, xx = np.mgrid[0:H, 0:W]
    return np.repeat(((yy + xx) & 1).astype(np.uint8)[None], N, axis=0)


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def torch_morph(mask_d, op, st, r):
    """the composition a torch user writes at C = 2: the class plane in float16, r (+ r) 3x3 max-pools with scipy's zero
    border, back to uint8 under the merge rule for operations that only remove pixels"""
    import torch.nn.functional as F
    x = (mask_d == 1).to(torch.float16)[:, None]

    def dilate(x):
        if st == 'square':
            return F.max_pool2d(x, 3, 1, 1)
        return torch.maximum(F.max_pool2d(x, (1, 3), 1, (0, 1)), F.max_pool2d(x, (3, 1), 1, (1, 0)))

    def erode(x):
        xp = -F.pad(x, (1, 1, 1, 1), value=0.0)                 # a zero border, not max_pool2d's -inf
        if st == 'square':
            return -F.max_pool2d(xp, 3, 1, 0)
        return -torch.maximum(F.max_pool2d(xp[:, :, 1:-1], (1, 3), 1, 0), F.max_pool2d(xp[:, :, :, 1:-1], (3, 1), 1, 0))

    for _ in range(r):
        x = erode(x)
    if op == 'open':
        for _ in range(r):
            x = dilate(x)
    return ((x[:, 0] > 0) & (mask_d == 1)).to(torch.uint8)


def host_morph(mask_d, op, st, r):
    from scipy import ndimage
    fn = ndimage.binary_opening if op == 'open' else ndimage.binary_erosion
    s = ndimage.generate_binary_structure(2, 1 if st == 'cross' else 2)
    mask = mask_d.cpu().numpy()
    return np.stack([fn(m == 1, s, iterations=r) for m in mask]).astype(np.uint8)


def host_fill(mask_d):
    from scipy import ndimage
    mask = mask_d.cpu().numpy()
    return np.stack([ndimage.binary_fill_holes(m == 1) for m in mask]).astype(np.uint8)


def host_clear(mask_d):
    from scipy import ndimage
    mask = mask_d.cpu().numpy()
    out = np.empty_like(mask)
    for i, m in enumerate(mask):
        lab, n = ndimage.label(m == 1)
        edge = np.zeros(n + 1, bool)
        for line in (lab[0], lab[-1], lab[:, 0], lab[:, -1]):
            edge[line] = True
        edge[0] = True
        out[i] = ~edge[lab]
    return out


def _host_ms(fn, iters):
    t, res = [], None
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return (round(float(np.median(t)), 1) if t else NM), res


def _rates(ms):
    gbs = MOVED / (ms * 1e-3) / 1e9
    return {'ms': round(ms, 4), 'gb_per_s': round(gbs, 1), 'share_of_hbm': round(gbs / (HBM_TBS * 1e3), 4)}


def run_case(dev, mask, args):
    from sequitr_amd import _lib, maskops
    lib = _lib.load()
    mask_d = torch.from_numpy(mask).to(dev)
    out = torch.empty_like(mask_d)
    ws_bytes = {'fill_holes': int(lib.sq_mask_fill_holes_workspace(N, H, W)), 'clear_border': int(lib.sq_mask_clear_border_workspace(N, H, W))}
    ws = torch.empty(max(ws_bytes.values()) // 4, dtype=torch.int32, device=dev)
    variants = {}
    for op, st in MORPHS:
        for r in RADII:
            variants[('k', op, st, r)] = lambda op=op, st=st, r=r: maskops.morph(mask_d, op, r, st, classes=C, out=out)
            variants[('t', op, st, r)] = lambda op=op, st=st, r=r: torch_morph(mask_d, op, st, r)
    variants[('k', 'fill_holes')] = lambda: maskops.fill_holes(mask_d, None, classes=C, out=out, workspace=ws)
    variants[('k', 'clear_border')] = lambda: maskops.clear_border(mask_d, classes=C, out=out, workspace=ws)

    agree = True
    for op, st in MORPHS:                                       # the kernel, torch and (at two radii) the host agree
        for r in RADII:
            agree = agree and torch.equal(variants[('k', op, st, r)](), variants[('t', op, st, r)]())
    host = {}
    for r in (1, 16):
        host['open_cross_r%d' % r], res = _host_ms(lambda r=r: host_morph(mask_d, 'open', 'cross', r), args.host_iters)
        if res is not None:
            agree = agree and np.array_equal(variants[('k', 'open', 'cross', r)]().cpu().numpy(), res)
    host['erode_square_r1'], res = _host_ms(lambda: host_morph(mask_d, 'erode', 'square', 1), args.host_iters)
    fill_ms, res = _host_ms(lambda: host_fill(mask_d), args.host_iters)
    if res is not None:
        agree = agree and np.array_equal(variants[('k', 'fill_holes')]().cpu().numpy(), res)
    clear_ms, res = _host_ms(lambda: host_clear(mask_d), args.host_iters)
    if res is not None:
        agree = agree and np.array_equal(variants[('k', 'clear_border')]().cpu().numpy(), res)

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
    res = {'morph': {}, 'loses_to_torch': []}
    for op, st in MORPHS:
        name = '%s_%s' % (op, st)
        row = {f: {} for f in ('ms', 'gb_per_s', 'share_of_hbm', 'torch_ms', 'torch_over_kernel', 'ms_min_max')}
        for r in RADII:
            k, tt = med[('k', op, st, r)], med[('t', op, st, r)]
            for f, v in _rates(k).items():
                row[f]['r%d' % r] = v
            row['torch_ms']['r%d' % r] = round(tt, 4)
            row['torch_over_kernel']['r%d' % r] = round(tt / k, 2)
            row['ms_min_max']['r%d' % r] = span[('k', op, st, r)]
            if tt < k:
                res['loses_to_torch'].append('%s r%d' % (name, r))
        row['r16_over_r1'] = round(med[('k', op, st, 16)] / med[('k', op, st, 1)], 2)
        res['morph'][name] = row
    for name, host_ms in (('fill_holes', fill_ms), ('clear_border', clear_ms)):
        k = med[('k', name)]
        res[name] = dict(_rates(k), host_ms=host_ms, host_over_kernel=round(host_ms / k, 1) if host_ms != NM else NM,
                         workspace_bytes=ws_bytes[name], ms_min_max=span[('k', name)])
    res['host_morph_ms'] = host
    res['agree'] = bool(agree)
    return res


def run_stream(dev, args):
    from sequitr_amd.frontend import segment_frames
    from sequitr_amd.maskops import MaskCleanup
    from sequitr_amd.networks.unet import UNet2D
    frames = np.random.default_rng(0).integers(100, 4000, (N, H, W)).astype(np.uint16)
    net = UNet2D({'shape': (512, 512), 'num_outputs': C, 'device': dev}, 'infer').initialize()
    cleanup = MaskCleanup(STEPS)

    def stream(**kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        segment_frames(net, frames, tile=512, margin=32, frames_per_batch=4, **kw)   # ends in a synchronise
        return (time.perf_counter() - t0) * 1e3 / N

    kinds = {'plain': {}, 'cleanup': {'postprocess': cleanup}}
    for kw in kinds.values():
        stream(**kw)
    t = {k: [] for k in kinds}
    for _ in range(args.stream_iters):
        for k, kw in kinds.items():
            t[k].append(stream(**kw))
    plain, clean = float(np.median(t['plain'])), float(np.median(t['cleanup']))
    return {'what': 'segment_frames over %d uint16 frames of %d x %d, tile 512, margin 32, 4 frames per batch, masks downloaded: '
                    'with postprocess = open 2 cross, fill_holes 400, clear_border against without, host clock per frame' % (N, H, W),
            'plain_ms_per_frame': round(plain, 3), 'cleanup_ms_per_frame': round(clean, 3),
            'ms_min_max': {k: [round(min(v), 3), round(max(v), 3)] for k, v in t.items()},
            'cleanup_share': round((clean - plain) / plain, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--host-iters', type=int, default=1)
    ap.add_argument('--stream-iters', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mask_cleanup_bench.json'))
    ap.add_argument('--placeholder', action='store_true', help='write "not measured" in every field (no GPU needed)')
    args = ap.parse_args()
    if args.placeholder:
        line = placeholder()
    else:
        if not torch.cuda.is_available():
            raise SystemExit('mask_cleanup_bench needs the GPU')
        torch.cuda.set_device(0)
        dev = 'cuda:0'
        line = {'workload': WORKLOAD, 'device': torch.cuda.get_device_name(0), 'warmup': args.warmup, 'iters': args.iters,
                'hbm_tb_per_s': HBM_TBS, 'bytes_moved_per_call': MOVED, 'cases': {}}
        for name, make in (('disks', disk_masks), ('checkerboard', checkerboard)):
            line['cases'][name] = run_case(dev, make(), args)
            print('mask_cleanup_bench: %s done' % name, file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
        line['stream'] = run_stream(dev, args)
    text = json.dumps(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
