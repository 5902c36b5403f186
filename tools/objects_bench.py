"""Object-measurement benchmark: one JSON line, also written to profiles/objects_bench.json.

Workload: 8 uint8 masks of 2048 x 2048 at C = 2 resident in HBM, generated once, each with a uint16 image --
  * disks        : ~2000 random disks per frame (cell-like objects);
  * checkerboard : every other pixel its own object, the worst case for labelling, slots and atomics.
HIP events round each call after warm-up, the variants alternated round by round; a call includes its host part (counter
read-back, the rows' download and sort), which is what a user waits for:
  * measure             : objects.measure_objects(mask)
  * measure_image       : ... with the uint16 image
  * measure_labels      : ... with the image and the label image
  * centroids           : centroids.mask_centroids on the same masks in the same run (kernels this change leaves alone)
  * host                : the path this replaces -- download mask and image and, per frame and class, scipy.ndimage label /
                          sum_labels / find_objects / minimum / maximum; host clock, `--host-iters` times.
`workspace_bytes` is what a measure call allocates beside its outputs; `objects` the number of rows.  `stream` is the share of
a measuring sink in frontend.segment_frames' stream over 8 uint16 frames of 2048 x 2048 (tile 512, margin 32, UNet2D default
filters): on_batch -> measure_objects against the raw frames, over on_masks -> mask_centroids, alternated.
Without a GPU the tool refuses to run; --placeholder writes the file with "not measured" in every field.
Usage: python tools/objects_bench.py [--warmup 2] [--iters 5] [--host-iters 1] [--stream-iters 3] [--out PATH] [--placeholder]
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
WORKLOAD = ('object measurements: %d x %d x %d uint8 masks at C = %d with uint16 images, ~2000 random disks per frame and the '
            'checkerboard worst case' % (N, H, W, C))
VARIANTS = ('measure', 'measure_image', 'measure_labels', 'centroids')
CASE_FIELDS = tuple('%s_ms' % v for v in VARIANTS) + ('ms_min_max', 'host_ms', 'host_over_measure_image',
                                                      'measure_over_centroids', 'objects', 'workspace_bytes', 'agree')
STREAM_FIELDS = ('what', 'centroids_ms_per_frame', 'measure_ms_per_frame', 'ms_min_max', 'measure_share')


def placeholder():
    return {'workload': WORKLOAD, 'device': NM, 'cases': {k: {f: NM for f in CASE_FIELDS} for k in ('disks', 'checkerboard')},
            'stream': {f: NM for f in STREAM_FIELDS}}


def disk_masks(seed=0, per_frame=2000):
    """N masks with ~per_frame disks of radius 3 .. 14 each, classes 1 and 2"""
    rng = np.random.default_rng(seed)
    m = np.zeros((N, H, W), np.uint8)
    for i in range(N):
        for _ in range(per_frame):
            cy, cx, r = int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(3, 15))
            y0, y1, x0, x1 = max(cy - r, 0), min(cy + r + 1, H), max(cx - r, 0), min(cx + r + 1, W)
            yy, xx = np.mgrid[y0:y1, x0:x1]
            m[i, y0:y1, x0:x1][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = rng.integers(1, C + 1)
    return m


def checkerboard():
    yy, xx = np.mgrid[0:H, 0:W]
    one = (((yy + xx) & 1) * (1 + ((yy >> 1) & 1))).astype(np.uint8)
    return np.repeat(one[None], N, axis=0)


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def host_path(mask_d, image_d):
    """download + scipy.ndimage per frame and class; returns (objects, total area, total intensity) for the agreement check"""
    from scipy import ndimage
    mask, image = mask_d.cpu().numpy(), image_d.cpu().numpy()
    k = area = total = 0
    for f in range(mask.shape[0]):
        img = image[f].astype(np.int64)
        for c in range(1, C + 1):
            lab, n = ndimage.label(mask[f] == c)
            if n == 0:
                continue
            idx = np.arange(1, n + 1)
            a = ndimage.sum_labels(np.ones(lab.shape, np.int64), lab, idx)
            ndimage.find_objects(lab)
            s = ndimage.sum_labels(img, lab, idx)
            ndimage.minimum(img, lab, idx)
            ndimage.maximum(img, lab, idx)
            k, area, total = k + n, area + int(a.sum()), total + int(s.sum())
    return k, area, total


def run_case(dev, mask, args):
    from sequitr_amd import centroids, objects
    mask_d = torch.from_numpy(mask).to(dev)
    image_d = torch.from_numpy(np.random.default_rng(1).integers(100, 4000, mask.shape).astype(np.uint16)).to(dev)
    box = {}
    variants = {
        'measure': lambda: box.__setitem__('t', objects.measure_objects(mask_d)),
        'measure_image': lambda: box.__setitem__('ti', objects.measure_objects(mask_d, image=image_d)),
        'measure_labels': lambda: box.__setitem__('tl', objects.measure_objects(mask_d, image=image_d, labels=True)),
        'centroids': lambda: box.__setitem__('c', centroids.mask_centroids(mask_d)),
    }
    for f in variants.values():                                 # also grows the tables to what the case needs
        f()
    found = box['ti'].found
    first_max_out = objects._MAX_OUT
    max_out = max(first_max_out, found)
    objects._MAX_OUT = max_out                                  # time the steady state: one attempt per call
    try:
        return _run_case_timed(mask_d, image_d, variants, box, max_out, args)
    finally:
        objects._MAX_OUT = first_max_out


def _run_case_timed(mask_d, image_d, variants, box, max_out, args):
    from sequitr_amd import _lib
    t_host, host = [], None
    for _ in range(args.host_iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = host_path(mask_d, image_d)
        t_host.append((time.perf_counter() - t0) * 1e3)
    ti = box['ti']
    agree = (host is None or host == (len(ti), int(ti.area.sum()), int(ti.intensity_sum.sum()))) and \
        sum(len(c) for c in box['c']) == len(box['t']) and \
        all(np.array_equal(a, b) for a, b in zip(box['t'].coords(), box['c']))
    for _ in range(args.warmup):
        for f in variants.values():
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(args.iters):                                 # interleaved rounds: drift hits all variants alike
        for k, f in variants.items():
            t[k].append(_time(f))
    med = {k: float(np.median(v)) for k, v in t.items()}
    res = {'%s_ms' % k: round(v, 3) for k, v in med.items()}
    res['ms_min_max'] = {k: [round(min(v), 3), round(max(v), 3)] for k, v in t.items()}
    res['host_ms'] = round(float(np.median(t_host)), 1) if t_host else NM
    res['host_over_measure_image'] = round(float(np.median(t_host)) / med['measure_image'], 1) if t_host else NM
    res['measure_over_centroids'] = round(med['measure'] / med['centroids'], 3)
    res['objects'] = len(ti)
    res['workspace_bytes'] = int(_lib.load().sq_objects_workspace(N, 1, H, W, max_out))
    res['agree'] = bool(agree)
    return res


def run_stream(dev, args):
    from sequitr_amd import centroids, objects
    from sequitr_amd.frontend import segment_frames
    from sequitr_amd.networks.unet import UNet2D
    frames = np.random.default_rng(0).integers(100, 4000, (N, H, W)).astype(np.uint16)
    net = UNet2D({'shape': (512, 512), 'num_outputs': C, 'device': dev}, 'infer').initialize()

    def stream(**sink):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        segment_frames(net, frames, tile=512, margin=32, frames_per_batch=4, **sink)   # ends in a synchronise
        return (time.perf_counter() - t0) * 1e3 / N

    sinks = {'centroids': {'on_masks': lambda first, m: centroids.mask_centroids(m)},
             'measure': {'on_batch': lambda first, raw, m: objects.measure_objects(m, image=raw)}}
    for sink in sinks.values():
        stream(**sink)
    t = {k: [] for k in sinks}
    for _ in range(args.stream_iters):
        for k, sink in sinks.items():
            t[k].append(stream(**sink))
    cen, mea = float(np.median(t['centroids'])), float(np.median(t['measure']))
    return {'what': 'segment_frames over %d uint16 frames of %d x %d, tile 512, margin 32, 4 frames per batch: a sink that '
                    'measures every object against the raw frames, against the centroid sink, host clock per frame' % (N, H, W),
            'centroids_ms_per_frame': round(cen, 3), 'measure_ms_per_frame': round(mea, 3),
            'ms_min_max': {k: [round(min(v), 3), round(max(v), 3)] for k, v in t.items()},
            'measure_share': round((mea - cen) / cen, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--host-iters', type=int, default=1)
    ap.add_argument('--stream-iters', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'objects_bench.json'))
    ap.add_argument('--placeholder', action='store_true', help='write "not measured" in every field (no GPU needed)')
    args = ap.parse_args()
    if args.placeholder:
        line = placeholder()
    else:
        if not torch.cuda.is_available():
            raise SystemExit('objects_bench needs the GPU')
        torch.cuda.set_device(0)
        dev = 'cuda:0'
        line = {'workload': WORKLOAD, 'device': torch.cuda.get_device_name(0), 'warmup': args.warmup, 'iters': args.iters,
                'cases': {}}
        for name, make in (('disks', disk_masks), ('checkerboard', checkerboard)):
            line['cases'][name] = run_case(dev, make(), args)
            print('objects_bench: %s done' % name, file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
        line['stream'] = run_stream(dev, args)
    text = json.dumps(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
