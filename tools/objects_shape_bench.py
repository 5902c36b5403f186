"""Shape-column benchmark: one JSON line, also written to profiles/objects_shape_bench.json.

Workloads, resident in HBM and generated once:
  * disks        : 8 uint8 masks of 2048 x 2048 at C = 2, ~2000 random disks per frame (objects_bench's masks);
  * checkerboard : the same size, every other pixel its own object -- the worst case for the atomics and for the
                   perimeter kernel's root look-ups (every diagonal neighbour is a same-class stranger);
  * balls        : one 64 x 1024 x 1024 volume at C = 2 with ~2000 random balls.
HIP events round each call after warm-up, the variants alternated round by round; a measure_objects call includes its host
part (counter read-back, the rows' download and sort), which is what a user waits for:
  * measure        : objects.measure_objects(mask)
  * measure_shape  : objects.measure_objects(mask, shape=True)
  * shape_call     : sq_objects_shape alone, on the workspace a measure call left behind (device time of its four kernels)
  * kernels        : per kernel of sq_objects_shape, from torch.profiler's device times ("not measured" when the profiler
                     reports no kernel of that name)
  * host           : the path this replaces -- download the mask and run the scipy restatement of the tests
                     (tests/objects_shape_cases.shape_ref: label, crops, shifted views, erosion, convolve + bincount per
                     object); host clock, `--host-iters` times; not run for the checkerboard (16.8 M objects)
`read_gbs` = the bytes a shape call must read -- the mask once (1 B per voxel), parent and slot once per run segment are
left out -- over shape_call's time, and its share of 6.3 TB/s.  `stream` is the share of a shape-measuring sink in
frontend.segment_frames' stream over 8 uint16 frames of 2048 x 2048 (tile 512, margin 32): on_batch ->
measure_objects(shape=True) against the raw frames, over the same sink without shape, alternated.
Without a GPU the tool refuses to run; --placeholder writes the file with "not measured" in every field.
Usage: python tools/objects_shape_bench.py [--warmup 2] [--iters 5] [--host-iters 1] [--stream-iters 3] [--out PATH] [--placeholder]
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

from objects_bench import C, H, N, W, _time, checkerboard, disk_masks  # noqa: E402

NM = 'not measured'
VD, VH, VW = 64, 1024, 1024
HBM_GBS = 6300.0
WORKLOAD = ('shape columns: %d x %d x %d uint8 masks at C = %d, ~2000 random disks per frame and the checkerboard worst '
            'case; one %d x %d x %d volume of ~2000 balls' % (N, H, W, C, VD, VH, VW))
KERNELS = ('shape_clear_kernel', 'shape_runs_kernel', 'shape_perimeter_kernel', 'shape_emit_kernel')
CASE_FIELDS = ('measure_ms', 'measure_shape_ms', 'shape_call_ms', 'ms_min_max', 'shape_over_measure', 'kernels_ms', 'host_ms',
               'host_over_measure_shape', 'read_gbs', 'read_share_of_hbm', 'objects', 'shape_workspace_bytes', 'agree')
STREAM_FIELDS = ('what', 'measure_ms_per_frame', 'measure_shape_ms_per_frame', 'ms_min_max', 'shape_share')


def placeholder():
    return {'workload': WORKLOAD, 'device': NM,
            'cases': {k: {f: NM for f in CASE_FIELDS} for k in ('disks', 'checkerboard', 'balls')},
            'stream': {f: NM for f in STREAM_FIELDS}}


def ball_volume(seed=0, count=2000):
    """one (1, VD, VH, VW) volume with ~count balls of radius 3 .. 10, classes 1 and 2"""
    rng = np.random.default_rng(seed)
    m = np.zeros((1, VD, VH, VW), np.uint8)
    for _ in range(count):
        cz, cy, cx, r = int(rng.integers(0, VD)), int(rng.integers(0, VH)), int(rng.integers(0, VW)), int(rng.integers(3, 11))
        z0, z1, y0, y1, x0, x1 = max(cz - r, 0), min(cz + r + 1, VD), max(cy - r, 0), min(cy + r + 1, VH), max(cx - r, 0), min(cx + r + 1, VW)
        zz, yy, xx = np.mgrid[z0:z1, y0:y1, x0:x1]
        m[0, z0:z1, y0:y1, x0:x1][(zz - cz) ** 2 + (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = rng.integers(1, C + 1)
    return m


class ShapeCall(object):
    """sq_objects_shape alone, on the workspace one sq_objects_measure call left behind"""

    def __init__(self, mask_d, max_out):
        from sequitr_amd import _lib
        self.lib, self.mask = _lib.load(), mask_d
        self.dims = tuple(int(s) for s in (mask_d.shape if mask_d.dim() == 4 else (mask_d.shape[0], 1) + tuple(mask_d.shape[1:])))
        dev, self.max_out = mask_d.device, max_out
        self.ws = torch.empty(self.lib.sq_objects_workspace(*self.dims, max_out) // 4 + 4, dtype=torch.int32, device=dev)
        self.ctr = torch.zeros(2, dtype=torch.int32, device=dev)
        self.rows_i = torch.empty((max_out, 12), dtype=torch.int64, device=dev)
        self.rows_f = torch.empty((max_out, 7), dtype=torch.float64, device=dev)
        self.slots = torch.empty(max_out, dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        _lib.check(self.lib.sq_objects_measure(mask_d.data_ptr(), *self.dims, None, 0, 1, 0, self.ws.data_ptr(),
                                               self.ctr.data_ptr(), self.ctr[1:].data_ptr(), self.rows_i.data_ptr(),
                                               self.rows_f.data_ptr(), self.slots.data_ptr(), max_out, st), 'sq_objects_measure')
        self.n = int(self.ctr[0])
        self.sbytes = int(self.lib.sq_objects_shape_workspace(max_out))
        self.sws = torch.empty(self.sbytes // 4 + 4, dtype=torch.int32, device=dev)
        self.out = torch.empty((max(self.n, 1), 16), dtype=torch.int64, device=dev)

    def __call__(self):
        from sequitr_amd import _lib
        _lib.check(self.lib.sq_objects_shape(self.mask.data_ptr(), *self.dims, self.ws.data_ptr(), self.max_out,
                                             self.slots.data_ptr(), self.n, self.sws.data_ptr(), self.out.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream), 'sq_objects_shape')


def kernel_times(call, iters):
    """mean device ms per kernel of sq_objects_shape over `iters` calls, from torch.profiler; NM where it reports none"""
    out = {k: NM for k in KERNELS}
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(iters):
                call()
            torch.cuda.synchronize()
        for e in prof.key_averages():
            for k in KERNELS:
                if k in e.key and e.count:
                    total = getattr(e, 'device_time_total', None) or getattr(e, 'cuda_time_total', 0.0)
                    out[k] = round(float(total) / e.count / 1e3, 4)
    except Exception as err:                                    # the profiler is optional: the call's own time stands
        out['error'] = repr(err)[:200]
    return out


def run_case(dev, mask, args, host=True):
    from sequitr_amd import objects
    from tests import objects_shape_cases as sc
    mask_d = torch.from_numpy(mask).to(dev)
    box = {}
    box['t'] = objects.measure_objects(mask_d)                  # also says how many slots the case needs
    first_max_out = objects._MAX_OUT
    max_out = max(first_max_out, box['t'].found)
    objects._MAX_OUT = max_out                                  # time the steady state: one attempt per call
    try:
        call = ShapeCall(mask_d, max_out)
        variants = {'measure': lambda: box.__setitem__('t', objects.measure_objects(mask_d)),
                    'measure_shape': lambda: box.__setitem__('ts', objects.measure_objects(mask_d, shape=True)),
                    'shape_call': call}
        for _ in range(max(args.warmup, 1)):
            for f in variants.values():
                f()
        torch.cuda.synchronize()
        t = {k: [] for k in variants}
        for _ in range(args.iters):                             # interleaved rounds: drift hits all variants alike
            for k, f in variants.items():
                t[k].append(_time(f))
        kernels = kernel_times(call, args.iters)
    finally:
        objects._MAX_OUT = first_max_out
    ts = box['ts']
    t_host, agree = [], len(ts) == len(box['t']) and np.array_equal(ts.area, box['t'].area)
    ri = call.rows_i[:call.n].cpu().numpy()
    raw = call.out[:call.n].cpu().numpy()[np.lexsort((ri[:, 2], ri[:, 1], ri[:, 0]))]
    agree = bool(agree and np.array_equal(raw, ts._shape_rows()))
    if host:
        for _ in range(args.host_iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ref = sc.shape_ref(mask_d.cpu().numpy())
            t_host.append((time.perf_counter() - t0) * 1e3)
            agree = bool(agree and np.array_equal(ref['shape'], ts._shape_rows()))
    med = {k: float(np.median(v)) for k, v in t.items()}
    res = {'%s_ms' % k: round(v, 3) for k, v in med.items()}
    res['ms_min_max'] = {k: [round(min(v), 3), round(max(v), 3)] for k, v in t.items()}
    res['shape_over_measure'] = round(med['measure_shape'] / med['measure'], 3)
    res['kernels_ms'] = kernels
    res['host_ms'] = round(float(np.median(t_host)), 1) if t_host else NM
    res['host_over_measure_shape'] = round(float(np.median(t_host)) / med['measure_shape'], 1) if t_host else NM
    gbs = mask.size / (med['shape_call'] * 1e-3) / 1e9
    res['read_gbs'], res['read_share_of_hbm'] = round(gbs, 1), round(gbs / HBM_GBS, 4)
    res['objects'], res['shape_workspace_bytes'], res['agree'] = len(ts), call.sbytes, agree
    return res


def run_stream(dev, args):
    from sequitr_amd import objects
    from sequitr_amd.frontend import segment_frames
    from sequitr_amd.networks.unet import UNet2D
    frames = np.random.default_rng(0).integers(100, 4000, (N, H, W)).astype(np.uint16)
    net = UNet2D({'shape': (512, 512), 'num_outputs': C, 'device': dev}, 'infer').initialize()

    def stream(**sink):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        segment_frames(net, frames, tile=512, margin=32, frames_per_batch=4, **sink)   # ends in a synchronise
        return (time.perf_counter() - t0) * 1e3 / N

    sinks = {'measure': {'on_batch': lambda first, raw, m: objects.measure_objects(m, image=raw)},
             'measure_shape': {'on_batch': lambda first, raw, m: objects.measure_objects(m, image=raw, shape=True)}}
    for sink in sinks.values():
        stream(**sink)
    t = {k: [] for k in sinks}
    for _ in range(args.stream_iters):
        for k, sink in sinks.items():
            t[k].append(stream(**sink))
    mea, sha = float(np.median(t['measure'])), float(np.median(t['measure_shape']))
    return {'what': 'segment_frames over %d uint16 frames of %d x %d, tile 512, margin 32, 4 frames per batch: a sink that '
                    'measures every object with its shape columns, against the same sink without them, host clock per frame'
                    % (N, H, W),
            'measure_ms_per_frame': round(mea, 3), 'measure_shape_ms_per_frame': round(sha, 3),
            'ms_min_max': {k: [round(min(v), 3), round(max(v), 3)] for k, v in t.items()},
            'shape_share': round((sha - mea) / mea, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--host-iters', type=int, default=1)
    ap.add_argument('--stream-iters', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'objects_shape_bench.json'))
    ap.add_argument('--placeholder', action='store_true', help='write "not measured" in every field (no GPU needed)')
    args = ap.parse_args()
    if args.placeholder:
        line = placeholder()
    else:
        if not torch.cuda.is_available():
            raise SystemExit('objects_shape_bench needs the GPU')
        torch.cuda.set_device(0)
        dev = 'cuda:0'
        line = {'workload': WORKLOAD, 'device': torch.cuda.get_device_name(0), 'warmup': args.warmup, 'iters': args.iters,
                'cases': {}}
        for name, make, host in (('disks', disk_masks, True), ('checkerboard', checkerboard, False), ('balls', ball_volume, True)):
            line['cases'][name] = run_case(dev, make(), args, host=host)
            print('objects_shape_bench: %s done' % name, file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
        line['stream'] = run_stream(dev, args)
    text = json.dumps(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
