"""Neighbourhood benchmark: one JSON line, also written to profiles/neighbors_bench.json.

Workload: 8 int32 label frames of 2048 x 2048 resident in HBM -- the label images measure_objects makes of
tools/objects_bench.py's disk masks (~2000 objects per frame) -- and, as the worst case for the row pass and the table,
the same frames with EVERY pixel a seed (labels cycling through 1 .. 2^21 - 1, the largest max_label).
Method (the repository's measuring habits): buffers allocated once, warm-up, then 20 windows per variant, the variants
alternated round by round, HIP events round each window; the median is reported with minimum and maximum beside it.
  * zones            : sq_label_zones_i32, unbounded, zones only
  * zones_d2         : ... with d2
  * zones_r32        : ... at max_distance 32, zones only (the column search stops at 32 rows)
  * graph            : sq_zone_graph on the unbounded zones, room for 8 pairs per object
  * edt              : sq_edt_sq_f32 on the same frames (the objects as features) in the same run: the unlabelled yardstick
  * neighbors        : the whole analysis.neighbors.neighbors() call, host part included (disks only)
  * host             : the path this replaces -- download the labels, scipy distance_transform_edt(return_indices=True)
                       per frame, numpy adjacency on shifted views; host clock, `--host-iters` times (disks only)
`gbs` is the bytes a call must move (zones: 4 B in + 6 B written and re-read + 4 B out, + 4 B with d2; graph: 4 B in;
edt: 4 + 2 + 2 + 4) over the median, against the 6.3 TB/s the card's HBM is rated at.  No torch composition gives Euclidean
zones, so there is no such baseline.  `stream` is the share of a neighbours sink in frontend.segment_frames' stream over
8 uint16 frames of 2048 x 2048 against the measure-only sink.
Without a GPU the tool refuses to run; --placeholder writes the file with "not measured" in every field.
Usage: python tools/neighbors_bench.py [--warmup 3] [--iters 20] [--host-iters 1] [--stream-iters 3] [--no-stream] [--out PATH]
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

from tools.objects_bench import C, H, N, W, _time, disk_masks  # noqa: E402

NM = 'not measured'
HBM_GBS = 6300.0
WORKLOAD = ('neighbourhoods: %d x %d x %d int32 label frames, ~2000 disk objects per frame, and every pixel a seed' % (N, H, W))
VARIANTS = ('zones', 'zones_d2', 'zones_r32', 'graph', 'edt')
BYTES = {'zones': 14, 'zones_d2': 18, 'zones_r32': 14, 'graph': 4, 'edt': 12}   # per pixel, what a call must move
CASE_FIELDS = tuple('%s_ms' % v for v in VARIANTS) + ('ms_min_max', 'gbs', 'share_of_hbm', 'zones_over_edt', 'pairs', 'objects',
                                                      'neighbors_ms', 'host_ms', 'host_over_neighbors', 'agree')
STREAM_FIELDS = ('what', 'measure_ms_per_frame', 'neighbors_ms_per_frame', 'ms_min_max', 'neighbors_share')


def placeholder():
    return {'workload': WORKLOAD, 'device': NM, 'torch_composition': 'none exists for Euclidean zones',
            'cases': {k: {f: NM for f in CASE_FIELDS} for k in ('disks', 'every_pixel')},
            'stream': {f: NM for f in STREAM_FIELDS}}


def host_path(labels_d):
    """download + scipy feature transform + numpy adjacency; returns (zones, number of pairs)"""
    from scipy import ndimage
    labels = labels_d.cpu().numpy()
    zones = np.empty_like(labels)
    pairs = 0
    for f in range(labels.shape[0]):
        ind = ndimage.distance_transform_edt(labels[f] == 0, return_distances=False, return_indices=True)
        z = zones[f] = labels[f][ind[0], ind[1]]
        keys = []
        for A, B in ((z[:, :-1], z[:, 1:]), (z[:-1], z[1:])):
            m = A != B
            keys.append(np.minimum(A[m], B[m]).astype(np.int64) << 32 | np.maximum(A[m], B[m]))
        pairs += len(np.unique(np.concatenate(keys)))
    return zones, pairs


def run_case(dev, labels_d, max_label, table, args):
    from sequitr_amd import _lib, ops
    from sequitr_amd.analysis import neighbors as nb
    lib = _lib.load()
    px = N * H * W
    st = torch.cuda.current_stream().cuda_stream
    zones, d2 = torch.empty_like(labels_d), torch.empty_like(labels_d)
    ws = torch.empty(int(lib.sq_label_zones_workspace(N, H, W)) // 4, dtype=torch.int32, device=dev)
    feat = (labels_d > 0).to(torch.float32)
    nb.label_zones(labels_d, max_label=max_label, out=zones, workspace=ws)
    max_pairs = 8 * len(table) if table is not None else 1 << 26   # every pixel a seed: about two pairs per pixel
    stats = torch.empty((N, max_label + 1, 2), dtype=torch.int64, device=dev)
    pairs = torch.empty((max_pairs, 4), dtype=torch.int32, device=dev)
    ctr = torch.empty(2, dtype=torch.int32, device=dev)
    gws = torch.empty(int(lib.sq_zone_graph_workspace(max_pairs)) // 4, dtype=torch.int32, device=dev)
    box = {}
    variants = {
        'zones': lambda: nb.label_zones(labels_d, max_label=max_label, out=zones, workspace=ws),
        'zones_d2': lambda: nb.label_zones(labels_d, max_label=max_label, out=zones, distance_out=d2, workspace=ws),
        'zones_r32': lambda: nb.label_zones(labels_d, 32, max_label=max_label, out=d2, workspace=ws),
        'graph': lambda: _lib.check(lib.sq_zone_graph(zones.data_ptr(), N, H, W, max_label, stats.data_ptr(), pairs.data_ptr(),
                                                      max_pairs, ctr.data_ptr(), ctr[1:].data_ptr(), gws.data_ptr(), st), 'graph'),
        'edt': lambda: box.__setitem__('edt', ops.edt_squared(feat)),
    }
    if table is not None:
        variants['neighbors'] = lambda: box.__setitem__('nt', nb.neighbors(labels_d, table.cls, table.centroid, table.frame,
                                                                           C + 1))
    for _ in range(args.warmup):
        for f in variants.values():
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(args.iters):                                 # interleaved rounds: drift hits all variants alike
        for k, f in variants.items():
            t[k].append(_time(f))
    med = {k: float(np.median(v)) for k, v in t.items()}
    res = {'%s_ms' % k: round(med[k], 3) for k in VARIANTS}
    res['ms_min_max'] = {k: [round(min(v), 3), round(max(v), 3)] for k, v in t.items()}
    res['gbs'] = {k: round(BYTES[k] * px / med[k] / 1e6, 1) for k in VARIANTS}
    res['share_of_hbm'] = {k: round(BYTES[k] * px / med[k] / 1e6 / HBM_GBS, 4) for k in VARIANTS}
    res['zones_over_edt'] = round(med['zones_d2'] / med['edt'], 3)
    variants['zones_d2']()
    variants['graph']()
    torch.cuda.synchronize()
    count, dropped = (int(v) for v in ctr.cpu().numpy())
    res['pairs'], res['objects'] = count, NM if table is None else len(table)
    agree = bool(torch.equal(d2, box['edt'])) and dropped == 0  # the same exact distances as the unlabelled transform
    if table is not None:
        t_host, host = [], None
        for _ in range(args.host_iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = host_path(labels_d)
            t_host.append((time.perf_counter() - t0) * 1e3)
        res['neighbors_ms'] = round(med['neighbors'], 3)
        res['host_ms'] = round(float(np.median(t_host)), 1) if t_host else NM
        res['host_over_neighbors'] = round(float(np.median(t_host)) / med['neighbors'], 1) if t_host else NM
        if host is not None:                                    # scipy breaks ties its own way: distances must agree, pairs nearly
            res['host_pairs'] = host[1]
            res['zones_equal_host_share'] = round(float((host[0] == zones.cpu().numpy()).mean()), 6)
    else:
        res['neighbors_ms'] = res['host_ms'] = res['host_over_neighbors'] = NM
    res['agree'] = agree
    return res


def run_stream(dev, args):
    from sequitr_amd import objects
    from sequitr_amd.analysis import neighbors as nb
    from sequitr_amd.frontend import segment_frames
    from sequitr_amd.networks.unet import UNet2D
    frames = np.random.default_rng(0).integers(100, 4000, (N, H, W)).astype(np.uint16)
    net = UNet2D({'shape': (512, 512), 'num_outputs': C, 'device': dev}, 'infer').initialize()

    def stream(**sink):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        segment_frames(net, frames, tile=512, margin=32, frames_per_batch=4, **sink)   # ends in a synchronise
        return (time.perf_counter() - t0) * 1e3 / N

    def both(first, raw, m):
        nb.neighbors_from_objects(objects.measure_objects(m, image=raw, labels=True), C)

    sinks = {'measure': {'on_batch': lambda first, raw, m: objects.measure_objects(m, image=raw, labels=True)},
             'neighbors': {'on_batch': both}}
    for sink in sinks.values():
        stream(**sink)
    t = {k: [] for k in sinks}
    for _ in range(args.stream_iters):
        for k, sink in sinks.items():
            t[k].append(stream(**sink))
    mea, nei = float(np.median(t['measure'])), float(np.median(t['neighbors']))
    return {'what': 'segment_frames over %d uint16 frames of %d x %d, tile 512, margin 32, 4 frames per batch, a seeded net: a '
                    'sink that measures and finds neighbours against the sink that measures (labels made), host clock per '
                    'frame' % (N, H, W),
            'measure_ms_per_frame': round(mea, 3), 'neighbors_ms_per_frame': round(nei, 3),
            'ms_min_max': {k: [round(min(v), 3), round(max(v), 3)] for k, v in t.items()},
            'neighbors_share': round((nei - mea) / mea, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--host-iters', type=int, default=1)
    ap.add_argument('--stream-iters', type=int, default=3)
    ap.add_argument('--no-stream', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'neighbors_bench.json'))
    ap.add_argument('--placeholder', action='store_true', help='write "not measured" in every field (no GPU needed)')
    args = ap.parse_args()
    if args.placeholder:
        line = placeholder()
    else:
        if not torch.cuda.is_available():
            raise SystemExit('neighbors_bench needs the GPU')
        from sequitr_amd.objects import measure_objects
        torch.cuda.set_device(0)
        dev = 'cuda:0'
        line = dict(placeholder(), device=torch.cuda.get_device_name(0), warmup=args.warmup, iters=args.iters)
        table = measure_objects(torch.from_numpy(disk_masks()).to(dev), labels=True)
        max_label = int(table.label.max())
        line['cases']['disks'] = run_case(dev, table.labels, max_label, table, args)
        print('neighbors_bench: disks done', file=sys.stderr, flush=True)
        table.labels = None
        torch.cuda.empty_cache()
        own = (torch.arange(N * H * W, dtype=torch.int64, device=dev) % ((1 << 21) - 1) + 1).to(torch.int32).view(N, H, W)
        line['cases']['every_pixel'] = run_case(dev, own, (1 << 21) - 1, None, args)
        print('neighbors_bench: every_pixel done', file=sys.stderr, flush=True)
        del own
        torch.cuda.empty_cache()
        if not args.no_stream:
            write(line, args.out)                               # the cases are kept whatever becomes of the stream
            line['stream'] = run_stream(dev, args)
    print(write(line, args.out))


def write(line, path):
    text = json.dumps(line)
    if path:
        with open(path, 'w') as f:
            f.write(text + '\n')
    return text


if __name__ == '__main__':
    main()
