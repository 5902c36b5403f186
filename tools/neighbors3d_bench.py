"""Volumetric neighbourhood benchmark: one JSON line, also written to profiles/neighbors3d_bench.json.

Workload: one resident (1, 64, 1024, 1024) int32 label volume generated here from a seed -- about 2000 random balls, ball k
holding label k + 1 -- at the depth spacings dz = 1 and dz = 3.
  * zones      : ms per sq_label_zones3d_i32 call (HIP events, median of --iters with minimum and maximum) in four
                 configurations: `unbounded`, `with_d2`, `reach32` (max_distance 32, no d2) and `global` (unbounded with
                 SQ_ZONES3D_LDS=0: the depth pass on global memory).  In the same run, alternated round by round:
                 `edt3d` -- ops.edt3d_squared on the seed indicator, the unlabelled yardstick -- and `planar` -- label_zones
                 on the (N D, H, W) view, the same voxels without the third axis (a different result).  `host_ms`: download +
                 scipy.ndimage.distance_transform_edt(sampling=(dz, 1, 1), return_indices=True) + a numpy adjacency, once per dz
                 (--host-iters 0 leaves it "not measured").
  * graph      : ms per zone_graph3d call on the unbounded zones (sq_zone_graph3d plus the download of its rows), and the
                 number of pairs.
  * neighbors3d: the whole call (zones, graph, downloads, the host table) by the host clock.
  * stream     : frontend.segment_volumes over the 64 x 1024 x 1024 uint16 volume of tools/volume_frontend_bench.py (bricks
                 32 x 128 x 128, margin 0) with a sink that runs neighbors3d on the resident ball labels per volume and with a
                 sink that does nothing, alternated, by the host clock: the share of the neighbours in the stream.  The
                 random network's mask is noise, so the sink's input is the ball volume, not the mask.
`agree` says that the configurations gave the same zones where they compute the same thing, that d2 is edt3d_squared bit
for bit and, when the host path ran, that d2 equals the squared distance to the voxel scipy's indices name.
Without a GPU the tool refuses to run; --placeholder writes the file with "not measured" in every field.  Reads nothing
outside the repository.
Usage: python tools/neighbors3d_bench.py [--warmup 1] [--iters 5] [--host-iters 1] [--stream-iters 2] [--out PATH] [--placeholder]
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
SPACINGS = (1.0, 3.0)
REACH = 32
WORKLOAD = 'volumetric neighbourhoods: one %d x %d x %d x %d int32 label volume, ~2000 balls, dz = 1 and dz = 3' % SHAPE
CONFIGS = ('unbounded', 'with_d2', 'reach32', 'global')
BASELINES = ('edt3d', 'planar')
STREAM_FIELDS = ('what', 'plain_ms_per_volume', 'neighbors_ms_per_volume', 'ms_min_max', 'neighbors_share')


def placeholder():
    per_dz = {c: {'ms': NM, 'ms_min_max': NM} for c in CONFIGS + BASELINES}
    per_dz.update(host_ms=NM, host_over_unbounded=NM, graph_ms=NM, graph_ms_min_max=NM, pairs=NM, neighbors3d_ms=NM,
                  neighbors3d_ms_min_max=NM)
    return {'workload': WORKLOAD, 'device': NM, 'labels': NM, 'zones_workspace_bytes': NM, 'graph_workspace_bytes': NM,
            'spacings': {'dz_%g' % dz: dict(per_dz) for dz in SPACINGS}, 'lds_form_is_faster': NM, 'agree': NM,
            'stream': {f: NM for f in STREAM_FIELDS}}


def ball_labels(seed=0, balls=2000):
    """labels (1,D,H,W) int32: ball k holds k + 1 where no later ball covers it"""
    rng = np.random.default_rng(seed)
    _, D, H, W = SHAPE
    m = np.zeros(SHAPE, np.int32)
    for k in range(balls):
        cz, cy, cx, rad = int(rng.integers(0, D)), int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(6, 14))
        z0, z1, y0, y1, x0, x1 = max(cz - rad, 0), min(cz + rad + 1, D), max(cy - rad, 0), min(cy + rad + 1, H), \
            max(cx - rad, 0), min(cx + rad + 1, W)
        zz, yy, xx = np.mgrid[z0:z1, y0:y1, x0:x1]
        box = m[0, z0:z1, y0:y1, x0:x1]
        box[(zz - cz) ** 2 + (yy - cy) ** 2 + (xx - cx) ** 2 <= rad * rad] = k + 1
    return m


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _r(x, n=4):
    return round(float(x), n)


def _stat(t):
    return {'ms': _r(np.median(t)), 'ms_min_max': [_r(min(t)), _r(max(t))]}


def host_path(labels_d, dz):
    """download + scipy's feature transform + a numpy adjacency -> (zones, squared distance to the voxel named, pairs)"""
    from scipy import ndimage
    lab = labels_d.cpu().numpy()[0]
    ind = ndimage.distance_transform_edt(lab == 0, sampling=(dz, 1, 1), return_distances=False, return_indices=True)
    zones = lab[ind[0], ind[1], ind[2]]
    zz, yy, xx = np.ogrid[0:lab.shape[0], 0:lab.shape[1], 0:lab.shape[2]]
    t = (ind[0] - zz).astype(np.float64) * dz
    d2 = t * t + ((ind[1] - yy).astype(np.float64) ** 2 + (ind[2] - xx).astype(np.float64) ** 2)
    keys = []
    for a, b in ((zones[:, :, :-1], zones[:, :, 1:]), (zones[:, :-1], zones[:, 1:]), (zones[:-1], zones[1:])):
        m = a != b
        keys.append(np.unique(np.minimum(a[m], b[m]).astype(np.int64) << 21 | np.maximum(a[m], b[m])))
    return zones[None], d2[None], len(np.unique(np.concatenate(keys)))


class env(object):
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = os.environ.get(self.name)
        os.environ[self.name] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.old


def measure(args):
    from sequitr_amd import _lib, ops
    from sequitr_amd.analysis import neighbors as nb
    from sequitr_amd.frontend import segment_volumes
    from sequitr_amd.networks.unet import UNet3D
    torch.cuda.set_device(0)
    dev = 'cuda:0'
    lib = _lib.load()
    host_labels = ball_labels(0)
    present = np.unique(host_labels)
    present = present[present > 0]
    remap = np.zeros(int(host_labels.max()) + 1, np.int32)      # the surviving balls, numbered 1 .. k without gaps
    remap[present] = np.arange(1, len(present) + 1)
    host_labels = remap[host_labels]
    k = len(present)
    labels = torch.from_numpy(host_labels).to(dev)
    N, D, H, W = SHAPE
    indicator = (labels > 0).to(torch.float32)
    planar_view = labels.view(N * D, H, W)
    ws_bytes = int(lib.sq_label_zones3d_workspace(N, D, H, W))
    ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=dev)
    zones = {c: torch.empty_like(labels) for c in CONFIGS}
    d2 = torch.empty(SHAPE, dtype=torch.float64, device=dev)
    planar_out = torch.empty_like(planar_view)

    def global_form(dz):
        with env('SQ_ZONES3D_LDS', '0'):
            nb.label_zones3d(labels, None, dz, max_label=k, out=zones['global'], workspace=ws)

    agree, out, lds_faster = True, {}, {}
    for dz in SPACINGS:
        fns = {'unbounded': lambda: nb.label_zones3d(labels, None, dz, max_label=k, out=zones['unbounded'], workspace=ws),
               'with_d2': lambda: nb.label_zones3d(labels, None, dz, max_label=k, out=zones['with_d2'], distance_out=d2,
                                                   workspace=ws),
               'reach32': lambda: nb.label_zones3d(labels, REACH, dz, max_label=k, out=zones['reach32'], workspace=ws),
               'global': lambda: global_form(dz),
               'edt3d': lambda: ops.edt3d_squared(indicator, spacing=dz),
               'planar': lambda: nb.label_zones(planar_view, max_label=k, out=planar_out)}
        for _ in range(args.warmup):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        t = {name: [] for name in fns}
        for _ in range(args.iters):                             # alternate the steps so drift hits all alike
            for name, fn in fns.items():
                t[name].append(_time(fn))
        row = {name: _stat(v) for name, v in t.items()}
        lds_faster['dz_%g' % dz] = bool(row['unbounded']['ms'] < row['global']['ms'])
        edt = ops.edt3d_squared(indicator, spacing=dz)
        same = torch.equal(zones['unbounded'], zones['global']) and torch.equal(zones['unbounded'], zones['with_d2']) \
            and torch.equal(d2.view(torch.int64), edt.view(torch.int64)) \
            and torch.equal(zones['reach32'], torch.where(d2 <= float(REACH * REACH), zones['unbounded'], 0))
        del edt
        # the graph and the whole call
        tg = [_time(lambda: nb.zone_graph3d(zones['unbounded'], k, 16 * k)) for _ in range(args.iters)]
        stats, pairs = nb.zone_graph3d(zones['unbounded'], k, 16 * k)
        cls, volume = np.ones(k, np.int64), np.zeros(k, np.int64)
        centroid = np.zeros((k, 3))                             # no pair is removed at d_thresh = inf: the centres do not matter
        tn = []
        for _ in range(args.iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            table = nb.neighbors3d(labels, cls, centroid, volume, 2, np.inf, None, 'objects', dz)
            tn.append((time.perf_counter() - t0) * 1e3)
        same = same and table.n_pairs == len(pairs)
        row.update(graph_ms=_r(np.median(tg)), graph_ms_min_max=[_r(min(tg)), _r(max(tg))], pairs=int(len(pairs)),
                   neighbors3d_ms=_r(np.median(tn), 2), neighbors3d_ms_min_max=[_r(min(tn), 2), _r(max(tn), 2)],
                   host_ms=NM, host_over_unbounded=NM)
        if args.host_iters > 0:
            th = []
            for _ in range(args.host_iters):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                hz, hd2, hpairs = host_path(labels, dz)
                th.append((time.perf_counter() - t0) * 1e3)
            same = same and np.array_equal(hd2, d2.cpu().numpy())
            row.update(host_ms=_r(np.median(th), 1), host_over_unbounded=_r(np.median(th) / row['unbounded']['ms'], 1),
                       host_pairs=int(hpairs), host_zones_differing=int((hz != zones['unbounded'].cpu().numpy()).sum()))
            del hz, hd2
        agree = agree and bool(same)
        out['dz_%g' % dz] = row
        print('dz = %g' % dz, row, file=sys.stderr, flush=True)
    graph_ws = int(lib.sq_zone_graph3d_workspace(16 * k))
    del ws, d2, planar_out, indicator
    for c in CONFIGS:
        del zones[c]
    torch.cuda.empty_cache()

    # a neighbours sink in segment_volumes' stream
    host = np.random.default_rng(0).integers(100, 4000, (2,) + SHAPE[1:]).astype(np.uint16)
    net = UNet3D({'shape': (BRICK[1], BRICK[2], BRICK[0]), 'num_outputs': 2, 'device': dev}, 'infer').initialize()
    cls, volume, centroid = np.ones(k, np.int64), np.zeros(k, np.int64), np.zeros((k, 3))

    def stream(sink):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        segment_volumes(net, host, BRICK, 0, bricks_per_batch=8, on_volume=sink)
        return (time.perf_counter() - t0) * 1e3 / host.shape[0]

    nothing = lambda i, raw, m: None                                              # noqa: E731
    sink = lambda i, raw, m: nb.neighbors3d(labels, cls, centroid, volume, 2, np.inf, None, 'objects', 1.0)   # noqa: E731
    stream(nothing), stream(sink)
    plain, full = [], []
    for _ in range(args.stream_iters):
        plain.append(stream(nothing))
        full.append(stream(sink))
    p, c = float(np.median(plain)), float(np.median(full))
    return {'workload': WORKLOAD, 'device': torch.cuda.get_device_name(0), 'labels': int(k), 'warmup': args.warmup,
            'iters': args.iters, 'zones_workspace_bytes': ws_bytes, 'graph_workspace_bytes': graph_ws, 'spacings': out,
            'lds_form_is_faster': lds_faster, 'agree': bool(agree),
            'stream': {'what': 'segment_volumes, 2 x 64 x 1024 x 1024 uint16, bricks 32 x 128 x 128, margin 0, on_volume sink: '
                               'neighbors3d on the resident ball labels at dz = 1 against a sink that does nothing',
                       'plain_ms_per_volume': _r(p, 2), 'neighbors_ms_per_volume': _r(c, 2),
                       'ms_min_max': [_r(min(plain + full), 2), _r(max(plain + full), 2)],
                       'neighbors_share': _r((c - p) / c, 4)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--host-iters', type=int, default=1)
    ap.add_argument('--stream-iters', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'neighbors3d_bench.json'))
    ap.add_argument('--placeholder', action='store_true', help='write "not measured" in every field (no GPU needed)')
    args = ap.parse_args()
    if args.placeholder:
        line = placeholder()
    elif not torch.cuda.is_available():
        raise SystemExit('neighbors3d_bench needs the GPU (--placeholder writes the file without one)')
    else:
        line = measure(args)
    text = json.dumps(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
