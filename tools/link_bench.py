"""Linking benchmark: one JSON line, also written to profiles/link_bench.json.

Workload: 9 int32 label frames of 2048 x 2048 resident in HBM -- the label image measure_objects makes of
tools/objects_bench.py's first disk mask (~2000 objects), each frame the previous one shifted by (2, 3) pixels -- so that
a = frames[:8] and b = frames[1:] are 8 steps of a movie in which every cell overlaps its successor.
Method (the repository's measuring habits): buffers allocated once, warm-up, then 20 windows per variant, the variants
alternated round by round, HIP events round each window; the median is reported with minimum and maximum beside it.
  * overlap_lane / overlap_lane_areas : sq_label_overlap in the one-lane form (SQ_LINK_VEC=0), without / with the areas
  * overlap_vec / overlap_vec_areas   : ... in the four-lane form (SQ_LINK_VEC=1)
  * zone_graph       : sq_zone_graph on the frames a, in the same run: the kernel whose form the one-lane form took over
  * torch_unique     : the torch composition -- the 64-bit keys where both labels are non-zero, torch.unique(return_counts)
  * relabel          : sq_relabel_lut_i32 over a, out of place
  * torch_lut        : the torch composition -- torch.where(a > 0, lut[offset + a - 1], 0)
  * link_r0 / link_r8: the whole analysis.linking.link_labels call over the 9 frames at reach 0 and 8, host part included
  * host             : the path this replaces -- download a and b, np.unique of the keys; host clock, `--host-iters` times
`gbs` is the bytes a call must move (overlap: 8 B per pixel read; zone_graph: 4 B read twice, the lower neighbour's row;
relabel: 4 B in + 4 B out) over the median, against the 6.3 TB/s the card's HBM is rated at.  `stream` is the share of a
linking sink in frontend.segment_frames' stream over 8 uint16 frames of 2048 x 2048 against the sink that measures.
Without a GPU the tool refuses to run; --placeholder writes the file with "not measured" in every field.
Usage: python tools/link_bench.py [--warmup 3] [--iters 20] [--host-iters 1] [--stream-iters 3] [--no-stream] [--out PATH]
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
SHIFT = (2, 3)
WORKLOAD = ('linking: %d steps between %d x %d int32 label frames of ~2000 disk objects, each frame the previous one shifted by '
            '%s pixels' % (N, H, W, SHIFT))
KERNELS = ('overlap_lane', 'overlap_lane_areas', 'overlap_vec', 'overlap_vec_areas', 'zone_graph', 'torch_unique', 'relabel',
           'torch_lut')
BYTES = {'overlap_lane': 8, 'overlap_lane_areas': 8, 'overlap_vec': 8, 'overlap_vec_areas': 8, 'zone_graph': 8, 'relabel': 8}
FIELDS = tuple('%s_ms' % v for v in KERNELS) + ('link_r0_ms', 'link_r8_ms', 'ms_min_max', 'gbs', 'share_of_hbm',
                                                'vec_over_lane', 'vec_over_lane_areas', 'torch_unique_over_overlap',
                                                'torch_lut_over_relabel', 'overlap_over_zone_graph', 'host_ms',
                                                'host_over_overlap', 'pairs', 'objects', 'tracks_r0', 'tracks_r8', 'agree')
STREAM_FIELDS = ('what', 'measure_ms_per_frame', 'link_ms_per_frame', 'ms_min_max', 'link_share')


def placeholder():
    return {'workload': WORKLOAD, 'device': NM, 'default_form': NM, 'case': {f: NM for f in FIELDS},
            'stream': {f: NM for f in STREAM_FIELDS}}


class form(object):
    """SQ_LINK_VEC for the calls inside (the variable is read per call)"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get('SQ_LINK_VEC')
        os.environ['SQ_LINK_VEC'] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop('SQ_LINK_VEC', None)
        else:
            os.environ['SQ_LINK_VEC'] = self.old


def default_form():
    """the form a call takes without SQ_LINK_VEC: SQ_LINK_VEC_DEFAULT of include/sequitr_hip.h"""
    import re
    text = open(os.path.join(ROOT, 'include', 'sequitr_hip.h')).read()
    return 'four-lane' if int(re.search(r'#define SQ_LINK_VEC_DEFAULT (\d)', text).group(1)) else 'one-lane'


def keys_of(a, b):
    n = torch.arange(a.shape[0], device=a.device, dtype=torch.int64).view(-1, 1, 1)
    both = (a > 0) & (b > 0)
    return ((n << 42) | (a.to(torch.int64) << 21) | b.to(torch.int64))[both]


def run_case(dev, stack, max_label, args):
    from sequitr_amd import _lib
    from sequitr_amd.analysis import linking
    lib = _lib.load()
    a, b = stack[:-1], stack[1:]
    px = N * H * W
    st = torch.cuda.current_stream().cuda_stream
    max_pairs = 16 * max_label
    area = torch.empty((2, N, max_label + 1), dtype=torch.int64, device=dev)
    stats = torch.empty((N, max_label + 1, 2), dtype=torch.int64, device=dev)
    pairs = torch.empty((max_pairs, 4), dtype=torch.int32, device=dev)
    ctr = torch.empty(2, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.sq_label_overlap_workspace(max_pairs)) // 4, dtype=torch.int32, device=dev)
    gws = torch.empty(int(lib.sq_zone_graph_workspace(max_pairs)) // 4, dtype=torch.int32, device=dev)
    out = torch.empty_like(a)
    offsets = torch.arange(N + 1, dtype=torch.int64, device=dev) * max_label
    lut = torch.arange(1, N * max_label + 1, dtype=torch.int32, device=dev).flip(0).contiguous()
    box = {}

    def overlap(vec, areas):
        def call():
            with form(vec):
                _lib.check(lib.sq_label_overlap(a.data_ptr(), b.data_ptr(), N, H * W, max_label,
                                                area[0].data_ptr() if areas else None, area[1].data_ptr() if areas else None,
                                                pairs.data_ptr(), max_pairs, ctr.data_ptr(), ctr[1:].data_ptr(), ws.data_ptr(),
                                                st), 'sq_label_overlap')
        return call

    def rows():
        torch.cuda.synchronize()
        count, dropped = (int(v) for v in ctr.cpu().numpy())
        r = pairs[:count].cpu().numpy().astype(np.int64)
        return r[np.lexsort((r[:, 2], r[:, 1], r[:, 0]))], dropped

    def torch_unique():
        box['u'] = torch.unique(keys_of(a, b), return_counts=True)

    def torch_lut():
        idx = (a.to(torch.int64) + offsets[:-1].view(-1, 1, 1) - 1).clamp_(min=0)
        box['l'] = torch.where(a > 0, lut[idx], torch.zeros((), dtype=torch.int32, device=dev))

    variants = {
        'overlap_lane': overlap('0', False), 'overlap_lane_areas': overlap('0', True),
        'overlap_vec': overlap('1', False), 'overlap_vec_areas': overlap('1', True),
        'zone_graph': lambda: _lib.check(lib.sq_zone_graph(a.data_ptr(), N, H, W, max_label, stats.data_ptr(), pairs.data_ptr(),
                                                           max_pairs, ctr.data_ptr(), ctr[1:].data_ptr(), gws.data_ptr(), st),
                                         'sq_zone_graph'),
        'torch_unique': torch_unique,
        'relabel': lambda: linking.relabel(a, offsets, lut, out=out),
        'torch_lut': torch_lut,
        'link_r0': lambda: box.__setitem__('r0', linking.link_labels(stack)),
        'link_r8': lambda: box.__setitem__('r8', linking.link_labels(stack, reach=8)),
    }
    for _ in range(args.warmup):
        for f in variants.values():
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(args.iters):                                 # interleaved rounds: drift hits all variants alike
        for k, f in variants.items():
            t[k].append(_time(f))
    med = {k: float(np.median(v)) for k, v in t.items()}
    res = {'%s_ms' % k: round(med[k], 3) for k in variants}
    res['ms_min_max'] = {k: [round(min(v), 3), round(max(v), 3)] for k, v in t.items()}
    res['gbs'] = {k: round(BYTES[k] * px / med[k] / 1e6, 1) for k in BYTES}
    res['share_of_hbm'] = {k: round(BYTES[k] * px / med[k] / 1e6 / HBM_GBS, 4) for k in BYTES}
    res['vec_over_lane'] = round(med['overlap_vec'] / med['overlap_lane'], 3)
    res['vec_over_lane_areas'] = round(med['overlap_vec_areas'] / med['overlap_lane_areas'], 3)
    best = min(med['overlap_lane'], med['overlap_vec'])
    res['torch_unique_over_overlap'] = round(med['torch_unique'] / best, 2)
    res['torch_lut_over_relabel'] = round(med['torch_lut'] / med['relabel'], 2)
    res['overlap_over_zone_graph'] = round(med['overlap_lane'] / med['zone_graph'], 3)
    # agreement: both forms give the torch composition's table, and the two relabellings are equal
    variants['overlap_lane_areas']()
    lane, d0 = rows()
    area_lane = area.cpu().numpy().copy()
    variants['overlap_vec_areas']()
    vec, d1 = rows()
    variants['torch_unique']()
    variants['relabel']()
    variants['torch_lut']()
    torch.cuda.synchronize()
    uk, uc = (v.cpu().numpy() for v in box['u'])
    want = np.stack([uk >> 42, (uk >> 21) & 0x1fffff, uk & 0x1fffff, uc], axis=1)
    agree = d0 == 0 and d1 == 0 and np.array_equal(lane, vec) and np.array_equal(lane, want) \
        and np.array_equal(area_lane, area.cpu().numpy()) and bool(torch.equal(out, box['l']))
    t_host = []
    for _ in range(args.host_iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ha, hb = a.cpu().numpy(), b.cpu().numpy()
        both = (ha > 0) & (hb > 0)
        n = np.broadcast_to(np.arange(N, dtype=np.int64).reshape(-1, 1, 1), ha.shape)
        hk, hc = np.unique((n[both] << 42) | (ha[both].astype(np.int64) << 21) | hb[both], return_counts=True)
        t_host.append((time.perf_counter() - t0) * 1e3)
        agree = agree and np.array_equal(hk, uk) and np.array_equal(hc, uc)
    res['host_ms'] = round(float(np.median(t_host)), 1) if t_host else NM
    res['host_over_overlap'] = round(float(np.median(t_host)) / best, 1) if t_host else NM
    res['pairs'], res['objects'] = len(lane), max_label
    res['tracks_r0'], res['tracks_r8'] = len(box['r0']), len(box['r8'])
    res['agree'] = bool(agree)
    return res


def run_stream(dev, args):
    from sequitr_amd import objects
    from sequitr_amd.analysis import linking
    from sequitr_amd.frontend import segment_frames
    from sequitr_amd.networks.unet import UNet2D
    frames = np.random.default_rng(0).integers(100, 4000, (N, H, W)).astype(np.uint16)
    net = UNet2D({'shape': (512, 512), 'num_outputs': C, 'device': dev}, 'infer').initialize()

    def stream(**sink):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        segment_frames(net, frames, tile=512, margin=32, frames_per_batch=4, **sink)   # ends in a synchronise
        return (time.perf_counter() - t0) * 1e3 / N

    def link_sink():
        linker = linking.FrameLinker()

        def both(first, raw, m):
            t = objects.measure_objects(m, image=raw, labels=True)
            linker.push(first, t.labels, t)
        return both

    sinks = {'measure': lambda: {'on_batch': lambda first, raw, m: objects.measure_objects(m, image=raw, labels=True)},
             'link': lambda: {'on_batch': link_sink()}}
    for sink in sinks.values():
        stream(**sink())
    t = {k: [] for k in sinks}
    for _ in range(args.stream_iters):
        for k, sink in sinks.items():
            t[k].append(stream(**sink()))
    mea, lnk = float(np.median(t['measure'])), float(np.median(t['link']))
    return {'what': 'segment_frames over %d uint16 frames of %d x %d, tile 512, margin 32, 4 frames per batch, a seeded net: a '
                    'sink that measures and links against the sink that measures (labels made), host clock per frame'
                    % (N, H, W),
            'measure_ms_per_frame': round(mea, 3), 'link_ms_per_frame': round(lnk, 3),
            'ms_min_max': {k: [round(min(v), 3), round(max(v), 3)] for k, v in t.items()},
            'link_share': round((lnk - mea) / mea, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--host-iters', type=int, default=1)
    ap.add_argument('--stream-iters', type=int, default=3)
    ap.add_argument('--no-stream', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'link_bench.json'))
    ap.add_argument('--placeholder', action='store_true', help='write "not measured" in every field (no GPU needed)')
    args = ap.parse_args()
    if args.placeholder:
        line = placeholder()
    else:
        if not torch.cuda.is_available():
            raise SystemExit('link_bench needs the GPU')
        from sequitr_amd import _lib
        from sequitr_amd.objects import measure_objects
        torch.cuda.set_device(0)
        dev = 'cuda:0'
        line = dict(placeholder(), device=torch.cuda.get_device_name(0), default_form=default_form(), warmup=args.warmup,
                    iters=args.iters)
        _lib.load()
        os.environ.pop('SQ_LINK_VEC', None)
        table = measure_objects(torch.from_numpy(disk_masks()[:1]).to(dev), labels=True)
        max_label = int(table.label.max())
        stack = torch.stack([torch.roll(table.labels[0], (SHIFT[0] * k, SHIFT[1] * k), (0, 1))
                             for k in range(N + 1)]).contiguous()
        table.labels = None
        line['case'] = run_case(dev, stack, max_label, args)
        print('link_bench: kernels done', file=sys.stderr, flush=True)
        del stack
        torch.cuda.empty_cache()
        if not args.no_stream:
            write(line, args.out)                               # the case is kept whatever becomes of the stream
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
