"""Per-kernel summary of ONE UNet3D volume from a rocprofv3 --kernel-trace CSV of a run that predicts twice (a warm-up
volume, then the measured one; e.g. `rocprofv3 --kernel-trace -f csv -d OUT -o unet3d -- python tools/unet3d_trace_summary.py
--run`).  The measured volume starts at the second launch of the first-layer conv (UNet3D.predict launches nothing
before it) and runs to the end of the trace.
  python tools/unet3d_trace_summary.py TRACE.csv > summary.csv"""
import csv
import os
import sys
from collections import OrderedDict


def run():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from sequitr_amd.networks.unet import UNet3D
    net = UNet3D({'shape': (256, 256, 64), 'num_outputs': 2, 'device': 'cuda:0'}).initialize()
    x = torch.randn((1, 64, 256, 256, 1), device='cuda:0')
    for _ in range(2):                                      # warm-up volume, measured volume
        net.predict(x)
        torch.cuda.synchronize()
    print("two volumes done")


def summarize(path, out=sys.stdout):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r['Start_Timestamp']))
    starts = [i for i, r in enumerate(rows) if 'conv3d_direct_f32_kernel' in r['Kernel_Name']]
    if len(starts) < 2:
        raise SystemExit('%s: expected two volumes (two first-layer launches), found %d' % (path, len(starts)))
    vol = rows[starts[1]:]
    stats = OrderedDict()
    for r in vol:
        ns = int(r['End_Timestamp']) - int(r['Start_Timestamp'])
        s = stats.setdefault(r['Kernel_Name'], [0, 0, None, 0])
        s[0] += 1
        s[1] += ns
        s[2] = ns if s[2] is None else min(s[2], ns)
        s[3] = max(s[3], ns)
    total = sum(s[1] for s in stats.values())
    w = csv.writer(out)
    w.writerow(['Name', 'Calls', 'TotalDurationNs', 'AverageNs', 'Percentage', 'MinNs', 'MaxNs'])
    for name, (n, t, lo, hi) in sorted(stats.items(), key=lambda kv: -kv[1][1]):
        w.writerow([name, n, t, round(t / n, 1), round(100.0 * t / total, 2), lo, hi])
    w.writerow(['# one volume: %d launches, kernel time %d ns' % (len(vol), total)])


if __name__ == '__main__':
    if sys.argv[1:] == ['--run']:
        run()
    else:
        summarize(sys.argv[1])
