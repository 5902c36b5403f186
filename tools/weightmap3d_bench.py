"""Volumetric EDT weight-map benchmark: one JSON line, also written to profiles/weightmap3d_bench.json.

Workloads: 8 label volumes of 32 x 128 x 128 and one of 64 x 256 x 256, random balls at a cell-like density generated here
from a seed.  Per workload, HIP events round windows of several back-to-back calls after warm-up, the variants alternated
in the same run:
  * map3d        : ops.weightmap_edt3d (float32 output): ms per call and Gvoxel/s;
  * planar_floor : the same voxels pushed through the planar ops.weightmap_edt as N*D images -- a floor, not a rival: the
                   3-D map does one more pass over an int32 field;
  * planar_passes: ops.edt_squared on the N*D slices, the two planar passes writing an int32 field as the 3-D map's planar
                   half does; depth_pass_ms_est = map3d - planar_passes;
  * scipy_cpu_s  : the reference's own call (distance_transform_edt + the float64 expression) on ONE volume on the host;
  * maps_identical_f32: that volume's device map equals the float32 rounding of the host map.
Usage: python tools/weightmap3d_bench.py [--spacing 1.0] [--warmup 3] [--iters 10] [--out PATH]
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

REPS = 8                                                        # calls per event pair
WORKLOADS = ((8, 32, 128, 128), (1, 64, 256, 256))
W0, SIGMA = 10., 5.


def ball_labels(shape, seed, spacing):
    """(N,D,H,W) float32: balls of radius 5..9 in-plane pixels, one per ~6000 voxels of physical volume (about a fifth of the
    volume is cell), flattened along depth by the slice spacing as a cell in an anisotropic stack is"""
    rng = np.random.default_rng(seed)
    N, D, H, W = shape
    lab = np.zeros(shape, np.float32)
    for n in range(N):
        for _ in range(max(1, int(D * spacing * H * W / 6000))):
            r = int(rng.integers(5, 10))
            cz, cx, cy = rng.integers(0, D), rng.integers(0, H), rng.integers(0, W)
            rz = int(np.ceil(r / spacing))
            z0, z1, x0, x1, y0, y1 = max(0, cz - rz), min(D, cz + rz + 1), max(0, cx - r), min(H, cx + r + 1), max(0, cy - r), \
                min(W, cy + r + 1)
            zz, xx, yy = np.mgrid[z0:z1, x0:x1, y0:y1]
            lab[n, z0:z1, x0:x1, y0:y1][((zz - cz) * spacing) ** 2 + (xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = 1
    return lab


def _time(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def host_map(vol, spacing):
    """ImageWeightMap.pipe (sequitr/pipeline.py:475-479) on one (Z, X, Y) volume, scipy on the host, float64"""
    from scipy.ndimage import distance_transform_edt
    image = vol.astype(np.float64)
    d = distance_transform_edt(1. - image, sampling=(spacing, 1, 1))
    return W0 * (1. - image) * np.exp(-(d * d) / (2. * SIGMA ** 2 + 1e-99)) + image + 1.


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--spacing', type=float, default=1.0)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'weightmap3d_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('weightmap3d_bench needs the GPU')
    from sequitr_amd import ops
    torch.cuda.set_device(0)
    rows = []
    for k, shape in enumerate(WORKLOADS):
        N, D, H, W = shape
        lab = ball_labels(shape, k, args.spacing)
        img = torch.from_numpy(lab).to('cuda:0')
        flat = img.reshape(N * D, H, W)
        variants = {'map3d': lambda: ops.weightmap_edt3d(img, W0, SIGMA, args.spacing),
                    'planar_floor': lambda: ops.weightmap_edt(flat, W0, SIGMA),
                    'planar_passes': lambda: ops.edt_squared(flat)}
        for _ in range(args.warmup):
            for fn in variants.values():
                fn()
        torch.cuda.synchronize()
        t = {name: [] for name in variants}
        for _ in range(args.iters):                             # alternate the variants so drift hits all alike
            for name, fn in variants.items():
                t[name].append(_time(fn, REPS))
        med = {name: float(np.median(v)) for name, v in t.items()}
        got = ops.weightmap_edt3d(img[:1], W0, SIGMA, args.spacing).cpu().numpy()[0]
        t0 = time.time()
        ref = host_map(lab[0], args.spacing)
        scipy_s = time.time() - t0
        vox = N * D * H * W
        depth = med['map3d'] - med['planar_passes']
        rows.append({'shape': list(shape), 'spacing': args.spacing, 'foreground_fraction': round(float(lab.mean()), 4),
                     'map3d_ms': round(med['map3d'], 4), 'map3d_gvoxel_per_s': round(vox / med['map3d'] / 1e6, 3),
                     'map3d_ms_min_max': [round(min(t['map3d']), 4), round(max(t['map3d']), 4)],
                     'planar_floor_ms': round(med['planar_floor'], 4),
                     'planar_floor_gvoxel_per_s': round(vox / med['planar_floor'] / 1e6, 3),
                     'planar_floor_ms_min_max': [round(min(t['planar_floor']), 4), round(max(t['planar_floor']), 4)],
                     'map3d_over_planar_floor': round(med['map3d'] / med['planar_floor'], 3),
                     'planar_passes_ms': round(med['planar_passes'], 4), 'depth_pass_ms_est': round(depth, 4),
                     'depth_pass_costs_more_than_planar_passes': bool(depth > med['planar_passes']),
                     'scipy_cpu_s_one_volume': round(scipy_s, 3),
                     'maps_identical_f32': bool(np.array_equal(got, ref.astype(np.float32)))})
    line = {'workload': 'volumetric EDT weight maps (ops.weightmap_edt3d, float32 output), w0 %g sigma %g' % (W0, SIGMA),
            'warmup': args.warmup, 'iters': args.iters, 'calls_per_window': REPS, 'device': torch.cuda.get_device_name(0),
            'rows': rows}
    text = json.dumps(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
