#!/usr/bin/env python3
"""A/B of an f32 inference conv kernel behind an environment switch that is read per call against the kernel the switch falls
back to, on the same tensors.  Default: the packed 64-channel-block conv (conv_mfma_f32_packed_kernel) against the unpacked kernel
(SQ_CONV_PACKED=0) for the ten <64,3,16> launches of the inference workload (32 tiles of 512 x 512, filters 16-32-64-128-256).
`--switch SQ_CONV_R32 --shapes name:entry:N:H:Cin:Cout,...` times another switch on another shape list (entry: conv2d or pool);
the arm with the switch on is called "packed" in the output whatever the switch, the arm with it at 0 "unpacked".  HIP events round `--calls` launches of one arm; the arms alternate measurement by measurement, so clock and
neighbour drift hits both alike.  Per arm: median and (max - min) / median of the per-call time.  A layer counts as faster only
when the packed median is below the unpacked one by more than the larger of the two spreads.
  python tools/conv_packed_ab.py [--out profiles/conv_packed_ab.json] [--reps 15] [--calls 30] [--lib other/libsequitr_hip.so]
  python tools/conv_packed_ab.py --switch SQ_CONV_R32 --shapes up1/conv1:conv2d:32:256:32:32,down1/conv2:pool:32:256:32:32 \
         --out profiles/conv_r32_ab.json
--lib times another build of the library (an experiment build of sq_conv_f32_packed.hip, say -DSQ_PK_RING=6)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, entry, N, H = W, Cin, Cout) in launch order of a step
LAYERS = [("down2/conv1", "conv2d", 32, 128, 32, 64), ("down2/conv2", "pool", 32, 128, 64, 64),
          ("down3/conv1", "conv2d", 32, 64, 64, 128), ("down3/conv2", "pool", 32, 64, 128, 128),
          ("down4/conv1", "conv2d", 32, 32, 128, 256), ("down4/conv2", "conv2d", 32, 32, 256, 256),
          ("up3/conv1", "conv2d", 32, 64, 128, 128), ("up3/conv2", "conv2d", 32, 64, 128, 128),
          ("up2/conv1", "conv2d", 32, 128, 64, 64), ("up2/conv2", "conv2d", 32, 128, 64, 64)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_packed_ab.json"))
    ap.add_argument("--reps", type=int, default=15, help="measurements per arm")
    ap.add_argument("--calls", type=int, default=30, help="launches per event pair (10 leave the 150 us layers a 3-5 %% spread)")
    ap.add_argument("--warm", type=int, default=100, help="warm-up launches per layer (the clocks settle)")
    ap.add_argument("--lib", default=None, help="another build of libsequitr_hip.so to time")
    ap.add_argument("--switch", default="SQ_CONV_PACKED", help="the environment switch of the kernel under test (0: the other kernel)")
    ap.add_argument("--shapes", default=None, help="name:entry:N:H:Cin:Cout,... instead of the ten 64-channel-block layers")
    a = ap.parse_args()
    layers = LAYERS
    if a.shapes:
        layers = [(f[0], f[1]) + tuple(int(v) for v in f[2:]) for f in (s.split(":") for s in a.shapes.split(","))]
        assert all(len(l) == 6 and l[1] in ("conv2d", "pool") for l in layers), "--shapes: name:entry:N:H:Cin:Cout"
    from sequitr_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    from sequitr_amd import ops
    os.environ.pop(a.switch, None)
    dev = "cuda:0"
    rows = []
    for name, entry, n, h, ci, co in layers:
        g = torch.Generator(device="cpu").manual_seed(ci * 1000 + co + h)
        x = torch.randn((n, h, h, ci), generator=g).to(dev)
        w = (torch.randn((3, 3, ci, co), generator=g) / float(np.sqrt(9 * ci))).to(dev)
        b = (torch.randn((co,), generator=g) * 0.1).to(dev)
        pk = ops.pack_filter(w)
        if a.switch == "SQ_CONV_R32":
            taken = ops.conv_r32_takes(tuple(x.shape), tuple(w.shape), pooled=entry == "pool")
        else:
            taken = ops.conv_packed_takes(tuple(x.shape), tuple(w.shape))

        def call():
            if entry == "pool":
                return ops.conv3x3_pool(x, w, b, act="relu", pack=pk)[0]
            return ops.conv2d(x, w, b, act="relu", pack=pk)

        def arm(packed):
            if packed:
                os.environ.pop(a.switch, None)
            else:
                os.environ[a.switch] = "0"

        arm(True)
        yp = call()
        arm(False)
        yu = call()
        same = bool(torch.equal(yp, yu))
        for _ in range(a.warm):
            call()
        times = {True: [], False: []}
        for _ in range(a.reps):
            for packed in (True, False):
                arm(packed)
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(a.calls):
                    call()
                e.record()
                e.synchronize()
                times[packed].append(s.elapsed_time(e) / a.calls * 1e3)
        arm(True)

        def stat(v):
            med = float(np.median(v))
            return {"median_us": round(med, 2), "spread": round((max(v) - min(v)) / med, 4), "min_us": round(min(v), 2),
                    "max_us": round(max(v), 2)}
        sp, su = stat(times[True]), stat(times[False])
        gain = 1.0 - sp["median_us"] / su["median_us"]
        noise = max(sp["spread"], su["spread"])
        tf = 2.0 * n * h * h * 9 * ci * co / 1e6
        rows.append({"layer": name, "entry": entry, "N": n, "H": h, "W": h, "Cin": ci, "Cout": co, "packed_kernel_taken": taken,
                     "bit_equal": same, "packed": sp, "unpacked": su, "gain": round(gain, 4), "larger_spread": noise,
                     "faster_beyond_spread": bool(gain > noise),
                     "tflops": {"packed": round(tf / sp["median_us"], 1), "unpacked": round(tf / su["median_us"], 1)}})
        print("%-12s %4d^2 %3d->%3d  packed %7.1f us (+-%.3f)  unpacked %7.1f us (+-%.3f)  gain %+.3f  %s%s" % (
            name, h, ci, co, sp["median_us"], sp["spread"], su["median_us"], su["spread"], gain,
            "FASTER" if gain > noise else "not beyond spread", "" if same else "  OUTPUTS DIFFER"), flush=True)
    tot_p = sum(r["packed"]["median_us"] for r in rows)
    tot_u = sum(r["unpacked"]["median_us"] for r in rows)
    out = {"what": "%s unset ('packed') vs %s=0 ('unpacked') on the same tensors, HIP events round %d calls, arms alternating, %d "
                   "measurements per arm after %d warm-up launches; spread = (max - min) / median" % (
                       a.switch, a.switch, a.calls, a.reps, a.warm),
           "switch": a.switch,
           "device": torch.cuda.get_device_name(0), "library": os.path.relpath(_lib.LIB_PATH, ROOT), "layers": rows,
           "sum_of_medians_us": {"packed": round(tot_p, 1), "unpacked": round(tot_u, 1)}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("sum of medians: packed %.1f us, unpacked %.1f us -> %s" % (tot_p, tot_u, a.out))


if __name__ == "__main__":
    main()
