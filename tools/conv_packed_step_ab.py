#!/usr/bin/env python3
"""The inference step of this tree against another tree's (the parent commit, built): `python bench.py`, the plain headline,
one fresh process per run, the two trees alternating, `--runs` processes per tree in one session on one box.  Writes the
`ms_per_step` of every run, the medians and (max - min) / median per tree, and the verdict: a gain only if the new median is
below the parent's by more than the larger of the two spreads.  `--full-once` adds one `bench.py --full --no-cpu-baseline
--no-end-to-end --no-side-lines` run per tree (after the timed ones; its own instrumentation, never compared with them) for
`roofline.frac`.  `--env NAME=VALUE` (repeatable) is set for the NEW tree's processes only: with `--parent` pointing at this very
tree it is an A/B of one of its per-call kernel switches (SQ_CONV_R32=0, SQ_CONV_PACKED=0, ...).
  python tools/conv_packed_step_ab.py --parent /path/to/built/parent/tree [--runs 5] [--out profiles/conv_packed_step_ab.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench(tree, extra=(), env=None):
    out = subprocess.run([sys.executable, os.path.join(tree, "bench.py")] + list(extra), stdout=subprocess.PIPE, text=True,
                         cwd=tree, check=True, timeout=600, env=env).stdout
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="the other tree: a checkout of the parent commit with its library built")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_packed_step_ab.json"))
    ap.add_argument("--full-once", action="store_true")
    ap.add_argument("--env", action="append", default=[], help="NAME=VALUE for the new tree's processes (a kernel switch)")
    a = ap.parse_args()
    envs = {"parent": None, "new": dict(os.environ, **dict(e.split("=", 1) for e in a.env)) if a.env else None}
    trees = {"parent": os.path.abspath(a.parent), "new": ROOT}
    ms = {"parent": [], "new": []}
    for i in range(a.runs):
        for name in ("parent", "new"):
            r = bench(trees[name], env=envs[name])
            ms[name].append(r["ms_per_step"])
            print("run %d %-6s %.4f ms" % (i, name, r["ms_per_step"]), flush=True)

    def stat(v):
        med = float(np.median(v))
        return {"ms_per_step": v, "median": round(med, 4), "spread": round((max(v) - min(v)) / med, 4)}
    res = {"what": "python bench.py (plain headline: 20 warm-up + 100 timed steps of 32 x 512^2 f32 inference), one process per "
                   "run, trees alternating, %d runs per tree; spread = (max - min) / median" % a.runs,
           "new_tree_env": a.env, "parent": stat(ms["parent"]), "new": stat(ms["new"])}
    gain = 1.0 - res["new"]["median"] / res["parent"]["median"]
    noise = max(res["parent"]["spread"], res["new"]["spread"])
    res["ratio_new_over_parent"] = round(res["new"]["median"] / res["parent"]["median"], 4)
    res["gain"] = round(gain, 4)
    res["larger_spread"] = noise
    res["gain_beyond_spread"] = bool(gain > noise)
    if a.full_once:
        res["roofline_frac"] = {}
        for name in ("parent", "new"):
            r = bench(trees[name], ["--full", "--no-cpu-baseline", "--no-end-to-end", "--no-side-lines"], env=envs[name])
            res["roofline_frac"][name] = {"frac": r["roofline"]["frac"], "achieved_tflops": r["roofline"]["achieved"],
                                          "kernel_ms_per_step": r["roofline"]["kernel_ms_per_step"],
                                          "ms_per_step_instrumented": r["ms_per_step"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "what"}))


if __name__ == "__main__":
    main()
