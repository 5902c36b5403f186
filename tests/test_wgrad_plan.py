"""CPU: the launch plans of the weight gradients (sq_wgrad_plan / sq_wgrad_group_plan, the host functions the launchers and the
workspace queries take their block shapes, prefetch depths, tile runs and workspaces from).  The plans of three workloads are
pinned, every plan the dispatchers can produce must be run by a case of the GPU sweep (tests/wgrad_sweep_cases.py), and the
environment switches act on the query as on the launchers."""
import os
import subprocess
import sys

import pytest

from sequitr_amd import _lib, ops
from tests import wgrad_sweep_cases as ws
from tests.test_conv_plan import UNET_FILTERS, gan_layers, unet_layers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("ni", "no", "kind", "pf", "gx", "tpb")

# 16 x 512^2 bf16 training step: (NI, NO, kind, PF, gx, tpb) of every 3x3 wgrad, the four transpose-conv wgrads (kind 3, the
# 1x1 kernel on Cout = 4 * Cout) and the first layer's (the small-Cin kernel, kind 5: NI = Cin, NO = 16)
TRAIN16 = {
    'down0/conv2': (1, 1, 0, 3, 512, -32), 'down1/conv1': (1, 2, 0, 1, 512, -8), 'down1/conv2': (1, 2, 0, 1, 256, -16),
    'down2/conv1': (1, 2, 0, 1, 128, -8), 'down2/conv2': (1, 2, 0, 1, 64, -16), 'down3/conv1': (1, 2, 0, 1, 32, -8),
    'down3/conv2': (1, 2, 0, 1, 16, -16), 'down4/conv1': (1, 2, 0, 1, 8, -8), 'down4/conv2': (1, 2, 0, 1, 4, -16),
    'up3/conv1': (1, 2, 0, 1, 16, -16), 'up3/conv2': (1, 2, 0, 1, 16, -16), 'up2/conv1': (1, 2, 0, 1, 64, -16),
    'up2/conv2': (1, 2, 0, 1, 64, -16), 'up1/conv1': (1, 2, 0, 1, 256, -16), 'up1/conv2': (1, 2, 0, 1, 256, -16),
    'up0/conv1': (1, 1, 0, 3, 512, -32), 'up0/conv2': (1, 1, 0, 3, 512, -32), 'convT0': (2, 4, 3, 1, 512, -8),
    'convT1': (2, 4, 3, 1, 128, -8), 'convT2': (2, 4, 3, 1, 32, -8), 'convT3': (2, 4, 3, 1, 8, -8),
    'down0/conv1': (1, 16, 5, 1, 2048, 8),
}
# ... and the group plan of its WgradQueue (every layer with 16-channel multiples, in backward order): (launch, gx, tpb,
# pair-major) after the shrink.  Three launches: the 16-channel 3x3 layers (three items: tile runs / 3), the transpose convs,
# the other 3x3 layers (16 items: / 4).
TRAIN16_GROUP = {
    'up0/conv2': (0, 169, -97, 0), 'up0/conv1': (0, 169, -97, 0), 'convT0': (1, 128, -32, 1), 'up1/conv2': (2, 64, -64, 1),
    'up1/conv1': (2, 64, -64, 1), 'convT1': (1, 32, -32, 1), 'up2/conv2': (2, 16, -64, 1), 'up2/conv1': (2, 16, -64, 1),
    'convT2': (1, 8, -32, 1), 'up3/conv2': (2, 4, -64, 0), 'up3/conv1': (2, 4, -64, 0), 'convT3': (1, 2, -32, 0),
    'down4/conv2': (2, 1, -64, 0), 'down4/conv1': (2, 2, -32, 0), 'down3/conv2': (2, 4, -64, 0),
    'down3/conv1': (2, 8, -32, 1), 'down2/conv2': (2, 16, -64, 1), 'down2/conv1': (2, 32, -32, 1),
    'down1/conv2': (2, 64, -64, 1), 'down1/conv1': (2, 128, -32, 1), 'down0/conv2': (0, 169, -97, 0),
}
# GAN level 6, batch 32, bf16 storage, as ops_gan_bf16.conv_wgrad issues them: sides below 16 as one mosaic (kind 1, with its
# (R, Cc)), the 8-channel layers ragged (kind 2)
GAN6 = {
    'G conv0': (1, 2, 1, 1, 1, -4, (11, 3)), 'G l1 conv1': (1, 2, 1, 1, 2, -6, (7, 5)), 'G l1 conv2': (1, 2, 1, 1, 4, -3, (7, 5)),
    'G l2 conv1': (1, 2, 0, 1, 8, -4), 'G l2 conv2': (1, 2, 0, 1, 16, -2), 'G l3 conv1': (1, 2, 0, 1, 32, -4),
    'G l3 conv2': (1, 2, 0, 1, 64, -2), 'G l4 conv1': (1, 2, 0, 1, 128, -4), 'G l4 conv2': (1, 2, 0, 1, 256, -2),
    'G l5 conv1': (2, 1, 0, 1, 512, -4), 'G l5 conv2': (1, 1, 0, 3, 512, -4), 'G l6 conv1': (1, 1, 2, 4, 512, -16),
    'G l6 conv2': (1, 1, 2, 4, 512, -16), 'D l0 conv1': (1, 1, 2, 4, 512, -16), 'D l0 conv2': (1, 1, 0, 3, 512, -16),
    'D l1 conv1': (1, 2, 0, 1, 512, -4), 'D l1 conv2': (1, 2, 0, 1, 256, -8), 'D l2 conv1': (1, 2, 0, 1, 128, -4),
    'D l2 conv2': (1, 2, 0, 1, 64, -8), 'D l3 conv1': (1, 2, 0, 1, 32, -4), 'D l3 conv2': (1, 2, 0, 1, 16, -8),
    'D l4 conv1': (1, 2, 0, 1, 8, -4), 'D l4 conv2': (1, 2, 0, 1, 4, -8), 'D l5 conv1': (1, 2, 1, 1, 2, -6, (7, 5)),
    'D l5 conv2': (1, 2, 1, 1, 1, -12, (7, 5)), 'D out': (1, 2, 1, 1, 1, -4, (11, 3)),
}
# the f32 U-Net training step, 16 x 512^2: (KC, BN, kind 4, 1, gx, tpb); the first layer on the small-Cin kernel
F32_TRAIN16 = {
    'down0/conv2': (16, 16, 4, 1, 512, 32), 'down1/conv1': (16, 32, 4, 1, 512, 8), 'down1/conv2': (16, 32, 4, 1, 256, 16),
    'down2/conv1': (16, 32, 4, 1, 128, 8), 'down2/conv2': (16, 32, 4, 1, 64, 16), 'down3/conv1': (16, 32, 4, 1, 32, 8),
    'down3/conv2': (16, 32, 4, 1, 16, 16), 'down4/conv1': (16, 32, 4, 1, 8, 8), 'down4/conv2': (16, 32, 4, 1, 4, 16),
    'up3/conv1': (16, 32, 4, 1, 16, 16), 'up3/conv2': (16, 32, 4, 1, 16, 16), 'up2/conv1': (16, 32, 4, 1, 64, 16),
    'up2/conv2': (16, 32, 4, 1, 64, 16), 'up1/conv1': (16, 32, 4, 1, 256, 16), 'up1/conv2': (16, 32, 4, 1, 256, 16),
    'up0/conv1': (16, 16, 4, 1, 512, 32), 'up0/conv2': (16, 16, 4, 1, 512, 32), 'down0/conv1': (1, 16, 5, 1, 2048, 8),
}


def _short(p):
    return tuple(p[k] for k in KEYS)


def train_queue():
    """the items the bf16 training step's WgradQueue collects, in backward order (group items of wgrad_sweep_cases)"""
    f = UNET_FILTERS
    items = []
    for i in range(4):
        s = 512 >> i
        items += [ws._gi(16, s, s, f[i], f[i], 3, "up%d/conv2" % i, "up%d/conv2 b" % i),
                  ws._gi(16, s, s, f[i], f[i], 3, "up%d/conv1" % i, "up%d/conv1 b" % i),
                  ws._gi(16, s // 2, s // 2, f[i + 1], 4 * f[i], 1, "convT%d" % i, "convT%d b" % i, convT=f[i])]
    for i in reversed(range(5)):
        s = 512 >> i
        items.append(ws._gi(16, s, s, f[i], f[i], 3, "down%d/conv2" % i, "down%d/conv2 b" % i))
        if i:
            items.append(ws._gi(16, s, s, f[i - 1], f[i], 3, "down%d/conv1" % i, "down%d/conv1 b" % i))
    return items


def test_bf16_training_step_plans_are_pinned():
    f = UNET_FILTERS
    got = {name: _short(ws.plan("bf16", 16, s, s, ci, co, 3)) for name, s, ci, co in unet_layers()}
    for i in range(4):
        s = 512 >> (i + 1)
        got["convT%d" % i] = _short(ws.plan("bf16", 16, s, s, f[i + 1], 4 * f[i], 1, convT=f[i]))
    got["down0/conv1"] = _short(ws.plan("first", 16, 512, 512, 1, 16, 3))
    assert got == TRAIN16


def test_bf16_training_step_group_plan_is_pinned():
    items = train_queue()
    nbk, ps = ws.group_plan(items)
    assert nbk == 3
    assert {it["dw"]: (p["bucket"], p["gx"], p["tpb"], p["pair_major"]) for it, p in zip(items, ps)} == TRAIN16_GROUP
    # each item's partials lie in the room the workspace query reserves for it, after those of the items before it in its launch
    lib = _lib.load()
    arr = ws.items_array(items)
    total = lib.sq_conv2d_nhwc_wgrad_group_workspace_bf16(arr, len(items))
    for b in range(nbk):
        off = 0
        for it, p in zip(items, ps):
            if p["bucket"] != b:
                continue
            alone = ws.plan("bf16", it["N"], it["H"], it["W"], it["Cin"], it["Cout"], it["K"], convT=it.get("convT", 0))
            assert p["offset"] == off and p["ws"] <= alone["ws"] and (p["ni"], p["no"], p["pf"]) == (alone["ni"], alone["no"], alone["pf"])
            off += alone["ws"]
        assert off * 4 <= total


def test_gan_level6_plans_are_pinned():
    got = {}
    for name, s, ci, co, _ in gan_layers():
        m = ops._mosaic_plan(32, s, s)
        got[name] = _short(ws.plan("bf16", 32, s, s, ci, co, 3, mosaic=m)) + ((m,) if m else ())
    assert got == GAN6


def test_f32_training_step_plans_are_pinned():
    got = {name: _short(ws.plan("f32", 16, s, s, ci, co, 3)) for name, s, ci, co in unet_layers()}
    got["down0/conv1"] = _short(ws.plan("f32", 16, 512, 512, 1, 16, 3))
    assert got == F32_TRAIN16


def test_plans_agree_with_the_workspace_queries():
    lib = _lib.load()
    for c in ws.CASES:
        p = ws.case_plan(c)
        N, H, W = (1, c["mosaic"][0] * (c["H"] + 1), c["mosaic"][1] * (c["W"] + 1)) if c["mosaic"] else (c["N"], c["H"], c["W"])
        q = {"bf16": lib.sq_conv2d_nhwc_wgrad_workspace_bf16, "mixed": lib.sq_conv2d_nhwc_wgrad_workspace_mixed_f32,
             "f32": lib.sq_conv2d_nhwc_wgrad_workspace_f32}.get(c["fam"])
        want = q(N, H, W, c["Cin"], c["Cout"], c["K"]) if q else \
            lib.sq_conv3x3_first_wgrad_workspace_bf16(N, H, W, c["Cin"], c["Cout"])
        assert p["ws"] * 4 == want, (c, p)
        assert p["gx"] == len(ws.block_counts(p, ws.tiles_of(c))) and sum(ws.block_counts(p, ws.tiles_of(c))) == ws.tiles_of(c)


def test_calls_no_kernel_takes_are_refused():
    for args, kw in [(("mixed", 1, 16, 16, 24, 32, 3), {}), (("bf16", 1, 16, 16, 16, 32, 2), {}),
                     (("bf16", 1, 16, 16, 16, 32, 3), dict(convT=8)), (("mixed", 1, 16, 16, 16, 32, 1), dict(convT=8)),
                     (("bf16", 4, 9, 9, 16, 32, 3), dict(mosaic=(2, 2))), (("bf16", 5, 4, 4, 16, 32, 3), dict(mosaic=(2, 2))),
                     (("bf16", 4, 4, 4, 24, 32, 3), dict(mosaic=(2, 2))), (("f32", 1, 16, 16, 12, 32, 3), {}),
                     (("f32", 1, 16, 16, 3, 32, 1), {}), (("f32", 1, 16, 16, 16, 30, 3), {})]:
        with pytest.raises(_lib.SequitrHipError):
            ws.plan(*args, **kw)


def expected_keys():
    """every (family, KS, NI, NO, kind) default dispatch can produce (f32: (KC, BN)); kind 4 of them need a partial last block"""
    k3 = [(1, 2), (2, 1), (1, 1)]
    k1 = [(2, 4), (2, 2), (2, 1), (1, 2), (1, 1)]
    want = set()
    for fam in ("bf16", "mixed"):
        want |= {(fam, 3, ni, no, kind) for ni, no in k3 for kind in (ws.PLAIN, ws.MOSAIC)}
        want |= {(fam, 1, ni, no, ws.PLAIN) for ni, no in k1}
    want |= {("bf16", 1, ni, no, ws.CONVT) for ni, no in k1}
    want |= {("bf16", 3, 1, 1, ws.RAGGED), ("bf16", 1, 1, 1, ws.RAGGED)}
    f32 = {("f32", K, kc, bn, ws.F32K) for K in (1, 3) for kc in (8, 16) for bn in (16, 32)}
    return want | f32, f32


def test_the_sweep_reaches_every_plan():
    keys, runs, partial, small, buckets, props = ws.reached()
    want, f32 = expected_keys()
    assert keys == want, ("missing", sorted(want - keys), "unexpected", sorted(keys - want))
    assert partial == f32, sorted(f32 - partial)
    assert small == {(fam, c) for fam in ("f32", "first") for c in range(1, 8)}
    for key, (pf, longest, residues) in runs.items():
        if pf > 1:
            assert longest >= pf + 1, (key, pf, longest)
            assert residues == set(range(pf)), (key, pf, residues)
    # every grouped bucket (kind, KS, NI, NO) and the group's own paths
    gwant = {(ws.PLAIN, 3, ni, no) for ni, no in [(1, 2), (2, 1), (1, 1)]} | {(ws.PLAIN, 1, ni, no) for ni, no in
                                                                                [(2, 4), (2, 2), (2, 1), (1, 2), (1, 1)]}
    gwant |= {(ws.MOSAIC, 3, ni, no) for ni, no in [(1, 2), (2, 1), (1, 1)]} | {(ws.RAGGED, 3, 1, 1), (ws.RAGGED, 1, 1, 1)}
    assert buckets == gwant, ("missing", sorted(gwant - buckets), "unexpected", sorted(buckets - gwant))
    assert props >= {"pair_major", "plain_mapping", "mixed_tile_counts", "spill", "acc0", "acc1", "acc2", "acc3", "db_null",
                     "scale", "convT"}, props


def test_the_exact_oracle_stays_exact():
    """operands in -3..3: |dW| <= 9 P and |db| <= 3 P (12 P for a transpose conv's folded bias), every partial sum an integer
    below 2^24 -- exact in f32 in any order"""
    for c in ws.CASES + [dict(it, fam="bf16") for g in ws.GROUPS.values() for it in g]:
        P = c["N"] * c["H"] * c["W"]
        assert 9 * P < 2 ** 24 and 12 * P < 2 ** 24, c


SWITCHES = {   # switch: (value, query, its result without the switch, with it)
    "SQ_WGRAD_BF16_NARROW": ("1", "ws.plan('bf16', 1, 16, 16, 64, 64, 3)['no']", 2, 1),
    "SQ_WGRAD_BF16_MAX": ("2,2", "ws.plan('mixed', 1, 16, 16, 64, 128, 1)['no']", 4, 2),
    "SQ_WGRAD_BF16_K3": ("2,2", "ws.plan('bf16', 1, 16, 16, 64, 64, 3)['ni']", 1, 2),
    "SQ_WGRAD_INTERLEAVE": ("0", "ws.plan('bf16', 16, 512, 512, 16, 16, 3)['tpb']", -32, 32),
    "SQ_WGRAD_GROUP_SHRINK": ("1", "ws.group_plan(ws.GROUPS['pair_major'])[1][0]['gx']", 16, 64),
    "SQ_WGRAD_PAIR_MAJOR": ("0", "ws.group_plan(ws.GROUPS['pair_major'])[1][0]['pair_major']", 1, 0),
}


@pytest.mark.parametrize("name", sorted(SWITCHES))
def test_environment_switches_act_on_the_query(name):
    """the launchers read the switches once per process: a fresh interpreter per setting"""
    value, query, default, switched = SWITCHES[name]
    code = "import sys; sys.path.insert(0, %r); from tests import wgrad_sweep_cases as ws; print(%s)" % (ROOT, query)
    clean = {k: v for k, v in os.environ.items() if not k.startswith("SQ_WGRAD")}
    for env, want in ((clean, default), (dict(clean, **{name: value}), switched)):
        r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        assert int(r.stdout.split()[-1]) == want, (name, env.get(name), r.stdout)
