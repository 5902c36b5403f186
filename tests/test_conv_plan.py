"""CPU: the launch plans of the implicit-GEMM convolutions (sq_conv_plan, the host functions the launchers take their block
widths and split-K factors from).  The plans of three workloads are pinned, every plan the dispatchers can produce must be run
by a case of the GPU sweep (tests/conv_sweep_cases.py), and the environment switches act on the query as on the launchers."""
import os
import subprocess
import sys

import pytest

from sequitr_amd import _lib
from tests import conv_sweep_cases as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNET_FILTERS = (16, 32, 64, 128, 256)
GAN_FILTERS = [512, 256, 128, 64, 32, 16, 8]               # level 6: 4x4 .. 256x256

# 32 x 512^2 f32 inference (bench.py): (BN, KC) of the v2 kernels, or "l0" where the level-0 kernel takes the layer
INFER32 = {
    'down0/conv2': 'l0', 'down1/conv1': 'l0', 'down1/conv2': (32, 32), 'down2/conv1': (64, 16), 'down2/conv2': (64, 16),
    'down3/conv1': (64, 16), 'down3/conv2': (64, 16), 'down4/conv1': (64, 16), 'down4/conv2': (64, 16), 'up3/conv1': (64, 16),
    'up3/conv2': (64, 16), 'up2/conv1': (64, 16), 'up2/conv2': (64, 16), 'up1/conv1': (32, 32), 'up1/conv2': (32, 32),
    'up0/conv1': 'l0', 'up0/conv2': 'l0',
}
# 16 x 512^2 bf16 training step: (BN, KC) of each forward conv and of its dgrad
TRAIN16 = {
    'down0/conv2 fwd': (16, 16), 'down0/conv2 dgrad': (16, 16), 'down1/conv1 fwd': (32, 16), 'down1/conv1 dgrad': (16, 32),
    'down1/conv2 fwd': (32, 32), 'down1/conv2 dgrad': (32, 32), 'down2/conv1 fwd': (64, 32), 'down2/conv1 dgrad': (32, 32),
    'down2/conv2 fwd': (64, 32), 'down2/conv2 dgrad': (64, 32), 'down3/conv1 fwd': (64, 32), 'down3/conv1 dgrad': (32, 32),
    'down3/conv2 fwd': (64, 32), 'down3/conv2 dgrad': (64, 32), 'down4/conv1 fwd': (32, 32), 'down4/conv1 dgrad': (16, 32),
    'down4/conv2 fwd': (32, 32), 'down4/conv2 dgrad': (32, 32), 'up3/conv1 fwd': (64, 32), 'up3/conv1 dgrad': (64, 32),
    'up3/conv2 fwd': (64, 32), 'up3/conv2 dgrad': (64, 32), 'up2/conv1 fwd': (64, 32), 'up2/conv1 dgrad': (64, 32),
    'up2/conv2 fwd': (64, 32), 'up2/conv2 dgrad': (64, 32), 'up1/conv1 fwd': (32, 32), 'up1/conv1 dgrad': (32, 32),
    'up1/conv2 fwd': (32, 32), 'up1/conv2 dgrad': (32, 32), 'up0/conv1 fwd': (16, 16), 'up0/conv1 dgrad': (16, 16),
    'up0/conv2 fwd': (16, 16), 'up0/conv2 dgrad': (16, 16),
}
# GAN level 6, batch 32, bf16 storage: (BN, KC, S) of every generator / discriminator conv and of its act-gated dgrad.  Sides
# below 16 run as one mosaic with the split-K room ops_gan_bf16 offers; generator convs to <= 64 channels fuse the pixel norm,
# the discriminator's second convs the average pool.
GAN6 = {
    'G conv0 fwd': (16, 32, 4), 'G conv0 dgrad': (16, 32, 4), 'G l1 conv1 fwd': (16, 32, 4), 'G l1 conv1 dgrad': (16, 32, 1),
    'G l1 conv2 fwd': (16, 32, 4), 'G l1 conv2 dgrad': (16, 32, 4), 'G l2 conv1 fwd': (16, 32, 1),
    'G l2 conv1 dgrad': (16, 32, 1), 'G l2 conv2 fwd': (16, 32, 1), 'G l2 conv2 dgrad': (16, 32, 1),
    'G l3 conv1 fwd': (64, 32, 1), 'G l3 conv1 dgrad': (32, 32, 1), 'G l3 conv2 fwd': (64, 32, 1),
    'G l3 conv2 dgrad': (16, 32, 1), 'G l4 conv1 fwd': (32, 32, 1), 'G l4 conv1 dgrad': (64, 32, 1),
    'G l4 conv2 fwd': (32, 32, 1), 'G l4 conv2 dgrad': (32, 32, 1), 'G l5 conv1 fwd': (16, 32, 1),
    'G l5 conv1 dgrad': (32, 16, 1), 'G l5 conv2 fwd': (16, 16, 1), 'G l5 conv2 dgrad': (16, 16, 1),
    'G l6 conv1 fwd': (16, 16, 1), 'G l6 conv1 dgrad': (16, 8, 1), 'G l6 conv2 fwd': (16, 8, 1),
    'G l6 conv2 dgrad': (16, 8, 1), 'D l0 conv1 fwd': (16, 8, 1), 'D l0 conv1 dgrad': (16, 16, 1),
    'D l0 conv2 fwd': (16, 16, 1), 'D l0 conv2 dgrad': (16, 16, 1), 'D l1 conv1 fwd': (32, 16, 1),
    'D l1 conv1 dgrad': (16, 32, 1), 'D l1 conv2 fwd': (32, 32, 1), 'D l1 conv2 dgrad': (32, 32, 1),
    'D l2 conv1 fwd': (64, 32, 1), 'D l2 conv1 dgrad': (32, 32, 1), 'D l2 conv2 fwd': (64, 32, 1),
    'D l2 conv2 dgrad': (64, 32, 1), 'D l3 conv1 fwd': (32, 32, 1), 'D l3 conv1 dgrad': (16, 32, 1),
    'D l3 conv2 fwd': (32, 32, 1), 'D l3 conv2 dgrad': (32, 32, 1), 'D l4 conv1 fwd': (16, 32, 1),
    'D l4 conv1 dgrad': (16, 32, 1), 'D l4 conv2 fwd': (16, 32, 1), 'D l4 conv2 dgrad': (16, 32, 1),
    'D l5 conv1 fwd': (16, 32, 1), 'D l5 conv1 dgrad': (16, 32, 4), 'D l5 conv2 fwd': (16, 32, 1),
    'D l5 conv2 dgrad': (16, 32, 1), 'D out fwd': (16, 32, 4), 'D out dgrad': (16, 32, 4),
}


def unet_layers():
    """(name, side at a 512 x 512 input, Cin, Cout) of every 3x3 conv after the single-channel first one"""
    f = UNET_FILTERS
    out = []
    for i, fi in enumerate(f):
        if i:
            out.append(("down%d/conv1" % i, 512 >> i, f[i - 1], fi))
        out.append(("down%d/conv2" % i, 512 >> i, fi, fi))
    for i in reversed(range(len(f) - 1)):
        out += [("up%d/conv1" % i, 512 >> i, f[i], f[i]), ("up%d/conv2" % i, 512 >> i, f[i], f[i])]
    return out


def gan_layers():
    """(name, side, Cin, Cout, kind): kind "norm" (generator), "pool" (discriminator conv2) or None"""
    F = GAN_FILTERS
    out = [("G conv0", 4, 512, 512, "norm")]
    for l in range(1, 7):
        out += [("G l%d conv1" % l, 4 << l, F[l - 1], F[l], "norm"), ("G l%d conv2" % l, 4 << l, F[l], F[l], "norm")]
    R = F[::-1]
    for l in range(6):
        out += [("D l%d conv1" % l, 256 >> l, R[l], R[l + 1], None), ("D l%d conv2" % l, 256 >> l, R[l + 1], R[l + 1], "pool")]
    return out + [("D out", 4, 512, 512, None)]


def test_inference_batch_plans_are_pinned():
    got = {}
    for name, s, ci, co in unet_layers():
        p = cs.plan(cs.F32, cs.PLAIN, 32, s, s, ci, co, 3, "relu")
        got[name] = "l0" if p["l0"] else (p["bn"], p["kc"])
    assert got == INFER32


def test_bf16_training_step_plans_are_pinned():
    got = {}
    for name, s, ci, co in unet_layers():
        for d, (a, b) in (("fwd", (ci, co)), ("dgrad", (co, ci))):
            p = cs.plan(cs.BF16, cs.PLAIN, 16, s, s, a, b, 3, "relu")
            got["%s %s" % (name, d)] = (p["bn"], p["kc"])
            assert p["gy"] == -(-b // p["bn"]) and p["s"] == 1
    assert got == TRAIN16


def test_gan_level6_plans_are_pinned():
    got = {}
    for name, s, ci, co, kind in gan_layers():
        for d, (a, b) in (("fwd", (ci, co)), ("dgrad", (co, ci))):
            if s < 16:
                R, Cc = cs.mosaic_grid(32, s, s)
                room = cs.splitk_room(32, s, s, b)
                p = cs.plan(cs.BF16, cs.PLAIN if d == "fwd" else cs.ACTGATE, 32, s, s, a, b, 3, "leaky", mosaic=(R, Cc),
                            workspace_bytes=room if room <= (64 << 20) else 0)
            else:
                form = cs.ACTGATE
                if d == "fwd":
                    form = cs.PIXELNORM if (kind == "norm" and b <= 64) else (cs.POOL if kind == "pool" else cs.PLAIN)
                p = cs.plan(cs.BF16, form, 32, s, s, a, b, 3, "leaky")
            got["%s %s" % (name, d)] = (p["bn"], p["kc"], p["s"])
    assert got == GAN6


def test_pixel_norm_holds_every_channel_in_one_block():
    for cout, bn in ((8, 16), (16, 16), (24, 32), (32, 32), (40, 64), (48, 64), (56, 64), (64, 64)):
        for shape in ((1, 16, 16), (4, 256, 256)):
            p = cs.plan(cs.BF16, cs.PIXELNORM, *shape, 32, cout, 3, "leaky")
            assert (p["bn"], p["gy"]) == (bn, 1), (cout, shape, p)


def test_forms_that_do_not_exist_are_refused():
    for args in [(cs.BF16, cs.PIXELNORM, 1, 32, 32, 16, 72, 3), (cs.BF16, cs.PIXELNORM, 1, 32, 32, 16, 32, 1),
                 (cs.BF16, cs.POOL, 1, 32, 32, 16, 32, 1), (cs.BF16, cs.MASK, 1, 32, 32, 16, 24, 3),
                 (cs.BF16, cs.JUNCTION, 1, 32, 32, 16, 32, 1), (cs.MIXED, cs.POOL, 1, 32, 32, 16, 32, 3),
                 (cs.BF16, cs.FIRSTBLOCK, 1, 32, 32, 16, 32, 3), (cs.F32, cs.POOL, 1, 32, 32, 16, 32, 1),
                 (cs.BF16, cs.PLAIN, 1, 32, 32, 12, 32, 3), (cs.F32, cs.CONCAT, 1, 32, 32, 8, 32, 3)]:
        with pytest.raises(_lib.SequitrHipError):
            cs.plan(*args)


def expected_plans():
    """every (family, form, BN, KC, K) the dispatchers can produce ("l0", Cout: the f32 level-0 kernel), and the
    (family, form, BN) that need a case whose last channel block is partial"""
    want = set()
    bns, kcs = (16, 32, 64), (8, 16, 32)
    for bn in bns:
        for kc in kcs:
            for fam in (cs.BF16, cs.MIXED):
                for K in (1, 3):
                    want |= {(fam, cs.PLAIN, bn, kc, K), (fam, cs.ACTGATE, bn, kc, K)}
            # the fused epilogues exist on bf16 tensors, at K = 3 only; the pixel norm at every width since it picks BN by Cout
            for form in (cs.POOL, cs.MASK, cs.MASKGATE, cs.JUNCTION, cs.PIXELNORM):
                want.add((cs.BF16, form, bn, kc, 3))
        for kc in (8, 16):
            want |= {(cs.F32, cs.PLAIN, bn, kc, 1), (cs.F32, cs.PLAIN, bn, kc, 3)}
        want |= {(cs.F32, cs.CONCAT, bn, 16, 3), (cs.F32, cs.POOL, bn, 16, 3)}
    want.add((cs.BF16, cs.FIRSTBLOCK, 16, 16, 3))           # FORM_FP: the 16-channel level-0 block only
    want |= {(cs.F32, cs.PLAIN, 32, 32, 3),                 # the stage-32 <32,3,32> form
             (cs.F32, cs.PLAIN, "l0", 16, 3), (cs.F32, cs.PLAIN, "l0", 32, 3), (cs.F32, cs.POOL, "l0", 16, 3)}
    partial = set()
    for fam, form, bn, kc, K in want:
        if bn == "l0" or form == cs.FIRSTBLOCK or (form in (cs.MASK, cs.MASKGATE) and bn == 16):
            continue                                        # 16 / 32 channels, or Cout % 16 == 0 on 16-channel blocks
        partial.add((fam, form, bn))
    return want, partial


def test_the_sweep_reaches_every_plan():
    got, svals = cs.reached()
    reached = {g[:5] for g in got}
    want, partial = expected_plans()
    assert not want - reached, "plans no sweep case runs: %s" % sorted(want - reached, key=str)
    assert not reached - want, "the sweep reaches plans the expected set does not list: %s" % sorted(reached - want, key=str)
    part = {g[:3] for g in got if g[5]}
    assert not partial - part, "(family, form, BN) without a partial last channel block: %s" % sorted(partial - part, key=str)
    assert svals == {1, 2, 4, 8}, svals


SWITCHES = {   # switch: (query, its value without the switch, its value with the switch at 0)
    "SQ_CONV_BF16_NARROW": ("cs.plan(cs.BF16, cs.PLAIN, 1, 16, 16, 32, 64, 3)['bn']", 16, 64),
    "SQ_CONV_STAGE32": ("cs.plan(cs.F32, cs.PLAIN, 1, 250, 262, 32, 48, 3)['kc']", 32, 16),
    "SQ_CONV_L0": ("cs.plan(cs.F32, cs.PLAIN, 2, 64, 80, 16, 32, 3, 'relu')['l0']", 1, 0),
    "SQ_CONV_SPLITK": ("cs.plan(cs.BF16, cs.PLAIN, 8, 4, 4, 512, 36, 3, mosaic=(2, 4), workspace_bytes=1 << 24)['s']", 8, 1),
}


@pytest.mark.parametrize("name", sorted(SWITCHES))
def test_environment_switches_act_on_the_query(name):
    """the launchers read most switches once per process: a fresh interpreter per setting"""
    query, default, off = SWITCHES[name]
    code = "import sys; sys.path.insert(0, %r); from tests import conv_sweep_cases as cs; print(%s)" % (ROOT, query)
    clean = {k: v for k, v in os.environ.items() if k != name}
    for env, want in ((clean, default), (dict(clean, **{name: "0"}), off)):
        r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        assert int(r.stdout.split()[-1]) == want, (name, env.get(name), r.stdout)
