"""CPU: the tile walks of the persistent f32 inference kernels (sq_conv_walk_plan, from the host functions launch_l0, launch_v2
and launch_ct take their grids from).  The walks of the benchmark's batch are pinned, and every case of the walk sweep
(tests/f32_walk_cases.py, run on the GPU by tests/test_gpu_f32_walk_sweep.py) must reach the regime it is there for: the seam
code between two tiles of a block only runs where a block has more than one tile."""
import os
import subprocess
import sys

import pytest

from sequitr_amd import _lib
from tests import conv_sweep_cases as cs
from tests import f32_walk_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def walks_seams(p):
    """a block with both kinds of prefetch (one and two tiles ahead) in flight, and blocks that stop at different tiles"""
    return p["tmax"] >= 3 and p["tmin"] < p["tmax"]


def test_walk_counts_are_those_of_the_kernels():
    """tmin / tmax against the kernels' own t_count = (items - vb + G - 1) / G over every block, the stride triple against
    tile + G decoded by division"""
    calls = [(wc.PLAIN, 3, 96, 80, 16, 16, "relu"), (wc.PLAIN, 2, 368, 736, 16, 16, "relu"), (wc.UP, 4, 320, 416, 16, 16, "relu"),
             (wc.PLAIN, 2, 250, 262, 32, 80, None), (wc.HEAD, 2, 366, 730, 16, 16, "leaky"), (wc.CONVT, 2, 60, 183, 64, 96, None)]
    for (form, N, H, W, ci, co, act) in calls:
        p = wc.walk(form, N, H, W, ci, co, 3, act, head_c=3 if form == wc.HEAD else 0)
        counts = [wc.block_count(p, b) for b in range(p["G"])]
        assert (min(counts), max(counts)) == (p["tmin"], p["tmax"]) and sum(counts) == p["items"], (form, p)
        if form != wc.CONVT:
            tx, ty = -(-W // 16), -(-H // 16)
            assert p["items"] == N * tx * ty and p["tilepx"] == 256
            assert p["G"] == (p["gn"] * ty + p["gy"]) * tx + p["gx"] and p["gx"] < tx and p["gy"] < ty
            for b in range(p["G"]):
                wc.carries_of_block(p, tx, ty, b)           # asserts every step lands on tile b + k G


def test_inference_batch_walks_are_pinned():
    """32 x 512^2 (bench.py): kernel, G, tiles of the idlest / busiest block, channel blocks"""
    got = {
        "down0 first+pool": wc.walk(wc.FIRST, 32, 512, 512, 1, 16, 3, "relu", pooled=True),
        "down1/conv1": wc.walk(wc.PLAIN, 32, 256, 256, 16, 32, 3, "relu"),
        "down1/conv2+pool": wc.walk(wc.POOL, 32, 256, 256, 32, 32, 3, "relu"),
        "down2/conv2+pool": wc.walk(wc.POOL, 32, 128, 128, 64, 64, 3, "relu"),
        "down4/conv2": wc.walk(wc.PLAIN, 32, 32, 32, 256, 256, 3, "relu"),
        "up0 convT+conv1": wc.walk(wc.UP, 32, 512, 512, 16, 16, 3, "relu"),
        "up0 conv2+head": wc.walk(wc.HEAD, 32, 512, 512, 16, 16, 3, "relu", head_c=2),
        "up3/upscale": wc.walk(wc.CONVT, 32, 32, 32, 256, 128),
        "up1/upscale": wc.walk(wc.CONVT, 32, 128, 128, 64, 32),
    }
    got = {k: (p["kernel"], p["G"], p["tmin"], p["tmax"], p["cblocks"], p["mtiles"]) for k, p in got.items()}
    assert got == {
        "down0 first+pool": (wc.L0, 1024, 32, 32, 1, 0), "down1/conv1": (wc.L0, 512, 16, 16, 1, 0),
        "down1/conv2+pool": (wc.V2, 512, 16, 16, 1, 0), "down2/conv2+pool": (wc.V2, 512, 4, 4, 1, 0),
        "down4/conv2": (wc.V2, 128, 1, 1, 4, 0), "up0 convT+conv1": (wc.L0, 512, 64, 64, 1, 0),
        "up0 conv2+head": (wc.L0, 1024, 32, 32, 1, 0), "up3/upscale": (wc.CT, 1024, 4, 4, 1, 4),
        "up1/upscale": (wc.CT, 1024, 16, 16, 1, 1),
    }


def test_which_kernel_walks():
    assert wc.walk(wc.PLAIN, 2, 64, 80, 16, 16, 3, "relu")["kernel"] == wc.L0
    assert wc.walk(wc.PLAIN, 2, 64, 80, 16, 16, 3, "leaky")["kernel"] == wc.V2             # ReLU only
    assert wc.walk(wc.PLAIN, 2, 64, 80, 16, 16, 3, "relu", wscale_one=False)["kernel"] == wc.V2
    assert wc.walk(wc.PLAIN, 2, 64, 82, 16, 16, 3, "relu")["kernel"] == wc.V2              # multiples of 16 only
    assert wc.walk(wc.POOL, 2, 64, 80, 16, 32, 3, "relu")["kernel"] == wc.V2
    assert wc.walk(wc.HEAD, 2, 64, 80, 16, 16, 3, "relu", head_c=2)["kernel"] == wc.L0
    assert wc.walk(wc.HEAD, 2, 64, 80, 16, 16, 3, "relu", head_c=3)["kernel"] == wc.V2     # two classes only
    assert wc.walk(wc.HEAD, 2, 64, 80, 32, 16, 3, "relu", head_c=2)["kernel"] == wc.V2
    assert wc.walk(wc.UP, 2, 64, 80, 16, 16, 3, "relu")["kernel"] == wc.L0
    assert wc.walk(wc.UP, 2, 62, 80, 16, 16, 3, "relu")["kernel"] == wc.V2
    assert wc.walk(wc.FIRST, 2, 64, 80, 1, 16, 3, "relu", pooled=True)["kernel"] == wc.L0
    assert wc.walk(wc.CONCAT, 2, 64, 80, 32, 16, 3, "relu")["kernel"] == wc.V2
    # the transpose conv v2 takes Cin, Cout multiples of 32; anything else has no walk
    assert wc.walk(wc.CONVT, 2, 9, 13, 64, 32)["kernel"] == wc.CT
    for cin, cout in ((48, 32), (64, 48), (16, 8)):
        p = wc.walk(wc.CONVT, 2, 9, 13, cin, cout)
        assert p["kernel"] == wc.NONE and not any(p[k] for k in wc.FIELDS[1:])
    for args in [(wc.UP, 1, 31, 32, 16, 16), (wc.POOL, 1, 32, 31, 16, 16), (wc.PLAIN, 1, 32, 32, 12, 16), (wc.FIRST, 1, 32, 32, 16, 16),
                 (wc.HEAD, 1, 32, 32, 16, 32), (wc.CONCAT, 1, 32, 32, 16, 16), (7, 1, 32, 32, 16, 16)]:
        with pytest.raises(_lib.SequitrHipError):
            wc.walk(*args, head_c=2 if args[0] == wc.HEAD else 0)


def test_level0_cases_walk_every_seam(monkeypatch):
    """each of the level-0 instantiations at two shapes: three or more tiles in a block, uneven walks, a stride with a column
    and a row part on a grid that is not square, and one block whose walk has all three carries of advance() -- the column alone
    (no carry), the column into the row, the row into the image; N >= 2.  Under SQ_CONV_L0=0 the same cases walk the generic
    kernel's seams."""
    monkeypatch.delenv("SQ_CONV_L0", raising=False)
    forms = {}
    for c in wc.L0_CASES:
        tx, ty = wc.tiles_xy(c)
        p = wc.walk_of(c)
        assert p["kernel"] == wc.L0 and p["G"] == (512 if c.form == wc.UP or c.Cout == 32 else 1024), (c, p)
        assert walks_seams(p), (c, p)
        assert p["gx"] and p["gy"] and tx != ty and c.N >= 2, (c, p)
        assert wc.blocks_with_every_carry(p, tx, ty), (c, p)
        assert any(t // (tx * ty) != (t + p["G"]) // (tx * ty) for t in range(p["items"] - p["G"])), "no walk crosses an image"
        forms.setdefault((c.form, c.Cout, c.opt), set()).add((c.N, c.H, c.W))
    want = {(wc.PLAIN, 16, None), (wc.PLAIN, 32, None), (wc.POOL, 16, None), (wc.HEAD, 16, 2), (wc.FIRST, 16, True),
            (wc.FIRST, 16, False)} | {(wc.UP, 16, b) for b in wc.BRIDGES}
    assert set(forms) == want and all(len(s) == 2 for s in forms.values()), forms
    assert {c.bias for c in wc.L0_CASES} == {"rand", "zero", None}
    monkeypatch.setenv("SQ_CONV_L0", "0")
    for c in wc.L0_CASES:
        p = wc.walk_of(c)
        assert p["kernel"] == wc.V2 and walks_seams(p), (c, p)


def test_ragged_cases_walk_the_generic_forms(monkeypatch):
    """UP (every bridge), FIRST with and without pool, the head at 1, 2 and 3 classes and the plain 16-channel-block form with
    two input chunks, at a shape the level-0 kernel declines by itself"""
    monkeypatch.delenv("SQ_CONV_L0", raising=False)
    got = set()
    for c in wc.RAGGED_CASES:
        p = wc.walk_of(c)
        assert c.H % 16 and c.W % 16 and c.H % 2 == 0 and c.W % 2 == 0, c
        assert p["kernel"] == wc.V2 and p["cblocks"] == 1 and walks_seams(p), (c, p)
        got.add((c.form, c.opt))
        if c.form == wc.PLAIN:
            assert cs.plan(cs.F32, cs.PLAIN, c.N, c.H, c.W, c.Cin, c.Cout, 3, c.act) == dict(bn=16, kc=16, gy=1, s=1, l0=0)
            assert c.Cin // 16 >= 2
    assert got == {(wc.UP, b) for b in wc.BRIDGES} | {(wc.FIRST, True), (wc.FIRST, False), (wc.HEAD, 1), (wc.HEAD, 2), (wc.HEAD, 3),
                                                      (wc.PLAIN, None)}
    for form in (wc.UP, wc.HEAD, wc.PLAIN):                 # the forms that take an activation also run without ReLU
        assert {c.act for c in wc.RAGGED_CASES if c.form == form} - {"relu"}, form


def test_wide_cases_walk_the_wide_blocks():
    got = set()
    for c, bn, kc, gy in wc.WIDE_CASES:
        p = wc.walk_of(c)
        q = cs.plan(cs.F32, c.form, c.N, c.H, c.W, c.Cin, c.Cout, 3, c.act)
        assert (q["bn"], q["kc"], q["gy"], q["l0"]) == (bn, kc, gy, 0), (c, q)
        assert p["kernel"] == wc.V2 and p["cblocks"] == gy and walks_seams(p), (c, p)
        assert c.Cout % bn, "the last channel block is partial"
        got.add((c.form, bn, kc))
        if (c.form, bn) == (wc.PLAIN, 64):
            assert gy == 2 and c.Cin // kc >= 2
    assert got == {(wc.PLAIN, 64, 16), (wc.PLAIN, 32, 16), (wc.PLAIN, 32, 32), (wc.CONCAT, 64, 16), (wc.POOL, 32, 16)}


def test_convT_cases_walk_every_row_tile_count():
    """row tiles 1 .. 5 at the default 32-pixel tiles: more than 2 G work items, a ragged last pixel tile, several chunks;
    every bridge at 3 and 4 row tiles, mul / none at the others"""
    bridges = {}
    for c in wc.CONVT_CASES:
        p = wc.walk_of(c)
        assert p["kernel"] == wc.CT and p["tilepx"] == 32, (c, p)
        assert p["mtiles"] == c.Cout // 32 and p["G"] % p["mtiles"] == 0, (c, p)
        assert p["items"] > 2 * p["G"] and walks_seams(p), (c, p)
        assert (c.N * c.H * c.W) % 32 != 0 and c.Cin >= 64, c
        bridges.setdefault(p["mtiles"], set()).add(c.opt)
    assert bridges == {1: {"eltwise_mul", None}, 2: {"eltwise_mul", None}, 3: set(wc.BRIDGES), 4: set(wc.BRIDGES),
                       5: {"eltwise_mul", None}}
    assert wc.walk_of(next(c for c in wc.CONVT_CASES if c.Cout == 96))["G"] == 1023      # trimmed to a multiple of 3


def test_transpose_conv_tile_width_switch_acts_on_the_walk():
    """SQ_CONVT_WNI is read once per process: a fresh interpreter per setting"""
    code = ("import sys; sys.path.insert(0, %r); from tests import f32_walk_cases as wc; "
            "p = wc.walk(wc.CONVT, 1, 90, 183, 256, 128); print(p['tilepx'], p['G'], p['tmax'])" % ROOT)
    clean = {k: v for k, v in os.environ.items() if k not in ("SQ_CONVT_WNI", "SQ_CONVT_V2")}
    for wni, want in ((None, (32, 1024, 3)), ("2", (64, 768, 2)), ("4", (128, 512, 2))):
        env = dict(clean, SQ_CONVT_WNI=wni) if wni else clean
        r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        assert tuple(int(v) for v in r.stdout.split()[-3:]) == want, (wni, r.stdout)


def test_a_mismatch_names_its_tile_and_its_place_in_the_walk(monkeypatch):
    """the report of the GPU sweep, on arrays made to differ in one known tile"""
    import numpy as np
    from tests.test_gpu_f32_walk_sweep import where
    monkeypatch.delenv("SQ_CONV_L0", raising=False)
    c = wc.L0_CASES[0]
    p, (tx, ty) = wc.walk_of(c), wc.tiles_xy(c)
    t = 5 + 2 * p["G"]                                      # the third tile of block 5
    n, tyi, txi = t // (tx * ty), (t // tx) % ty, t % tx
    ref = np.zeros((c.N, c.H, c.W, 16), np.float32)
    got = ref.copy()
    got[n, 16 * tyi + 3, 16 * txi + 15, 2] = 1.0
    msg = where(got, ref, c, p, "y")
    assert "tile (n %d, ty %d, tx %d), item 2 of 3 of block 5 (of 1024 blocks)" % (n, tyi, txi) in msg, msg
    assert "[((2, 3), 1)]" in msg, msg
    got[n, 16 * tyi + 4, 16 * txi + 14, 2] = 1.0            # pooled pixel (y, x) lies in the tile of (2y, 2x)
    msg = where(np.ascontiguousarray(got[:, ::2, ::2]), np.ascontiguousarray(ref[:, ::2, ::2]), c, p, "pooled")
    assert "tile (n %d, ty %d, tx %d), item 2 of 3 of block 5" % (n, tyi, txi) in msg, msg
    c = next(k for k in wc.CONVT_CASES if k.Cout == 96)
    p = wc.walk_of(c)
    item = 7 + p["G"]                                       # the second item of block 7: row tile 1 of its pixel tile
    pt, rt = item // 3, item % 3
    assert (rt, p["G"]) == (1, 1023)
    pix = 32 * pt + 9                                       # an input pixel of the tile, and row 128 + 40 = tap 1, channel 72
    n, i, j = pix // (c.H * c.W), (pix // c.W) % c.H, pix % c.W
    ref = np.zeros((c.N, 2 * c.H, 2 * c.W, c.Cout), np.float32)
    got = ref.copy()
    got[n, 2 * i, 2 * j + 1, 72] = 1.0
    msg = where(got, ref, c, p, "y")
    assert "row tile 1, pixel tile %d, item 1 of 3 of block 7 (of 1023 blocks)" % pt in msg, msg
