"""Case tables of the convolution sweep (tests/test_gpu_conv_sweep.py) and the launch plans they reach.

A plain module: the CPU suite reads the same tables through sq_conv_plan (tests/test_conv_plan.py) to check that every
(family, form, BN, KC, K) the dispatchers can produce -- and every split-K factor of the mosaic launch -- is run by a case."""
import ctypes

from sequitr_amd import _lib

BF16, MIXED, F32 = 0, 1, 2                                     # SQ_PLAN_* families
PLAIN, JUNCTION, POOL, MASK, MASKGATE, ACTGATE, FIRSTBLOCK, PIXELNORM, CONCAT = 0, 1, 2, 3, 4, 5, 8, 9, 10
ACT = {None: 0, "relu": 1, "leaky": 2}
WSCALE = 1                                                     # SQ_PLAN_WSCALE


def plan(family, form, N, H, W, Cin, Cout, K=3, act=None, wscale_one=True, mosaic=None, workspace_bytes=0):
    """dict(bn, kc, gy, s, l0) of the launch the call would make (sq_conv_plan); raises where no kernel takes it"""
    lib = _lib.load()
    out = (ctypes.c_int * 5)()
    mos = (ctypes.c_int * 2)(*mosaic) if mosaic is not None else None
    rc = lib.sq_conv_plan(family, form, N, H, W, Cin, Cout, K, ACT[act], 0 if wscale_one else WSCALE,
                          ctypes.cast(mos, ctypes.c_void_p) if mos is not None else None, int(workspace_bytes),
                          ctypes.cast(out, ctypes.c_void_p))
    if rc != 0:
        raise _lib.SequitrHipError("sq_conv_plan: %s" % lib.sq_last_error().decode())
    return dict(bn=out[0], kc=out[1], gy=out[2], s=out[3], l0=out[4])


def mosaic_grid(N, h, w):
    """the (R, Cc) cell grid ops._mosaic_plan picks for N images of h x w"""
    best = None
    for cc in range(1, N + 1):
        r = -(-N // cc)
        tiles = -(-(r * (h + 1)) // 16) * -(-(cc * (w + 1)) // 16)
        if best is None or tiles < best[0]:
            best = (tiles, r, cc)
    return best[1], best[2]


def splitk_room(N, h, w, Cout):
    """the split-K workspace ops_gan_bf16 offers a mosaic conv (room for 8 slices)"""
    return 8 * N * h * w * Cout * 4


# Shapes by block width.  BN 16: small ragged images (the dispatcher narrows); BN 32 / 64: 272 - 544 pixel tiles x gy >= 2
# keep the starting width.  Cout leaves the last channel block partial: 24 at BN 16, 48 at BN 32, 80 at BN 64 (multiples of 16
# for the mask forms), plus Cout % 8 == 4 (20 / 36 / 100) on the plain form.
CIN_OF_KC = {8: (8, 24), 16: (16, 48), 32: (32, 64)}
SMALL = [(1, 35, 21), (2, 21, 19), (1, 19, 37)]
WIDE = [(1, 250, 262), (1, 256, 259), (1, 249, 264)]
PARTIAL_COUT = {16: 24, 32: 48, 64: 80}
ACTS = ["relu", "leaky", None]


def _shape(bn, i):
    return SMALL[i % 3] if bn == 16 else WIDE[i % 3]


# ---- bf16 forward, plain form: (N, H, W, Cin, Cout, K, act, bias) -- every BN x KC x K, a partial and a full last block
BF16_PLAIN = []
for _bn in (16, 32, 64):
    for _kc in (8, 16, 32):
        for _k in (1, 3):
            _i = len(BF16_PLAIN)
            _N, _H, _W = _shape(_bn, _i)
            _cin = CIN_OF_KC[_kc][_i % 2]
            BF16_PLAIN.append((_N, _H, _W, _cin, PARTIAL_COUT[_bn], _k, ACTS[_i % 3], _i % 4 != 3))
            BF16_PLAIN.append((_N, _H, _W, _cin, _bn if _bn > 16 else 32, _k, ACTS[(_i + 1) % 3], True))
BF16_PLAIN += [
    (1, 1, 83, 8, 16, 3, "relu", True), (1, 45, 1, 48, 16, 3, None, False),     # a single row, a single column
    (2, 21, 19, 24, 20, 3, "leaky", True), (1, 30, 33, 64, 36, 1, None, True),  # Cout % 8 == 4 at BN 16
    (1, 256, 250, 32, 36, 3, "relu", True),                                     # ... at BN 32 (gy 2)
    (1, 256, 250, 16, 100, 3, None, True),                                      # ... at BN 64 (gy 2)
]

# ---- wide grids: ntiles > 2048 / gy, so that every block walks >= 2 tiles at any occupancy <= 8, ntiles not a multiple of
# the grid.  (4, 250, 264): 4 x 16 x 17 = 1088 tiles.
BF16_WIDE = [
    (4, 250, 264, 16, 64, 3, "relu", True),            # 1088 tiles x gy 1 (BN 64)
    (2, 256, 264, 8, 256, 3, "leaky", True),           # 544 tiles x gy 4 (BN 64)
    (4, 250, 264, 16, 48, 3, None, True),              # 1088 tiles x gy 2 (BN 32, partial last block)
    (2, 128, 264, 8, 252, 3, "relu", True),            # 136 tiles x gy 4 (BN 64 kept by gy alone, Cout % 8 == 4)
]

# ---- every epilogue form at every BN x KC: (form, N, H, W, Cin, Cout), the last channel block partial where the form allows
# (the mask forms need Cout % 16 == 0).  The dgrad forms' (Cin, Cout) are those of the dgrad conv.  Pixel norm picks its width
# from Cout alone (8 -> 16, 24 -> 32, 40 / 48 / 56 -> 64) and keeps small images.
FORM_CASES = []
for _form in (POOL, MASK, MASKGATE, JUNCTION, ACTGATE, PIXELNORM):
    for _bn in (16, 32, 64):
        for _j, _kc in enumerate((8, 16, 32)):
            _i = len(FORM_CASES)
            _N, _H, _W = _shape(_bn, _i)
            if _form in (POOL, JUNCTION):                   # even sides
                _H, _W = _H + _H % 2, _W + _W % 2
            _cout = PARTIAL_COUT[_bn]
            if _form in (MASK, MASKGATE) and _bn == 16:
                _cout = 16
            if _form == PIXELNORM:
                _N, _H, _W = (2, 34, 22) if _j != 1 else (1, 19, 37)
                _cout = {16: 8, 32: 24, 64: (40, 48, 56)[_j]}[_bn]
            FORM_CASES.append((_form, _N, _H, _W, CIN_OF_KC[_kc][_i % 2], _cout))
for _bn in (16, 32, 64):                                # the act-gated dgrad also exists as a 1x1 form
    for _kc in (8, 16, 32):
        _i = len(FORM_CASES)
        FORM_CASES.append(("actgate1",) + _shape(_bn, _i) + (CIN_OF_KC[_kc][_i % 2], PARTIAL_COUT[_bn]))
FORM_CASES += [
    ("avgpool", 2, 256, 264, 16, 40), ("avgpool", 1, 250, 262, 32, 80), ("avgpool", 1, 34, 22, 16, 24),
    ("relugate", 1, 250, 262, 32, 48), ("relugate", 1, 250, 263, 16, 80), ("relugate", 1, 21, 35, 16, 20),
    ("dropgate", 1, 250, 264, 16, 40), ("dropgate", 1, 249, 264, 32, 64),
    ("dropout", 1, 256, 264, 16, 40), ("dropout", 1, 249, 262, 32, 80), ("dropout", 2, 21, 19, 8, 20),
    (FIRSTBLOCK, 2, 34, 50, 16, 16),
]
JUNCTION_KINDS = ["eltwise_mul", "eltwise_add", "eltwise_sub"]

# ---- mixed (f32 tensors, bf16 operands): the plain table through ops.conv2d under mixed_precision() (channel counts the
# mixed entry takes), and the act-gated dgrad at every BN x KC: (N, H, W, Cin, Cout, K) of the dgrad conv
MIXED_PLAIN = [c for c in BF16_PLAIN if c[3] % 8 == 0 and c[4] % 4 == 0]
MIXED_DGRAD = []
for _bn in (16, 32, 64):
    for _kc in (8, 16, 32):
        for _k in (1, 3):
            _i = len(MIXED_DGRAD)
            MIXED_DGRAD.append(_shape(_bn, _i) + (CIN_OF_KC[_kc][_i % 2], PARTIAL_COUT[_bn], _k))

# ---- mosaic and split-K: (Nimg, h, w, Cin, Cout, gated); S as sq_conv_plan reports it with room for 8 slices
MOSAIC = [
    (32, 4, 4, 512, 512, False),     # S 1 (enough blocks)
    (8, 4, 4, 512, 36, True),        # S 8, Cout tail
    (6, 4, 4, 64, 20, False),        # S 2
    (16, 8, 8, 128, 48, True),       # S 2
    (4, 4, 4, 128, 52, False),       # S 4
    (8, 8, 8, 256, 40, False),       # S 4
    (8, 4, 4, 256, 20, True),        # S 8
    (5, 7, 5, 48, 24, True),         # S 1 (KC 16, three chunks)
]
MIXED_MOSAIC = [(32, 4, 4, 64, 36, False), (7, 8, 8, 32, 48, True), (16, 4, 4, 24, 16, True)]

# ---- f32 v2, bit-exact against the C oracle: (form, N, H, W, Cin, Cout, K, act) -- every BN x KC x K of the plain form at
# ragged shapes, the stage-32 <32,3,32> path (BN 32, Cin % 32 == 0), the level-0 kernel, concat and pooled forms
F32_CASES = []
for _bn in (16, 32, 64):
    for _cin in (8, 16, 48):
        for _k in (1, 3):
            _i = len(F32_CASES)
            _N, _H, _W = _shape(_bn, _i)
            F32_CASES.append((PLAIN, _N, _H, _W, _cin, (PARTIAL_COUT[_bn], 96 if _bn == 64 else 40)[_i % 2], _k, ACTS[_i % 3]))
F32_CASES += [
    (PLAIN, 1, 250, 262, 32, 48, 3, "leaky"),        # BN 32, stage-32
    (PLAIN, 1, 256, 264, 64, 40, 3, "relu"),         # BN 32, stage-32, Cout tail
    (PLAIN, 2, 64, 80, 16, 32, 3, "relu"),           # the level-0 kernel (32 channels)
    (PLAIN, 2, 64, 80, 16, 16, 3, "relu"),           # the level-0 kernel (16 channels)
    (CONCAT, 1, 250, 262, 32, 80, 3, "relu"),        # BN 64 over the two sources
    (CONCAT, 1, 256, 264, 32, 48, 3, None),          # BN 32 (no stage-32 with two sources)
    (CONCAT, 1, 35, 21, 32, 24, 3, "leaky"),         # BN 16
    (POOL, 1, 250, 262, 32, 80, 3, "relu"),          # BN 64 pooled
    (POOL, 1, 256, 262, 16, 48, 3, "relu"),          # BN 32 pooled
    (POOL, 2, 36, 22, 16, 24, 3, "leaky"),           # BN 16 pooled
    (POOL, 2, 64, 48, 16, 16, 3, "relu"),            # the level-0 pooled kernel
]


def bf16_form_of(name):
    """plan form of a FORM_CASES entry (the gate / dropout / avg-pool variants run the plain or pooled instantiation)"""
    return {"avgpool": POOL, "relugate": PLAIN, "dropgate": PLAIN, "dropout": PLAIN, "actgate1": ACTGATE}.get(name, name)


def reached():
    """{(family, form, BN, KC, K)} the sweep runs, and the set of mosaic split-K factors"""
    got, svals = set(), set()
    for (N, H, W, Cin, Cout, K, act, _) in BF16_PLAIN + BF16_WIDE:
        p = plan(BF16, PLAIN, N, H, W, Cin, Cout, K, act)
        got.add((BF16, PLAIN, p["bn"], p["kc"], K, Cout % p["bn"] != 0))
    for (form, N, H, W, Cin, Cout) in FORM_CASES:
        f, K = bf16_form_of(form), 1 if form == "actgate1" else 3
        p = plan(BF16, f, N, H, W, Cin, Cout, K, "relu")
        got.add((BF16, f, p["bn"], p["kc"], K, Cout % p["bn"] != 0))
    for (N, H, W, Cin, Cout, K, act, _) in MIXED_PLAIN:
        p = plan(MIXED, PLAIN, N, H, W, Cin, Cout, K, act)
        got.add((MIXED, PLAIN, p["bn"], p["kc"], K, Cout % p["bn"] != 0))
    for (N, H, W, Cin, Cout, K) in MIXED_DGRAD:
        p = plan(MIXED, ACTGATE, N, H, W, Cin, Cout, K, "leaky")
        got.add((MIXED, ACTGATE, p["bn"], p["kc"], K, Cout % p["bn"] != 0))
    for (n, h, w, Cin, Cout, gated) in MOSAIC:
        p = plan(BF16, ACTGATE if gated else PLAIN, n, h, w, Cin, Cout, 3, "leaky", mosaic=mosaic_grid(n, h, w),
                 workspace_bytes=splitk_room(n, h, w, Cout))
        svals.add(p["s"])
    for (form, N, H, W, Cin, Cout, K, act) in F32_CASES:
        p = plan(F32, form, N, H, W, Cin, Cout, K, act)
        got.add((F32, form, p["bn"], p["kc"], K, Cout % p["bn"] != 0) if not p["l0"] else (F32, form, "l0", Cout, K, False))
    return got, svals
