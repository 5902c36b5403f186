"""Case tables of the weight-gradient sweep (tests/test_gpu_wgrad_sweep.py) and the launch plans they reach.

A plain module: the CPU suite reads the same tables through sq_wgrad_plan / sq_wgrad_group_plan (tests/test_wgrad_plan.py) to
check that every block shape, kind and prefetch phase the dispatchers can produce is run by a case.  A case is a dict:
fam ("bf16", "mixed", "f32", "first": the small-Cin kernel with a bf16 dY), N, H, W, Cin, Cout (the kernel's: 4 * convT for a
transpose conv), K, mosaic (R, Cc) or None, convT (its Cout) or 0, scale (dw_scale), bias (db wanted)."""
import ctypes

from sequitr_amd import _lib

BF16, MIXED, F32 = 0, 1, 2                                     # SQ_PLAN_* families
PLAIN, MOSAIC, RAGGED, CONVT, F32K, F32SMALL = 0, 1, 2, 3, 4, 5   # SQ_WGP_* kinds
FAMILY = {"bf16": BF16, "mixed": MIXED, "f32": F32, "first": F32}
FIELDS = ("ks", "ni", "no", "kind", "pf", "npairs", "gx", "tpb", "g", "ws")
GROUP_MAX = 16


def plan(fam, N, H, W, Cin, Cout, K, mosaic=None, convT=0):
    """dict of FIELDS: the launch a one-layer call would make (sq_wgrad_plan); raises where no kernel takes it"""
    lib = _lib.load()
    out = (ctypes.c_int64 * len(FIELDS))()
    mos = (ctypes.c_int * 2)(*mosaic) if mosaic else None
    rc = lib.sq_wgrad_plan(FAMILY[fam], N, H, W, Cin, Cout, K, ctypes.cast(mos, ctypes.c_void_p) if mos else None, convT,
                           ctypes.cast(out, ctypes.c_void_p))
    if rc != 0:
        raise _lib.SequitrHipError("sq_wgrad_plan: %s" % lib.sq_last_error().decode())
    return dict(zip(FIELDS, out))


def case_plan(c):
    return plan(c["fam"], c["N"], c["H"], c["W"], c["Cin"], c["Cout"], c["K"], c.get("mosaic"), c.get("convT", 0))


def items_array(items, ptrs=None):
    """sq_wgrad_item array of group items (dicts: N, H, W, Cin, Cout, K, convT, scale, acc, mosaic, dw, db -- dw / db name a
    destination: items with the same name share it).  ptrs: {name: address}; without, distinct fake addresses (plan only)."""
    arr = (_lib.WgradItem * len(items))()
    fake = {}
    for i, it in enumerate(items):
        def addr(name):
            return ptrs[name] if ptrs is not None else fake.setdefault(name, 0x10000 * (len(fake) + 1))
        a = arr[i]
        a.x, a.dy = addr(("x", i)), addr(("dy", i))
        a.dw = addr(it["dw"])
        a.db = addr(it["db"]) if it.get("db") else None
        a.N, a.H, a.W, a.Cin, a.Cout, a.K = it["N"], it["H"], it["W"], it["Cin"], it["Cout"], it["K"]
        a.convT_cout, a.dw_scale, a.accumulate = it.get("convT", 0), it.get("scale", 1.0), it.get("acc", 0)
        R, Cc = it.get("mosaic") or (0, 0)
        a.mosaic_R, a.mosaic_Cc = R, Cc
    return arr


def group_plan(items):
    """(number of launches, [dict of FIELDS + bucket, pair_major, offset] per item) of sq_wgrad_group_plan"""
    lib = _lib.load()
    n = len(items)
    out = (ctypes.c_int64 * (n * (len(FIELDS) + 3)))()
    nbk = lib.sq_wgrad_group_plan(items_array(items), n, ctypes.cast(out, ctypes.c_void_p))
    if nbk < 0:
        raise _lib.SequitrHipError("sq_wgrad_group_plan: %s" % lib.sq_last_error().decode())
    res = []
    for i in range(n):
        o = list(out[i * (len(FIELDS) + 3):(i + 1) * (len(FIELDS) + 3)])
        d = dict(zip(FIELDS, o[1:1 + len(FIELDS)]))
        d.update(bucket=o[0], pair_major=o[-2], offset=o[-1])
        res.append(d)
    return nbk, res


def mosaic_grid(N, h, w):
    """the (R, Cc) cell grid ops._mosaic_plan picks for N images of h x w"""
    best = None
    for cc in range(1, N + 1):
        r = -(-N // cc)
        tiles = -(-(r * (h + 1)) // 16) * -(-(cc * (w + 1)) // 16)
        if best is None or tiles < best[0]:
            best = (tiles, r, cc)
    return best[1], best[2]


def block_counts(p, ntiles):
    """tiles walked by each tile range of plan p over ntiles tiles (interleaved: block b takes b, b + gx, ...)"""
    gx, t = p["gx"], p["tpb"]
    if t < 0:
        return [-(-(ntiles - b) // gx) for b in range(gx)]
    return [max(0, min(t, ntiles - b * t)) for b in range(gx)]


def _c(fam, N, H, W, Cin, Cout, K, mosaic=None, convT=0, scale=1.0, bias=True):
    return dict(fam=fam, N=N, H=H, W=W, Cin=Cin, Cout=Cout, K=K, mosaic=mosaic, convT=convT, scale=scale, bias=bias)


def tiles_of(c):
    if c.get("mosaic"):
        R, Cc = c["mosaic"]
        return -(-(R * (c["H"] + 1)) // 16) * -(-(Cc * (c["W"] + 1)) // 16)
    return -(-c["H"] // 16) * -(-c["W"] // 16) * c["N"]


def counts_of(c):
    return block_counts(case_plan(c), tiles_of(c))


def _long_run(fam, H, W, Cin, Cout, K, t, convT=0, mos=False, scale=1.0):
    """the first batch size whose plan walks runs of t and t - 1 tiles (H x W images; mos: as a mosaic of h x w images)"""
    for N in range(1, 4000):
        mosaic = mosaic_grid(N, H, W) if mos else None
        c = _c(fam, N, H, W, Cin, Cout, K, mosaic, convT, scale)
        cnt = counts_of(c)
        if max(cnt) == t and min(cnt) == t - 1:
            return c
    raise AssertionError("no batch size gives runs of %d tiles: %s" % (t, (fam, H, W, Cin, Cout, K, convT, mos)))


# ---- the bf16 / mixed kernel: every default block shape, kind and prefetch phase --------------------------------------------
# channel counts per (K, NI, NO) of the default dispatch (Cin % 32 -> NI 2; Cout % 32 (3x3) or % 64 / % 32 (1x1) -> NO);
# many channel pairs keep the images small while the blocks walk long runs
SHAPES = {(3, 1, 2): (144, 96), (3, 2, 1): (96, 48), (3, 1, 1): (48, 80),
          (1, 2, 4): (160, 192), (1, 2, 2): (96, 224), (1, 2, 1): (160, 80), (1, 1, 2): (80, 160), (1, 1, 1): (112, 48)}
# transpose convs (the 1x1 kernel, Cout = 4 * convT) at the five 1x1 shapes
CONVT_CH = {(1, 2, 4): (64, 48), (1, 2, 2): (96, 40), (1, 2, 1): (64, 12), (1, 1, 2): (48, 24), (1, 1, 1): (80, 4)}
RAGGED_CH = {3: (40, 24), 1: (104, 88)}                           # Cin / Cout 8 mod 16

SINGLE = []
for (K, ni, no), (ci, co) in sorted(SHAPES.items()):
    for fam in ("bf16", "mixed"):
        SINGLE.append(_c(fam, 2, 21, 19, ci, co, K, scale=0.5 if K == 3 else 1.0))          # partial tiles, short runs
        for t in (5, 7):                                        # PF + 1 and two more: every residue of the run mod PF
            SINGLE.append(_long_run(fam, 16, 16, ci, co, K, t, scale=1.0 if t == 5 else 0.25))
    if K == 3:
        for fam in ("bf16", "mixed"):
            SINGLE.append(_c(fam, 5, 4, 4, ci, co, 3, mosaic=mosaic_grid(5, 4, 4)))         # fewer images than cells
            SINGLE.append(_c(fam, 3, 7, 5, ci, co, 3, mosaic=(2, 2), scale=0.5))
            for t in (5, 7):
                SINGLE.append(_long_run(fam, 8, 8, ci, co, 3, t, mos=True))
for (K, ni, no), (ci, c) in sorted(CONVT_CH.items()):
    SINGLE.append(_c("bf16", 2, 13, 22, ci, 4 * c, 1, convT=c))
    for t in (5, 7):
        SINGLE.append(_long_run("bf16", 16, 16, ci, 4 * c, 1, t, convT=c))
for K, (ci, co) in sorted(RAGGED_CH.items()):
    SINGLE.append(_c("bf16", 2, 21, 19, ci, co, K, scale=0.5))
    SINGLE.append(_c("bf16", 1, 17, 33, 8, 24, K, bias=False))
    for t in (5, 7):
        SINGLE.append(_long_run("bf16", 16, 16, ci, co, K, t))
SINGLE.append(_c("bf16", 1, 1, 83, 16, 32, 3))                   # a single row
SINGLE.append(_c("bf16", 1, 45, 1, 32, 16, 3, bias=False))      # a single column

# ---- the f32 kernels: every (BN, KS, KC), each with a partial last channel block; the small-Cin kernel at Cin 1..7 ------------
F32_CASES = []
for K in (1, 3):
    for ci in (8, 48):                                          # KC 8, 16
        for co in (12, 48):                                     # BN 16 (Cout <= 16), BN 32 -- neither divides the block
            F32_CASES.append(_c("f32", 2, 21, 19, ci, co, K, scale=0.5 if co == 48 else 1.0))
            F32_CASES.append(_c("f32", 3, 33, 40, ci, co + 4 if co == 12 else co + 16, K))  # a full last block too
for ci in range(1, 8):
    F32_CASES.append(_c("f32", 2, 35, 21, ci, 20 if ci % 2 else 16, 3, bias=ci != 4))
    F32_CASES.append(_c("first", 2, 21, 35, ci, 16 if ci % 2 else 36, 3, bias=ci != 5))

F32_CASES.append(_long_run("f32", 16, 16, 48, 48, 3, 3))       # the f32 kernel's prefetch over runs of 3 and 2 tiles
F32_CASES.append(_c("f32", 2052, 16, 16, 3, 16, 3))               # the small-Cin kernel's over runs of 2 and 1 (2048 blocks)

CASES = SINGLE + F32_CASES


# ---- the grouped launch -----------------------------------------------------------------------------------------------------
def _gi(N, H, W, Cin, Cout, K, dw, db=None, **kw):
    d = dict(N=N, H=H, W=W, Cin=Cin, Cout=Cout, K=K, dw=dw, db=db)
    d.update(kw)
    return d


def _group_cases():
    g = {}
    # every bucket (kind, KS, NI, NO): plain items of two sizes (different tile counts), a transpose conv among the 1x1 ones
    items = []
    for (K, ni, no), (ci, co) in sorted(SHAPES.items()):
        items.append(_gi(2, 21, 19, ci, co, K, "w%d%d%d" % (K, ni, no), "b%d%d%d" % (K, ni, no), scale=0.5))
        items.append(_gi(9, 16, 16, ci, co, K, "v%d%d%d" % (K, ni, no), "c%d%d%d" % (K, ni, no)))
    for (K, ni, no), (ci, c) in sorted(CONVT_CH.items()):
        items.append(_gi(3, 13, 10, ci, 4 * c, 1, "t%d%d" % (ni, no), "tb%d%d" % (ni, no), convT=c))
    g["plain_and_convT"] = items
    items = []
    for (K, ni, no), (ci, co) in sorted(SHAPES.items()):
        if K == 3:
            items.append(_gi(5, 4, 4, ci, co, 3, "m%d%d" % (ni, no), "mb%d%d" % (ni, no), mosaic=mosaic_grid(5, 4, 4)))
            items.append(_gi(40, 8, 8, ci, co, 3, "n%d%d" % (ni, no), None, mosaic=mosaic_grid(40, 8, 8), scale=2.0))
    for K, (ci, co) in sorted(RAGGED_CH.items()):
        items.append(_gi(2, 21, 19, ci, co, K, "r%d" % K, "rb%d" % K))
        items.append(_gi(1, 40, 40, 8, 24, K, "s%d" % K, None))
    g["mosaic_and_ragged"] = items
    # accumulate: the same destinations written, then accumulate bits 2, 1, 3 in item order -- the last item adds to both, so
    # both bits show in the result; more than GROUP_MAX items of one bucket spill into a second launch; a long bucket of
    # 16-channel 3x3 layers whose tile ranges are multiples of 8 (pair-major)
    items = [_gi(2, 24, 20, 48, 80, 3, "a", "ab")]
    items += [_gi(1, 30, 17, 48, 80, 3, "a", "ab", acc=2), _gi(2, 16, 33, 48, 80, 3, "a", "ab", acc=1),
              _gi(1, 20, 20, 48, 80, 3, "a", "ab", acc=3, scale=0.25)]
    items += [_gi(1, 16 + i, 24, 48, 80, 3, "f%d" % i, "fb%d" % i if i % 3 else None) for i in range(GROUP_MAX)]
    g["accumulate_and_spill"] = items
    g["pair_major"] = [_gi(64, 16, 16, 48, 16, 3, "p0", "pb0"), _gi(8, 32, 32, 48, 16, 3, "p1", "pb1"),
                       _gi(3, 19, 23, 48, 16, 3, "p2", None)]
    return g


GROUPS = _group_cases()


def reached():
    """(single-launch keys (fam, KS, NI, NO, kind), {key: (PF, max run, residues of the runs mod PF)}, partial f32 blocks,
    small-Cin (fam, Cin), group bucket keys (kind, KS, NI, NO), group properties)"""
    keys, runs, partial, small = set(), {}, set(), set()
    for c in CASES:
        p = case_plan(c)
        fam = "bf16" if c["fam"] == "first" else c["fam"]
        if p["kind"] == F32SMALL:
            small.add((c["fam"], c["Cin"]))
            continue
        key = (fam, p["ks"], p["ni"], p["no"], p["kind"])
        keys.add(key)
        if p["kind"] == F32K and c["Cout"] % p["no"]:
            partial.add(key)
        cnt = counts_of(c)
        pf, mx, res = runs.get(key, (p["pf"], 0, set()))
        runs[key] = (pf, max(mx, max(cnt)), res | {n % p["pf"] for n in cnt if n > 0})
    buckets, props = set(), set()
    for name, items in GROUPS.items():
        nbk, ps = group_plan(items)
        per = {}
        for it, p in zip(items, ps):
            kind = MOSAIC if it.get("mosaic") else (RAGGED if it["Cin"] % 16 or it["Cout"] % 16 else PLAIN)
            buckets.add((kind, p["ks"], p["ni"], p["no"]))
            per.setdefault(p["bucket"], []).append((it, p))
            props.add("pair_major" if p["pair_major"] else "plain_mapping")
            props.add("acc%d" % it.get("acc", 0))
            if not it.get("db"):
                props.add("db_null")
            if it.get("scale", 1.0) != 1.0:
                props.add("scale")
            if p["kind"] == CONVT:
                props.add("convT")
        for b, lst in per.items():
            if len({tiles_of(dict(it, convT=0)) // max(1, abs(p["tpb"])) for it, p in lst}) > 1 or \
                    len({abs(p["tpb"]) for it, p in lst}) > 1:
                props.add("mixed_tile_counts")
        shapes = {}
        for it, p in zip(items, ps):
            shapes.setdefault((p["ks"], p["ni"], p["no"], it.get("mosaic") is not None), set()).add(p["bucket"])
        if any(len(s) > 1 and sum(1 for p in ps if p["bucket"] in s) > GROUP_MAX for s in shapes.values()):
            props.add("spill")
    return keys, runs, partial, small, buckets, props
