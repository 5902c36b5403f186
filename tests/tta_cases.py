"""The numpy restatement of include/sequitr_hip.h "Tile views and probability stitch": views of (N, T, T, E) tile batches
under the eight symmetries of the square, the op-ordered float32 merge, sq_argmax_u8's loop, the softmax (float32 as the
kernel evaluates it, float64 as the reference) and the owner-map stitch from frontend.axis_tiles.  No GPU, no torch."""
import numpy as np

from sequitr_amd.frontend import axis_tiles

OPS = tuple(range(8))
SETS = {None: (0,), "flips": (0, 1, 2, 3), "dihedral": OPS}
INVERSE = {0: 0, 1: 1, 2: 2, 3: 3, 4: 4, 5: 6, 6: 5, 7: 7}      # the header's op' with unview_op == view_op'
E_MAX = 16


def view(x, op):
    """view_op(x)[n, i, j, e] = x[n, a, b, e]; (p, q) = (j, i) if op & 4 else (i, j); a, b mirror p, q under bits 0, 1"""
    x = np.asarray(x)
    T = x.shape[1]
    i, j = np.meshgrid(np.arange(T), np.arange(T), indexing="ij")
    p, q = (j, i) if op & 4 else (i, j)
    a = T - 1 - p if op & 1 else p
    b = T - 1 - q if op & 2 else q
    return np.ascontiguousarray(x[:, a, b, :])


def unview(y, op):
    """the inverse, by scattering: x[n, a, b, e] = y[n, i, j, e]"""
    y = np.asarray(y)
    T = y.shape[1]
    i, j = np.meshgrid(np.arange(T), np.arange(T), indexing="ij")
    p, q = (j, i) if op & 4 else (i, j)
    a = T - 1 - p if op & 1 else p
    b = T - 1 - q if op & 2 else q
    x = np.empty_like(y)
    x[:, a, b, :] = y
    return x


def merge(logits_by_op, ops):
    """acc = unview_0(L_0); acc = acc + unview_op(L_op) for op ascending: one float32 add per element per op"""
    assert tuple(ops) == tuple(sorted(ops)) and ops[0] == 0
    acc = unview(np.asarray(logits_by_op[0], np.float32), 0).copy()
    for op in ops[1:]:
        acc = (acc + unview(np.asarray(logits_by_op[op], np.float32), op)).astype(np.float32)
    return acc


def argmax_rows(z):
    """sq_argmax_u8's loop over the last axis: ties to the lowest class, NaN never wins, a row that starts with NaN is 0"""
    z = np.asarray(z)
    best = np.zeros(z.shape[:-1], np.uint8)
    bv = z[..., 0].copy()
    with np.errstate(invalid="ignore"):
        for c in range(1, z.shape[-1]):
            win = z[..., c] > bv
            bv = np.where(win, z[..., c], bv)
            best[win] = c
    return best


def _softmax(acc, inv_n, dtype, exp):
    acc = np.asarray(acc, np.float32)
    pc = argmax_rows(acc)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        l = (acc * np.float32(inv_n)).astype(dtype)             # exact: inv_n is a power of two
        m = np.take_along_axis(l, pc[..., None].astype(np.int64), -1)
        e = exp((l - m).astype(dtype)).astype(dtype)
        s = np.zeros(e.shape[:-1], dtype)
        for k in range(e.shape[-1]):                            # in index order
            s = (s + e[..., k]).astype(dtype)
        p = (e / s[..., None]).astype(dtype)
    bad = ~np.isfinite(m[..., 0]) | np.isnan(l).any(-1)
    p[bad] = np.nan
    return p


def softmax64(acc, inv_n=1.0):
    """the reference: the header's expression in float64 on the float32 values of acc"""
    return _softmax(acc, inv_n, np.float64, np.exp)


def softmax32(acc, inv_n=1.0):
    """the header's expression in numpy float32, the same order of operations as the kernel"""
    return _softmax(acc, inv_n, np.float32, np.exp)


def prob_bound(K):
    """(K + 4) * 2^-23: one rounding of l - m (at most 2^-24 / e in e_k), about an ulp each for expf, the K - 1 adds and
    the divide on values <= 1, doubled"""
    return (K + 4) * 2.0 ** -23


def to_u8(p):
    """(uint8) floorf(p * 255 + 0.5f), NaN -> 0, on float64 probabilities"""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(p), 0, np.floor(p * 255.0 + 0.5)).astype(np.uint8)


def owner_maps(H, W, T, margin):
    """(ymap, xmap, TR, TC) as FrameTiler holds them"""
    oy, ymap = axis_tiles(H, T, margin)
    ox, xmap = axis_tiles(W, T, margin)
    return ymap, xmap, len(oy), len(ox)


def stitch(tile_values, H, W, T, margin):
    """(F*TR*TC, T, T[, K]) per-tile values -> (F, H, W[, K]): every frame pixel from its owner tile"""
    ymap, xmap, TR, TC = owner_maps(H, W, T, margin)
    v = np.asarray(tile_values)
    F = v.shape[0] // (TR * TC)
    v = v.reshape((F, TR, TC) + v.shape[1:])
    ty, ly = (ymap >> 16)[:, None], (ymap & 0xffff)[:, None]
    tx, lx = (xmap >> 16)[None, :], (xmap & 0xffff)[None, :]
    return v[:, ty, tx, ly, lx]


def stitch_probs(acc, inv_n, H, W, T, margin):
    """(mask (F,H,W) uint8, probabilities (F,K,H,W) float64) of merged tile logits acc (F*TR*TC, T, T, K)"""
    rows = stitch(acc, H, W, T, margin)                         # (F, H, W, K)
    return argmax_rows(rows), np.moveaxis(softmax64(rows, inv_n), -1, 1)


def check_probs(got, want64, K, what=""):
    """float32 probabilities against the float64 restatement: NaN where it is NaN, else within prob_bound(K)"""
    got, want64 = np.asarray(got), np.asarray(want64)
    assert got.shape == want64.shape, (what, got.shape, want64.shape)
    nan = np.isnan(want64)
    assert np.array_equal(np.isnan(got), nan), "%s: NaN positions differ" % what
    err = np.abs(got.astype(np.float64) - want64)[~nan]
    worst = float(err.max()) if err.size else 0.0
    print("%s K=%d: max |p - p64| = %.3g (bound %.3g)" % (what, K, worst, prob_bound(K)))
    assert worst <= prob_bound(K), (what, worst, prob_bound(K))
    return worst


def check_probs_u8(got, want64, K, what=""):
    """uint8 probabilities: equal to the float64 rounding wherever 255 p is farther than 255 * bound from a half-integer,
    within one count elsewhere; fewer than 1 % of the values may be of the second kind"""
    got, want64 = np.asarray(got), np.asarray(want64)
    assert got.dtype == np.uint8 and got.shape == want64.shape, (what, got.dtype, got.shape)
    nan = np.isnan(want64)
    assert (got[nan] == 0).all(), "%s: NaN must write 0" % what
    v = 255.0 * want64[~nan]
    near = np.abs(v - np.floor(v) - 0.5) <= 255.0 * prob_bound(K)
    ref, g = to_u8(want64)[~nan].astype(np.int64), got[~nan].astype(np.int64)
    share = float(near.mean()) if near.size else 0.0
    print("%s K=%d: %.4f %% of the values lie at a rounding boundary" % (what, K, 100 * share))
    assert share < 0.01, (what, share)
    assert np.array_equal(g[~near], ref[~near]), "%s: uint8 differs away from a rounding boundary" % what
    assert (np.abs(g[near] - ref[near]) <= 1).all(), "%s: uint8 off by more than one count" % what


def special_rows(K, rng):
    """rows of K logits built to stress the rules: ties, -0 against +0, NaN first / middle / everywhere, +inf, all -inf,
    spreads of 0, 1e-3, 20, 88, 104 and beyond"""
    rows = []
    base = rng.standard_normal(K).astype(np.float32)
    rows.append(np.zeros(K, np.float32))                                        # all tied
    rows.append(np.full(K, 3.25, np.float32))
    r = np.zeros(K, np.float32); r[0] = -0.0; rows.append(r)                    # -0 first against +0
    r = np.zeros(K, np.float32); r[-1] = -0.0; rows.append(r)
    r = base.copy(); r[0] = np.nan; rows.append(r)                              # NaN first: class 0
    r = base.copy(); r[K // 2] = np.nan; rows.append(r)                         # NaN in the middle never wins
    rows.append(np.full(K, np.nan, np.float32))
    r = base.copy(); r[K - 1] = np.inf; rows.append(r)
    r = base.copy(); r[0] = np.inf; r[K - 1] = np.inf; rows.append(r)
    rows.append(np.full(K, -np.inf, np.float32))
    r = base.copy(); r[0] = -np.inf; rows.append(r)                             # one class impossible
    for spread in (0.0, 1e-3, 20.0, 88.0, 104.0, 120.0, 300.0):
        r = (rng.random(K) * spread).astype(np.float32)
        r[rng.integers(K)] = spread
        r[rng.integers(K)] = 0.0
        rows.append(r)
        rows.append(-r)
    r = base.copy(); r[:] = r.max(); r[K - 1] = np.nextafter(r[0], np.float32(np.inf)); rows.append(r)   # one ulp wins
    r = np.full(K, 1e-42, np.float32); r[K // 2] = 2e-42; rows.append(r)       # subnormal logits
    return np.stack(rows).astype(np.float32)


def special_values(shape, rng):
    """float32 data for the view tests: normal values with +-0, NaN (two payloads), +-inf and subnormals strewn in"""
    x = rng.standard_normal(shape).astype(np.float32)
    flat = x.reshape(-1)
    specials = np.array([0.0, -0.0, np.inf, -np.inf, 1e-42, -3e-44], np.float32)
    idx = rng.permutation(flat.size)[:max(1, flat.size // 7)]
    flat[idx] = specials[np.arange(len(idx)) % len(specials)]
    bits = flat.view(np.uint32)
    nan_at = rng.permutation(flat.size)[:max(1, flat.size // 11)]
    bits[nan_at] = np.where(np.arange(len(nan_at)) % 2 == 0, 0x7fc00000, 0xffc12345).astype(np.uint32)
    return x


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits_nan_aware(got, want):
    """accumulated values: the same bits where the result is a number, NaN where it is NaN (an add may quieten or pick
    either operand's payload)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])
