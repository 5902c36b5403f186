"""The numpy restatement of include/sequitr_hip.h "Seam blending": the per-axis tent weights written densely from the
definition, the slot tables made of them, the float32 sum over up to 3 x 3 tiles in the stated order as nine masked vector
steps, the divide, sq_argmax_u8's loop and the float64 softmax of the float32 l_k (both from tests/tta_cases.py), and the
case builders the CPU and the GPU tests share.  No GPU, no torch."""
import functools

import numpy as np

from sequitr_amd.frontend import axis_tiles
from tests import tta_cases as tc

BIG = 1 << 30                                                   # +infinity of the definition


def admissible(T, margin, B):
    return 0 <= B <= margin and 2 * B <= T - 2 * margin and B <= 255


def axis_weights(L, T, margin, B):
    """(origins, s, w): s[k] .. s[k+1] is tile k's run, w (n, L) the weight of every tile at every coordinate"""
    assert admissible(T, margin, B), (T, margin, B)
    origins, _ = axis_tiles(L, T, margin)
    n = len(origins)
    s = np.array([0] + [int(o) + margin for o in origins[1:]] + [L], np.int64)
    p = np.arange(L, dtype=np.int64)[None, :]
    k = np.arange(n)[:, None]
    dl = np.where(k > 0, p - s[:-1, None], BIG)
    dr = np.where(k < n - 1, s[1:, None] - 1 - p, BIG)
    return origins, s, np.clip(np.minimum(dl, dr) + B + 1, 0, 2 * B + 1)


@functools.lru_cache(maxsize=None)
def axis_blend(L, T, margin, B):
    """(origins, slots (L, 3, 2) int32): per coordinate (tile << 16 | local, weight) of the contributors, ascending; kept
    per geometry, so read only"""
    origins, _, w = axis_weights(L, T, margin, B)
    slots = np.zeros((L, 3, 2), np.int32)
    for p in range(L):
        ks = np.flatnonzero(w[:, p])
        assert 1 <= len(ks) <= 3, (L, T, margin, B, p, ks)
        for i, k in enumerate(ks):
            slots[p, i] = ((int(k) << 16) | (p - int(origins[k])), w[k, p])
    slots.setflags(write=False)
    return origins, slots


def blend_rows(acc, H, W, T, margin, B):
    """b (F, H, W, K) float32 of merged tile logits acc (F*TR*TC, T, T, K): S = +0; S = S + (float)(wy * wx) * acc over the
    contributing tiles, ky ascending then kx ascending, one float32 multiply and one float32 add per term; b = S / Wt"""
    acc = np.asarray(acc, np.float32)
    (oy, ys), (ox, xs) = axis_blend(H, T, margin, B), axis_blend(W, T, margin, B)
    TR, TC, K = len(oy), len(ox), acc.shape[-1]
    F = acc.shape[0] // (TR * TC)
    v = acc.reshape(F, TR, TC, T, T, K)
    S = np.zeros((F, H, W, K), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(3):
            for j in range(3):
                w = ys[:, i, 1].astype(np.int64)[:, None] * xs[:, j, 1][None, :]
                yy, xx = np.nonzero(w > 0)                      # terms with zero weight are not read and not added
                if not len(yy):
                    continue
                ty, ly = ys[yy, i, 0] >> 16, ys[yy, i, 0] & 0xffff
                tx, lx = xs[xx, j, 0] >> 16, xs[xx, j, 0] & 0xffff
                term = w[yy, xx].astype(np.float32)[None, :, None] * v[:, ty, tx, ly, lx, :]
                S[:, yy, xx, :] = S[:, yy, xx, :] + term
        Wt = (ys[:, :, 1].sum(1).astype(np.int64)[:, None] * xs[:, :, 1].sum(1)[None, :]).astype(np.float32)
        b = S / Wt[None, :, :, None]
    assert S.dtype == np.float32 and b.dtype == np.float32
    return b


def stitch_blend(acc, inv_n, H, W, T, margin, B):
    """(mask (F,H,W) uint8, probabilities (F,K,H,W) float64) of merged tile logits acc under blend width B"""
    b = blend_rows(acc, H, W, T, margin, B)
    return tc.argmax_rows(b), np.moveaxis(tc.softmax64(b, inv_n), -1, 1)


def used_positions(H, W, T, margin, B):
    """bool (TR*TC, T, T): the tile positions some frame pixel reads with a positive weight"""
    (oy, ys), (ox, xs) = axis_blend(H, T, margin, B), axis_blend(W, T, margin, B)
    uy, ux = np.zeros((len(oy), T), bool), np.zeros((len(ox), T), bool)
    for slots, u in ((ys, uy), (xs, ux)):
        live = slots[:, :, 1] > 0
        u[(slots[:, :, 0] >> 16)[live], (slots[:, :, 0] & 0xffff)[live]] = True
    return (uy[:, None, :, None] & ux[None, :, None, :]).reshape(len(oy) * len(ox), T, T)


def contributors(slots, p):
    """[(tile, local, weight)] of coordinate p"""
    return [(int(s[0]) >> 16, int(s[0]) & 0xffff, int(s[1])) for s in slots[p] if s[1] > 0]


# ---- the cases of tests/test_gpu_blend.py, built here so that the CPU suite can check what they promise ---------------------
GEOMETRIES = [(37, 53, 16, 4), (64, 64, 16, 4), (16, 80, 16, 4), (53, 53, 16, 4)]      # (H, W, T, margin)
BLENDS = (1, 2, 4)
BIG_GEOMETRY, BIG_BLEND = (70, 45, 32, 8), 8
KS = (1, 2, 3, 4, 7, 8, 16)


def geometry_cases():
    return [g + (B,) for g in GEOMETRIES for B in BLENDS] + [BIG_GEOMETRY + (BIG_BLEND,)]


def write_row(acc, ys, xs, TR, TC, f, y, x, row):
    """the K values `row` at frame pixel (f, y, x) in every tile that contributes to it: the blend of equal rows"""
    for ky, ly, _ in contributors(ys, y):
        for kx, lx, _ in contributors(xs, x):
            acc[(f * TR + ky) * TC + kx, ly, lx] = row


def blend_case(H, W, T, margin, B, F, K, inv_n, seed):
    """(acc, poisoned): tile sums whose mean has a spread of 20; every special row of tta_cases written once at a frame
    pixel through all its contributors (so that the blend of the pixel is that row: ties, +-0, +-inf, NaN, wide spreads);
    at pixels of a seam band +inf against -inf and a NaN in one contributor only.  `poisoned` is acc with NaN at every
    tile position that no pixel reads with a positive weight: it must give the same result."""
    rng = np.random.default_rng(seed)
    (oy, ys), (ox, xs) = axis_blend(H, T, margin, B), axis_blend(W, T, margin, B)
    TR, TC = len(oy), len(ox)
    acc = ((rng.random((F * TR * TC, T, T, K)) * 20.0).astype(np.float32) / np.float32(inv_n)).astype(np.float32)
    rows = tc.special_rows(K, rng)
    where = rng.permutation(F * H * W)
    for r, flat in zip(rows, where[:len(rows)]):
        write_row(acc, ys, xs, TR, TC, flat // (H * W), (flat // W) % H, flat % W, r / np.float32(inv_n))
    taken = set(int(v) for v in where[:len(rows)])
    band = [(y, x) for y in range(H) for x in range(W) if len(contributors(ys, y)) * len(contributors(xs, x)) > 1
            and (F - 1) * H * W + y * W + x not in taken]
    if B > 0 and len(band) >= 2:
        f = F - 1
        for n_case, (y, x) in enumerate((band[0], band[len(band) // 2])):
            tiles = [((f * TR + ky) * TC + kx, ly, lx) for ky, ly, _ in contributors(ys, y) for kx, lx, _ in contributors(xs, x)]
            if n_case == 0:                                      # inf + -inf across two tiles: NaN in that class, the NaN row
                acc[tiles[0]][0], acc[tiles[1]][0] = np.inf, -np.inf
            else:                                               # a NaN in one contributing tile only
                acc[tiles[-1]][K - 1] = np.nan
    poisoned = acc.copy()
    unused = ~used_positions(H, W, T, margin, B)
    poisoned.reshape(F, TR * TC, T, T, K)[:, unused] = np.nan
    return acc, poisoned


def u8_boundary_share(p64, K):
    """the share of the finite probabilities whose 255 p lies within 255 * bound of a rounding boundary"""
    v = 255.0 * p64[~np.isnan(p64)]
    return float((np.abs(v - np.floor(v) - 0.5) <= 255.0 * tc.prob_bound(K)).mean()) if v.size else 0.0
