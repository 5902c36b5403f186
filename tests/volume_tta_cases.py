"""The numpy restatement of include/sequitr_hip.h "Brick views and probability scatter": views of (N, BZ, BX, BY, E) brick
batches under the 16 symmetries of the volume sampler, by index arrays; the op-ordered float32 merge; the owner boxes of
frontend.volume_bricks and the scatter of classes and probabilities into whole volumes.  The per-voxel rules (argmax,
softmax, bounds) are the planar restatement's, tests/tta_cases.py.  No GPU, no torch."""
import numpy as np

from sequitr_amd.frontend import volume_bricks
from tests.tta_cases import (argmax_rows, softmax64, softmax32, prob_bound, check_probs, check_probs_u8, special_rows,  # noqa: F401
                       special_values, bits, same_bits_nan_aware, to_u8)

OPS = tuple(range(16))
SETS = {None: (0,), "flips": tuple(range(8)), "dihedral": OPS}
# the header's op' with unview_op == view_op': bits 1 and 2 swap under bit 3
INVERSE = {0: 0, 1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 6, 7: 7, 8: 8, 9: 9, 10: 12, 11: 13, 12: 10, 13: 11, 14: 14, 15: 15}
E_MAX = 16


def _sources(shape, op):
    """index arrays (zs, a, b): view_op(x)[n, z, x, y, e] = x[n, zs, a, b, e]"""
    BZ, BX, BY = shape[1:4]
    if op & 8:
        assert BX == BY, "bit 3 transposes x and y"
    z, x, y = np.meshgrid(np.arange(BZ), np.arange(BX), np.arange(BY), indexing="ij")
    zs = BZ - 1 - z if op & 1 else z
    fx = BX - 1 - x if op & 2 else x
    fy = BY - 1 - y if op & 4 else y
    a, b = (fy, fx) if op & 8 else (fx, fy)
    return zs, a, b


def view(x, op):
    """view_op(x)[n, z, x, y, e] = x[n, fz(z), a, b, e], (a, b) = (fx(x), fy(y)), or (fy(y), fx(x)) under bit 3"""
    x = np.asarray(x)
    zs, a, b = _sources(x.shape, op)
    return np.ascontiguousarray(x[:, zs, a, b, :])


def unview(y, op):
    """the inverse, by scattering: x[n, fz(z), a, b, e] = y[n, z, x, y, e]"""
    y = np.asarray(y)
    zs, a, b = _sources(y.shape, op)
    x = np.empty_like(y)
    x[:, zs, a, b, :] = y
    return x


def view_sampler_text(x, op):
    """the "Volume sampler" numpy text, per brick"""
    out = []
    for b in np.asarray(x):
        if op & 8:
            b = b.transpose(0, 2, 1, 3)
        if op & 1:
            b = b[::-1]
        if op & 2:
            b = b[:, ::-1]
        if op & 4:
            b = b[:, :, ::-1]
        out.append(b)
    return np.ascontiguousarray(np.stack(out))


def merge(logits_by_op, ops):
    """acc = unview_0(L_0); acc = acc + unview_op(L_op) for op ascending: one float32 add per element per op"""
    assert tuple(ops) == tuple(sorted(ops)) and ops[0] == 0
    acc = unview(np.asarray(logits_by_op[0], np.float32), 0).copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for op in ops[1:]:
            acc = (acc + unview(np.asarray(logits_by_op[op], np.float32), op)).astype(np.float32)
    return acc


def owner_boxes(vol_shape, brick, margin):
    """per brick of one volume, in brick order: (origin (z, x, y), low (z, x, y), high (z, x, y)) of frontend.volume_bricks --
    absolute coordinates, the owned box [low, high) clamped into brick and volume as the kernels clamp it"""
    g = volume_bricks(vol_shape, brick, margin)
    table = g.table()
    KZ, KX, KY = g.counts
    n = KZ + KX + KY
    org, low, high = table[:n], table[n:2 * n], table[2 * n:3 * n]
    boxes = []
    for kz in range(KZ):
        for kx in range(KX):
            for ky in range(KY):
                idx = (kz, KZ + kx, KZ + KX + ky)
                o = tuple(int(org[i]) for i in idx)
                lo = tuple(max(int(low[i]), o[d], 0) for d, i in enumerate(idx))
                hi = tuple(min(int(high[i]), o[d] + g.brick[d], g.shape[d]) for d, i in enumerate(idx))
                boxes.append((o, lo, hi))
    return boxes


def scatter(values, out, vol_shape, brick, margin, first=0):
    """values (count, BZ, BX, BY[, ...]) of bricks first .. -> their owned boxes of out (V, Z, X, Y[, ...]), in place"""
    boxes = owner_boxes(vol_shape, brick, margin)
    for i, val in enumerate(values):
        v, k = divmod(first + i, len(boxes))
        o, lo, hi = boxes[k]
        out[v, lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = val[lo[0] - o[0]:hi[0] - o[0], lo[1] - o[1]:hi[1] - o[1],
                                                          lo[2] - o[2]:hi[2] - o[2]]
    return out


def scatter_probs(acc, inv_n, vol_shape, brick, margin, mask_out=None, prob_out=None, first=0):
    """merged brick logits acc (count, BZ, BX, BY, K) of bricks first .. -> the classes in mask_out (V, Z, X, Y) uint8 and
    the float64 probabilities in prob_out (V, K, Z, X, Y), in place, owned boxes only"""
    acc = np.asarray(acc, np.float32)
    if mask_out is not None:
        scatter(argmax_rows(acc), mask_out, vol_shape, brick, margin, first)
    if prob_out is not None:
        scatter(softmax64(acc, inv_n), np.moveaxis(prob_out, 1, -1), vol_shape, brick, margin, first)
    return mask_out, prob_out


def scatter_case(vol_shape, brick, margin, V, K, inv_n, seed, specials=True):
    """merged logits (V * bricks, BZ, BX, BY, K) whose mean has a spread of 20 (the planar GPU case: under 0.1 % of the
    uint8 values of its float64 softmax lie at a rounding boundary, tests/test_volume_tta_cpu.py), with every special row
    written once at an owned voxel of some brick when `specials` (their ties sit on a uint8 rounding boundary by
    construction: a volume of a few hundred voxels leaves them out to stay under check_probs_u8's cap)"""
    rng = np.random.default_rng(seed)
    boxes = owner_boxes(vol_shape, brick, margin)
    acc = ((rng.random((V * len(boxes),) + tuple(brick) + (K,)) * 20.0).astype(np.float32) / np.float32(inv_n)).astype(np.float32)
    for r in special_rows(K, rng) if specials else ():
        b = int(rng.integers(V * len(boxes)))
        o, lo, hi = boxes[b % len(boxes)]
        z, x, y = (int(rng.integers(lo[d], hi[d])) - o[d] for d in range(3))
        acc[b, z, x, y] = r / np.float32(inv_n)
    return acc


def boundary_share(p64, K):
    """the share of finite uint8 probabilities within 255 * bound of a rounding boundary: check_probs_u8's condition"""
    v = 255.0 * p64[~np.isnan(p64)]
    return float((np.abs(v - np.floor(v) - 0.5) <= 255.0 * prob_bound(K)).mean()) if v.size else 0.0


SCATTER_VOLUMES = (((9, 21, 37), (4, 8, 16), (1, 2, 3)), ((3, 5, 11), (4, 8, 16), (1, 2, 3)))   # the second: shorter than the brick
SCATTER_K = (1, 2, 3, 4, 5, 8, 16)
SCATTER_N = (1, 8, 16)


def scatter_seed(K, n, which):
    return 100 * K + 10 * which + n
