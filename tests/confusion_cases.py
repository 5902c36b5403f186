"""Shared by the CPU and the GPU confusion tests: the definition of sq_confusion (include/sequitr_hip.h "Scoring") restated
in numpy, and the inputs the GPU tests run.  Every quantity is an integer count, so every comparison is exact."""
import numpy as np

CLASSES = (1, 2, 3, 5, 16)
SIZES = (1, 15, 16, 17, 63, 4099)
ITEMS = (1, 3)


def argmax_lowest(logits):
    """sq_argmax_u8's loop (sequitr_amd/csrc/sq_pointwise.hip: argmax_u8_kernel; oracle/sq_oracle.c: oracle_argmax_u8):
    best = 0; for c = 1 .. C-1: if z[c] > z[best]: best = c.  A tie keeps the lowest index; a comparison with NaN is
    false, so a NaN never replaces the best and a leading NaN is never replaced (np.argmax would return the NaN)."""
    z = np.asarray(logits, np.float32)
    best = np.zeros(z.shape[:-1], np.int64)
    bv = z[..., 0].copy()
    with np.errstate(invalid='ignore'):
        for c in range(1, z.shape[-1]):
            win = z[..., c] > bv
            best[win] = c
            bv[win] = z[..., c][win]
    return best.astype(np.uint8)


def onehot_class(onehot):
    """the lowest non-zero channel; 255 (no class) for an all-zero row"""
    y = np.asarray(onehot) != 0
    return np.where(y.any(-1), y.argmax(-1), 255).astype(np.uint8)


def confusion_ref(pred, truth, C):
    """(counts int64 (items, C, C), ignored int64 (items,)) of pred (items, n) uint8 | (items, n, C) float32 against truth
    (items, n) uint8 | (items, n, C) uint8: row = truth, column = prediction; a pixel whose truth or mask class is >= C (or
    has none) is ignored"""
    pred, truth = np.asarray(pred), np.asarray(truth)
    pc = argmax_lowest(pred) if pred.dtype == np.float32 else pred
    tc = onehot_class(truth) if truth.ndim == pc.ndim + 1 else truth
    assert pc.shape == tc.shape and pc.dtype == np.uint8 and tc.dtype == np.uint8
    items = pc.shape[0]
    counts, ignored = np.zeros((items, C, C), np.int64), np.zeros((items,), np.int64)
    for i in range(items):
        p, t = pc[i].reshape(-1).astype(np.int64), tc[i].reshape(-1).astype(np.int64)
        ok = (p < C) & (t < C)
        counts[i] = np.bincount(t[ok] * C + p[ok], minlength=C * C).reshape(C, C)
        ignored[i] = int((~ok).sum())
    return counts, ignored


def class_bytes(rng, shape, C):
    """class bytes that are mostly valid, with values >= C and 255 mixed in"""
    v = rng.integers(0, C, size=shape).astype(np.uint8)
    r = rng.random(shape)
    v[r < 0.06] = 255
    v[(r >= 0.06) & (r < 0.12)] = min(C, 255)
    v[(r >= 0.12) & (r < 0.16)] = rng.integers(C, 256, size=shape).astype(np.uint8)[(r >= 0.12) & (r < 0.16)]
    return v


def onehot_labels(rng, shape, C):
    """one-hot rows (any non-zero byte counts) with all-zero rows and rows with two channels set mixed in"""
    cls = rng.integers(0, C, size=shape)
    y = np.zeros(tuple(shape) + (C,), np.uint8)
    np.put_along_axis(y, cls[..., None], rng.integers(1, 256, size=tuple(shape) + (1,)).astype(np.uint8), -1)
    r = rng.random(shape)
    y[r < 0.1] = 0
    two = (r >= 0.1) & (r < 0.25)
    if C > 1:
        other = rng.integers(0, C, size=shape)
        yy = y[two]
        yy[np.arange(yy.shape[0]), other[two]] = 1
        y[two] = yy
    return y


def logits_cases(rng, shape, C):
    """float32 logits: random rows, constructed ties, and rows with NaN, +inf, -inf and +-0 at random channels"""
    z = rng.standard_normal(tuple(shape) + (C,)).astype(np.float32)
    flat = z.reshape(-1, C)
    n = flat.shape[0]
    kind = rng.integers(0, 10, size=n)
    for k, row in zip(kind, flat):
        if k == 0:                                              # every channel ties
            row[:] = row[0]
        elif k == 1:                                            # the maximum twice
            row[rng.integers(0, C)] = row[rng.integers(0, C)] = 7.0
        elif k == 2:
            row[rng.integers(0, C)] = np.nan
        elif k == 3:
            row[0] = np.nan
        elif k == 4:
            row[rng.integers(0, C)] = np.inf
            row[rng.integers(0, C)] = np.inf
        elif k == 5:
            row[:] = -np.inf
            row[rng.integers(0, C)] = rng.choice([-np.inf, -1.0])
        elif k == 6:                                            # -0 == +0: the lower index wins whatever the signs
            row[:] = -1.0
            row[rng.integers(0, C)] = -0.0
            row[rng.integers(0, C)] = 0.0
        elif k == 7:
            row[:] = np.nan
    return z


def offset_view(torch, host, offset, device):
    """`host` in GPU memory as a contiguous view that starts `offset` bytes (of the element size) into an allocation, so
    that its base is not aligned to the allocation's 256 bytes"""
    t = torch.from_numpy(np.ascontiguousarray(host))
    raw = torch.empty(t.numel() + offset + 16, dtype=t.dtype, device=device)
    view = raw[offset:offset + t.numel()].view(t.shape)
    view.copy_(t)
    return view
