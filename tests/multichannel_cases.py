"""Multi-channel frames on the CPU -- the numpy restatements of include/sequitr_hip.h's _mc paragraphs ("Tile front end",
"Tile sampler") that tests/test_multichannel_cpu.py and tests/test_gpu_multichannel.py compare against, and their cases.

Layout: a batch is channel-major planes, (C, F, H, W); channel c of frame f is plane [c, f].  Per-channel statistics are
(C, F).  The tile cutter writes interleaved (F*TR*TC, TS, TS, C) float32 tiles, channel c under mode[c]:

    SQ_CH_CAST    (0): float32(v)
    SQ_CH_NORM    (1): (float32(v) - mean32[c,f]) / std32[c,f]                       in float32
    SQ_CH_BG      (2): float32(r),  r = float64(x) - bg(u, v)  from coef[c,f,0..5]
    SQ_CH_BG_NORM (3): float32((r - mean64[c,f]) / (1e-99 + std64[c,f]))            in float64

with s = (u - (W-1)/2) * (1 / ((W-1)/2)), t likewise for the row v, and the surface by rows, every multiply-add ONE fused
operation (one rounding):  a = fma(t, fma(c5, t, c2), c0);  b = fma(c4, t, c1);  bg = fma(s, fma(c3, s, b), a).

The sampler is tests/tile_sampler_cases.np_sample per image channel: coordinates, corners and weights do not depend on the
channel."""
from fractions import Fraction

import numpy as np

from tests import tile_sampler_cases as tsc

CAST, NORM, BG, BG_NORM = 0, 1, 2, 3
MIXED = (NORM, BG_NORM, BG, CAST)

FRAME_SHAPES = [(37, 53), (64, 64)]
TILE, MARGIN = 15, 2                                            # odd: TS*TS*C is no multiple of 4 or 64
CHANNELS = (1, 2, 3, 4, 8)
DTYPES = (np.uint8, np.uint16, np.float32)

SAMPLER_FRAME = (40, 56)
SAMPLER_TILE = (16, 24)
SAMPLER_COUNT = 5


def planes(C, F, shape, dtype, seed):
    """(C, F, H, W) raw planes: every channel its own level, spread and a smooth uneven illumination, so that no two
    channels share statistics or a background surface"""
    rng = np.random.default_rng(seed)
    H, W = shape
    v, u = np.mgrid[0:H, 0:W]
    out = np.empty((C, F, H, W), np.float64)
    for c in range(C):
        for f in range(F):
            bg = 40 + 9 * c + (0.3 + 0.05 * c) * u - 0.2 * v + 0.002 * (f + 1) * (u - W / 3.) * (v - H / 2.)
            out[c, f] = bg + rng.standard_normal((H, W)) * (4 + c)
    out = np.clip(out, 0, 250)
    if np.dtype(dtype) == np.uint16:
        out = out * 200
    if np.dtype(dtype) != np.float32:
        out = np.rint(out)
    return out.astype(dtype)


def _fma(a, b, c):
    """fma(a, b, c) of float64 arrays with ONE rounding: exact rational arithmetic, rounded once by float()"""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    flat = [float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a.ravel().tolist(), b.ravel().tolist(),
                                                                             c.ravel().tolist())]
    return np.asarray(flat, np.float64).reshape(a.shape)


def bg_surface(coef, H, W):
    """bg(u, v) of one plane, (H, W) float64, in the kernel's order of operations"""
    k = np.asarray(coef, np.float64)
    cu, cv = 0.5 * float(W - 1), 0.5 * float(H - 1)
    s = (np.arange(W, dtype=np.float64) - cu) * (1.0 / cu)
    t = (np.arange(H, dtype=np.float64) - cv) * (1.0 / cv)
    a = _fma(t, _fma(k[5], t, k[2]), k[0])                     # per row
    b = _fma(k[4], t, k[1])
    s2, b2, a2 = np.broadcast_arrays(s[None, :], b[:, None], a[:, None])
    return _fma(s2, _fma(k[3], s2, b2), a2)


def np_plane(x, mode, mean32=None, std32=None, coef=None, mean64=None, std64=None):
    """one (H, W) plane under `mode`: float32 (H, W)"""
    x32 = np.array(x, dtype='float').astype(np.float32)         # ImagePipe.__call__'s cast
    if mode == CAST:
        return x32
    if mode == NORM:
        return ((x32 - np.float32(mean32)) / np.float32(std32)).astype(np.float32)
    r = x32.astype(np.float64) - bg_surface(coef, *x.shape)
    if mode == BG_NORM:
        r = (r - np.float64(mean64)) / (1e-99 + np.float64(std64))
    return r.astype(np.float32)


def np_frame_stats(x):
    """sq_frame_stats of one plane: numpy's own float32 mean and std of the float32 frame"""
    x32 = np.array(x, dtype='float').astype(np.float32)
    return np.mean(x32), np.std(x32)


def np_tiles_mc(frames, modes, oy, ox, T, mean32=None, std32=None, coef=None, mean64=None, std64=None):
    """the _mc tile definition: frames (C, F, H, W), modes C ints, statistics (C, F) (coef (C, F, 6)) where a mode reads
    them -> (F*TR*TC, T, T, C) float32"""
    C, F = frames.shape[:2]
    pick = lambda a, c, f: None if a is None else a[c][f]
    out = np.empty((F * len(oy) * len(ox), T, T, C), np.float32)
    for c in range(C):
        k = 0
        for f in range(F):
            g = np_plane(frames[c, f], modes[c], pick(mean32, c, f), pick(std32, c, f), pick(coef, c, f), pick(mean64, c, f),
                         pick(std64, c, f))
            for y in oy:
                for x in ox:
                    out[k, :, :, c] = g[y:y + T, x:x + T]
                    k += 1
    return out


def np_sample_mc(normed, labels, weights, plan, coef, tile, C):
    """the _mc sampler definition in float32: `normed` (CI, F, H, W) normalised planes (or None) -> (image (count, TH, TW,
    CI), onehot, weights); the coordinates of a pixel are computed once and every channel is interpolated at them"""
    F, H, W = next(t for t in (None if normed is None else normed[0], labels, weights) if t is not None).shape
    img = []
    for row, cf in zip(np.asarray(plan), np.asarray(coef)):
        f = int(row[0])
        sx, sy, ok = tsc.np_coords(row, cf, tile, np.float32)
        if normed is not None:
            img.append(np.stack([np.where(ok, tsc.np_bilinear(np.asarray(p, np.float32), f, sx, sy), 0).astype(np.float32)
                                 for p in normed], -1))
    _, hot, wts = tsc.np_sample(None, labels, weights, plan, coef, tile, C) if (labels is not None or weights is not None) \
        else (None, None, None)
    return (np.stack(img) if img else None), hot, wts


def sampler_rows(seed=5):
    """SAMPLER_COUNT rows: theta = 0, pi/4 and a random angle at origins inside and up to four pixels outside the frame,
    then a frame index outside the stack on either side (f = -1, f = F)"""
    H, W = SAMPLER_FRAME
    plan, coef = tsc.random_rows((3, H, W), SAMPLER_TILE, SAMPLER_COUNT - 2, seed)
    coef[0] = tsc.rotation_coef([0.0], (H, W))[0]
    coef[1] = tsc.rotation_coef([np.pi / 4], (H, W))[0]
    return plan, coef


def hostile_rows():
    """rows whose every pixel is out of range: NaN in the linear part, a 1e30 offset, 1e30 in the linear part"""
    plan, coef = tsc.bad_rows()
    keep = [0, 4, 8]
    return plan[keep], coef[keep]
