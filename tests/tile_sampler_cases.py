"""Tile sampler on the CPU -- the numpy restatement of include/sequitr_hip.h "Tile sampler" that the tests of
sequitr_amd.frontend.tile_sample_plan / TileSampler compare against, and their case tables.

A sample is two rows, plan[k] = [f, oy, ox, 0] (int32, the fourth entry reserved and ignored) and
coef[k] = [a0, a1, a2, b0, b1, b2] (float32).  The definition, word for word; for pixel (i, j) of sample k, with tiles of
(TH, TW) and frames (F, H, W):

    x = float32(ox + j);  y = float32(oy + i)
    sx = (a0*x + a1*y) + a2;   sy = (b0*x + b1*y) + b2     # float32, every * and + rounded on its own, no FMA
    read_T(r, c) = T[f, r, c] if 0 <= f < F and 0 <= r < H and 0 <= c < W else 0
    bilinear(T):  x0 = floor(sx), y0 = floor(sy), x1 = x0 + 1, y1 = y0 + 1
        top = (x1 - sx) * read_T(y0, x0) + (sx - x0) * read_T(y0, x1)
        bot = (x1 - sx) * read_T(y1, x0) + (sx - x0) * read_T(y1, x1)
        val = (y1 - sy) * top + (sy - y0) * bot
    nearest:  r = roundf(sy), c = roundf(sx)  (half away from zero);  inside = (r, c) in the frame and 0 <= f < F
    image  [k,i,j,0] = bilinear(normalised frame)
    onehot [k,i,j,q] = (read_labels(r, c) == q)                            # label 0 outside; label >= C: all zero
    weights[k,i,j,0] = bilinear(weight map) + (inside ? 0.0f : 1.0f)

A pixel whose sx or sy is NaN, or at or beyond +-2^23, reads fill everywhere: image 0, label 0, weight 1.  ox + j and
oy + i are exact integer sums, rounded once to the working type.

np_sample evaluates this in `dtype`: float32 is the definition, float64 the same formulas on the same float32 inputs (the
rows and the frames are cast, nothing else changes), which is what the error bound and scipy are compared with.  The
normalised frame is oracle.frontend_ref.image_norm's, the one FrameTiler.tiles is held to."""
import numpy as np

from oracle import frontend_ref

FRAMES_SHAPE = (2, 37, 45)                                      # (F, H, W)
# 24: one partial 32 x 32 patch; (16, 40): a partial row of two patches; 40: four patches, three of them partial, and
# taller than the frame
TILES = [(24, 24), (16, 40), (40, 40)]
BIG_TILE = (48, 48)                                             # larger than the frame along both axes
CLASSES = (1, 2, 5, 16)
MAX_LABEL = 6
LIMIT = 2.0 ** 23


def np_round(v):
    """roundf: truncate, then step away from zero where the dropped fraction is at least one half"""
    t = np.trunc(v)
    return t + np.where(np.abs(v - t) >= 0.5, np.sign(v), 0).astype(v.dtype)


def random_frames(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype) == np.float32:
        return (rng.standard_normal(shape) * 30 + 100).astype(np.float32)
    return rng.integers(0, np.iinfo(dtype).max // 3, shape).astype(dtype)


def random_labels(shape, seed):
    return np.random.default_rng(seed).integers(0, MAX_LABEL + 1, shape).astype(np.uint8)


def random_weights(shape, seed):
    return (1 + 9 * np.random.default_rng(seed).random(shape)).astype(np.float32)


def np_normalised(frames, normalise=True):
    """what ImageNorm makes of every whole frame, float32 (F, H, W); the plain cast without `normalise`"""
    if not normalise:
        return np.asarray(frames, np.float32)
    return np.stack([frontend_ref.image_norm(np.array(f, dtype='float'))[..., 0] for f in frames]).astype(np.float32)


def np_coords(row, cf, tile, dtype=np.float32):
    """(sx, sy, ok) of one sample, (TH, TW) each; where ok is False the coordinates are out of range and set to 0"""
    TH, TW = tile
    c = np.asarray(cf, np.float32).astype(dtype)
    x = (int(row[2]) + np.arange(TW, dtype=np.int64)).astype(dtype)[None, :]
    y = (int(row[1]) + np.arange(TH, dtype=np.int64)).astype(dtype)[:, None]
    with np.errstate(all='ignore'):
        sx = (c[0] * x + c[1] * y) + c[2]
        sy = (c[3] * x + c[4] * y) + c[5]
        ok = (np.abs(sx) < LIMIT) & (np.abs(sy) < LIMIT)        # False for NaN
    return np.where(ok, sx, 0).astype(dtype), np.where(ok, sy, 0).astype(dtype), ok


def np_read(T, f, r, c):
    """read_T: zero outside the frame and for f outside 0 .. F-1; r, c integer arrays"""
    F, H, W = T.shape
    if not 0 <= f < F:
        return np.zeros(r.shape, T.dtype)
    valid = (r >= 0) & (r < H) & (c >= 0) & (c < W)
    return np.where(valid, T[f][np.clip(r, 0, H - 1), np.clip(c, 0, W - 1)], 0).astype(T.dtype)


def np_bilinear(T, f, sx, sy):
    x0, y0 = np.floor(sx), np.floor(sy)
    x1, y1 = x0 + 1, y0 + 1
    c0, r0 = x0.astype(np.int64), y0.astype(np.int64)
    top = (x1 - sx) * np_read(T, f, r0, c0) + (sx - x0) * np_read(T, f, r0, c0 + 1)
    bot = (x1 - sx) * np_read(T, f, r0 + 1, c0) + (sx - x0) * np_read(T, f, r0 + 1, c0 + 1)
    return (y1 - sy) * top + (sy - y0) * bot


def np_sample(normed, labels, weights, plan, coef, tile, C, dtype=np.float32):
    """(image (count, TH, TW, 1), onehot (count, TH, TW, C) uint8, weights (count, TH, TW, 1)) in `dtype`; `normed` is
    np_normalised(frames, normalise), `weights` (F, H, W).  A source that is None gives None."""
    shape = next(t for t in (normed, labels, weights) if t is not None).shape
    F, H, W = shape
    img, hot, wts = [], [], []
    for row, cf in zip(np.asarray(plan), np.asarray(coef)):
        f = int(row[0])
        sx, sy, ok = np_coords(row, cf, tile, dtype)
        r, c = np_round(sy).astype(np.int64), np_round(sx).astype(np.int64)
        inside = ok & (0 <= f < F) & (r >= 0) & (r < H) & (c >= 0) & (c < W)
        if normed is not None:
            img.append(np.where(ok, np_bilinear(normed.astype(dtype), f, sx, sy), 0).astype(dtype))
        if labels is not None:
            lab = np.where(ok, np_read(labels, f, r, c), 0)
            hot.append((lab[..., None] == np.arange(C)).astype(np.uint8))
        if weights is not None:
            val = np.where(ok, np_bilinear(weights.astype(dtype), f, sx, sy), 0).astype(dtype)
            wts.append(val + np.where(inside, 0, 1).astype(dtype))
    return (np.stack(img)[..., None] if img else None, np.stack(hot) if hot else None,
            np.stack(wts)[..., None] if wts else None)


def rotation_coef(theta, frame_hw):
    """the float64 formula of tile_sample_plan, rounded once to float32: (count, 6)"""
    H, W = frame_hw
    th = np.asarray(theta, np.float64).reshape(-1)
    c, s = np.cos(th), np.sin(th)
    a2 = ((W - 1) - (c * (W - 1) - s * (H - 1))) / 2.
    b2 = ((H - 1) - (s * (W - 1) + c * (H - 1))) / 2.
    return np.stack([c, -s, a2, s, c, b2], 1).astype(np.float32)


def origin_range(L, T, slack=4):
    """the closed range of origins the random cases draw from: -slack .. L - T + slack, whichever way round"""
    return tuple(sorted((-slack, L - T + slack)))


def random_rows(frames_shape, tile, count, seed):
    """`count` random-angle rows with origins that leave the frame by up to four pixels, the two extreme origins among
    them, then one row with f = -1 and one with f = F"""
    F, H, W = frames_shape
    rng = np.random.default_rng(seed)
    (ylo, yhi), (xlo, xhi) = origin_range(H, tile[0]), origin_range(W, tile[1])
    plan = np.zeros((count + 2, 4), np.int32)
    plan[:, 0] = rng.integers(0, F, count + 2)
    plan[:, 1] = rng.integers(ylo, yhi + 1, count + 2)
    plan[:, 2] = rng.integers(xlo, xhi + 1, count + 2)
    plan[0, 1:3], plan[1, 1:3] = (ylo, xlo), (yhi, xhi)
    plan[count, 0], plan[count + 1, 0] = -1, F
    plan[:, 3] = rng.integers(-5, 5, count + 2)                 # reserved: ignored
    return plan, rotation_coef(rng.uniform(0, 2 * np.pi, count + 2), (H, W))


def identity_rows(origins, f=0):
    """rows (1,0,0, 0,1,0) at the (oy, ox) pairs `origins`"""
    plan = np.asarray([[f, oy, ox, 0] for oy, ox in origins], np.int32)
    return plan, np.tile(np.asarray([1, 0, 0, 0, 1, 0], np.float32), (len(plan), 1))


def quarter_turn_rows(S, f=0):
    """the exact quarter turn of an S x S frame: sx = (S-1) - y, sy = x, that is out[i, j] = frame[j, S-1-i] = rot90(frame)"""
    return np.asarray([[f, 0, 0, 0]], np.int32), np.asarray([[0, -1, S - 1, 1, 0, 0]], np.float32)


def large_footprint_rows():
    """rows whose 32 x 32 patches have footprints beyond the 48 x 48 LDS patch -- a scale by 3 about two different points,
    two shears -- between rows that fit (a zoom-in by 3, a plain rotation), so that one launch takes both forms"""
    plan = np.asarray([[0, 0, 0, 0], [1, -2, 3, 0], [0, 1, 2, 0], [1, 0, 0, 0], [0, 2, 1, 0], [1, 3, 0, 0]], np.int32)
    coef = np.asarray([[3, 0, -40, 0, 3, -30],
                       [3, 0.5, -50.25, -0.5, 3, -20.5],
                       [1, 2.5, -20, 0, 1, 0],
                       [1, 0, 0.5, -1.75, 1, 30.25],
                       [1 / 3., 0, 10, 0, 1 / 3., 12],
                       list(rotation_coef([0.7], FRAMES_SHAPE[1:])[0])], np.float32)
    return plan, coef


def bad_rows():
    """rows whose every pixel is out of range: a NaN coefficient in each position of the linear part, an infinite and a
    1e30 offset, 1e30 in the linear part at origins that keep x and y away from 0"""
    plan, coef = [], []
    for pos in (0, 1, 3, 4):
        cf = [1, 0, 0, 0, 1, 0]
        cf[pos] = np.nan
        plan.append([0, 3, 5, 0]), coef.append(cf)
    for pos, val in ((2, 1e30), (5, -1e30), (2, np.inf), (5, np.nan), (0, 1e30), (4, -1e30), (1, 1e30), (3, 1e30)):
        cf = [1, 0, 0, 0, 1, 0]
        cf[pos] = val
        plan.append([1, 3, 5, 0]), coef.append(cf)
    return np.asarray(plan, np.int32), np.asarray(coef, np.float32)
