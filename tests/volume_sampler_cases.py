"""Volume sampler on the CPU -- the numpy restatement of include/sequitr_hip.h "Volume sampler" that the tests of
sequitr_amd.frontend.sample_plan / VolumeSampler compare against, and their case tables.

A plan row is [v, oz, ox, oy, op]; the definition, word for word:

    box = zero-padded crop vol[v, oz:oz+BZ, ox:ox+BX, oy:oy+BY]      # fill where the box leaves the volume
    if op & 8: box = box.transpose(0, 2, 1)
    if op & 1: box = box[::-1];  if op & 2: box = box[:, ::-1];  if op & 4: box = box[:, :, ::-1]

np_crop pads coordinate by coordinate, so a negative origin, an origin beyond the volume and a volume index outside
0 .. V-1 are covered by the same code.  ImageNorm's statistics and cast are volume_frontend_cases' (np_stats,
reference_cast)."""
import numpy as np

from tests.volume_frontend_cases import np_stats, reference_cast

VOL_SHAPE = (2, 19, 37, 45)                                    # (V, Z, X, Y)
SHORT_SHAPE = (1, 5, 37, 45)                                   # Z shorter than the brick
FLIPS, TRANSPOSED, ALL_OPS = tuple(range(8)), tuple(range(8, 16)), tuple(range(16))
# (brick (BZ, BX, BY), ops).  BY = 18 and 24: float32 rows of 72 and 96 bytes, the 72-byte ones alternate between 16-byte
# aligned and not, so the scalar head, the 16-byte body and the tail all run.  40 and 17 are no multiples of the 64-voxel
# LDS tile (40 > X = 37 also pads in x); 16 is a partial tile too.
IMAGE_CASES = [((8, 16, 16), ALL_OPS), ((8, 16, 18), FLIPS), ((8, 12, 24), FLIPS), ((4, 40, 40), TRANSPOSED),
               ((3, 17, 17), TRANSPOSED)]
BIG_TILE_CASE = ((2, 70, 70), TRANSPOSED)                      # more than one LDS tile per plane, the second one partial


def np_crop(arr, row, brick, fill=0):
    """the padded crop of arr (V, Z, X, Y, ...) at row's volume and origin: (BZ, BX, BY, ...)"""
    v, o = int(row[0]), [int(t) for t in row[1:4]]
    box = np.full(tuple(brick) + arr.shape[4:], fill, arr.dtype)
    if not 0 <= v < arr.shape[0]:
        return box
    lo = [max(o[a], 0) for a in range(3)]
    hi = [min(o[a] + brick[a], arr.shape[1 + a]) for a in range(3)]
    if all(h > l for l, h in zip(lo, hi)):
        dst = tuple(slice(lo[a] - o[a], hi[a] - o[a]) for a in range(3))
        box[dst] = arr[v, lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
    return box


def np_apply(box, op):
    if op & 8:
        box = box.transpose((0, 2, 1) + tuple(range(3, box.ndim)))
    if op & 1:
        box = box[::-1]
    if op & 2:
        box = box[:, ::-1]
    if op & 4:
        box = box[:, :, ::-1]
    return box


def np_unapply(box, op):
    """the inverse of np_apply: the flips (each its own inverse) first, then the transpose"""
    if op & 4:
        box = box[:, :, ::-1]
    if op & 2:
        box = box[:, ::-1]
    if op & 1:
        box = box[::-1]
    if op & 8:
        box = box.transpose((0, 2, 1) + tuple(range(3, box.ndim)))
    return box


def np_sample(arr, plan, brick, fill=0, opmask=15):
    return np.stack([np.ascontiguousarray(np_apply(np_crop(arr, r, brick, fill), int(r[4]) & opmask)) for r in plan])


def np_normalised(vols, normalise=True):
    """what ImageNorm makes of every whole volume, float32 (V, Z, X, Y)"""
    out = []
    for vol in vols:
        g = reference_cast(vol)
        if normalise:
            mean, std = np_stats(vol)
            g = (g - mean) / (1e-99 + std)
        out.append(g)
    return np.stack(out).astype(np.float32)


def np_images(vols, plan, brick, normalise=True, normalised=None):
    """(count, BZ, BX, BY, 1) float32; pass `normalised` = np_normalised(vols, normalise) to share it between calls"""
    g = np_normalised(vols, normalise) if normalised is None else normalised
    return np_sample(g, plan, brick, 0, 15 if brick[1] == brick[2] else 7)[..., None]


def np_copy(src, plan, brick):
    return np_sample(src, plan, brick, 0, 15 if brick[1] == brick[2] else 7)


def np_onehot(labels, C, plan, brick):
    full = (labels[..., None] == np.arange(C, dtype=labels.dtype)).astype(np.uint8)
    return np_copy(full, plan, brick)


def case_plan(vol_shape, brick, ops, seed=0):
    """A handcrafted plan: under every op the two extreme corners (all origins 0, all origins L - T; 0 along an axis
    shorter than the brick), one corner with the extremes mixed, and two random rows."""
    V, L = vol_shape[0], vol_shape[1:]
    last = [max(L[a] - brick[a], 0) for a in range(3)]
    rng = np.random.default_rng(seed)
    rows = []
    for op in ops:
        rows.append([0, 0, 0, 0, op])
        rows.append([V - 1] + last + [op])
        rows.append([rng.integers(V), last[0], 0, last[2], op])
        for _ in range(2):
            rows.append([rng.integers(V)] + [rng.integers(0, last[a] + 1) for a in range(3)] + [op])
    return np.asarray(rows, np.int32)


def hostile_plan(vol_shape, brick):
    """rows whose boxes lie wholly outside every volume (-> pure fill), then rows that straddle a face (-> part fill)"""
    V, (Z, X, Y) = vol_shape[0], vol_shape[1:]
    BZ, BX, BY = brick
    big = 2 ** 31 - 1
    outside = [[0, -BZ, 0, 0, 0], [0, 0, -BX, 0, 11], [0, 0, 0, -BY, 5], [0, Z, 0, 0, 0], [0, 0, X, 0, 6], [0, 0, 0, Y, 13],
               [V, 0, 0, 0, 8], [-1, 0, 0, 0, 7], [big, 0, 0, 0, 0], [0, big, big, big, 7], [0, -big - 1, -big - 1, -big - 1, 2],
               [0, big - 2, 0, 0, 1], [0, 0, -big, 0, 0], [-big - 1, 1, 1, 1, 4]]
    straddle = [[0, -3, -5, -7, 0], [V - 1, Z - 2, X - 3, Y - 1, 7], [0, -1, X - 1, -2, 13], [0, 2, -BX + 1, Y - 1, 2]]
    return np.asarray(outside, np.int32), np.asarray(straddle, np.int32)
