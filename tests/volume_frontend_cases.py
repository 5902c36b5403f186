"""Volume front end on the CPU -- numpy restatements the tests of sequitr_amd.frontend's volume path compare against.

np_stats restates what np.mean / np.std do to a contiguous float32 array (ImageNorm.pipe, sequitr/pipeline.py:352-355):
float32 pairwise sums per 8192-element chunk (np.add.reduce of a chunk is numpy's pairwise sum) added in order, and a
division by the integer count, which numpy carries out in float64.  np_bricks / np_scatter restate the brick cutting and
the scatter with plain slicing from a BrickGeometry's boxes."""
import numpy as np

CHUNK = 8192
STATS_SHAPES = [((5, 7, 9), np.uint8), ((20, 40, 52), np.uint16), ((24, 100, 130), np.float32), ((3, 17, 8191), np.float32),
                ((65, 511, 513), np.uint16)]                   # the last: 17 039 295 voxels, odd and above 2^24


def random_volume(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype) == np.float32:
        return (rng.standard_normal(shape) * 30 + 100).astype(np.float32)
    return rng.integers(0, np.iinfo(dtype).max // 3, shape).astype(dtype)


def reference_cast(vol):
    """the float32 array ImageNorm sees: OctopusData's float frames, ImagePipe.__call__'s astype (pipeline.py:178-179)"""
    return np.ascontiguousarray(np.array(vol, dtype='float')[..., None].astype('float32')[..., 0])


def chunked_sum(a):
    res = np.float32(0)
    for c in range(0, a.size, CHUNK):
        res = np.float32(res + np.add.reduce(a[c:c + CHUNK]))
    return res


def np_stats(vol):
    """(mean, std) float32 of one volume by the stated definition"""
    a = reference_cast(vol).ravel()
    n = np.float64(a.size)
    mean = np.float32(np.float64(chunked_sum(a)) / n)
    d = a - mean
    var = np.float32(np.float64(chunked_sum(d * d)) / n)
    return mean, np.sqrt(var)


def np_bricks(vols, geometry, normalise=True):
    """(V * per_volume, BZ, BX, BY, 1) float32: every brick of every volume, 0.0 beyond the volume"""
    BZ, BX, BY = geometry.brick
    out = np.zeros((len(vols) * geometry.per_volume, BZ, BX, BY, 1), np.float32)
    for v, vol in enumerate(vols):
        g = reference_cast(vol)
        if normalise:
            mean, std = np_stats(vol)
            g = (g - mean) / (1e-99 + std)
        for k in range(geometry.per_volume):
            (oz, ox, oy), _, _ = geometry.box(k)
            src = g[oz:oz + BZ, ox:ox + BX, oy:oy + BY]
            out[v * geometry.per_volume + k, :src.shape[0], :src.shape[1], :src.shape[2], 0] = src
    return out


def np_scatter(values, out, geometry, first=0):
    """owned boxes of bricks first .. first+len(values)-1 copied from `values` (n, BZ, BX, BY[, C]) into `out`, in place"""
    for j in range(len(values)):
        v, k = divmod(first + j, geometry.per_volume)
        (oz, ox, oy), (lz, lx, ly), (hz, hx, hy) = geometry.box(k)
        out[v, lz:hz, lx:hx, ly:hy] = values[j, lz - oz:hz - oz, lx - ox:hx - ox, ly - oy:hy - oy]
    return out
