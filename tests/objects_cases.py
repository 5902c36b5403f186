"""Object measurements: the numpy / scipy restatement the GPU path is pinned against, an independent pure-Python flood fill
that checks the restatement, and the mask generators the tests share.

``objects_ref(mask, image, min_area, max_area)`` measures per frame and per class ascending with scipy.ndimage.label
(default structure: 4 neighbours in a plane, 6 in a volume), sum_labels of ones, find_objects, center_of_mass(out, lab, idx)
-- the calls CentroidWriter.write makes (sequitr/utils.py:531-578) and their siblings -- and sum_labels / minimum / maximum
on the image: int64 for integer images; for float32 images math.fsum per object of the float64 values and of their exact
squares.  Labels are renumbered per frame in table order.
"""
import math

import numpy as np
from scipy import ndimage


def objects_ref(mask, image=None, min_area=1, max_area=None):
    """mask (N,H,W) or (N,D0,D1,D2) uint8.  Returns a dict of columns in the reference's order (frame, class ascending,
    scipy label order): frame, cls, key, area, bbox (k,6) [lo_plane, lo_row, lo_col, hi_plane, hi_row, hi_col], centroid
    (k,3) float64 along (plane, row, column), label, with an image also sum, sumsq, min, max (int64, or float64 for float32
    images); plus 'found' (components before the size filter), 'labels' int32 of the mask's shape (kept objects numbered
    per frame in table order) and 'mask' (the mask with dropped objects zeroed)."""
    mask = np.asarray(mask)
    vol = mask.ndim == 4
    cols = {k: [] for k in ('frame', 'cls', 'key', 'area', 'bbox', 'centroid', 'label', 'sum', 'sumsq', 'min', 'max')}
    labels = np.zeros(mask.shape, np.int32)
    kept_mask = np.zeros_like(mask)
    found = 0
    for f in range(mask.shape[0]):
        out = mask[f]
        rank = 0
        for c in [int(v) for v in np.unique(out) if v > 0]:
            lab, n = ndimage.label(out == c)
            if n == 0:
                continue
            found += n
            idx = np.arange(1, n + 1)
            area = ndimage.sum_labels(np.ones(out.shape, np.int64), lab, idx).astype(np.int64)
            boxes = ndimage.find_objects(lab)
            centres = np.asarray(ndimage.center_of_mass(out, lab, idx), np.float64).reshape(n, out.ndim)
            first = ndimage.minimum(np.arange(out.size, dtype=np.int64).reshape(out.shape), lab, idx).astype(np.int64)
            if image is not None:
                img = np.asarray(image)[f]
                if img.dtype.kind == 'u':
                    wide = img.astype(np.int64)
                    s = ndimage.sum_labels(wide, lab, idx).astype(np.int64)
                    q = ndimage.sum_labels(wide * wide, lab, idx).astype(np.int64)
                    assert np.all(q < 2 ** 53)                  # sum_labels adds in float64: exact below this
                    lo, hi = ndimage.minimum(wide, lab, idx).astype(np.int64), ndimage.maximum(wide, lab, idx).astype(np.int64)
                else:
                    wide = img.astype(np.float64)
                    s = np.array([math.fsum(wide[lab == i]) for i in idx])
                    q = np.array([math.fsum(wide[lab == i] * wide[lab == i]) for i in idx])
                    with np.errstate(invalid='ignore'):
                        lo = np.array([np.nanmin(wide[lab == i]) if not np.all(np.isnan(wide[lab == i])) else np.inf for i in idx])
                        hi = np.array([np.nanmax(wide[lab == i]) if not np.all(np.isnan(wide[lab == i])) else -np.inf for i in idx])
            for k in range(n):
                if area[k] < min_area or (max_area is not None and area[k] > max_area):
                    continue
                rank += 1
                sl = boxes[k]
                if not vol:
                    sl = (slice(0, 1),) + tuple(sl)
                cols['frame'].append(f)
                cols['cls'].append(c)
                cols['key'].append(first[k])
                cols['area'].append(area[k])
                cols['bbox'].append([s_.start for s_ in sl] + [s_.stop for s_ in sl])
                cols['centroid'].append(list(centres[k]) if vol else [0.0] + list(centres[k]))
                cols['label'].append(rank)
                if image is not None:
                    for name, v in (('sum', s), ('sumsq', q), ('min', lo), ('max', hi)):
                        cols[name].append(v[k])
                labels[f][lab == k + 1] = rank
                kept_mask[f][lab == k + 1] = c
    res = {}
    for name in ('frame', 'cls', 'key', 'area', 'label'):
        res[name] = np.asarray(cols[name], np.int64)
    res['bbox'] = np.asarray(cols['bbox'], np.int64).reshape(-1, 6)
    res['centroid'] = np.asarray(cols['centroid'], np.float64).reshape(-1, 3)
    if image is not None:
        dt = np.int64 if np.asarray(image).dtype.kind == 'u' else np.float64
        for name in ('sum', 'sumsq', 'min', 'max'):
            res[name] = np.asarray(cols[name], dt)
    res['found'], res['labels'], res['mask'] = found, labels, kept_mask
    return res


def flood_objects(mask):
    """independent check of objects_ref: pure-Python flood fill in raster order, per frame; returns rows
    (frame, class, key, area, lo..., hi..., sum of coordinates as exact integers) sorted by (frame, class, key)"""
    mask = np.asarray(mask)
    vol = mask.ndim == 4
    m4 = mask if vol else mask[:, None]
    N, P, H, W = m4.shape
    rows = []
    for f in range(N):
        seen = np.zeros((P, H, W), bool)
        for p in range(P):
            for r in range(H):
                for c in range(W):
                    v = int(m4[f, p, r, c])
                    if v == 0 or seen[p, r, c]:
                        continue
                    stack, cells = [(p, r, c)], []
                    seen[p, r, c] = True
                    while stack:
                        a, b, d = stack.pop()
                        cells.append((a, b, d))
                        for da, db, dd in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
                            x, y, z = a + da, b + db, d + dd
                            if 0 <= x < P and 0 <= y < H and 0 <= z < W and not seen[x, y, z] and int(m4[f, x, y, z]) == v:
                                seen[x, y, z] = True
                                stack.append((x, y, z))
                    cells = np.array(cells)
                    rows.append((f, v, (p * H + r) * W + c, len(cells)) + tuple(cells.min(0)) + tuple(cells.max(0) + 1)
                                + tuple(int(t) for t in cells.sum(0)))
    rows.sort(key=lambda t: t[:3])
    return rows


def disks(seed, n, h, w, count, classes=1, rmax=9):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((n, h, w), np.uint8)
    for i in range(n):
        for _ in range(count):
            cy, cx, r = rng.integers(0, h), rng.integers(0, w), rng.integers(1, rmax)
            m[i][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = rng.integers(1, classes + 1)
    return m


def blobs3d(seed, n, z, x, y, count, classes=2, rmax=5):
    rng = np.random.default_rng(seed)
    zz, xx, yy = np.mgrid[0:z, 0:x, 0:y]
    m = np.zeros((n, z, x, y), np.uint8)
    for i in range(n):
        for _ in range(count):
            cz, cx, cy, r = rng.integers(0, z), rng.integers(0, x), rng.integers(0, y), rng.integers(1, rmax)
            m[i][(zz - cz) ** 2 + (xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = rng.integers(1, classes + 1)
    return m


def spiral(h=33, w=70, cls=2):
    """one long winding component, drawn by a walk that turns right whenever the cell two ahead is taken: merges that
    re-root again and again"""
    m = np.zeros((1, h, w), np.uint8)
    r, c, dr, dc = 0, 0, 0, 1
    m[0, r, c] = cls
    while True:
        for _ in range(2):                                      # straight on, else one right turn
            nr, nc, ar, ac = r + dr, c + dc, r + 2 * dr, c + 2 * dc
            if 0 <= nr < h and 0 <= nc < w and m[0, nr, nc] == 0 and not (0 <= ar < h and 0 <= ac < w and m[0, ar, ac]):
                break
            dr, dc = dc, -dr
        else:
            return m
        r, c = nr, nc
        m[0, r, c] = cls


def comb(h=33, w=70):
    """teeth hanging from the bottom row: every tooth is its own run until the last row joins them"""
    m = np.zeros((1, h, w), np.uint8)
    m[0, :, ::2] = 1
    m[0, h - 1, :] = 1
    return m


def sized_objects():
    """one (1, 12, 64) mask with nine objects of areas 1 .. 9 (horizontal bars and an L), class 1 and 2 alternating"""
    m = np.zeros((1, 12, 64), np.uint8)
    col = 0
    for a in range(1, 10):
        c = 1 + (a % 2)
        if a < 6:
            m[0, 2, col:col + a] = c
            col += a + 1
        else:                                                   # an L: (a - 3) across, 3 more down
            m[0, 5, col:col + a - 3] = c
            m[0, 6:9, col] = c
            col += a - 3 + 1
    return m
