"""Shape columns of segmented objects: the numpy / scipy restatement of include/sequitr_hip.h's text for sq_objects_shape
that the GPU path is pinned against, and the masks the tests share.

``shape_ref(mask, min_area, max_area)`` works per frame, per class ascending and per object of scipy.ndimage.label
(default structure: 4 neighbours in a plane, 6 in a volume) on the object's own crop O:
  sums      np.nonzero(O) + the crop's origin, products in int64
  faces     along every axis, O & ~(O shifted by +1) and O & ~(O shifted by -1), counted; a neighbour with the object's byte is
            in the object (4- / 6-connected labelling), so "not in O" is "outside the frame or another byte"; faces along
            the plane axis are 0 when the frame has one plane
  boundary  O & ~binary_erosion(O, cross, border_value=0), the cross planar when the frame has one plane
  perimeter (one plane only) ndimage.convolve of the boundary image with [[10,2,10],[2,1,2],[10,2,10]], constant 0 outside,
            then bincount: codes 5 7 15 17 25 27 straight, 21 33 diagonal, 13 23 mixed
Rows are sorted by (frame, class, key), key = the first voxel's linear index within its frame.
"""
import numpy as np
from scipy import ndimage

from tests import objects_cases as oc

NAMES = ('s_p', 's_r', 's_c', 's_pp', 's_rr', 's_cc', 's_pr', 's_pc', 's_rc', 'faces_p', 'faces_r', 'faces_c', 'boundary',
         'per_straight', 'per_diag', 'per_mixed')
KERNEL = np.array([[10, 2, 10], [2, 1, 2], [10, 2, 10]])
STRAIGHT, DIAG, MIXED = (5, 7, 15, 17, 25, 27), (21, 33), (13, 23)
PT_W, PT_H = 64, 32                                             # the perimeter kernel's tile (sq_objects_shape.hip)


def perimeter_counts(border):
    """[straight, diagonal, mixed] of one object's 2-D boundary image"""
    codes = ndimage.convolve(border.astype(np.int64), KERNEL, mode='constant', cval=0)
    hist = np.bincount(codes.ravel(), minlength=50)
    return [int(sum(hist[c] for c in group)) for group in (STRAIGHT, DIAG, MIXED)]


def object_shape(O, origin, one_plane):
    """the 16 columns of one object: O its boolean (p, r, c) crop, origin the crop's first voxel within the frame"""
    coords = [ax.astype(np.int64) + int(o) for ax, o in zip(np.nonzero(O), origin)]
    p, r, c = coords
    row = [int(p.sum()), int(r.sum()), int(c.sum())]
    row += [int((a * b).sum()) for a, b in ((p, p), (r, r), (c, c), (p, r), (p, c), (r, c))]
    pad = np.pad(O, 1)
    core = (slice(1, -1),) * 3
    for axis in range(3):
        if axis == 0 and one_plane:
            row.append(0)
            continue
        faces = 0
        for step in (1, -1):
            neighbour = np.roll(pad, step, axis=axis)[core]     # the padding keeps the roll from wrapping anything in
            faces += int((O & ~neighbour).sum())
        row.append(faces)
    if one_plane:
        border = O[0] & ~ndimage.binary_erosion(O[0], ndimage.generate_binary_structure(2, 1), border_value=0)
        row += [int(border.sum())] + perimeter_counts(border)
    else:
        border = O & ~ndimage.binary_erosion(O, ndimage.generate_binary_structure(3, 1), border_value=0)
        row += [int(border.sum()), 0, 0, 0]
    return row


def shape_ref(mask, min_area=1, max_area=None):
    """mask (N,H,W) or (N,D0,D1,D2) uint8 -> dict: frame, cls, key, area (k,) int64 and shape (k,16) int64 in NAMES' order,
    rows sorted by (frame, class, key); objects with an area outside [min_area, max_area] left out"""
    mask = np.asarray(mask)
    m4 = mask if mask.ndim == 4 else mask[:, None]
    N, P, H, W = m4.shape
    linear = np.arange(P * H * W, dtype=np.int64).reshape(P, H, W)
    head, rows = [], []
    for f in range(N):
        for cls in [int(v) for v in np.unique(m4[f]) if v > 0]:
            lab, n = ndimage.label(m4[f] == cls)
            per_class = []
            for k, sl in enumerate(ndimage.find_objects(lab)):
                O = lab[sl] == k + 1
                area = int(O.sum())
                if area < min_area or (max_area is not None and area > max_area):
                    continue
                key = int(linear[sl][O].min())
                per_class.append(((f, cls, key, area), object_shape(O, [s.start for s in sl], P == 1)))
            per_class.sort(key=lambda t: t[0])
            head += [t[0] for t in per_class]
            rows += [t[1] for t in per_class]
    head = np.asarray(head, np.int64).reshape(-1, 4)
    return {'frame': head[:, 0], 'cls': head[:, 1], 'key': head[:, 2], 'area': head[:, 3],
            'shape': np.asarray(rows, np.int64).reshape(-1, 16)}


# ---- masks ---------------------------------------------------------------------------------------------------------------
def noise(seed, shape, classes, fill=None):
    """random class bytes; with `fill` the fraction of non-zero pixels (else uniform over 0 .. classes)"""
    rng = np.random.default_rng(seed)
    m = rng.integers(1 if fill is not None else 0, classes + 1, shape)
    if fill is not None:
        m = np.where(rng.random(shape) < fill, m, 0)
    return m.astype(np.uint8)


def disk(radius, pad=2, cls=1):
    yy, xx = np.mgrid[-radius - pad:radius + pad + 1, -radius - pad:radius + pad + 1]
    return ((yy * yy + xx * xx <= radius * radius) * cls).astype(np.uint8)[None]


def checkerboard(h, w):
    """C = 2: every pixel is its own object with four exposed faces, every diagonal neighbour a same-class stranger"""
    yy, xx = np.mgrid[0:h, 0:w]
    return (1 + ((yy + xx) & 1)).astype(np.uint8)[None]


def seam_runs(w=200):
    """one run per second row: starting and ending on each side of the 64-lane seams at 64 and 128, through three
    segments, and the whole row; classes alternate"""
    spans = [(a, b) for a in (62, 63, 64, 65) for b in (63, 64, 65, 66) if a < b]
    spans += [(a + 64, b + 64) for a, b in spans] + [(3, 197), (0, w), (63, 129), (64, 128), (0, 64), (0, 65), (127, 128),
                                                     (128, 129), (w - 1, w), (0, 1)]
    m = np.zeros((1, 2 * len(spans) + 1, w), np.uint8)
    for i, (a, b) in enumerate(spans):
        m[0, 2 * i + 1, a:b] = 1 + (i % 2)
    return m


def diagonal_strangers():
    """two same-class pixels touching only at a corner (two objects), next to one object whose diagonal pixels connect the
    long way round, and pairs that a third pixel of the byte joins directly"""
    m = np.zeros((1, 12, 24), np.uint8)
    m[0, 1, 1] = m[0, 2, 2] = 1                                 # strangers
    m[0, 1, 6] = m[0, 2, 5] = 1                                 # strangers, the other diagonal
    for r, c in ((5, 5), (5, 4), (6, 4), (7, 4), (7, 5), (7, 6), (6, 6)):
        m[0, r, c] = 1                                          # (5,5) and (6,6): one object, joined round (6,5) = 0
    m[0, 6, 5] = 2                                              # ... with another class in the gap
    m[0, 4:6, 10] = m[0, 5, 11] = 1                             # an L: the diagonal pair is joined directly
    m[0, 8, 14] = m[0, 9, 15] = m[0, 10, 16] = 2                # a diagonal line of strangers of class 2
    m[0, 9, 14] = 1                                             # between two of them another class
    return m


def walls():
    """two classes in contact along a line, and a third class as a wall between two objects of one class"""
    m = np.zeros((1, 9, 70), np.uint8)
    m[0, 1:8, 2:30] = 1
    m[0, 1:8, 30:40] = 2
    m[0, 3:5, 40:66] = 1
    m[0, 1:8, 50] = 3                                           # cuts the bar in two
    return m


def flush():
    """objects flush with each frame edge and corner"""
    m = np.zeros((2, 37, 129), np.uint8)
    m[0, 0, :] = m[0, -1, :] = 1
    m[0, :, 0] = m[0, :, -1] = 1
    m[0, 10:20, 50:60] = 2
    m[1, 0, 0] = m[1, 0, -1] = m[1, -1, 0] = m[1, -1, -1] = 3
    m[1, 17:, 127:] = 1
    m[1, 0:3, 60:70] = 2
    m[1, 20:30, 0:2] = 2
    return m


def stacked_frames(n=3, h=5, w=70):
    """every frame's first and last rows full: the row above row 0 belongs to another frame"""
    m = np.zeros((n, h, w), np.uint8)
    m[:, 0, :] = 1
    m[:, -1, :] = 1
    m[:, :, 3] = 1
    return m


def stacked_volumes(n=2, p=3, h=4, w=66):
    m = np.zeros((n, p, h, w), np.uint8)
    m[:, 0] = 1
    m[:, -1] = 1
    m[:, :, 1, 5] = 1
    return m


def tile_seams(h=2 * PT_H + 6, w=2 * PT_W + 7):
    """boundary pixels on every seam and corner of the perimeter tiles: a diagonal line of strangers through each tile
    corner and bars lying on and crossing the seams in frame 0, a connected staircase across each corner in frame 1"""
    m = np.zeros((2, h, w), np.uint8)
    for r0 in range(PT_H, h, PT_H):
        for c0 in range(PT_W, w, PT_W):
            for d in range(-3, 3):                              # strangers: ... (r0-1, c0-1), (r0, c0) ...
                m[0, r0 + d, c0 + d] = 1
            for d in range(-3, 3):                              # a staircase two wide on the other diagonal, class 2
                m[1, r0 + d, c0 - d - 1] = 2
                m[1, r0 + d, c0 - d - 2] = 2
    for r0 in range(PT_H, h, PT_H):
        m[0, r0 - 1, 10:20] = 1                                 # a bar above the seam, one below, one across
        m[0, r0, 22:30] = 1
        m[0, r0 - 2:r0 + 2, 40:43] = 2
    for c0 in range(PT_W, w, PT_W):
        m[0, 5:12, c0 - 1] = 1
        m[0, 14:20, c0] = 1
        m[0, 22:26, c0 - 2:c0 + 2] = 2
    return m


def ball(radius, pad=1, cls=1):
    n = 2 * (radius + pad) + 1
    zz, yy, xx = np.mgrid[0:n, 0:n, 0:n] - (radius + pad)
    return ((zz * zz + yy * yy + xx * xx <= radius * radius) * cls).astype(np.uint8)[None]


def plates_and_shell():
    """plates one voxel thick along each axis and a hollow shell whose inner faces count"""
    m = np.zeros((1, 9, 20, 70), np.uint8)
    m[0, 1, 2:9, 2:30] = 1                                      # a plate in a plane
    m[0, 3:8, 12, 2:30] = 1                                     # a plate standing on a row
    m[0, 3:8, 14:19, 64] = 2                                    # ... and on a column, at the segment seam
    m[0, 2:9, 2:9, 40:47] = 2
    m[0, 3:8, 3:8, 41:46] = 0                                   # the shell: 7^3 - 5^3 voxels
    m[0, 5, 5, 43] = 1                                          # a voxel inside it
    return m


def far_object():
    """a 300 x 300 object at rows / columns >= 1700 of a 2048 x 2048 frame: products above 2^32, their sums above 2^48"""
    m = np.zeros((1, 2048, 2048), np.uint8)
    m[0, 1700:2000, 1710:2010] = 1
    m[0, 1800:1810, 1800:1810] = 0                              # a hole: inner boundary
    return m


spiral, comb, sized_objects, disks, blobs3d = oc.spiral, oc.comb, oc.sized_objects, oc.disks, oc.blobs3d
