"""Volume clean-up, splitting: the numpy / scipy restatement of include/sequitr_hip.h ("Volume clean-up: splitting") the
GPU path is pinned against, an independent pure-Python version that checks the restatement on small volumes, and the mask
generators the tests share.  Masks are (N, D, H, W) uint8.

The restatement loops over volumes and classes: scipy.ndimage.binary_erosion makes the seeds, scipy.ndimage.label (its
default 3-D structure, 6 neighbours) numbers them, T steps of a padded 6-neighbour minimum grow them back (all reads of a
step see the step before), one more padded minimum finds the cut.  Every comparison is exact.
"""
import numpy as np
from scipy import ndimage

from tests import volume_cleanup_cases as vc

STRUCTURES = ('cross', 'cube', 'plane_cross', 'plane_square')


def default_reach(r, structure):
    return (3 if structure == 'cube' else 2) * int(r)


def _min6(L, none):
    """the smallest label among the 6 neighbours of every voxel; `none` where there is no label, and outside the volume"""
    p = np.pad(np.where(L > 0, L, none), 1, constant_values=none)
    c = p[1:-1, 1:-1, 1:-1]
    out = np.full(c.shape, none, p.dtype)
    for sl in ((slice(0, -2), slice(1, -1), slice(1, -1)), (slice(2, None), slice(1, -1), slice(1, -1)),
               (slice(1, -1), slice(0, -2), slice(1, -1)), (slice(1, -1), slice(2, None), slice(1, -1)),
               (slice(1, -1), slice(1, -1), slice(0, -2)), (slice(1, -1), slice(1, -1), slice(2, None))):
        out = np.minimum(out, p[sl])
    return out


def volume_labels(P, r, structure, T):
    """one class plane of one volume: (seeds, L_0, L_T).  Labels live on voxels of P only, so "a neighbour of the same
    class" is any neighbour that carries a label."""
    S = ndimage.binary_erosion(P, vc.structure(structure), iterations=int(r))
    L0, n = ndimage.label(S)                                    # 6 neighbours, numbered by the first voxel in raster order
    L0 = L0.astype(np.int64)
    L = L0
    for _ in range(int(T)):
        nb = _min6(L, n + 1)
        new = np.where(P & (L == 0) & (nb <= n), nb, L)         # a new array: nothing is updated in place
        if np.array_equal(new, L):
            break                                               # a step that changes nothing: so does every later one
        L = new
    return S, L0, L


def split3d_ref(mask, r, structure='cross', reach=None, C=2):
    mask = np.asarray(mask, np.uint8)
    assert mask.ndim == 4
    T = default_reach(r, structure) if reach is None else int(reach)
    out = mask.copy()
    for v in range(mask.shape[0]):
        for c in range(1, C):
            P = mask[v] == c
            if not P.any():
                continue
            _, _, L = volume_labels(P, r, structure, T)
            out[v][(L > 0) & (_min6(L, L.max() + 1) < L)] = 0
    return out


def step_ref(mask, step, C):
    if step['op'] == 'split3d':
        return split3d_ref(mask, step['erosions'], step.get('structure', 'cross'), step.get('reach'), C)
    return vc.step_ref(mask, step, C)


def steps_ref(mask, steps, C):
    for s in steps:
        mask = step_ref(mask, s, C)
    return mask


def count_objects(mask, C):
    mask = np.asarray(mask)
    return sum(ndimage.label(mask[v] == c)[1] for v in range(mask.shape[0]) for c in range(1, C))


def most_seeds_in_a_component(mask, r, structure, C):
    """over all volumes and classes: the largest number of seeds that lie in one component"""
    best = 0
    for v in range(mask.shape[0]):
        for c in range(1, C):
            P = mask[v] == c
            S, L0, _ = volume_labels(P, r, structure, 0)
            comp, _ = ndimage.label(P)
            per = {}
            for k, _l in set(zip(comp[S].tolist(), L0[S].tolist())):
                per[k] = per.get(k, 0) + 1
            best = max([best] + list(per.values()))
    return best


# ---- the header's text with loops and sets: no scipy ---------------------------------------------------------------

NB6 = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))


def _erosion_offsets(structure):
    offs = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)]
    if structure == 'cube':
        return offs
    if structure == 'cross':
        return [o for o in offs if abs(o[0]) + abs(o[1]) + abs(o[2]) <= 1]
    if structure == 'plane_square':
        return [o for o in offs if o[0] == 0]
    assert structure == 'plane_cross', structure
    return [o for o in offs if o[0] == 0 and abs(o[1]) + abs(o[2]) <= 1]


def brute_split3d(mask, r, structure, reach, C):
    mask = np.asarray(mask, np.uint8)
    N, D, H, W = mask.shape
    T = default_reach(r, structure) if reach is None else reach
    offs = _erosion_offsets(structure)
    out = mask.copy()

    def add(p, o):
        return (p[0] + o[0], p[1] + o[1], p[2] + o[2])

    for v in range(N):
        for c in range(1, C):
            P = set((z, y, x) for z in range(D) for y in range(H) for x in range(W) if mask[v, z, y, x] == c)
            S = set(P)
            for _ in range(r):                                  # a voxel outside the volume is in no set: border value 0
                S = set(p for p in S if all(add(p, o) in S for o in offs))
            L, n = {}, 0
            for p in sorted(S):                                 # raster order
                if p in L:
                    continue
                n += 1
                L[p] = n
                stack = [p]
                while stack:
                    q0 = stack.pop()
                    for o in NB6:
                        q = add(q0, o)
                        if q in S and q not in L:
                            L[q] = n
                            stack.append(q)
            for _ in range(T):
                new = dict(L)                                   # the second buffer: reads see the step before
                for p in P:
                    if p in L:
                        continue
                    near = [L[add(p, o)] for o in NB6 if add(p, o) in L]
                    if near:
                        new[p] = min(near)
                L = new
            for p, l in L.items():
                if any(L.get(add(p, o), l) < l for o in NB6):
                    out[v][p] = 0
    return out


# ---- generators -----------------------------------------------------------------------------------------------------

def ball(m, centre, rad, cls=1):
    zz, yy, xx = np.mgrid[0:m.shape[0], 0:m.shape[1], 0:m.shape[2]]
    m[(zz - centre[0]) ** 2 + (yy - centre[1]) ** 2 + (xx - centre[2]) ** 2 <= rad * rad] = cls


def chain(m, neck, axis, rad, dist, count=2, cls=1):
    """`count` touching balls of radius `rad`, centres `dist` apart along `axis`, the chain centred on the voxel `neck`"""
    for i in range(count):
        c = list(neck)
        c[axis] += int(round((i - (count - 1) / 2.0) * dist))
        ball(m, c, rad, cls)


def ball_params(r):
    """(radius, distance of the centres) of touching balls whose neck an erosion by r removes while both cores survive:
    the figures checked with scipy for r = 4 (all four structures) and r = 8 (cross and the plane structures)"""
    return {3: (6, 10), 4: (8, 14), 8: (12, 21)}[r]


def pair(shape, neck, axis, r, cls=1):
    m = np.zeros(shape, np.uint8)
    chain(m, neck, axis, *ball_params(r), cls=cls)
    return m


def seam_pairs(tile, r=4, cls=1):
    """(12, 4 TD + 4, 2 TH + 8, TW + 24) for the (8, 16, 32) brick: one touching pair per volume, along each of the three
    axes, its neck on a brick face, on each of the two edges and on the corner that the face has"""
    TD, TH, TW = tile
    shape = (4 * TD + 4, 2 * TH + 8, TW + 24)
    seam, mid = (2 * TD, TH, TW), (2 * TD - 4, TH + 6, TW - 12)
    vols = []
    for axis in range(3):
        for on in ((False, False), (True, False), (False, True), (True, True)):
            others = [a for a in range(3) if a != axis]
            neck = [0, 0, 0]
            neck[axis] = seam[axis]
            for a, s in zip(others, on):
                neck[a] = seam[a] if s else mid[a]
            vols.append(pair(shape, neck, axis, r, cls))
    return np.stack(vols)


SEAM_VOLUMES = 12


def chain_of_three(tile, cls=1):
    """three balls in a row along y across two brick seams; 1 object -> 3"""
    TD, TH, TW = tile
    m = np.zeros((1, 2 * TD + 4, 3 * TH, TW - 8), np.uint8)
    chain(m[0], (TD + 1, TH + TH // 2, (TW - 8) // 2), 1, 8, 14, count=3, cls=cls)
    return m


def blob(m, p, cls=1, half=2):
    m[max(p[0] - half, 0):p[0] + half + 1, max(p[1] - half, 0):p[1] + half + 1, max(p[2] - half, 0):p[2] + half + 1] = cls


def path(m, points, cls=1):
    for a, b in zip(points[:-1], points[1:]):
        m[min(a[0], b[0]):max(a[0], b[0]) + 1, min(a[1], b[1]):max(a[1], b[1]) + 1, min(a[2], b[2]):max(a[2], b[2]) + 1] = cls


GAP_WIDTHS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 17, 18, 19, 20, 21, 22, 29, 30)


def gaps(tile, axis, widths=GAP_WIDTHS):
    """5 x 5 x 5 blobs (one seed each at erosions = 1) facing each other along one-voxel corridors of even and odd length
    that run along `axis` and cross a brick seam of that axis: whether and where the cut falls depends on the
    step at which each growth arrives.  The blob nearer the origin has the smaller label."""
    T = tile[axis] * -(-24 // tile[axis])                       # the first seam of that axis at 24 or beyond
    m = np.zeros((7, 8 * len(widths) + 2, T + 36), np.uint8)    # (thickness, lanes, along the corridor)
    for i, g in enumerate(widths):
        v, lo = 8 * i + 4, T - g // 2 - 3
        blob(m, (3, v, lo))
        blob(m, (3, v, lo + g + 5))
        m[3, v, lo:lo + g + 5] = 1
    return np.ascontiguousarray(np.moveaxis(m, 2, axis))[None]


def elbows(tile):
    """two one-voxel corridors with a blob at each end, bent round a brick edge in the (z, y) and in the (z, x) plane: the
    growths cross a z seam and a y (or x) seam and meet after about 15 steps"""
    TD, TH, TW = tile
    m = np.zeros((1, 2 * TD + 8, TH + 16, TW + 16), np.uint8)
    for pts in ([(TD - 4, TH - 10, 4), (TD - 4, TH + 5, 4), (TD + 9, TH + 5, 4)],
                [(TD + 9, 4, TW - 10), (TD + 9, 4, TW + 5), (TD - 4, 4, TW + 5)]):
        path(m[0], pts)
        blob(m[0], pts[0])
        blob(m[0], pts[-1])
    return m


def junction():
    """three blobs whose corridors of lengths 4, 7 and 11 along z, y and x meet in one voxel"""
    m = np.zeros((1, 12, 16, 24), np.uint8)
    j = (8, 3, 3)
    path(m[0], [(2, 3, 3), j])
    path(m[0], [j, (8, 12, 3)])
    path(m[0], [j, (8, 3, 20)])
    for p in ((2, 3, 3), (8, 12, 3), (8, 3, 20)):
        blob(m[0], p)
    return m


def dumbbell(r, cls=1):
    """two boxes of side 2 r + 3 (a 3 x 3 x 3 core survives r erosions with every structure) joined along x by a
    one-voxel corridor of 2 voxels, one voxel of background around: the growths meet after r + 1 steps"""
    s = 2 * r + 3
    m = np.zeros((1, s + 2, s + 2, 2 * s + 4), np.uint8)
    m[0, 1:s + 1, 1:s + 1, 1:s + 1] = cls
    m[0, 1:s + 1, 1:s + 1, s + 3:2 * s + 3] = cls
    h = s // 2 + 1
    m[0, h, h, s + 1:s + 3] = cls
    return m


def necked(m, p, axis=2, cls=1):
    """two 5 x 5 x 5 blobs, the first centred on p, joined by a corridor of two voxels along `axis`: cut at erosions = 1"""
    q = list(p)
    q[axis] += 7
    blob(m, p, cls)
    blob(m, q, cls)
    path(m, [tuple(p), tuple(q)], cls)


def slices_stacked():
    """(1, 13, 12, 30): blobs in the last rows of slices 0 .. 4 and in the first rows of slices 5 .. 9 -- row H - 1 of
    slice 4 and row 0 of slice 5 are linear neighbours through + W, not neighbours in the volume -- at the same and at
    other columns; a necked pair elsewhere"""
    m = np.zeros((1, 13, 12, 30), np.uint8)
    m[0, 0:5, 7:12, 2:7] = 1
    m[0, 5:10, 0:5, 2:7] = 1                                    # the same columns
    m[0, 0:5, 7:12, 10:15] = 1
    m[0, 5:10, 0:5, 16:21] = 1                                  # other columns
    necked(m[0], (10, 8, 18))
    return m


def row_ends():
    """a blob at the end of rows 0 .. 4 and one at the start of rows 5 .. 9: the last voxel of a row and the first of the
    next are no neighbours"""
    m = np.zeros((1, 7, 18, 16), np.uint8)
    m[0, 1:6, 0:5, 11:16] = 1
    m[0, 1:6, 5:10, 0:5] = 1
    necked(m[0], (3, 14, 3))
    return m


def volumes_stacked():
    """(3, 6, 9, 30): a blob flush with the last slice of volume n at the rows and columns of one flush with the first
    slice of volume n + 1 -- linear neighbours through + H W, in different volumes; a necked pair in every volume"""
    m = np.zeros((3, 6, 9, 30), np.uint8)
    cols = (slice(1, 6), slice(8, 13))
    for n in range(3):
        m[n, 1:6, 2:7, cols[n % 2]] = 1                         # flush with the last slice
        m[n, 0:5, 2:7, cols[(n + 1) % 2]] = 1                   # flush with the first, under volume n - 1's blob
        necked(m[n], (3, 4, 17))
    return m


def contact():
    """two classes touching along a plane, each with two cores joined by a neck: a cut inside each class, no label crosses
    from one class into the other and nothing is cut between them"""
    m = np.zeros((1, 9, 30, 24), np.uint8)
    for cls, x in ((1, 1), (2, 12)):                            # columns 11 | 12 are the contact plane
        m[0, 1:8, 2:12, x:x + 11] = cls
        m[0, 3:6, 12:18, x + 4:x + 7] = cls                     # the neck
        m[0, 1:8, 18:28, x:x + 11] = cls
    return m


def unknown_wall():
    """C = 3: a class-1 bar with a core at each end, cut through by a wall of bytes 3, 7 and 255: each half keeps its one
    seed, nothing conducts through the wall, nothing is cut; and beside it the same bar whole, which is cut"""
    m = np.zeros((1, 9, 22, 40), np.uint8)
    for y0 in (1, 12):
        m[0, 1:8, y0:y0 + 9, 2:13] = 1
        m[0, 3:6, y0 + 3:y0 + 6, 13:27] = 1
        m[0, 1:8, y0:y0 + 9, 27:38] = 1
    m[0, 3:6, 4, 19], m[0, 3:6, 5, 19], m[0, 3:6, 6, 19] = 3, 7, 255
    return m


def splitting_cases(tile):
    """(name, mask, C, erosions, structure, reach): every one has a component with two seeds or more, loses a voxel or more
    and gains an object (tests/test_volume_split_cpu.py checks it)"""
    cases = []
    for st in STRUCTURES:
        cases.append(('seam pairs r=4 %s' % st, seam_pairs(tile), 2, 4, st, 12 if st == 'cube' else 8))
    cases.append(('seam pairs, class 2 of 3', seam_pairs(tile, cls=2), 3, 4, 'cross', None))
    cases.append(('chain of three', chain_of_three(tile), 2, 4, 'cross', None))
    for st in ('cross', 'plane_cross', 'plane_square'):
        cases.append(('pair r=8 %s' % st, pair((28, 28, 50), (14, 14, 25), 2, 8)[None], 2, 8, st, None))
    for axis in range(3):
        cases.append(('gaps along axis %d' % axis, gaps(tile, axis), 2, 1, 'cross', 64))
    cases.append(('elbows', elbows(tile), 2, 1, 'cube', 64))
    cases.append(('junction', junction(), 2, 1, 'cross', 20))
    cases.append(('slices stacked', slices_stacked(), 2, 1, 'cross', None))
    cases.append(('row ends', row_ends(), 2, 1, 'plane_square', None))
    cases.append(('volumes stacked', volumes_stacked(), 2, 1, 'cube', None))
    cases.append(('classes in contact', contact(), 3, 2, 'cube', None))
    cases.append(('unknown wall', unknown_wall(), 3, 2, 'cross', 16))
    return cases


def unchanged_cases(tile):
    """(name, mask, C, erosions, structure, reach): the mask comes back as it is"""
    TD, TH, TW = tile
    single = np.zeros((2, 20, 24, 40), np.uint8)
    ball(single[0], (10, 12, 12), 8)
    ball(single[0], (8, 10, 31), 6)
    ball(single[1], (9, 12, 20), 7)
    return [('no seed: the erosion eats the cores', seam_pairs(tile)[:3], 2, 9, 'cube', 27),
            ('one seed per component', single, 2, 2, 'cross', None),
            ('beyond reach', gaps(tile, 2, widths=(20, 21, 30)), 2, 1, 'cross', 5),
            ('uniform class 1', np.ones((2, TD + 3, TH + 5, TW + 7), np.uint8), 2, 3, 'cross', None),
            ('uniform class 1, small', np.ones((1, 3, 5, 7), np.uint8), 2, 1, 'plane_square', 64),
            ('all background', np.zeros((2, 9, 20, 40), np.uint8), 2, 2, 'cube', None),
            ('bytes >= C', np.full((1, 5, 9, 10), 200, np.uint8), 3, 1, 'cross', 5)]


def erosion_chain_cases():
    """(name, mask, C, erosions, structure): one to four chained 3-D erosion launches, and the planar one at both ends"""
    cases = [('dumbbell r=%d %s' % (r, st), dumbbell(r), 2, r, st) for st in ('cross', 'cube') for r in (1, 4, 5, 8, 9, 16)]
    cases += [('dumbbell r=%d %s' % (r, st), dumbbell(r), 2, r, st) for st in ('plane_cross', 'plane_square') for r in (1, 16)]
    return cases


def split_shapes(tile):
    """(N, D, H, W): every axis at 1, 2, 3, T - 1, T, T + 1 and 2 T + 1 with the other two small; W at 63 .. 65 and
    127 .. 130 (the row scan's and the morph kernels' 64-lane segments); volumes smaller than the halo on one, two and
    three axes; N = 1 and 2"""
    TD, TH, TW = tile
    out = [(1 + i % 2, d, 9, 21) for i, d in enumerate((1, 2, 3, TD - 1, TD, TD + 1, 2 * TD + 1))]
    out += [(1 + i % 2, 5, h, 21) for i, h in enumerate((1, 2, 3, TH - 1, TH, TH + 1, 2 * TH + 1))]
    out += [(1 + i % 2, 5, 9, w) for i, w in enumerate((1, 2, 3, TW - 1, TW, TW + 1, 2 * TW + 1))]
    out += [(2, 3, 5, w) for w in (63, 64, 65, 127, 128, 129, 130)]
    out += [(1, 1, 1, 1), (2, 2, 2, 2), (2, 3, 3, 3), (1, 3, 3, 40), (1, 2, 20, 2), (2, 12, 1, 3), (2, TD + 1, TH + 1, TW + 1)]
    return out
