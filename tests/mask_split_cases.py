"""Mask clean-up, splitting: the numpy / scipy restatement of include/sequitr_hip.h ("Mask clean-up: splitting") the GPU
path is pinned against, an independent pure-Python version that checks the restatement on small frames, and the mask
generators the tests share.

The restatement loops over frames and classes: scipy.ndimage.binary_erosion makes the seeds, scipy.ndimage.label numbers
them, T steps of a padded 4-neighbour minimum grow them back (all reads of a step see the step before), one more
padded minimum finds the cut.  Every comparison is exact.
"""
import numpy as np
from scipy import ndimage

from tests import mask_cleanup_cases as mc
from tests import objects_cases as oc

STRUCTURES = mc.STRUCTURES


def _min4(L, none):
    """the smallest label among the 4 neighbours of every pixel; `none` where there is no label, and outside the frame"""
    p = np.pad(np.where(L > 0, L, none), 1, constant_values=none)
    return np.minimum(np.minimum(p[:-2, 1:-1], p[2:, 1:-1]), np.minimum(p[1:-1, :-2], p[1:-1, 2:]))


def plane_labels(P, r, structure, T):
    """one class plane: (seeds, L_0, L_T).  Labels live on pixels of P only, so "a neighbour of the same class" is any
    neighbour that carries a label."""
    st = ndimage.generate_binary_structure(2, 1 if structure == 'cross' else 2)
    S = ndimage.binary_erosion(P, st, iterations=int(r))
    L0, n = ndimage.label(S)                                    # 4 neighbours, numbered by the first pixel in raster order
    L0 = L0.astype(np.int64)
    L = L0
    for _ in range(int(T)):
        nb = _min4(L, n + 1)
        L = np.where(P & (L == 0) & (nb <= n), nb, L)           # a new array: nothing is updated in place
    return S, L0, L


def split_ref(mask, r, structure='cross', reach=None, C=2):
    mask = np.asarray(mask, np.uint8)
    T = 2 * int(r) if reach is None else int(reach)
    out = mask.copy()
    for f in range(mask.shape[0]):
        for c in range(1, C):
            P = mask[f] == c
            if not P.any():
                continue
            _, _, L = plane_labels(P, r, structure, T)
            out[f][(L > 0) & (_min4(L, L.max() + 1) < L)] = 0
    return out


def step_ref(mask, step, C):
    if step['op'] == 'split':
        return split_ref(mask, step['erosions'], step.get('structure', 'cross'), step.get('reach'), C)
    return mc.step_ref(mask, step, C)


def steps_ref(mask, steps, C):
    for s in steps:
        mask = step_ref(mask, s, C)
    return mask


def count_objects(mask, C):
    mask = np.asarray(mask)
    return sum(ndimage.label(mask[f] == c)[1] for f in range(mask.shape[0]) for c in range(1, C))


def most_seeds_in_a_component(mask, r, structure, C):
    """over all frames and classes: the largest number of seeds that lie in one component"""
    best = 0
    for f in range(mask.shape[0]):
        for c in range(1, C):
            P = mask[f] == c
            S, L0, _ = plane_labels(P, r, structure, 0)
            comp, _ = ndimage.label(P)
            pairs = set(zip(comp[S].tolist(), L0[S].tolist()))
            per = {}
            for k, _l in pairs:
                per[k] = per.get(k, 0) + 1
            best = max([best] + list(per.values()))
    return best


# ---- the header's text with loops and sets: no scipy ---------------------------------------------------------------

def brute_split(mask, r, structure, reach, C):
    mask = np.asarray(mask, np.uint8)
    N, H, W = mask.shape
    T = 2 * r if reach is None else reach
    offs = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if structure == 'square' or dy == 0 or dx == 0]
    nb4 = ((-1, 0), (1, 0), (0, -1), (0, 1))
    out = mask.copy()
    for f in range(N):
        for c in range(1, C):
            P = set((y, x) for y in range(H) for x in range(W) if mask[f, y, x] == c)
            S = set(P)
            for _ in range(r):                                  # a pixel outside the frame is in no set: border value 0
                S = set(p for p in S if all((p[0] + dy, p[1] + dx) in S for dy, dx in offs))
            L, n = {}, 0
            for p in sorted(S):                                 # raster order
                if p in L:
                    continue
                n += 1
                L[p] = n
                stack = [p]
                while stack:
                    y, x = stack.pop()
                    for dy, dx in nb4:
                        q = (y + dy, x + dx)
                        if q in S and q not in L:
                            L[q] = n
                            stack.append(q)
            for _ in range(T):
                new = dict(L)                                   # the second buffer: reads see the step before
                for p in P:
                    if p in L:
                        continue
                    near = [L[(p[0] + dy, p[1] + dx)] for dy, dx in nb4 if (p[0] + dy, p[1] + dx) in L]
                    if near:
                        new[p] = min(near)
                L = new
            for p, l in L.items():
                if any(L.get((p[0] + dy, p[1] + dx), l) < l for dy, dx in nb4):
                    out[f, p[0], p[1]] = 0
    return out


# ---- generators -----------------------------------------------------------------------------------------------------

def _disk(m, cy, cx, rad, cls=1):
    yy, xx = np.mgrid[0:m.shape[0], 0:m.shape[1]]
    m[(yy - cy) ** 2 + (xx - cx) ** 2 <= rad * rad] = cls


def chain(m, cy, cx, rad, dist, count=2, vertical=False, cls=1):
    """`count` touching disks of radius `rad`, centres `dist` apart, the chain centred on (cy, cx)"""
    for i in range(count):
        o = int(round((i - (count - 1) / 2.0) * dist))
        _disk(m, cy + (o if vertical else 0), cx + (0 if vertical else o), rad, cls)


def disk_params(r):
    """(radius, distance of the centres) of touching disks whose neck an erosion by r removes while both cores survive
    it with either structure: the issue's figures for r = 8, scaled for r = 4"""
    return {4: (8, 14), 8: (12, 21)}[r]


def seam_pairs(tile, r, cls=1):
    """(1, 2R + 62, 2Cc + 44) with R x Cc tiles: a touching pair on every tile seam and every seam crossing, a chain of
    five across both vertical seams and a chain of three across a horizontal one; 10 objects made of 24 disks"""
    R, Cc = tile
    rad, dist = disk_params(r)
    m = np.zeros((2 * R + 62, 2 * Cc + 44), np.uint8)
    chain(m, R, Cc, rad, dist, cls=cls)
    chain(m, R, 2 * Cc, rad, dist, vertical=True, cls=cls)
    chain(m, 2 * R, Cc, rad, dist, vertical=True, cls=cls)
    chain(m, 2 * R, 2 * Cc, rad, dist, cls=cls)
    chain(m, 14, Cc, rad, dist, cls=cls)
    chain(m, 14, 2 * Cc, rad, dist, cls=cls)
    chain(m, R, 14, rad, dist, vertical=True, cls=cls)
    chain(m, 2 * R, 14, rad, dist, vertical=True, cls=cls)
    chain(m, 2 * R + 42, Cc + Cc // 2, rad, dist, count=5, cls=cls)
    chain(m, R, 2 * Cc + 28, rad, dist, count=3, vertical=True, cls=cls)
    return m[None]


SEAM_OBJECTS, SEAM_DISKS = 10, 24


def _blob(m, y, x, cls=1, half=2):
    m[max(y - half, 0):y + half + 1, max(x - half, 0):x + half + 1] = cls


def _path(m, points, cls=1):
    for (y0, x0), (y1, x1) in zip(points[:-1], points[1:]):
        m[min(y0, y1):max(y0, y1) + 1, min(x0, x1):max(x0, x1) + 1] = cls


def gaps(tile, widths=(1, 2, 3, 4, 5, 6, 13, 14, 15, 16, 17, 18, 19, 20, 37, 38, 39, 40)):
    """5 x 5 blobs (one seed each at erosions = 1) facing each other across one-pixel corridors of even and odd length that
    cross the first vertical tile seam: whether and where the cut falls depends on the step at which each growth arrives.
    The left blob has the smaller label."""
    Cc = tile[1]
    m = np.zeros((8 * len(widths) + 2, Cc + 40), np.uint8)
    for i, g in enumerate(widths):
        y, xl = 8 * i + 4, Cc - g // 2 - 3
        _blob(m, y, xl)
        _blob(m, y, xl + g + 5)
        m[y, xl:xl + g + 5] = 1
    return m[None]


def elbows(tile):
    """two one-pixel corridors with a blob at each end, bent around a tile corner: the growths from the four ends cross a
    vertical seam rightwards and leftwards and a horizontal one downwards and upwards, and meet after about 35 steps"""
    R, Cc = tile
    m = np.zeros((2 * R + 32, 2 * Cc + 32), np.uint8)
    for pts in ([(R - 14, Cc - 24), (R - 14, Cc + 16), (R + 16, Cc + 16)],
                [(2 * R + 12, 2 * Cc + 22), (2 * R + 12, 2 * Cc - 18), (2 * R - 18, 2 * Cc - 18)]):
        _path(m, pts)
        _blob(m, *pts[0])
        _blob(m, *pts[-1])
    return m[None]


def junction():
    """three blobs whose corridors of lengths 6, 9 and 13 meet in one pixel, and a side pocket next to the nearest one"""
    m = np.zeros((40, 44), np.uint8)
    _path(m, [(20, 4), (20, 20)])
    _path(m, [(8, 20), (20, 20)])
    _path(m, [(20, 20), (20, 39)])
    _path(m, [(24, 10), (20, 10)])
    for p in ((20, 11), (8, 20), (20, 36)):
        _blob(m, *p)
    return m[None]


def chambers(kind='spiral'):
    """objects_cases' spiral or comb, three pixels wide, with a 5 x 5 chamber every few cells along the winding corridor:
    at erosions = 2 the straight corridor holds no seed, each chamber one, and a growth arrives by the way along the
    corridor, not by the straight line.  One object."""
    small = (oc.spiral(h=11, w=15, cls=1) if kind == 'spiral' else oc.comb(h=9, w=15))[0]
    dist = np.full(small.shape, -1)                             # geodesic order along the corridor from its first pixel
    dist[0, 0], todo = 0, [(0, 0)]
    while todo:
        y, x = todo.pop(0)
        for dy, dx in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            p, q = y + dy, x + dx
            if 0 <= p < small.shape[0] and 0 <= q < small.shape[1] and small[p, q] and dist[p, q] < 0:
                dist[p, q] = dist[y, x] + 1
                todo.append((p, q))
    m = np.pad(np.kron(small, np.ones((3, 3), np.uint8)), 2)
    for d in range(0, int(dist.max()) + 1, 8 if kind == 'spiral' else 11):
        y, x = np.argwhere(dist == d)[0]
        _blob(m, 3 * y + 3, 3 * x + 3)
    return m[None]


def contact():
    """two classes touching along a line, each with two cores joined by a neck: a cut inside each class, no label crosses
    from one class into the other and nothing is cut between them"""
    m = np.zeros((44, 60), np.uint8)
    for cls, x in ((1, 2), (2, 30)):                            # columns 29 | 30 are the contact line
        m[4:18, x:x + 28] = cls
        m[18:26, x + 11:x + 17] = cls                           # the neck
        m[26:40, x:x + 28] = cls
    return m[None]


def frames_stacked():
    """(3, 20, 30): a blob in the last rows of a frame above one in the first rows of the next (labels must not leak), and
    a touching pair in every frame"""
    m = np.zeros((3, 20, 30), np.uint8)
    for f in range(3):
        m[f, 14:20, 3:12] = 1
        m[f, 0:6, 3:12] = 1
        chain(m[f], 10, 21, 4, 7)
    return m


def unknown_wall():
    """C = 3: a class-1 bar with a core at each end, cut through by a wall of bytes 3, 7 and 255: each half keeps its one
    seed, nothing conducts through the wall, nothing is cut; and beside it the same bar whole, which is cut"""
    m = np.zeros((1, 30, 40), np.uint8)
    for y0 in (2, 17):
        m[0, y0:y0 + 9, 2:13] = 1
        m[0, y0 + 3:y0 + 6, 13:27] = 1
        m[0, y0:y0 + 9, 27:38] = 1
    m[0, 5, 19], m[0, 6, 19], m[0, 7, 19] = 3, 7, 255
    return m


def splitting_cases(tile):
    """(name, mask, C, erosions, structure, reach): every one has a component with two seeds or more, loses a pixel or more
    and gains an object (tests/test_mask_split_cpu.py checks it)"""
    cases = []
    for r in (4, 8):
        for st in STRUCTURES:
            cases.append(('seam pairs r=%d %s' % (r, st), seam_pairs(tile, r), 2, r, st, None))
    cases.append(('seam pairs, class 2 of 3', seam_pairs(tile, 4, cls=2), 3, 4, 'cross', 8))
    cases.append(('gaps', gaps(tile), 2, 1, 'cross', 64))
    cases.append(('elbows', elbows(tile), 2, 1, 'square', 64))
    cases.append(('junction', junction(), 2, 1, 'cross', 20))
    cases.append(('spiral chambers', chambers('spiral'), 2, 2, 'cross', 64))
    cases.append(('comb chambers', chambers('comb'), 2, 2, 'cross', 64))
    cases.append(('classes in contact', contact(), 3, 3, 'square', 12))
    cases.append(('stacked frames', frames_stacked(), 2, 2, 'cross', None))
    cases.append(('unknown wall', unknown_wall(), 3, 2, 'cross', 16))
    return cases


def unchanged_cases(tile):
    """(name, mask, C, erosions, structure, reach): the mask comes back as it is"""
    R, Cc = tile
    cases = [('no seed: square erosion eats the cores', seam_pairs(tile, 8), 2, 16, 'square', 32),
             ('one-pixel corridors', oc.comb(), 2, 1, 'cross', 64),
             ('uniform class 1', np.ones((2, R + 3, Cc + 5), np.uint8), 2, 3, 'cross', None),
             ('uniform class 1, small', np.ones((1, 5, 7), np.uint8), 2, 1, 'square', 64),
             ('all background', np.zeros((2, 40, 70), np.uint8), 2, 2, 'cross', None),
             ('bytes >= C', np.full((1, 9, 10), 200, np.uint8), 3, 1, 'cross', 5),
             ('beyond reach', gaps(tile, widths=(30, 31, 40)), 2, 1, 'cross', 8),
             ('single disks', oc.disks(3, 1, 70, 130, 6, rmax=9), 2, 2, 'cross', None)]
    return cases


def split_shapes(tile):
    return mc.morph_shapes(tile) + [(2, 5, 7), (2, 1, 9), (2, 6, 1), (1, 3, 3)]
