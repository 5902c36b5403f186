"""Volume clean-up: the numpy / scipy restatement of include/sequitr_hip.h ("Volume clean-up") the GPU path is pinned
against, an independent pure-Python brute force that checks the restatement on small volumes, and the mask generators the
tests share.  Masks are (N, D, H, W) uint8.

The restatement loops over volumes and classes, calls scipy.ndimage.binary_erosion / dilation / opening / closing with the
3-D structures, binary_fill_holes, label (its default 3-D structure is generate_binary_structure(3, 1)) and numpy's
bincount, and applies the two merge rules of tests/mask_cleanup_cases.py.  Every comparison is exact.
"""
import numpy as np
from scipy import ndimage

from tests import mask_cleanup_cases as mc

OPS = mc.OPS
STRUCTURES = ('cross', 'cube')
PLANE_STRUCTURES = ('plane_cross', 'plane_square')
FACES = ('all', 'lateral')
_SCIPY = mc._SCIPY
merge_extensive, merge_anti = mc.merge_extensive, mc.merge_anti


def structure(name):
    if name in PLANE_STRUCTURES:
        return ndimage.generate_binary_structure(2, 1 if name == 'plane_cross' else 2)[None]
    return ndimage.generate_binary_structure(3, 1 if name == 'cross' else 3)


def _per_volume(mask, C, plane_fn, merge):
    mask = np.asarray(mask, np.uint8)
    assert mask.ndim == 4
    out = np.empty_like(mask)
    for v in range(mask.shape[0]):
        planes = {c: plane_fn(mask[v] == c) for c in range(1, C)}
        out[v] = merge(mask[v], planes, C)
    return out


def morph_ref(mask, op, iterations, st, C):
    merge = merge_extensive if op in ('dilate', 'close') else merge_anti
    return _per_volume(mask, C, lambda P: _SCIPY[op](P, structure(st), iterations=int(iterations)), merge)


def _as_slices(mask):
    mask = np.asarray(mask, np.uint8)
    return mask.reshape((-1,) + mask.shape[2:])


def fill_ref(mask, max_voxels, C, planar=False):
    if planar:                                                  # the planar restatement slice by slice
        return mc.fill_holes_ref(_as_slices(mask), max_voxels, C).reshape(np.shape(mask))

    def plane(P):
        cav = ndimage.binary_fill_holes(P) & ~P
        if max_voxels is not None and max_voxels > 0:
            lab, n = ndimage.label(cav)                         # 6-connected: the components of ~P away from the faces
            keep = np.bincount(lab.ravel(), minlength=n + 1) <= max_voxels
            keep[0] = False
            cav = keep[lab]
        return P | cav
    return _per_volume(mask, C, plane, merge_extensive)


def clear_border_ref(mask, C, faces='all'):
    def plane(P):
        lab, n = ndimage.label(P)
        hit = np.zeros(n + 1, bool)
        sides = [lab[:, 0], lab[:, -1], lab[:, :, 0], lab[:, :, -1]]    # the four lateral faces: h = 0, H-1, w = 0, W-1
        if faces == 'all':
            sides += [lab[0], lab[-1]]
        else:
            assert faces == 'lateral', faces
        for side in sides:
            hit[side] = True
        hit[0] = True
        return ~hit[lab]
    return _per_volume(mask, C, plane, merge_anti)


def step_ref(mask, step, C):
    op = step['op']
    if op in OPS:
        return morph_ref(mask, op, step.get('iterations', 1), step.get('structure', 'cross'), C)
    if op == 'fill_holes':
        return fill_ref(mask, step.get('max_voxels'), C, step.get('planar', False))
    assert op == 'clear_border', op
    return clear_border_ref(mask, C, step.get('faces', 'all'))


def steps_ref(mask, steps, C):
    for s in steps:
        mask = step_ref(mask, s, C)
    return mask


# ---- brute force: no scipy, sets of voxels --------------------------------------------------------------------------

def offsets(cube):
    offs = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)]
    return offs if cube else [o for o in offs if sum(abs(i) for i in o) <= 1]


def brute_step(S, shape, dilate, cube):
    """one elementary erosion / dilation of the voxel set S inside `shape`; outside the volume there is nothing"""
    D, H, W = shape
    offs = offsets(cube)
    out = set()
    for z in range(D):
        for y in range(H):
            for x in range(W):
                vals = [(z + a, y + b, x + c) in S for a, b, c in offs]
                if any(vals) if dilate else all(vals):
                    out.add((z, y, x))
    return out


def brute_morph_plane(P, op, r, cube):
    S = set(zip(*np.nonzero(P)))
    seq = {'erode': [False] * r, 'dilate': [True] * r, 'open': [False] * r + [True] * r, 'close': [True] * r + [False] * r}[op]
    for dilate in seq:
        S = brute_step(S, P.shape, dilate, cube)
    Q = np.zeros(P.shape, bool)
    for v in S:
        Q[v] = True
    return Q


def brute_components(P):
    """flood fill, 6 neighbours: a list of (cells, on a z-face, on a lateral face)"""
    D, H, W = P.shape
    seen = np.zeros(P.shape, bool)
    comps = []
    for start in zip(*np.nonzero(P)):
        if seen[start]:
            continue
        stack, cells, zface, side = [start], [], False, False
        seen[start] = True
        while stack:
            z, y, x = stack.pop()
            cells.append((z, y, x))
            zface = zface or z in (0, D - 1)
            side = side or y in (0, H - 1) or x in (0, W - 1)
            for a, b, c in offsets(False):
                q = (z + a, y + b, x + c)
                if 0 <= q[0] < D and 0 <= q[1] < H and 0 <= q[2] < W and P[q] and not seen[q]:
                    seen[q] = True
                    stack.append(q)
        comps.append((cells, zface, side))
    return comps


def brute(mask, step, C):
    """the header's text for one step, with loops instead of scipy (3-D structures, planar=False only)"""
    mask = np.asarray(mask, np.uint8)
    op = step['op']
    out = np.empty_like(mask)
    for v in range(mask.shape[0]):
        planes = {}
        for c in range(1, C):
            P = mask[v] == c
            if op in OPS:
                Q = brute_morph_plane(P, op, step.get('iterations', 1), step.get('structure', 'cross') == 'cube')
            elif op == 'fill_holes':
                Q = P.copy()
                for cells, zface, side in brute_components(~P):
                    if not zface and not side and (not step.get('max_voxels') or len(cells) <= step['max_voxels']):
                        for q in cells:
                            Q[q] = True
            else:
                Q = np.zeros_like(P)
                for cells, zface, side in brute_components(P):
                    if not side and not (zface and step.get('faces', 'all') == 'all'):
                        for q in cells:
                            Q[q] = True
            planes[c] = Q
        merge = merge_extensive if op in ('dilate', 'close', 'fill_holes') else merge_anti
        out[v] = merge(mask[v], planes, C)
    return out


# ---- generators -----------------------------------------------------------------------------------------------------

def random_volume(seed, n, d, h, w, C, density, unknown=True):
    """classes 1 .. C-1 at the given density; with `unknown` a sprinkle of bytes C, C + 3 and 255"""
    return mc.random_mask(seed, n * d, h, w, C, density, unknown).reshape(n, d, h, w)


def morph_shapes(tile):
    """(N, D, H, W): every axis at T - 1, T, T + 1 and 2T + 1 with the other two small, extents 1, 2, 3 on every axis,
    W at 63 .. 65 and 127 .. 130, and one volume of several bricks each way"""
    TD, TH, TW = tile
    out = [(1, d, 9, 70) for d in (TD - 1, TD, TD + 1, 2 * TD + 1)]
    out += [(1, 3, h, 70) for h in (TH - 1, TH, TH + 1, 2 * TH + 1)]
    out += [(1, 3, 9, w) for w in (TW - 1, TW, TW + 1, 2 * TW + 1)]
    out += [(2, 1, 9, 70), (1, 2, 9, 70), (2, 3, 1, 70), (1, 3, 2, 70), (1, 3, 3, 70), (2, 3, 9, 1), (1, 3, 9, 2), (1, 3, 9, 3),
            (1, 1, 1, 1), (2, 2, 2, 2), (1, 1, 1, 70), (1, 1, 9, 1), (2, 3, 1, 1), (1, 3, 3, 3)]
    out += [(1, 3, 5, w) for w in (63, 64, 65, 127, 128, 129, 130)]
    out += [(2, TD + 1, TH + 1, TW + 1), (1, 2 * TD + 1, TH + 3, 66)]
    return out


def seams(tile, cls=1):
    """(1, 2TD + 3, 2TH + 5, 2TW + 7): bars along each axis, plates and octahedra centred on every brick seam, edge and
    corner"""
    TD, TH, TW = tile
    D, H, W = 2 * TD + 3, 2 * TH + 5, 2 * TW + 7
    m = np.zeros((1, D, H, W), np.uint8)
    zz, yy, xx = np.mgrid[0:D, 0:H, 0:W]
    for z in (TD, 2 * TD):
        for y in (TH, 2 * TH):
            for x in (TW, 2 * TW):
                m[0][np.abs(zz - z) + np.abs(yy - y) + np.abs(xx - x) <= 5] = cls    # octahedra on the corners
            m[0, z - 2:z + 2, y - 2:y + 2, 20:60] = cls         # a bar along x on a (z, y) edge
        for x in (TW, 2 * TW):
            m[0, z - 2:z + 2, 10:22, x - 2:x + 2] = cls         # a bar along y on a (z, x) edge
        m[0, z - 1:z + 1, 40:52, 70:100] = cls                  # a plate lying in a z seam
        m[0, z - 6:z + 6, 24:27, 70:100] = cls                  # and one standing across it
    for y in (TH, 2 * TH):
        for x in (TW, 2 * TW):
            m[0, 3:6, y - 2:y + 2, x - 2:x + 2] = cls           # a short bar along z on a (y, x) edge
        m[0, 11:14, y - 1:y + 1, 104:120] = cls                 # a plate lying in a y seam
    for x in (TW, 2 * TW):
        m[0, 10:15, 44:54, x - 1:x + 1] = cls                   # a plate lying in an x seam
        m[0, 4:7, 56:60, x - 9:x + 9] = cls                     # a bar across it
    return m


def flush(d=12, h=40, w=70):
    """objects flush with each of the six faces, with an edge and a corner, one free in the middle"""
    m = np.zeros((1, d, h, w), np.uint8)
    m[0, 0:4, 10:20, 10:30] = 1
    m[0, d - 3:d, 22:34, 35:60] = 1
    m[0, 4:9, 0:6, 30:50] = 1
    m[0, 3:8, h - 5:h, 5:25] = 1
    m[0, 4:9, 12:24, 0:7] = 1
    m[0, 2:9, 8:20, w - 6:w] = 1
    m[0, 0:4, 0:4, 0:4] = 1
    m[0, d - 4:d, h - 4:h, w - 4:w] = 1
    m[0, d - 3:d, 0:5, 58:66] = 1                               # an edge
    m[0, 4:9, 24:32, 30:45] = 1
    return m


def shell(d, h, w, z0, y0, x0, z1, y1, x1, cls=1, thick=1):
    m = np.zeros((1, d, h, w), np.uint8)
    m[0, z0:z1, y0:y1, x0:x1] = cls
    m[0, z0 + thick:z1 - thick, y0 + thick:y1 - thick, x0 + thick:x1 - thick] = 0
    return m


def checkerboard(d, h, w, phase=0):
    zz, yy, xx = np.mgrid[0:d, 0:h, 0:w]
    return ((zz + yy + xx + phase) % 2)[None].astype(np.uint8)


def fill_cases():
    """(name, mask, C, max_voxels values)"""
    cases = []
    m = np.ones((1, 5, 7, 9), np.uint8)
    m[0, 1, 2, 3] = m[0, 3, 4, 7] = m[0, 2, 5, 5] = 0
    m[0, 0, 3, 3] = m[0, 2, 0, 4] = m[0, 2, 3, 8] = 0           # on a face: no cavities
    cases.append(('one-voxel cavities', m, 2, (None, 1)))
    cases.append(('several segments and planes', shell(9, 8, 230, 1, 1, 10, 8, 7, 215), 2,
                  (None, 5 * 4 * 203 - 1, 5 * 4 * 203, 5 * 4 * 203 + 1)))
    m = shell(8, 9, 20, 1, 1, 1, 7, 8, 12)
    m[0, 3, 4, 11] = 0                                          # one voxel of the wall is gone: no cavity any more
    t = m.copy()
    t[0, 2:5, 3:6, 12:20] = 1
    t[0, 3, 4, 11:20] = 0                                       # a tube from the hole in the wall to the face w = W - 1
    cases.append(('pierced shell', m, 2, (None,)))
    cases.append(('tunnel to a face', t, 2, (None,)))
    m = shell(7, 9, 10, 0, 1, 1, 6, 8, 9)
    m[0, 0] = np.where(m[0, 1] > 0, 1, 0)                       # no lid on plane 0: closed in every slice, open along z
    cases.append(('open to the first plane', m, 2, (None,)))
    m = shell(9, 10, 11, 1, 1, 1, 8, 9, 10)
    m[0, 4, 5, 5] = 2                                           # a foreign voxel inside: 5 * 6 * 7 = 210 voxels with it
    cases.append(('foreign voxel inside', m, 3, (None, 209, 210, 211, 208)))
    m = shell(13, 14, 15, 0, 0, 0, 13, 14, 15, cls=0)
    m[0, 1:12, 1:13, 1:14] = 2
    m[0, 2:11, 2:12, 2:13] = 0
    m[0, 3:10, 3:11, 3:12] = 1
    m[0, 4:9, 4:10, 4:11] = 0
    m[0, 6, 6, 6] = 7                                           # an unknown byte in the innermost cavity
    cases.append(('shells in shells', m, 3, (None, 5 * 6 * 7, 5 * 6 * 7 - 1, 500)))
    cases.append(('checkerboard', checkerboard(9, 10, 70), 2, (None, 1)))
    cases.append(('checkerboard, inverse', checkerboard(9, 10, 70, 1), 2, (None,)))
    cases.append(('one plane', np.stack([mc.object_in_ring()]), 3, (None,)))
    cases.append(('random', random_volume(5, 2, 9, 12, 70, 3, 0.75), 3, (None, 1, 3)))
    return cases


def border_cases():
    """(name, mask, C)"""
    cases = []
    D, H, W = 8, 12, 14
    m = np.zeros((1, D, H, W), np.uint8)
    m[0, 0:3, 3, 3] = 1                                         # a stick that touches z = 0 by one voxel
    m[0, D - 2:D, 8, 4] = 2                                     # z = D - 1
    m[0, 3, 0:3, 7] = 1                                         # h = 0
    m[0, 4, H - 2:H, 9] = 2                                     # h = H - 1
    m[0, 5, 5, 0:3] = 1                                         # w = 0
    m[0, 2, 6, W - 2:W] = 2                                     # w = W - 1
    m[0, 3:5, 5:7, 5:8] = 1                                     # free
    m[0, 5:7, 8:10, 10:12] = 2
    cases.append(('one voxel on each face', m, 3))
    m = np.zeros((1, D, H, W), np.uint8)
    for z in (0, D - 1):
        for y in (0, H - 1):
            for x in (0, W - 1):
                m[0, z, y, x] = 1                               # the eight corners
                m[0, abs(z - 1), abs(y - 1), abs(x - 1)] = 1    # touch them only diagonally: kept
    m[0, 0, 0, 5:8] = 1                                         # on an edge of two faces, one of them a z-face
    m[0, 3:5, 0, 0] = 2                                         # on a lateral edge
    m[0, 0, 5:7, 6] = 2                                         # on the z-face only: `lateral` keeps it
    m[0, D - 1, 8, 8:11] = 1
    cases.append(('edges and corners', m, 3))
    cases.append(('one plane', np.stack([mc.border_cases()[0][1]]), 3))
    m = np.zeros((1, 6, 8, 12), np.uint8)
    m[0, 2:4, 2:5, 0:3] = 1
    m[0, 2:4, 2:5, 3:6] = 2                                     # beside the class-1 object on the face, itself away from it
    m[0, 0, 6, 4:9] = 1
    m[0, 1, 6, 6] = 2                                           # under a class-1 object on the z-face, itself not on it
    m[0, 5, 1, 1] = 255
    m[0, 4, 1, 1] = 1                                           # under an unknown byte on the face: no class, no link
    cases.append(('two classes side by side', m, 3))
    cases.append(('random', random_volume(6, 2, 9, 20, 70, 3, 0.35), 3))
    cases.append(('random, dense', random_volume(7, 1, 10, 33, 130, 2, 0.8), 2))
    return cases


def volumes_u16(seed=5, N=2, Z=16, X=48, Y=48):
    """smooth blobs on a noisy background: the seeded net's mask has objects, cavities and specks"""
    rng = np.random.default_rng(seed)
    zz, xx, yy = np.mgrid[0:Z, 0:X, 0:Y]
    out = rng.integers(100, 600, (N, Z, X, Y)).astype(np.float64)
    for v in range(N):
        for _ in range(10):
            cz, cx, cy, r = rng.integers(0, Z), rng.integers(0, X), rng.integers(0, Y), rng.integers(3, 9)
            out[v] += 3000.0 * np.exp(-((zz - cz) ** 2 + (xx - cx) ** 2 + (yy - cy) ** 2) / (2.0 * r * r))
    return np.clip(out, 0, 65535).astype(np.uint16)
