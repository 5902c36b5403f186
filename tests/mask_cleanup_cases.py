"""Mask clean-up: the numpy / scipy restatement of include/sequitr_hip.h ("Mask clean-up") the GPU path is pinned against,
an independent pure-Python brute force that checks the restatement on small frames, and the mask generators the tests share.

The restatement loops over frames and classes, calls scipy.ndimage.binary_erosion / dilation / opening / closing,
binary_fill_holes, label and numpy's bincount, and applies the header's two merge rules.  Every comparison is exact.
"""
import numpy as np
from scipy import ndimage

from tests import objects_cases as oc

OPS = ('erode', 'dilate', 'open', 'close')
STRUCTURES = ('cross', 'square')
_SCIPY = {'erode': ndimage.binary_erosion, 'dilate': ndimage.binary_dilation, 'open': ndimage.binary_opening,
          'close': ndimage.binary_closing}


def merge_extensive(mask, planes, C):
    """out = mask wherever mask > 0, elsewhere the smallest c whose processed plane is set, else 0"""
    out = mask.copy()
    for c in range(1, C):
        out[(out == 0) & planes[c]] = c                         # ascending: a pixel a smaller class took is no longer 0
    return out


def merge_anti(mask, planes, C):
    """out = c where the processed plane of c is set and mask == c, else 0; bytes >= C stay"""
    out = np.where(mask >= C, mask, 0).astype(np.uint8)
    for c in range(1, C):
        out[planes[c] & (mask == c)] = c
    return out


def _per_frame(mask, C, plane_fn, merge):
    mask = np.asarray(mask, np.uint8)
    out = np.empty_like(mask)
    for f in range(mask.shape[0]):
        planes = {c: plane_fn(mask[f] == c) for c in range(1, C)}
        out[f] = merge(mask[f], planes, C)
    return out


def morph_ref(mask, op, iterations, structure, C):
    st = ndimage.generate_binary_structure(2, 1 if structure == 'cross' else 2)
    merge = merge_extensive if op in ('dilate', 'close') else merge_anti
    return _per_frame(mask, C, lambda P: _SCIPY[op](P, st, iterations=int(iterations)), merge)


def fill_holes_ref(mask, max_area, C):
    def plane(P):
        holes = ndimage.binary_fill_holes(P) & ~P
        if max_area is not None and max_area > 0:
            lab, n = ndimage.label(holes)                       # 4-connected: the components of ~P away from the edge
            keep = np.bincount(lab.ravel(), minlength=n + 1) <= max_area
            keep[0] = False
            holes = keep[lab]
        return P | holes
    return _per_frame(mask, C, plane, merge_extensive)


def clear_border_ref(mask, C):
    def plane(P):
        lab, n = ndimage.label(P)
        edge = np.zeros(n + 1, bool)
        for line in (lab[0], lab[-1], lab[:, 0], lab[:, -1]):
            edge[line] = True
        edge[0] = True
        return ~edge[lab]
    return _per_frame(mask, C, plane, merge_anti)


def step_ref(mask, step, C):
    op = step['op']
    if op in OPS:
        return morph_ref(mask, op, step.get('iterations', 1), step.get('structure', 'cross'), C)
    if op == 'fill_holes':
        return fill_holes_ref(mask, step.get('max_area'), C)
    assert op == 'clear_border', op
    return clear_border_ref(mask, C)


def steps_ref(mask, steps, C):
    for s in steps:
        mask = step_ref(mask, s, C)
    return mask


# ---- brute force: no scipy ------------------------------------------------------------------------------------------

def brute_step(P, dilate, square):
    """one 3x3 erosion / dilation of a Boolean plane on a zero-padded copy, pixel by pixel"""
    H, W = P.shape
    pad = np.zeros((H + 2, W + 2), bool)
    pad[1:-1, 1:-1] = P
    offs = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if square or dy == 0 or dx == 0]
    out = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            vals = [bool(pad[1 + y + dy, 1 + x + dx]) for dy, dx in offs]
            out[y, x] = any(vals) if dilate else all(vals)
    return out


def brute_morph_plane(P, op, r, square):
    seq = {'erode': [False] * r, 'dilate': [True] * r, 'open': [False] * r + [True] * r, 'close': [True] * r + [False] * r}[op]
    for dilate in seq:
        P = brute_step(P, dilate, square)
    return P


def brute_components(P):
    """flood fill, 4 neighbours: a list of (cells, touches the frame edge)"""
    H, W = P.shape
    seen = np.zeros((H, W), bool)
    comps = []
    for y in range(H):
        for x in range(W):
            if not P[y, x] or seen[y, x]:
                continue
            stack, cells, edge = [(y, x)], [], False
            seen[y, x] = True
            while stack:
                a, b = stack.pop()
                cells.append((a, b))
                edge = edge or a in (0, H - 1) or b in (0, W - 1)
                for da, db in ((1, 0), (-1, 0), (0, 1), (0, -1)):
                    p, q = a + da, b + db
                    if 0 <= p < H and 0 <= q < W and P[p, q] and not seen[p, q]:
                        seen[p, q] = True
                        stack.append((p, q))
            comps.append((cells, edge))
    return comps


def brute(mask, step, C):
    """the header's text for one step, with loops instead of scipy"""
    mask = np.asarray(mask, np.uint8)
    op = step['op']
    out = np.empty_like(mask)
    for f in range(mask.shape[0]):
        planes = {}
        for c in range(1, C):
            P = mask[f] == c
            if op in OPS:
                Q = brute_morph_plane(P, op, step.get('iterations', 1), step.get('structure', 'cross') == 'square')
            elif op == 'fill_holes':
                Q = P.copy()
                for cells, edge in brute_components(~P):
                    if not edge and (not step.get('max_area') or len(cells) <= step['max_area']):
                        for y, x in cells:
                            Q[y, x] = True
            else:
                Q = np.zeros_like(P)
                for cells, edge in brute_components(P):
                    if not edge:
                        for y, x in cells:
                            Q[y, x] = True
            planes[c] = Q
        merge = merge_extensive if op in ('dilate', 'close', 'fill_holes') else merge_anti
        out[f] = merge(mask[f], planes, C)
    return out


# ---- generators -----------------------------------------------------------------------------------------------------

def random_mask(seed, n, h, w, C, density, unknown=True):
    """classes 1 .. C-1 at the given density; with `unknown` a sprinkle of bytes C, C + 3 and 255"""
    rng = np.random.default_rng(seed)
    m = ((rng.random((n, h, w)) < density) * rng.integers(1, C, (n, h, w))).astype(np.uint8)
    if unknown:
        u = rng.random((n, h, w))
        m[u < 0.01] = 255
        m[(u >= 0.01) & (u < 0.02)] = C
        m[(u >= 0.02) & (u < 0.025)] = min(C + 3, 254)
    return m


def morph_shapes(tile):
    """(N, H, W): widths 1, 2, 63, 64, 65, 130 and the tile's columns +- 1, heights 1, 2 and the tile's rows +- 1"""
    R, Cc = tile
    return [(1, 1, 1), (3, 2, 2), (1, 1, 63), (3, 2, 64), (1, 5, 65), (3, 7, 130), (1, 2, Cc - 1), (1, 3, Cc), (3, 2, Cc + 1),
            (1, R - 1, 2), (1, R, 63), (3, R + 1, 1), (1, R - 1, Cc + 1), (1, R + 1, Cc - 1), (1, R, Cc), (1, R + 1, 130)]


def seams(tile, cls=1):
    """(1, 2R + 9, 2Cc + 11): a bar across and a diamond on every tile seam and seam crossing, far enough apart not to touch"""
    R, Cc = tile
    H, W = 2 * R + 9, 2 * Cc + 11
    m = np.zeros((1, H, W), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for y in (R, 2 * R):
        for x in (Cc, 2 * Cc):
            m[0][np.abs(yy - y) + np.abs(xx - x) <= 5] = cls     # diamonds on the crossings
        m[0, y - 2:y + 2, 20:60] = cls                          # a bar lying along a horizontal seam
        m[0, y - 7:y + 7, 100:104] = cls                        # and one standing across it
    for x in (Cc, 2 * Cc):
        m[0, 20:50, x - 2:x + 2] = cls                          # along a vertical seam
        m[0, 30:34, x - 30:x - 8] = cls
        m[0, 40:44, x - 9:x + 9] = cls                          # across it
    return m


def flush(h=40, w=70):
    """objects flush with each frame edge and corner, one free in the middle"""
    m = np.zeros((1, h, w), np.uint8)
    m[0, 0:6, 10:30] = 1
    m[0, h - 5:h, 35:60] = 1
    m[0, 12:30, 0:7] = 1
    m[0, 10:25, w - 6:w] = 1
    m[0, 0:4, 0:4] = 1
    m[0, h - 4:h, w - 4:w] = 1
    m[0, 15:25, 25:45] = 1
    return m


def ring(h, w, y0, x0, y1, x1, cls=1, thick=1):
    m = np.zeros((1, h, w), np.uint8)
    m[0, y0:y1, x0:x1] = cls
    m[0, y0 + thick:y1 - thick, x0 + thick:x1 - thick] = 0
    return m


def object_in_ring():
    """a class-2 object inside a class-1 ring: the object stays, the ring's background fills with 1"""
    m = ring(12, 13, 1, 1, 11, 12)
    m[0, 4:7, 5:8] = 2
    return m


def nested_rings():
    """a class-2 ring around a class-1 ring around background: everything enclosed goes to the lowest class that encloses it"""
    m = ring(12, 13, 0, 0, 12, 13, cls=0)
    m[0, 1:11, 1:12] = 2
    m[0, 2:10, 2:11] = 0
    m[0, 3:9, 3:10] = 1
    m[0, 4:8, 4:9] = 0
    return m


def unknown_bytes():
    """C = 3, two frames: bytes 7 and 255 inside a ring's hole and 255, 3 on the frame edge; in the second frame a byte 3
    also replaces a pixel of the ring's wall -- it is in no class, so the wall is open there and the hole is none"""
    m = np.repeat(ring(12, 13, 2, 2, 10, 11), 2, axis=0)
    m[:, 5, 5], m[:, 6, 7], m[:, 0, 3], m[:, 7, 0] = 255, 7, 255, 3
    m[:, 5, 12] = 2
    m[1, 2, 6] = 3
    return m


def fill_cases():
    """(name, mask, C, max_area values)"""
    cases = []
    m = np.ones((1, 9, 11), np.uint8)
    m[0, 2, 3] = m[0, 4, 7] = m[0, 7, 9] = 0
    cases.append(('one-pixel holes', m, 2, (None, 1)))
    m = ring(12, 230, 2, 10, 9, 215)
    cases.append(('three segments wide', m, 2, (None, 5 * 203 - 1, 5 * 203, 5 * 203 + 1)))
    sp = oc.spiral(cls=1)[0]
    m = np.pad(1 - sp, 2, constant_values=1)[None].astype(np.uint8)
    cases.append(('spiral hole', m, 2, (None, int(sp.sum()) - 1, int(sp.sum()))))
    cb = oc.comb()[0]
    m = np.pad(1 - cb, 2, constant_values=1)[None].astype(np.uint8)
    cases.append(('comb hole', m, 2, (None,)))
    m = np.ones((1, 8, 9), np.uint8)
    m[0, 0, 0] = 0                                              # the corner pixel itself: on the edge, no hole
    m[0, 7, 8] = 0
    m[0, 6, 7] = 0                                              # touches the corner pixel's background only diagonally: a hole
    m[0, 1:3, 1:3] = 0                                          # touches (0, 0) only diagonally: a hole
    cases.append(('corners', m, 2, (None, 1, 4)))
    m = ring(11, 12, 1, 1, 9, 10)
    m[0, 1, 1] = 0                                              # the ring's corner is gone: a diagonal leak, still a hole
    m[0, 8, 9] = 0
    cases.append(('diagonal leak', m, 2, (None, 6 * 7 - 1, 6 * 7)))
    yy, xx = np.mgrid[0:33, 0:70]
    cases.append(('checkerboard', ((yy + xx) % 2)[None].astype(np.uint8), 2, (None, 1)))
    cases.append(('checkerboard, inverse', ((yy + xx + 1) % 2)[None].astype(np.uint8), 2, (None,)))
    cases.append(('object in ring', object_in_ring(), 3, (None, 8 * 9 - 1, 8 * 9, 8 * 9 - 9)))
    cases.append(('nested rings', nested_rings(), 3, (None, 20, 54)))
    cases.append(('unknown bytes', unknown_bytes(), 3, (None, 6 * 7 - 1, 6 * 7)))
    cases.append(('disks', np.concatenate([oc.disks(3, 2, 70, 130, 25, classes=2), random_mask(4, 1, 70, 130, 3, 0.6)]), 3,
                  (None, 2, 9)))
    cases.append(('one row', np.array([[[1, 0, 1, 1, 0, 2, 0, 0, 1]]], np.uint8), 3, (None,)))
    cases.append(('one column', np.array([[[1, 0, 1, 1, 0, 2, 0, 0, 1]]], np.uint8).reshape(1, 9, 1), 3, (None,)))
    return cases


def border_cases():
    """(name, mask, C)"""
    cases = []
    m = np.zeros((1, 20, 30), np.uint8)
    m[0, 0, 5] = m[0, 1, 5] = m[0, 2, 5:8] = 1                   # touches the top edge by one pixel
    m[0, 19, 12] = m[0, 18, 10:13] = 1                          # the bottom
    m[0, 8, 0] = m[0, 8, 1] = m[0, 7:10, 2] = 2                 # the left
    m[0, 12, 29] = m[0, 12, 27:29] = 2                          # the right
    m[0, 5:8, 14:18] = 1                                        # free
    m[0, 10:13, 14:18] = 2
    cases.append(('edges', m, 3))
    m = np.zeros((1, 9, 10), np.uint8)
    m[0, 0, 0] = m[0, 0, 9] = m[0, 8, 0] = m[0, 8, 9] = 1       # the four corner pixels
    m[0, 1, 1] = m[0, 1, 8] = m[0, 7, 1] = m[0, 7, 8] = 1       # touch them only diagonally: kept
    m[0, 3:5, 3:6] = 1
    cases.append(('corners and diagonals', m, 2))
    cases.append(('one row', np.array([[[0, 1, 1, 0, 2, 0, 1]]], np.uint8), 3))
    m = np.zeros((1, 8, 12), np.uint8)
    m[0, 2:5, 0:3] = 1
    m[0, 2:5, 3:6] = 2                                          # beside the class-1 object at the edge, itself away from it: kept
    m[0, 6, 4:9] = 1
    m[0, 7, 6] = 2                                              # on the edge, under a class-1 object that is not
    cases.append(('two classes side by side', m, 3))
    m = unknown_bytes()
    m[0, 0, 4:7] = 1                                            # joins the unknown byte on the edge; that byte stays
    cases.append(('unknown bytes', m, 3))
    cases.append(('disks', np.concatenate([oc.disks(5, 2, 70, 130, 25, classes=2), random_mask(6, 1, 70, 130, 3, 0.55)]), 3))
    cases.append(('spiral', oc.spiral(cls=1), 2))
    cases.append(('spiral inside', np.pad(oc.spiral(cls=1)[0], 1)[None], 2))
    cases.append(('comb', oc.comb(), 2))
    return cases


def frames_u16(seed=5, F=3, H=96, W=130):
    """smooth blobs on a noisy background: the seeded net's mask has objects, holes and specks"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = rng.integers(100, 600, (F, H, W)).astype(np.float64)
    for f in range(F):
        for _ in range(12):
            cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(3, 12)
            out[f] += 3000.0 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * r * r))
    return np.clip(out, 0, 65535).astype(np.uint16)
