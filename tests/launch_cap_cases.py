"""Launches above the grid caps of the mask-analysis kernels: the table of caps, the inputs that pass them, and the
generators the CPU plan test (tests/test_launch_cap_plan.py) and the GPU test (tests/test_gpu_launch_caps.py) share.

Every kernel of the post-processing family that walks voxels, words or chunks does so in a grid-stride loop whose block
count one of four helpers caps.  An input of `items = k * cap_items + r` makes the grid walk it in k + 1 trips; with
0 < r < cap_items and r % 256 != 0 only part of the grid takes the last trip and its last wave has idle lanes.

Content is placed by construction: around the first item, around every multiple of cap_items and down to the last item a
generator stamps objects of two classes (labels) -- necked pairs that a split cuts, rings whose holes a fill closes, bars
on the frame's edge -- and one bar (in a volume: one column through the planes) that starts in one trip and ends in the
next; the last element belongs to a component of its own.  Between the windows a small random case is tiled.  The
generators take the cap as a parameter, so the plan test runs them at a cap of a few blocks against the pure-Python
restatements of the case files.
"""
import numpy as np
from scipy import ndimage

from tests import link_cases as lc
from tests import mask_cleanup_cases as mc
from tests import neighbors3d_cases as n3
from tests import neighbors_cases as nc
from tests import mask_split_cases as sc
from tests import volume_split_cases as vs

THREADS = 256
# helper -> where it is defined (the plan test holds the line to the source), its block cap, and what one block covers of
# the unit the table counts in
CAPS = {
    'cc_grid': {'file': 'sequitr_amd/csrc/sq_ccl.h', 'line': 115, 'blocks': 8192, 'per_block': 256},          # voxels
    'nb_grid': {'file': 'sequitr_amd/csrc/sq_zones.h', 'line': 148, 'blocks': 16384, 'per_block': 256},       # voxels, words
    'fe_grid': {'file': 'sequitr_amd/csrc/sq_frontend.hip', 'line': 101, 'blocks': 16384, 'per_block': 256},  # pixels
    # sq_link.hip: a block of the overlap kernels walks 4 wave-chunks at a time, a block of the relabel kernel one chunk
    'chunk_grid/overlap': {'file': 'sequitr_amd/csrc/sq_link.hip', 'line': 259, 'blocks': 32768, 'per_block': 4},
    'chunk_grid/relabel': {'file': 'sequitr_amd/csrc/sq_link.hip', 'line': 259, 'blocks': 32768, 'per_block': 1},
}


def cap_items(helper, blocks=None):
    c = CAPS[helper]
    return (c['blocks'] if blocks is None else blocks) * c['per_block']


# objects of the windows: erosions r and (radius, centre distance) of the touching disks / balls a split by r cuts
PLANE_FULL = {'r': 4, 'rad': 8, 'dist': 14}                     # mask_split_cases.disk_params(4)
PLANE_SMALL = {'r': 1, 'rad': 3, 'dist': 6}
VOLUME_FULL = {'r': 4, 'rad': 8, 'dist': 14}                    # volume_split_cases.ball_params(4): cut under every structure
VOLUME_SMALL = {'r': 1, 'rad': 2, 'dist': 4}
MAX_LABEL = 8                                                   # zones_ref runs one EDT per label
SMALL_AREA = 12                                                 # max_area / max_voxels: between a window's two holes

# name -> kind of generator, shape; `link` inputs: (N, P); `stitch`: (F, H, W)
INPUTS = {
    'plane2': ('mask', (1, 1560, 1451)),
    'plane3': ('mask', (3, 1000, 1451)),                        # three trips; frame 2 starts inside the second
    'volume2': ('volume', (1, 64, 199, 201)),
    'volume3': ('volume', (3, 40, 189, 191)),                   # three trips; volume 2 starts inside the second
    # 2 D (H + W) lateral face voxels against D H W voxels: only a thin volume has more of the former, and a volume in which
    # N * face_count passes the cap with H, W of a real stack would have some 10^8 voxels
    'thin': ('thin', (2, 70001, 3, 5)),
    'labels2': ('labels', (1, 2150, 2051)),
    'labels3': ('labels', (3, 1400, 2051)),
    'labelvol2': ('labelvol', (1, 24, 459, 461)),
    'labelvol3': ('labelvol', (3, 14, 459, 461)),
    'stitch2': ('stitch', (2, 1100, 2051)),
    'stitch3': ('stitch', (3, 1400, 2051)),
    'overlap1': ('link', (3, 65599 * 256 + 77)),                # one lane per position: chunks of 256, cpf = 65 600
    'overlap4': ('link', (45000, 1028)),                        # four per lane: chunks of 512, cpf = 3
    'relabel1': ('link', (5, 8199 * 256 + 77)),                 # P odd: V = 1, chunks of 256
    'relabel1x3': ('link', (5, 13199 * 256 + 77)),
    'relabel4': ('link', (5, 8199 * 1024 + 308)),               # P % 4 == 0: V = 4, chunks of 1024
}

# entry point, input, helper, items of the capped launches, trips.  `items` counts what the helper is given: voxels,
# words, wave-chunks or block-chunks.
ROWS = [
    ('maskops.fill_holes', 'plane2', 'cc_grid', 2263560, 2),
    ('maskops.fill_holes', 'plane3', 'cc_grid', 4353000, 3),
    ('maskops.clear_border', 'plane2', 'cc_grid', 2263560, 2),
    ('maskops.clear_border', 'plane3', 'cc_grid', 4353000, 3),
    ('maskops.split', 'plane2', 'cc_grid', 2263560, 2),
    ('maskops.split', 'plane3', 'cc_grid', 4353000, 3),
    ('volumeops.fill_cavities', 'volume2', 'cc_grid', 2559936, 2),
    ('volumeops.fill_cavities', 'volume3', 'cc_grid', 4331880, 3),
    ('volumeops.fill_cavities', 'thin', 'cc_grid', 2100030, 2),
    ('volumeops.clear_border3d', 'volume2', 'cc_grid', 2559936, 2),
    ('volumeops.clear_border3d', 'volume3', 'cc_grid', 4331880, 3),
    ('volumeops.clear_border3d', 'thin', 'cc_grid', 2100030, 2),
    ('volumeops.split3d', 'volume2', 'cc_grid', 2559936, 2),
    ('volumeops.split3d', 'volume3', 'cc_grid', 4331880, 3),
    ('neighbors.label_zones', 'labels2', 'nb_grid', 4409650, 2),
    ('neighbors.label_zones', 'labels3', 'nb_grid', 8614200, 3),
    ('neighbors.label_zones3d', 'labelvol2', 'nb_grid', 5078376, 2),
    ('neighbors.label_zones3d', 'labelvol3', 'nb_grid', 8887158, 3),
    ('FrameTiler.stitch', 'stitch2', 'fe_grid', 4512200, 2),
    ('FrameTiler.stitch', 'stitch3', 'fe_grid', 8614200, 3),
    ('linking.overlap_table/one-lane', 'overlap1', 'chunk_grid/overlap', 196800, 2),
    ('linking.overlap_table/four-lane', 'overlap4', 'chunk_grid/overlap', 135000, 2),
    ('linking.relabel/V=1', 'relabel1', 'chunk_grid/relabel', 41000, 2),
    ('linking.relabel/V=1', 'relabel1x3', 'chunk_grid/relabel', 66000, 3),
    ('linking.relabel/V=4', 'relabel4', 'chunk_grid/relabel', 41000, 2),
]
# No cap row: zone_graph_kernel (with and without depth) takes a wave per row and its grid is not capped, the capped launches
# of these entries walk the pair table (TABLE_ROWS).  The graphs are run on the zones of two big inputs all the same, as the
# issue asks: (entry, input).
BIG_INPUT_ROWS = [('neighbors.zone_graph', 'labels2'), ('neighbors.zone_graph3d', 'labelvol2')]
# the face enumerator's own launch (face_roots_kernel) on the thin volumes: N * face_count items, lateral / all faces
FACE_ROWS = [('thin', True, 2240032, 2), ('thin', False, 2240092, 2)]

# max_pairs = 2^22 gives 2^23 slots: the clear walks 3 (4 in 3-D) words per slot, the compaction one slot per thread, both
# in whole trips (a power of two divides by the cap: no ragged trip here, the ragged ones are the rows above)
BIG_PAIRS = 1 << 22
TABLE_ROWS = [
    ('neighbors.zone_graph', 'clear_words_kernel', 3 << 23, 6),
    ('neighbors.zone_graph', 'zone_graph_compact_kernel', 1 << 23, 2),
    ('neighbors.zone_graph3d', 'clear_words_kernel', 4 << 23, 8),
    ('neighbors.zone_graph3d', 'zone_graph3d_compact_kernel', 1 << 23, 2),
    ('linking.overlap_table', 'label_overlap_clear_kernel', 3 << 23, 6),
    ('linking.overlap_table', 'label_overlap_compact_kernel', 1 << 23, 2),
]


def row_items(entry, name):
    """the item count of a row from its input's shape"""
    kind, shape = INPUTS[name]
    if kind != 'link':
        return int(np.prod(shape))
    N, P = shape
    chunk = {'linking.overlap_table/one-lane': 256, 'linking.overlap_table/four-lane': 512, 'linking.relabel/V=1': 256,
             'linking.relabel/V=4': 1024}[entry]
    return N * ((P + chunk - 1) // chunk)


def face_count(D, H, W, lateral):
    return 2 * D * W + 2 * D * H + (0 if lateral else 2 * H * W)


def first_difference(got, want, cap, what):
    """equality of every element; a mismatch is reported with its first index, the trip it lies in and its offset there"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s, want %s %s" % (what, got.dtype, got.shape,
                                                                                           want.dtype, want.shape)
    if got.tobytes() == want.tobytes():
        return
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    i = int(bad[0])
    raise AssertionError("%s: %d of %d elements differ, first at flat index %d = trip %d + %d (cap %d): got %r, want %r"
                         % (what, len(bad), got.size, i, i // cap, i % cap, cap, got.reshape(-1)[i], want.reshape(-1)[i]))


# ---- where the windows lie --------------------------------------------------------------------------------------------
def boundaries(items, cap):
    return list(range(cap, items, cap))


def _centres(shape, cap, margin, apart=0):
    """[(name, boundary item or None, outer index, centre along the slab axis)]: the outer index is the frame (volume),
    the slab axis its rows (planes).  A centre keeps `margin` slabs from both ends of its frame, and `apart` slabs from
    the other centres of its frame."""
    outer, L = shape[0], shape[1]
    slab = int(np.prod(shape[2:]))
    out = [('first', None, 0, margin)]
    for b in boundaries(outer * L * slab, cap):
        f, s = divmod(b // slab, L)
        assert 1 <= s < L - 1, "boundary %d lies in slab %d of %d: the crossing component needs one on both sides" % (b, s, L)
        out.append(('trip%d' % (b // cap), b, f, min(max(s, margin), L - 1 - margin)))
    out.append(('last', None, outer - 1, L - 1 - margin))
    for i, a in enumerate(out):
        assert all(a[2] != c[2] or abs(a[3] - c[3]) >= apart for c in out[:i]), "the windows %s collide" % (out,)
    return out


def _ring(m, y0, x0, h, w, cls):
    m[y0:y0 + h, x0:x0 + w] = cls
    m[y0 + 1:y0 + h - 1, x0 + 1:x0 + w - 1] = 0


# ---- planar masks -----------------------------------------------------------------------------------------------------
def plane_mask(shape, cap, obj=PLANE_FULL, seed=1):
    """(mask (N,H,W) uint8 of classes 0 .. 2 and unknown bytes, info): info['windows'] = [{name, boundary, frame, rows,
    patches: [(kind, cls, y0, y1, x0, x1)], bar: (cls, x, y0, y1) or None}], rows and patches within the frame"""
    N, H, W = shape
    rad, dist = obj['rad'], obj['dist']
    block = mc.random_mask(seed, 1, 37, 41, 3, 0.3)[0]
    frame = np.tile(block, (H // 37 + 1, W // 41 + 1))[:H, :W]
    m = np.stack([np.roll(frame, 5 * f, axis=1) for f in range(N)])
    windows = []
    pw = 2 * rad + dist + 1                                     # a chain's width
    assert W >= 6 + 2 * (pw + 3) + 20 + 5, "too narrow for a window's objects"
    for name, b, f, yc in _centres(shape, cap, rad + 2, 2 * rad + 5):
        y0, y1 = yc - rad - 2, yc + rad + 3
        m[f, y0:y1] = 0
        patches, x = [], 6
        for cls in (1, 2):                                      # two necked pairs
            sc.chain(m[f, y0 + 1:y1 - 1, x:x + pw + 1], rad + 1, pw // 2, rad, dist, cls=cls)
            patches.append(('pair', cls, y0 + 1, y1 - 1, x, x + pw + 1))
            x += pw + 3
        _ring(m[f], yc - 2, x, 5, 5, 1)                         # a hole of 9 pixels with a pixel of the other class in it
        m[f, yc, x + 2] = 2
        patches.append(('ring', 1, yc - 2, yc + 3, x, x + 5))
        x += 7
        _ring(m[f], yc - 3, x, 7, 9, 2)                         # a hole of 35 pixels
        patches.append(('ring', 2, yc - 3, yc + 4, x, x + 9))
        x += 11
        m[f, yc - 1:yc + 1, 0:4] = 1                            # on the frame's first and last column
        m[f, yc, W - 4:W] = 2
        patches += [('edge', 1, yc - 1, yc + 1, 0, 4), ('edge', 2, yc, yc + 1, W - 4, W)]
        bar = None
        if b is not None:                                       # from rows of one trip into rows of the next
            s = (b // W) % H
            m[f, s - 1:s + 2, x:x + 2] = 2
            bar = (2, x, s - 1, s + 2)
        windows.append({'name': name, 'boundary': b, 'frame': f, 'rows': (y0, y1), 'patches': patches, 'bar': bar})
    m[0, 0, 8:20] = 1                                           # on the first and on the last row; the last element
    m[N - 1, H - 1, W - 6:W] = 2
    return m, {'windows': windows, 'last': (2, N - 1, H - 1, W - 6, W)}


# ---- volumes ----------------------------------------------------------------------------------------------------------
def volume_mask(shape, cap, obj=VOLUME_FULL, seed=2):
    """(mask (N,D,H,W) uint8, info) as plane_mask: windows = [{name, boundary, frame, rows: the planes, box: (y0, y1),
    patches: [(kind, cls, z0, z1, y0, y1, x0, x1)], bar: (cls, y, x, z0, z1) or None}]"""
    N, D, H, W = shape
    rad, dist = obj['rad'], obj['dist']
    block = mc.random_mask(seed, D, 23, 29, 3, 0.2)
    vol = np.tile(block, (1, H // 23 + 1, W // 29 + 1))[:, :H, :W]
    m = np.stack([np.roll(vol, 3 * v, axis=2) for v in range(N)])
    centres = _centres(shape, cap, rad)
    side, pw = 2 * rad + 1, 2 * rad + dist + 1
    assert D >= side and H >= len(centres) * (side + 3) + 2 and W >= 4 + 2 * (pw + 3) + 14 + 4 and rad >= 2, \
        "too small for the windows' objects"
    windows = []
    for k, (name, b, v, zc) in enumerate(centres):
        z0, z1 = zc - rad, zc + rad + 1
        y0 = 1 + k * (side + 3)                                 # every window has rows of its own: planes may be shared
        y1 = y0 + side + 2
        yc = y0 + rad + 1
        m[v, z0:z1, y0:y1] = 0
        patches, x = [], 4
        for cls in (1, 2):                                      # two necked pairs along w
            vs.chain(m[v, z0:z1, y0 + 1:y1 - 1, x:x + pw + 1], (rad, rad, pw // 2), 2, rad, dist, cls=cls)
            patches.append(('pair', cls, z0, z1, y0 + 1, y1 - 1, x, x + pw + 1))
            x += pw + 3
        m[v, zc - 2:zc + 3, yc - 2:yc + 3, x:x + 5] = 1         # a cavity of 27 voxels with a voxel of the other class in it
        m[v, zc - 1:zc + 2, yc - 1:yc + 2, x + 1:x + 4] = 0
        m[v, zc, yc, x + 2] = 2
        patches.append(('shell', 1, zc - 2, zc + 3, yc - 2, yc + 3, x, x + 5))
        x += 7
        m[v, zc - 2:zc + 3, yc - 2:yc + 3, x:x + 5] = 2         # a cavity of 9 voxels
        m[v, zc, yc - 1:yc + 2, x + 1:x + 4] = 0
        patches.append(('shell', 2, zc - 2, zc + 3, yc - 2, yc + 3, x, x + 5))
        x += 7
        m[v, zc, yc, 0:2] = 1                                   # on a lateral face
        m[v, zc, yc, W - 2:W] = 2
        patches += [('edge', 1, zc, zc + 1, yc, yc + 1, 0, 2), ('edge', 2, zc, zc + 1, yc, yc + 1, W - 2, W)]
        bar = None
        if b is not None:                                       # a column through planes on both sides of the boundary
            s = (b // (H * W)) % D
            m[v, s - 1:s + 2, yc, x] = 2
            bar = (2, yc, x, s - 1, s + 2)
        windows.append({'name': name, 'boundary': b, 'frame': v, 'rows': (z0, z1), 'box': (y0, y1), 'patches': patches,
                        'bar': bar})
    m[0, 0, H - 1, 3:9] = 1
    m[N - 1, D - 1, H - 1, W - 4:W] = 2                         # the last element
    return m, {'windows': windows, 'last': (2, N - 1, D - 1, H - 1, W - 4, W)}


def face_voxels(D, H, W, lateral):
    """sq_component_ops.hip's face_voxel for k = 0 .. face_count - 1: the linear index into one (D, H, W) volume of every
    item the face enumerator visits, in its order (z = 0 and z = D - 1 unless `lateral`, then h = 0, H - 1 and w = 0, W - 1)"""
    HW = H * W
    k, j = np.arange(D * W, dtype=np.int64), np.arange(D * H, dtype=np.int64)
    parts = [] if lateral else [np.arange(HW, dtype=np.int64), (D - 1) * HW + np.arange(HW, dtype=np.int64)]
    parts += [(k // W) * HW + k % W, (k // W) * HW + (H - 1) * W + k % W, (j // H) * HW + (j % H) * W,
              (j // H) * HW + (j % H) * W + (W - 1)]
    return np.concatenate(parts)


def face_items_of(shape, lateral, n, limit=None):
    """the face voxels of volume n that the first `limit` items of the launch (all N volumes, item i = n * face_count + k)
    reach, and those that only later items reach"""
    N, D, H, W = shape
    vox = face_voxels(D, H, W, lateral)
    cut = len(vox) if limit is None else min(max(limit - n * len(vox), 0), len(vox))
    return vox[:cut], np.setdiff1d(vox[cut:], vox[:cut])


def _roots(P, vox):
    """(labels of the 6-connected components of P, the labels that own one of the voxels `vox`)"""
    lab, _ = ndimage.label(P)
    hit = np.unique(lab.reshape(-1)[vox])
    return lab, hit[hit > 0]


def clear_border_limited(mask, C, faces, limit=None):
    """volume_cleanup_cases.clear_border_ref with the faces enumerated item by item as face_roots_kernel does, by the
    first `limit` items only (None: all of them, which must give clear_border_ref itself)"""
    mask = np.asarray(mask, np.uint8)
    out = np.where(mask >= C, mask, 0).astype(np.uint8)
    for v in range(mask.shape[0]):
        vox = face_items_of(mask.shape, faces == 'lateral', v, limit)[0]
        for c in range(1, C):
            lab, hit = _roots(mask[v] == c, vox)
            out[v][(lab > 0) & ~np.isin(lab, hit)] = c
    return out


def fill_limited(mask, C, limit=None):
    """volume_cleanup_cases.fill_ref (all cavities, not planar) the same way: a component of a complement plane is no cavity
    when one of the first `limit` face items lies in it"""
    mask = np.asarray(mask, np.uint8)
    out = mask.copy()
    for v in range(mask.shape[0]):
        vox = face_items_of(mask.shape, False, v, limit)[0]
        for c in range(1, C):
            lab, hit = _roots(mask[v] != c, vox)
            out[v][(out[v] == 0) & (lab > 0) & ~np.isin(lab, hit)] = c
    return out


def late_face_column(shape, cap, length):
    """(volume, z) of the first run of `length` planes whose voxel (z, h = 1, w = W - 1) is reached only by face items >= cap,
    under both settings of `faces` -- a voxel of the thin volumes that lies on no other face"""
    N, D, H, W = shape
    for v in range(N):
        late = np.intersect1d(face_items_of(shape, True, v, cap)[1], face_items_of(shape, False, v, cap)[1])
        z = late[(late % (H * W)) == 1 * W + (W - 1)] // (H * W)
        z = z[(z >= 1) & (z < D - 1)]
        for z0 in z:
            if z0 + length <= D - 1 and np.isin(np.arange(z0, z0 + length), z).all():
                return v, int(z0)
    raise AssertionError("no face item past the cap in %s" % (shape,))


def thin_volume(shape, cap, seed=3):
    """(N, D, 3, 5): every voxel but the middle column lies on a lateral face, so N * face_count passes the cap with the
    voxels (FACE_ROWS).  Runs along D of both classes, some only in the middle column (they stay under faces='lateral', and
    go under 'all' when they reach a volume's end), middle columns closed on all sides, a first, a last and a boundary
    window of three objects of two classes, and info['late']: where only face items of the second trip reach -- runs of
    both classes at (h = 1, w = W - 1), which lie on no other face, and a pocket of background in a slab of each class that
    opens onto that column alone, so that the complement plane's border depends on those items too"""
    N, D, H, W = shape
    assert H == 3 and W == 5
    rng = np.random.default_rng(seed)
    period = 97
    blk = np.zeros((period, H, W), np.uint8)
    blk[3:20, 1, 1:4] = 1                                       # an inner bar: touches no lateral face
    blk[25:31] = 2
    blk[26:30, 1, 2] = 0                                        # a cavity of 4 voxels inside class 2
    blk[40:60] = 1
    blk[41:59, 1, 1] = 0                                        # and of 18 inside class 1
    blk[70:75, 0, :] = 2                                        # on the face h = 0
    blk[80:90, 1, 2] = rng.integers(0, 3, 10)
    m = np.stack([np.roll(np.tile(blk, (D // period + 1, 1, 1))[:D], 11 * v, axis=0) for v in range(N)])
    m[0, :12] = 0
    m[0, :4, 1, 2] = 1                                          # an inner run that reaches the first plane
    m[0, 5:8, 0, :] = 2
    m[0, 9:11] = 1
    windows = [{'name': 'first', 'boundary': None, 'frame': 0, 'rows': (0, 12), 'bar': None,
                'patches': [('run', 1, 0, 4, 1, 2, 2, 3), ('edge', 2, 5, 8, 0, 1, 0, W), ('slab', 1, 9, 11, 0, H, 0, W)]}]
    for b in boundaries(N * D * H * W, cap):
        v, s = divmod(b // (H * W), D)
        assert 8 <= s < D - 8
        m[v, s - 8:s + 8] = 0
        m[v, s - 6:s + 6, 1, 1:4] = 1                           # an inner bar across the boundary
        m[v, s - 7:s + 7, 0, 0] = 2                             # and a run of the other class and one of its own on the edges
        m[v, s - 7:s + 7, 2, 4] = 1
        windows.append({'name': 'trip%d' % (b // cap), 'boundary': b, 'frame': v, 'rows': (s - 8, s + 8),
                        'bar': (1, 1, 2, s - 6, s + 6),
                        'patches': [('bar', 1, s - 6, s + 6, 1, 2, 1, 4), ('edge', 2, s - 7, s + 7, 0, 1, 0, 1),
                                    ('edge', 1, s - 7, s + 7, 2, 3, 4, 5)]})
    m[N - 1, D - 12:] = 0
    m[N - 1, D - 9:, 2, 2:] = 2                                 # ends in the last element
    m[N - 1, D - 11:D - 3, 0, 0:2] = 1
    m[N - 1, D - 8:D - 1, 1, 1] = 1
    windows.append({'name': 'last', 'boundary': None, 'frame': N - 1, 'rows': (D - 12, D), 'bar': None,
                    'patches': [('run', 2, D - 9, D, 2, 3, 2, W), ('edge', 1, D - 11, D - 3, 0, 1, 0, 2),
                                ('run', 1, D - 8, D - 1, 1, 2, 1, 2)]})
    v, z = late_face_column(shape, cap, 36 + 8)
    z += 8                                                      # clear of the item boundary under either setting of `faces`
    assert all(w['frame'] != v or w['rows'][1] <= z or w['rows'][0] >= z + 36 for w in windows), \
        "the late column meets a window"
    m[v, z:z + 36] = 0
    m[v, z + 2:z + 8, 1, W - 1] = 1
    m[v, z + 10:z + 16, 1, W - 1] = 2
    pockets = []
    for c, p in ((1, z + 18), (2, z + 26)):
        m[v, p:p + 6] = c
        m[v, p + 1:p + 5, 1, 2:W] = 0                           # 12 voxels of background behind (h = 1, w = W - 1)
        pockets.append((c, p + 1, p + 5))
    late = {'frame': v, 'rows': (z, z + 36), 'runs': [(1, z + 2, z + 8), (2, z + 10, z + 16)], 'pockets': pockets}
    return m, {'windows': windows, 'last': (2, N - 1, D - 1, 2, 2, 5), 'late': late}


# ---- labels for the zones ---------------------------------------------------------------------------------------------
TIE_HALF = (8, 11)                                              # rows / columns cleared round a tie: no other seed is as near


def label_frames(shape, cap, seed=4):
    """(labels (N,H,W) int32 of seeds 1 .. MAX_LABEL and background values, info): per window blobs of three labels, two
    seeds of different labels at distance 3 on either side of a pixel (info ties: (frame, y, x, smaller label)), and a
    bar of label 7 across the boundary; the last element is a seed of label 8"""
    N, H, W = shape
    block = nc.random_labels(seed, 1, 61, 67, MAX_LABEL, 0.004)[0]
    frame = np.tile(block, (H // 61 + 1, W // 67 + 1))[:H, :W]
    lab = np.stack([np.roll(frame, 7 * f, axis=1) for f in range(N)])
    windows, ties = [], []
    assert W >= 70
    for k, (name, b, f, yc) in enumerate(_centres(shape, cap, TIE_HALF[0], 2 * TIE_HALF[0] + 1)):
        y0, y1 = yc - TIE_HALF[0], yc + TIE_HALF[0] + 1
        lab[f, y0:y1, 0:70] = 0
        patches = []
        for i, L in enumerate((1, 2, 3)):
            lab[f, yc - 1 + i, 4 + 6 * i:6 + 6 * i] = L
            patches.append(('blob', L, yc - 1 + i, yc + i, 4 + 6 * i, 6 + 6 * i))
        a, c = ((5, 2), (2, 5))[k % 2]                          # the smaller label to the right, then to the left
        x = 40
        lab[f, yc, x - 3], lab[f, yc, x + 3] = a, c
        ties.append((f, yc, x, min(a, c)))
        patches += [('seed', a, yc, yc + 1, x - 3, x - 2), ('seed', c, yc, yc + 1, x + 3, x + 4)]
        bar = None
        if b is not None:
            s = (b // W) % H
            lab[f, s - 1:s + 2, 60] = 7
            bar = (7, 60, s - 1, s + 2)
        windows.append({'name': name, 'boundary': b, 'frame': f, 'rows': (y0, y1), 'patches': patches, 'bar': bar})
    lab[N - 1, H - 1, W - 1] = 8
    return lab, {'windows': windows, 'ties': ties, 'last': (8, N - 1, H - 1, W - 1, W)}


def label_volumes(shape, cap, seed=5):
    """label_frames in (N,D,H,W): the ties lie in one plane with the planes within 4 of it cleared round them, the bar is a
    column of label 7 through the planes on both sides of the boundary"""
    N, D, H, W = shape
    block = n3.random_volume(seed, 1, D, 61, 67, MAX_LABEL, 0.002)[0]
    vol = np.tile(block, (1, H // 61 + 1, W // 67 + 1))[:, :H, :W]
    lab = np.stack([np.roll(vol, 7 * v, axis=2) for v in range(N)])
    centres = _centres(shape, cap, 1)
    windows, ties = [], []
    side = 2 * TIE_HALF[0] + 1
    assert W >= 70 and H >= len(centres) * side and D >= 3
    for k, (name, b, v, zc) in enumerate(centres):
        y0 = k * side
        y1, yc = y0 + side, y0 + TIE_HALF[0]
        z0, z1 = max(0, zc - 4), min(D, zc + 5)
        lab[v, z0:z1, y0:y1, 0:70] = 0
        patches = []
        for i, L in enumerate((1, 2, 3)):
            lab[v, zc, yc - 1 + i, 4 + 6 * i:6 + 6 * i] = L
            patches.append(('blob', L, zc, zc + 1, yc - 1 + i, yc + i, 4 + 6 * i, 6 + 6 * i))
        a, c = ((5, 2), (2, 5))[k % 2]
        x = 40
        lab[v, zc, yc, x - 3], lab[v, zc, yc, x + 3] = a, c
        ties.append((v, zc, yc, x, min(a, c)))
        patches += [('seed', a, zc, zc + 1, yc, yc + 1, x - 3, x - 2), ('seed', c, zc, zc + 1, yc, yc + 1, x + 3, x + 4)]
        bar = None
        if b is not None:
            s = (b // (H * W)) % D
            lab[v, s - 1:s + 2, yc, 60] = 7
            bar = (7, yc, 60, s - 1, s + 2)
        windows.append({'name': name, 'boundary': b, 'frame': v, 'rows': (z0, z1), 'box': (y0, y1), 'patches': patches,
                        'bar': bar})
    lab[N - 1, D - 1, H - 1, W - 1] = 8
    return lab, {'windows': windows, 'ties': ties, 'last': (8, N - 1, D - 1, H - 1, W - 1, W)}


# ---- label stacks for the linking -------------------------------------------------------------------------------------
OVERLAP_MAX_LABEL = 17


def _runs(values, lengths, n):
    p = np.repeat(np.asarray(values, np.int32), lengths)
    return np.tile(p, n // len(p) + 2)


def overlap_stacks(N, P):
    """(a, b) (N, P) int32 out of np.repeat / np.tile of short run patterns, dense everywhere.  Frame n reads the patterns
    from an offset of its own, and carries a label no other frame has wherever a's pattern holds 1 (10 + n % 3 with more than
    three frames: then no neighbour, and no frame a whole number of grid steps away, has it) -- a chunk counted into
    another frame's row changes that row."""
    ra = _runs([1, 0, 2, 2, 3, 0, 4, -5, 1, 18, 2], [5, 3, 7, 1, 4, 2, 9, 1, 6, 2, 3], P + 512)
    rb = _runs([2, 2, 0, 1, 3, 0, 5, 1], [4, 6, 5, 8, 3, 1, 7, 2], P + 512)
    if N <= 8:
        a = np.stack([ra[13 * n:13 * n + P] for n in range(N)])
        b = np.stack([rb[7 * n:7 * n + P] for n in range(N)])
        for n in range(N):
            a[n][a[n] == 1] = 10 + n
        return a, b
    block_a = np.stack([np.where(ra[13 * n:13 * n + P] == 1, 10 + n % 3, ra[13 * n:13 * n + P]) for n in range(21)])
    block_b = np.stack([rb[7 * n:7 * n + P] for n in range(21)])
    reps = N // 21 + 1
    return np.tile(block_a, (reps, 1))[:N].copy(), np.tile(block_b, (reps, 1))[:N].copy()


def overlap_packed(a, b, max_label):
    """overlap_ref out of one np.bincount per group of frames over the packed keys (n K + la) K + lb, K = max_label + 1: the
    whole contingency table with its zero row and column, so both area tables are its margins.  The plan test shows it equal
    to link_cases.overlap_ref, whose np.unique over stacked triples takes minutes on 5 * 10^7 positions."""
    a, b = np.asarray(a), np.asarray(b)
    N, K = a.shape[0], max_label + 1
    a, b = a.reshape(N, -1), b.reshape(N, -1)
    group = max(1, (1 << 24) // a.shape[1])
    pairs, area_a, area_b = [], np.zeros((N, K), np.int64), np.zeros((N, K), np.int64)
    for n0 in range(0, N, group):
        A, B = lc.in_range(a[n0:n0 + group], max_label), lc.in_range(b[n0:n0 + group], max_label)
        g = A.shape[0]
        key = (np.arange(g, dtype=np.int64)[:, None] * K + A) * K + B
        table = np.bincount(key.reshape(-1), minlength=g * K * K).reshape(g, K, K)
        area_a[n0:n0 + g], area_b[n0:n0 + g] = table.sum(2), table.sum(1)
        n, la, lb = np.nonzero(table[:, 1:, 1:])
        pairs.append(np.stack([n + n0, la + 1, lb + 1, table[n, la + 1, lb + 1]], 1))
    area_a[:, 0] = 0
    area_b[:, 0] = 0
    return np.concatenate(pairs).astype(np.int64).reshape(-1, 4), area_a, area_b


def relabel_case(N, P):
    """(labels (N, P) int32, offsets (N + 1), lut): every frame has another number of objects, so a wrong frame index reads
    another frame's slice of the table or takes a label for out of range"""
    counts = np.array([9, 5, 0, 7, 11, 3, 8], np.int64)[np.arange(N) % 7]
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    lut = (np.arange(offsets[-1], dtype=np.int32) * 3 + 100)
    r = _runs([1, 0, 2, 9, 3, 0, 4, -5, 5, 11, 6, 7, 8, 12, 10], [5, 3, 7, 1, 4, 2, 9, 1, 6, 2, 3, 2, 5, 1, 4], P + 16 * N)
    return np.stack([r[11 * n:11 * n + P] for n in range(N)]), offsets, lut


# ---- WaveWalk of sq_link.hip, restated --------------------------------------------------------------------------------
class WaveWalk(object):
    """wave-chunk w = (frame n, chunk c of the frame's cpf), walked as w, w + step, ...: the divisions once, then two adds
    and a carry per step"""

    def __init__(self, w, step, cpf):
        self.w, self.step = w, step
        self.n, self.c = divmod(w, cpf)
        self.dn, self.dc = divmod(step, cpf)

    def next(self, cpf, carry=True):
        self.w += self.step
        self.n += self.dn
        self.c += self.dc
        if carry and self.c >= cpf:
            self.c -= cpf
            self.n += 1


def walk(N, cpf, grid_waves, carry=True):
    """every (n, c) the grid's waves visit, in wave order, with the number of steps that carried and that did not"""
    total = N * cpf
    seen, carried, plain = [], 0, 0
    for w0 in range(min(grid_waves, total)):
        k = WaveWalk(w0, grid_waves, cpf)
        while k.w < total:
            seen.append((k.n, k.c))
            if k.w + k.step < total:
                if k.c + k.dc >= cpf:
                    carried += 1
                else:
                    plain += 1
            k.next(cpf, carry)
    return seen, carried, plain


def walk_counts(N, cpf, grid_waves):
    """carried / plain of walk() for the full-size rows, without the visit list: vectorised over the starting waves"""
    total = N * cpf
    dc = grid_waves % cpf
    carried = plain = 0
    w = np.arange(min(grid_waves, total), dtype=np.int64)
    while len(w):
        w = w[w + grid_waves < total]
        c = w % cpf
        carried += int((c + dc >= cpf).sum())
        plain += int((c + dc < cpf).sum())
        w = w + grid_waves
    return carried, plain
