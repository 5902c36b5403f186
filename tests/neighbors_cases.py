"""Label zones, the zone contact graph and the neighbour table: the numpy / scipy restatements of include/sequitr_hip.h,
"Label zones and the zone contact graph", that the GPU path is pinned against, pure-Python all-pairs versions that check
the restatements on small frames, and the cases the CPU and GPU tests share.

``zones_ref`` is the header's text over scipy: per label L, distance_transform_edt(labels != L, return_indices=True), the
integer squared distance from the indices, and the lexicographic minimum of (d2, L) over the labels.
``graph_ref`` is numpy on shifted views plus np.unique;  ``neighbors_ref`` is the whole table of
sequitr_amd/analysis/neighbors.py, written with Python loops over the pairs.
"""
import numpy as np
from scipy import ndimage, spatial

NO_SEED = 0x7fffffff
SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 130, 200)


def seeds_of(labels, max_label):
    labels = np.asarray(labels).astype(np.int64)
    return np.where((labels >= 1) & (labels <= max_label), labels, 0)


def zones_ref(labels, max_label, max_distance=0):
    """labels (N,H,W) -> (zones, d2), both int32"""
    lab = seeds_of(labels, max_label)
    N, H, W = lab.shape
    yy, xx = np.mgrid[0:H, 0:W]
    zones = np.zeros((N, H, W), np.int64)
    d2 = np.full((N, H, W), NO_SEED, np.int64)
    for n in range(N):
        for L in np.unique(lab[n]):                             # ascending: a later label wins only when strictly nearer
            if L == 0:
                continue
            ind = ndimage.distance_transform_edt(lab[n] != L, return_distances=False, return_indices=True)
            d = (ind[0] - yy).astype(np.int64) ** 2 + (ind[1] - xx).astype(np.int64) ** 2
            nearer = d < d2[n]
            zones[n][nearer] = L
            d2[n][nearer] = d[nearer]
    if max_distance:
        zones[d2 > max_distance * max_distance] = 0
    return zones.astype(np.int32), d2.astype(np.int32)


def zones_allpairs(labels, max_label, max_distance=0):
    """the definition, pixel by pixel over all seeds (pure Python; small frames only)"""
    lab = seeds_of(labels, max_label)
    N, H, W = lab.shape
    zones = np.zeros((N, H, W), np.int32)
    d2 = np.full((N, H, W), NO_SEED, np.int32)
    for n in range(N):
        seeds = [(int(y), int(x), int(lab[n, y, x])) for y, x in zip(*np.nonzero(lab[n]))]
        for y in range(H):
            for x in range(W):
                best = (NO_SEED, 0)
                for sy, sx, L in seeds:
                    best = min(best, ((y - sy) ** 2 + (x - sx) ** 2, L))
                d2[n, y, x] = best[0]
                if not max_distance or best[0] <= max_distance * max_distance:
                    zones[n, y, x] = best[1]
    return zones, d2


def tie_pixels(labels, max_label):
    """pixels whose nearest seeds carry more than one label"""
    lab = seeds_of(labels, max_label)
    N, H, W = lab.shape
    out = np.zeros((N, H, W), bool)
    for n in range(N):
        ys, xs = np.nonzero(lab[n])
        if not len(ys):
            continue
        yy, xx = np.mgrid[0:H, 0:W]
        d = (yy[..., None] - ys) ** 2 + (xx[..., None] - xs) ** 2
        near = d == d.min(-1, keepdims=True)
        ls = lab[n][ys, xs]
        lo = np.where(near, ls, NO_SEED).min(-1)
        hi = np.where(near, ls, 0).max(-1)
        out[n] = lo != hi
    return out


def graph_ref(zones, max_label):
    """zones (N,H,W) -> stats (N, max_label+1, 2) int64 and pairs (k,4) int64 [frame, a, b, border] sorted"""
    z = seeds_of(zones, max_label)
    N, H, W = z.shape
    stats = np.zeros((N, max_label + 1, 2), np.int64)
    edge = np.zeros((H, W), bool)
    edge[0] = edge[-1] = edge[:, 0] = edge[:, -1] = True
    rows = []
    for n in range(N):
        stats[n, :, 0] = np.bincount(z[n].ravel(), minlength=max_label + 1)
        stats[n, :, 1] = np.bincount(z[n][edge], minlength=max_label + 1)
        for A, B in ((z[n][:, :-1], z[n][:, 1:]), (z[n][:-1], z[n][1:])):
            m = (A != B) & (A > 0) & (B > 0)
            a, b = np.minimum(A[m], B[m]), np.maximum(A[m], B[m])
            rows.append(np.stack([np.full(a.shape, n, np.int64), a, b], 1))
    stats[:, 0] = 0
    rows = np.concatenate(rows) if rows else np.zeros((0, 3), np.int64)
    if len(rows):
        uniq, counts = np.unique(rows, axis=0, return_counts=True)
        pairs = np.concatenate([uniq, counts[:, None]], 1).astype(np.int64)
    else:
        pairs = np.zeros((0, 4), np.int64)
    return stats, pairs


def graph_allpairs(zones, max_label):
    """the definition, pixel pair by pixel pair (pure Python)"""
    z = seeds_of(zones, max_label)
    N, H, W = z.shape
    stats = np.zeros((N, max_label + 1, 2), np.int64)
    table = {}
    for n in range(N):
        for y in range(H):
            for x in range(W):
                a = int(z[n, y, x])
                if a:
                    stats[n, a, 0] += 1
                    stats[n, a, 1] += y in (0, H - 1) or x in (0, W - 1)
                for y2, x2 in ((y, x + 1), (y + 1, x)):
                    if y2 < H and x2 < W:
                        b = int(z[n, y2, x2])
                        if a and b and a != b:
                            key = (n, min(a, b), max(a, b))
                            table[key] = table.get(key, 0) + 1
    pairs = np.array([k + (v,) for k, v in sorted(table.items())], np.int64).reshape(-1, 4)
    return stats, pairs


def centroid_seed_image(frame, label, centroid, shape):
    N, H, W = shape
    out = np.zeros(shape, np.int32)
    yx = np.asarray(centroid, np.float64).reshape(len(frame), -1)[:, -2:]
    for k in range(len(frame) - 1, -1, -1):                     # descending: the smallest label is written last
        sy = int(min(max(np.floor(yx[k, 0] + 0.5), 0), H - 1))
        sx = int(min(max(np.floor(yx[k, 1] + 0.5), 0), W - 1))
        out[frame[k], sy, sx] = label[k]
    return out


def neighbors_ref(labels, cls, centroid, frame, num_classes, d_thresh=100., max_distance=None, seeds='objects'):
    """the columns of NeighborTable as a dict (plus 'zones'), by Python loops over the zone pairs"""
    labels = np.asarray(labels)
    N = labels.shape[0]
    frame, cls = np.asarray(frame, np.int64), np.asarray(cls, np.int64)
    k = len(frame)
    label = np.array([1 + i - int(np.sum(frame < frame[i])) for i in range(k)], np.int64)
    max_label = max([1] + [int(np.sum(frame == f)) for f in range(N)])
    yx = np.asarray(centroid, np.float64).reshape(k, -1)[:, -2:]
    src = labels if seeds == 'objects' else centroid_seed_image(frame, label, centroid, labels.shape)
    zones, _ = zones_ref(src, max_label, max_distance or 0)
    stats, pairs = graph_ref(zones, max_label)
    row_of = {(int(frame[i]), int(label[i])): i for i in range(k)}
    adj = [[] for _ in range(k)]
    removed = np.zeros(k, np.int64)
    n_pairs = n_removed = 0
    for f, a, b, border in pairs:
        i, j = row_of[(int(f), int(a))], row_of[(int(f), int(b))]
        dx, dy = yx[i, 1] - yx[j, 1], yx[i, 0] - yx[j, 0]
        dist = np.sqrt(dx ** 2 + dy ** 2)
        if dist > d_thresh:
            removed[i] += 1
            removed[j] += 1
            n_removed += 1
            continue
        n_pairs += 1
        adj[i].append((j, int(border), dist))
        adj[j].append((i, int(border), dist))
    res = {'frame': frame, 'label': label, 'cls': cls, 'n_removed': removed, 'zones': zones,
           'n_pairs': n_pairs, 'n_pairs_removed': n_removed}
    res['n_total'] = np.array([len(a) for a in adj], np.int64)
    res['n_class'] = np.zeros((k, num_classes), np.int64)
    indptr, indices, border, distance = [0], [], [], []
    for i in range(k):
        for j, b, d in sorted(adj[i]):
            res['n_class'][i, cls[j]] += 1
            indices.append(j)
            border.append(b)
            distance.append(d)
        indptr.append(len(indices))
    res['indptr'], res['indices'], res['border'] = (np.array(v, np.int64) for v in (indptr, indices, border))
    res['distance'] = np.array(distance, np.float64)
    res['zone_area'] = np.array([stats[frame[i], label[i], 0] for i in range(k)], np.int64)
    res['zone_edge'] = np.array([stats[frame[i], label[i], 1] for i in range(k)], np.int64)
    with np.errstate(divide='ignore'):
        res['local_density'] = 1.0 / res['zone_area'].astype(np.float64)
    return res


TABLE_COLUMNS = ('frame', 'label', 'cls', 'n_total', 'n_class', 'n_removed', 'zone_area', 'zone_edge', 'local_density',
                 'indptr', 'indices', 'border', 'distance')


def assert_table(got, want, what=''):
    """got: a dict of columns (NeighborTable.columns() or a loaded .npz); every column equal, floats bit for bit"""
    for name in TABLE_COLUMNS:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        assert g.shape == w.shape and g.dtype == w.dtype, "%s %s: %s %s against %s %s" % (what, name, g.shape, g.dtype,
                                                                                          w.shape, w.dtype)
        if g.dtype == np.float64:
            g, w = g.view(np.uint64), w.view(np.uint64)
        assert np.array_equal(g, w), "%s %s differs" % (what, name)


# ---- zone cases: (name, labels (N,H,W) int32, max_label, reaches) ---------------------------------------------------
def random_labels(seed, N, H, W, max_label=6, density=0.03):
    """sparse seeds of labels 1 .. max_label, sprinkled with values that are background: negative and max_label + 1"""
    rng = np.random.default_rng(seed)
    lab = np.zeros((N, H, W), np.int32)
    u = rng.random((N, H, W))
    lab[u < density] = rng.integers(1, max_label + 1, int((u < density).sum()))
    lab[(u > 0.5) & (u < 0.5 + density)] = -3
    lab[(u > 0.7) & (u < 0.7 + density)] = max_label + 1
    return lab


def shape_cases():
    """every width and every height of SIZES, N = 1 and 3"""
    out = []
    for i, s in enumerate(SIZES):
        t = SIZES[(3 * i + 1) % len(SIZES)]
        for N, H, W in ((1 + 2 * (i % 2), t, s), (3 - 2 * (i % 2), s, t)):
            out.append(("rand_%dx%dx%d" % (N, H, W), random_labels(100 * H + W, N, H, W), 6, (0, 5)))
    return out


def seam_case():
    lab = np.zeros((1, 9, 200), np.int32)
    lab[0, 0, 63], lab[0, 0, 64] = 2, 1                         # on both sides of the first seam
    lab[0, 1, 127], lab[0, 1, 128] = 1, 2                       # and of the second
    lab[0, 2, 64], lab[0, 2, 127] = 3, 1                        # first and last lane of the middle segment
    lab[0, 4, 3] = 4                                            # the only seed in the first segment: the carry runs right
    lab[0, 5, 197] = 5                                          # the only seed in the last segment: the carry runs left
    lab[0, 6, 0], lab[0, 6, 199] = 6, 2                         # the row's ends
    lab[0, 8, 63], lab[0, 8, 192] = 5, 1                        # equidistant across a whole segment
    return ("seams", lab, 6, (0, 64))


def empty_and_single_case():
    lab = np.zeros((3, 66, 70), np.int32)
    lab[1, 40, 65] = 3
    lab[2, 5, 5] = 9                                            # larger than max_label: frame 2 has no seed either
    return ("no_seed_one_seed", lab, 4, (0, 5))


def tie_cases():
    out = []
    for a, b in ((1, 2), (2, 1)):                               # both orders: the smaller label is met first / second
        lab = np.zeros((3, 9, 9), np.int32)
        lab[0, 4, 1], lab[0, 4, 7] = a, b                       # left / right
        lab[1, 1, 4], lab[1, 7, 4] = a, b                       # up / down
        lab[2, 0, 0], lab[2, 8, 8] = a, b                       # diagonal
        out.append(("ties_%d%d" % (a, b), lab, 2, (0, 5)))
        lab = np.zeros((2, 7, 70), np.int32)
        lab[0, 3, 66], lab[0, 0, 63] = 5, 2                     # pixel (3,63): 5 in its row at distance 3, 2 three rows up --
        lab[1, 3, 60], lab[1, 6, 63] = 5, 2                     # the column search meets it at dy*dy == best (<=, not <)
        if a > b:
            lab[lab == 5] = 1
        out.append(("tie_le_%d%d" % (a, b), lab, 5, (0, 3)))
    return out


def reach_case():
    lab = np.zeros((1, 140, 141), np.int32)
    lab[0, 70, 70] = 2
    lab[0, 3, 130] = 1
    return ("reach", lab, 2, (0, 1, 5, 64))


def label_value_case():
    lab = np.zeros((1, 20, 66), np.int32)
    lab[0, 2, 2], lab[0, 10, 60], lab[0, 18, 30] = 5, 1, 5      # max_label itself, twice
    lab[0, 10, 10], lab[0, 5, 40], lab[0, 15, 64] = -1, 6, -2 ** 31   # background: negative and max_label + 1
    lab[0, 0, 65] = 2 ** 31 - 1
    return ("label_values", lab, 5, (0,))


def frame_leak_case():
    lab = np.zeros((3, 65, 64), np.int32)
    lab[0, 64, :] = 1                                           # the last row of frame 0
    lab[2, 0, :] = 2                                            # the first row of frame 2; frame 1 has only a far seed
    lab[1, 32, 0] = 3
    lab2 = lab.copy()
    lab2[1] = 0                                                 # ... or none at all
    return [("frame_leak", lab, 3, (0, 5)), ("frame_leak_empty", lab2, 3, (0,))]


def zone_cases():
    return shape_cases() + [seam_case(), empty_and_single_case(), reach_case(), label_value_case()] + tie_cases() \
        + frame_leak_case()


# ---- graph cases: (name, zones (N,H,W) int32, max_label) -------------------------------------------------------------
def straight_border():
    z = np.ones((1, 6, 200), np.int32)
    z[0, 3:] = 2                                                # a horizontal border 200 pixel pairs long
    return ("straight_border", z, 2)


def corner_case():
    z = np.zeros((2, 5, 70), np.int32)
    z[0, :2, :3] = 1                                            # covers the corner (0,0): 6 pixels, 4 on the border
    z[0, 2:, :3] = 2                                            # meets 1 vertically (3) ...
    z[0, :2, 3:5] = 2                                           # ... and horizontally (2)
    z[0, :, 10] = 3                                             # zone 0 between 2 and 3: no pair
    z[0, 4, 69] = 4
    z[1, :2, :3] = 1                                            # the same (1,2) in a second frame
    z[1, 2:, :3] = 2
    z[1, 0, 60:] = -7                                           # out of range either way: counts as 0
    z[1, 1, 60:] = 5
    return ("corner_both_ways_two_frames", z, 4)


def five_pairs():
    z = np.zeros((1, 3, 12), np.int32)
    z[0, :, :] = np.repeat(np.arange(1, 7), 2)[None]            # six stripes: five pairs of border 3
    return ("five_pairs", z, 6)


def own_labels():
    H, W = 33, 65
    return ("own_labels", np.arange(1, H * W + 1, dtype=np.int32).reshape(1, H, W), H * W)


def random_zones(seed, N, H, W, max_label):
    """zones of random seeds: irregular borders over several segments"""
    z, _ = zones_ref(random_labels(seed, N, H, W, max_label, 0.01 if H * W > 2000 else 0.1), max_label)
    return ("zones_%dx%dx%d" % (N, H, W), z, max_label)


def graph_cases():
    return [straight_border(), corner_case(), five_pairs(), own_labels(), random_zones(1, 3, 65, 130, 9),
            random_zones(2, 1, 1, 200, 5), random_zones(3, 2, 129, 1, 5), random_zones(4, 1, 2, 63, 3)]


# ---- neighbour cases ---------------------------------------------------------------------------------------------------
def object_frames(seed=3, N=3, H=90, W=131, count=14, classes=2):
    """disks of `classes` classes -> (labels int32 in table order, cls, centroid (k,3), frame): what measure_objects
    reports, from scipy (the object table itself is pinned in tests/test_gpu_objects.py)"""
    from tests import objects_cases as oc
    mask = oc.disks(seed, N, H, W, count, classes=classes, rmax=8)
    ref = oc.objects_ref(mask)
    return mask, ref['labels'], ref['cls'], ref['centroid'], ref['frame']


def shared_seed_objects():
    """two objects whose centres round to one pixel: a ring of class 1 around a dot of class 2, and a third object"""
    mask = np.zeros((1, 40, 70), np.uint8)
    yy, xx = np.mgrid[0:40, 0:70]
    r2 = (yy - 20) ** 2 + (xx - 20) ** 2
    mask[0][(r2 <= 100) & (r2 >= 36)] = 1
    mask[0][r2 <= 4] = 2
    mask[0][(yy - 20) ** 2 + (xx - 55) ** 2 <= 25] = 1
    return mask


def threshold_values(ref):
    """d_thresh at the centroid distance of a pair of neighbours (the median one of a table made without a threshold), just
    below it and just above it"""
    d = float(np.sort(ref['distance'])[len(ref['distance']) // 2])
    return d, float(np.nextafter(d, 0.0)), float(np.nextafter(d, np.inf))


# ---- the relation to the reference's Delaunay: a record, not a gate ---------------------------------------------------
def delaunay_agreement(seed, n_points, H, W):
    """uniform random points as one-pixel seeds: (zone pairs, Delaunay edges, shared) -- DESIGN.md quotes these figures"""
    rng = np.random.default_rng(seed)
    idx = np.sort(rng.choice(H * W, n_points, replace=False))
    lab = np.zeros((1, H, W), np.int32)
    lab.reshape(-1)[idx] = np.arange(1, n_points + 1)
    ind = ndimage.distance_transform_edt(lab[0] == 0, return_distances=False, return_indices=True)
    _, pairs = graph_ref(lab[0][ind[0], ind[1]][None], n_points)
    zone_pairs = {(int(a), int(b)) for _, a, b, _ in pairs}
    tri = spatial.Delaunay(np.stack([idx // W, idx % W], 1))
    edges = set()
    for s in tri.simplices:
        for i in range(3):
            a, b = sorted((int(s[i]) + 1, int(s[(i + 1) % 3]) + 1))
            edges.add((a, b))
    return len(zone_pairs), len(edges), len(zone_pairs & edges)


if __name__ == '__main__':
    for seed, n, hw in ((0, 40, 96), (1, 200, 256), (2, 800, 512)):
        zp, de, both = delaunay_agreement(seed, n, hw, hw)
        print("seed %d, %d points on %dx%d: %d zone pairs, %d Delaunay edges, %d shared (%.1f %% of the edges, %.1f %% of "
              "the pairs)" % (seed, n, hw, hw, zp, de, both, 100.0 * both / de, 100.0 * both / zp))
