"""Label zones, the contact graph and the neighbour table in volumes: the numpy / scipy restatements of
include/sequitr_hip.h, "Label zones and the contact graph in volumes", that the GPU path is pinned against, pure-Python
all-pairs versions that check the restatements on small volumes, and the cases the CPU and GPU tests share.

``zones3d_ref`` is the header's text: per slice (P, L) from neighbors_cases.zones_ref (scipy, per label), then the
lexicographic minimum over z' of (fl(A(z - z') + P), L) in numpy float64, A(k) = fl(fl(k dz) fl(k dz)).
``graph3d_ref`` is numpy on shifted views plus np.unique along the three axes, lateral and axial kept apart;
``neighbors3d_ref`` is the volumetric table of sequitr_amd/analysis/neighbors.py, written with Python loops over the pairs.
"""
import numpy as np

from tests import neighbors_cases as nc

NO_SEED = nc.NO_SEED
STRIP = 32                                                      # the depth pass's strip of columns
DZS = (1.0, 2.0, 0.5, 2.5, 1.0 / 3.0, 1e-3, 50.0)
EXACT_DZS = (1.0, 2.0, 0.5, 1.5)                                # every A(k) + P is exact: the all-pairs definition holds


def depth_term(k, dz):
    """A(k) = fl(fl(k dz) fl(k dz)) in float64; k an int or an int array"""
    t = np.asarray(k, np.float64) * np.float64(dz)
    return t * t


# ---- zones -----------------------------------------------------------------------------------------------------------
def planar_ref(labels, max_label):
    """labels (N,D,H,W) -> (P, L) of every slice on its own, both (N,D,H,W): P float64 with +inf in a slice without a
    seed, L int64.  The part of zones3d_ref that does not depend on dz or the reach: compute once, share."""
    lab = np.asarray(labels)
    N, D, H, W = lab.shape
    L, P = nc.zones_ref(lab.reshape(N * D, H, W), max_label)
    P = np.where(P == NO_SEED, np.inf, P.astype(np.float64))
    return P.reshape(N, D, H, W), L.astype(np.int64).reshape(N, D, H, W)


def zones3d_from_planar(P, L, dz=1.0, max_distance=0):
    """the depth combine: (zones int32, d2 float64), +inf and 0 in a volume without a seed"""
    N, D, H, W = P.shape
    zones = np.zeros((N, D, H, W), np.int32)
    d2 = np.full((N, D, H, W), np.inf)
    big = np.iinfo(np.int64).max
    for z in range(D):
        a = depth_term(np.abs(np.arange(D) - z), dz)            # (D,)
        s = a[None, :, None, None] + P                          # (N, D', H, W): one double add each
        best = s.min(1)
        lab = np.where(s == best[:, None], L, big).min(1)
        d2[:, z] = best
        zones[:, z] = np.where(np.isinf(best), 0, lab)
    if max_distance:
        zones[d2 > float(max_distance) * float(max_distance)] = 0
    return zones, d2


def zones3d_ref(labels, max_label, max_distance=0, dz=1.0):
    """labels (N,D,H,W) -> (zones int32, d2 float64)"""
    return zones3d_from_planar(*planar_ref(labels, max_label), dz=dz, max_distance=max_distance)


def zones3d_allpairs(labels, max_label, max_distance=0, dz=1.0):
    """the nearest seed in 3-D, the smallest label at a tie: voxel by voxel over all seeds (pure Python; small volumes, and
    spacings at which every sum is exact)"""
    lab = nc.seeds_of(labels, max_label)
    N, D, H, W = lab.shape
    zones = np.zeros((N, D, H, W), np.int32)
    d2 = np.full((N, D, H, W), np.inf)
    for n in range(N):
        seeds = [(int(z), int(y), int(x), int(lab[n, z, y, x])) for z, y, x in zip(*np.nonzero(lab[n]))]
        for z in range(D):
            for y in range(H):
                for x in range(W):
                    best = (np.inf, 0)
                    for sz, sy, sx, lb in seeds:
                        best = min(best, (float(depth_term(abs(z - sz), dz)) + float((y - sy) ** 2 + (x - sx) ** 2), lb))
                    d2[n, z, y, x] = best[0]
                    if not max_distance or best[0] <= float(max_distance) ** 2:
                        zones[n, z, y, x] = best[1]
    return zones, d2


# ---- graph -----------------------------------------------------------------------------------------------------------
def graph3d_ref(zones, max_label):
    """zones (N,D,H,W) -> stats (N, max_label+1, 2) int64 [voxels, face] and pairs (k,5) int64
    [volume, a, b, lateral, axial] sorted"""
    z = nc.seeds_of(zones, max_label)
    N, D, H, W = z.shape
    stats = np.zeros((N, max_label + 1, 2), np.int64)
    face = np.zeros((D, H, W), bool)
    face[0] = face[-1] = face[:, 0] = face[:, -1] = face[:, :, 0] = face[:, :, -1] = True
    rows = []
    for n in range(N):
        v = z[n]
        stats[n, :, 0] = np.bincount(v.ravel(), minlength=max_label + 1)
        stats[n, :, 1] = np.bincount(v[face], minlength=max_label + 1)
        for axial, (A, B) in ((0, (v[:, :, :-1], v[:, :, 1:])), (0, (v[:, :-1], v[:, 1:])), (1, (v[:-1], v[1:]))):
            m = (A != B) & (A > 0) & (B > 0)
            a, b = np.minimum(A[m], B[m]), np.maximum(A[m], B[m])
            rows.append(np.stack([np.full(a.shape, n, np.int64), a, b, np.full(a.shape, axial, np.int64)], 1))
    stats[:, 0] = 0
    rows = np.concatenate(rows) if rows else np.zeros((0, 4), np.int64)
    if not len(rows):
        return stats, np.zeros((0, 5), np.int64)
    uniq, inverse = np.unique(rows[:, :3], axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    pairs = np.zeros((len(uniq), 5), np.int64)
    pairs[:, :3] = uniq
    pairs[:, 3] = np.bincount(inverse[rows[:, 3] == 0], minlength=len(uniq))
    pairs[:, 4] = np.bincount(inverse[rows[:, 3] == 1], minlength=len(uniq))
    return stats, pairs


def graph3d_allpairs(zones, max_label):
    """the definition, voxel pair by voxel pair (pure Python)"""
    z = nc.seeds_of(zones, max_label)
    N, D, H, W = z.shape
    stats = np.zeros((N, max_label + 1, 2), np.int64)
    table = {}
    for n in range(N):
        for d in range(D):
            for y in range(H):
                for x in range(W):
                    a = int(z[n, d, y, x])
                    if a:
                        stats[n, a, 0] += 1
                        stats[n, a, 1] += d in (0, D - 1) or y in (0, H - 1) or x in (0, W - 1)
                    for axial, (d2, y2, x2) in ((0, (d, y, x + 1)), (0, (d, y + 1, x)), (1, (d + 1, y, x))):
                        if d2 < D and y2 < H and x2 < W:
                            b = int(z[n, d2, y2, x2])
                            if a and b and a != b:
                                table.setdefault((n, min(a, b), max(a, b)), [0, 0])[axial] += 1
    pairs = np.array([k + tuple(v) for k, v in sorted(table.items())], np.int64).reshape(-1, 5)
    return stats, pairs


# ---- neighbour table -------------------------------------------------------------------------------------------------
def centroid_seed_volume(volume, label, centroid, shape):
    out = np.zeros(shape, np.int32)
    c = np.asarray(centroid, np.float64).reshape(len(volume), 3)
    for k in range(len(volume) - 1, -1, -1):                    # descending: the smallest label is written last
        s = [int(min(max(np.floor(c[k, a] + 0.5), 0), shape[1 + a] - 1)) for a in range(3)]
        out[volume[k], s[0], s[1], s[2]] = label[k]
    return out


TABLE_COLUMNS = nc.TABLE_COLUMNS + ('border_lateral', 'border_axial', 'contact_area')


def neighbors3d_ref(labels, cls, centroid, volume, num_classes, d_thresh=100., max_distance=None, seeds='objects', spacing=1.0):
    """the columns of a volumetric NeighborTable as a dict (plus 'zones'), by Python loops over the zone pairs"""
    labels = np.asarray(labels)
    N = labels.shape[0]
    volume, cls = np.asarray(volume, np.int64), np.asarray(cls, np.int64)
    k = len(volume)
    dz = float(spacing)
    label = np.array([1 + i - int(np.sum(volume < volume[i])) for i in range(k)], np.int64)
    max_label = max([1] + [int(np.sum(volume == f)) for f in range(N)])
    c = np.asarray(centroid, np.float64).reshape(k, 3)
    src = labels if seeds == 'objects' else centroid_seed_volume(volume, label, c, labels.shape)
    zones, _ = zones3d_ref(src, max_label, max_distance or 0, dz)
    stats, pairs = graph3d_ref(zones, max_label)
    row_of = {(int(volume[i]), int(label[i])): i for i in range(k)}
    adj = [[] for _ in range(k)]
    removed = np.zeros(k, np.int64)
    n_pairs = n_removed = 0
    for f, a, b, lateral, axial in pairs:
        i, j = row_of[(int(f), int(a))], row_of[(int(f), int(b))]
        dp, dr, dc = c[i, 0] - c[j, 0], c[i, 1] - c[j, 1], c[i, 2] - c[j, 2]
        dist = np.sqrt((dz * dp) ** 2 + dr ** 2 + dc ** 2)
        if dist > d_thresh:
            removed[i] += 1
            removed[j] += 1
            n_removed += 1
            continue
        n_pairs += 1
        adj[i].append((j, int(lateral), int(axial), dist))
        adj[j].append((i, int(lateral), int(axial), dist))
    res = {'frame': volume, 'label': label, 'cls': cls, 'n_removed': removed, 'zones': zones,
           'n_pairs': n_pairs, 'n_pairs_removed': n_removed}
    res['n_total'] = np.array([len(a) for a in adj], np.int64)
    res['n_class'] = np.zeros((k, num_classes), np.int64)
    indptr, indices, lat, axi, distance = [0], [], [], [], []
    for i in range(k):
        for j, la, ax, d in sorted(adj[i]):
            res['n_class'][i, cls[j]] += 1
            indices.append(j)
            lat.append(la)
            axi.append(ax)
            distance.append(d)
        indptr.append(len(indices))
    res['indptr'], res['indices'] = np.array(indptr, np.int64), np.array(indices, np.int64)
    res['border_lateral'], res['border_axial'] = np.array(lat, np.int64), np.array(axi, np.int64)
    res['border'] = res['border_lateral'] + res['border_axial']
    res['contact_area'] = res['border_lateral'].astype(np.float64) * dz + res['border_axial'].astype(np.float64)
    res['distance'] = np.array(distance, np.float64)
    res['zone_area'] = np.array([stats[volume[i], label[i], 0] for i in range(k)], np.int64)
    res['zone_edge'] = np.array([stats[volume[i], label[i], 1] for i in range(k)], np.int64)
    with np.errstate(divide='ignore'):
        res['local_density'] = 1.0 / (res['zone_area'].astype(np.float64) * dz)
    return res


def assert_table(got, want, what=''):
    """every column of a volumetric table equal, floats bit for bit"""
    for name in TABLE_COLUMNS:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        assert g.shape == w.shape and g.dtype == w.dtype, "%s %s: %s %s against %s %s" % (what, name, g.shape, g.dtype,
                                                                                          w.shape, w.dtype)
        if g.dtype == np.float64:
            g, w = g.view(np.uint64), w.view(np.uint64)
        assert np.array_equal(g, w), "%s %s differs" % (what, name)


# ---- zone cases: (name, labels (N,D,H,W) int32, max_label, reaches, spacings) ----------------------------------------
def random_volume(seed, N, D, H, W, max_label=6, density=0.03):
    """sparse seeds of labels 1 .. max_label, sprinkled with background values (negative, max_label + 1); whole slices
    are emptied so that slices without a seed lie between slices with seeds"""
    lab = nc.random_labels(seed, N * D, H, W, max_label, density).reshape(N, D, H, W)
    if D > 2:
        lab[:, 1::3] = 0
    return lab


SHAPES = ((1, 1, 1, 1), (3, 2, 2, 2), (1, 3, 5, 63), (3, 9, 1, 64), (1, 33, 2, 65), (3, 1, 5, 127), (1, 2, 1, 128),
          (3, 3, 2, 129), (1, 9, 5, 130),
          (1, 33, 5, STRIP - 1), (3, 9, 2, STRIP), (1, 3, 1, STRIP + 1), (1, 5, 2, 2 * STRIP + 1))


def shape_cases():
    """W at 1, 2, 63 .. 65, 127 .. 130 and around the strip, H at 1, 2, 5, D at 1, 2, 3, 9, 33, N = 1 and 3"""
    out = []
    for i, (N, D, H, W) in enumerate(SHAPES):
        lab = random_volume(7 + i, N, D, H, W, density=0.08 if D * H * W < 500 else 0.03)
        if not lab.any():
            lab[0, 0, 0, 0] = 1
        out.append(("rand_%dx%dx%dx%d" % (N, D, H, W), lab, 6, (0, 5), DZS))
    return out


def seam_case():
    """seeds on both sides of the strip seams, in different slices"""
    lab = np.zeros((1, 5, 2, 2 * STRIP + 1), np.int32)
    lab[0, 0, 0, STRIP - 1], lab[0, 4, 0, STRIP] = 2, 1
    lab[0, 2, 1, 2 * STRIP - 1], lab[0, 1, 1, 2 * STRIP] = 1, 3
    lab[0, 3, 0, 0] = 4
    return ("strip_seams", lab, 4, (0, 5), DZS)


def empty_cases():
    lab = np.zeros((3, 9, 5, 40), np.int32)                     # volume 0: no seed;  volume 1: one seed;  volume 2: a value
    lab[1, 6, 3, 33] = 3                                        # above max_label only -- no seed either
    lab[2, 2, 2, 2] = 9
    gaps = np.zeros((1, 9, 4, 35), np.int32)                    # seeds in slices 0, 4 and 8 only
    gaps[0, 0, 0, 0], gaps[0, 4, 3, 20], gaps[0, 8, 1, 34], gaps[0, 8, 2, 5] = 2, 1, 3, 2
    return [("no_seed_one_seed", lab, 4, (0, 5), DZS), ("empty_slices_between", gaps, 3, (0, 3), DZS)]


def tie_cases():
    out = []
    for a, b in ((1, 2), (2, 1)):                               # both orders: the smaller label is met first / second
        lab = np.zeros((4, 11, 8, 12), np.int32)
        lab[0, 4, 3, 5], lab[0, 6, 3, 5] = a, b                 # z - 1 against z + 1 (voxel (5,3,5) and its whole slice)
        lab[1, 5, 3, 2], lab[1, 2, 3, 5] = a, b                 # 3 pixels across against 3 voxels deep, at voxel (5,3,5)
        lab[2, 10, 3, 5], lab[2, 8, 7, 5], lab[2, 5, 0, 1] = a, b, 3    # 3-4-5 at (5,3,5): 25 + 0, 9 + 16, 0 + (9 + 16)
        lab[3, 8, 3, 9], lab[3, 0, 3, 5] = a, b                 # best 9 + 16 from slice z + 3; P = 0 at slice z - 5: A(5) == best
        out.append(("ties_%d%d" % (a, b), lab, 3, (0, 5), (1.0, 2.0, 0.5)))
    return out


def reach_case():
    lab = np.zeros((1, 9, 6, 140), np.int32)
    lab[0, 4, 2, 70] = 2                                        # (4,2,6) and (4,2,134): D3 = 64^2, kept at R = 64;  (3,2,6): 64^2 + 1
    lab[0, 0, 5, 139] = 1                                       # (1,2,74): 9 + 16 = 5^2 kept at R = 5, (1,3,74): 26 dropped
    return ("reach", lab, 2, (0, 1, 5, 64), (1.0,))


def label_value_case():
    lab = np.zeros((1, 4, 6, 40), np.int32)
    lab[0, 0, 1, 2], lab[0, 2, 4, 30], lab[0, 3, 5, 15] = 5, 1, 5       # max_label itself, twice
    lab[0, 1, 3, 10], lab[0, 2, 0, 20], lab[0, 3, 2, 38] = -1, 6, -2 ** 31   # background: negative and max_label + 1
    lab[0, 0, 0, 39] = 2 ** 31 - 1
    return ("label_values", lab, 5, (0,), (1.0, 2.5))


def volume_leak_cases():
    lab = np.zeros((3, 3, 4, 33), np.int32)
    lab[0, 2] = 1                                               # the last slice of volume 0
    lab[2, 0] = 2                                               # the first slice of volume 2; volume 1 has only a far seed
    lab[1, 1, 3, 0] = 3
    lab2 = lab.copy()
    lab2[1] = 0                                                 # ... or none at all
    return [("volume_leak", lab, 3, (0, 5), (1.0, 1e-3, 50.0)), ("volume_leak_empty", lab2, 3, (0,), (1.0, 1e-3))]


def deep_case():
    """D = 700: 8 B x 700 x 32 columns exceed 160 KiB of LDS, so the call takes the global-memory form by itself"""
    lab = np.zeros((1, 700, 2, 33), np.int32)
    assert lab.shape[1] * STRIP * 8 > 160 * 1024                # more than a CU's whole LDS: no per-block limit admits it
    rng = np.random.default_rng(11)
    for _ in range(12):
        lab[0, rng.integers(0, 700), rng.integers(0, 2), rng.integers(0, 33)] = rng.integers(1, 5)
    lab[0, 0, 0, 0], lab[0, 699, 1, 32] = 3, 1
    return ("deep_700", lab, 4, (0, 64), (1.0, 1.0 / 3.0))


def zone_cases():
    return shape_cases() + [seam_case(), reach_case(), label_value_case(), deep_case()] + empty_cases() + tie_cases() \
        + volume_leak_cases()


def small_cases():
    """volumes up to 4 x 5 x 6 for the all-pairs checks: (name, labels, max_label)"""
    out = [("small_%d" % s, nc.random_labels(s, 2 * 4, 5, 6, 4, 0.08).reshape(2, 4, 5, 6), 4) for s in range(3)]
    lab = np.zeros((2, 4, 5, 6), np.int32)
    lab[0, 0, 2, 2], lab[0, 2, 2, 2] = 2, 1                     # z - 1 against z + 1 at voxel (1,2,2)
    lab[1, 0, 2, 0], lab[1, 3, 2, 3] = 2, 1                     # 3 pixels across against 3 voxels deep at voxel (0,2,3), dz = 1
    out.append(("small_ties", lab, 3))
    lab = np.zeros((2, 4, 5, 6), np.int32)
    lab[1, 3, 4, 5] = 2
    out.append(("small_empty_and_single", lab, 3))
    return out


# ---- graph cases: (name, zones (N,D,H,W) int32, max_label) -----------------------------------------------------------
def plane_borders():
    lateral = np.ones((1, 3, 4, 70), np.int32)                  # a border along h only: 3 x 70 lateral pairs, no axial one
    lateral[0, :, 2:] = 2
    axial = np.ones((1, 4, 3, 70), np.int32)                    # a border along d only
    axial[0, 2:] = 2
    return [("lateral_only", lateral, 2), ("axial_only", axial, 2)]


def l_shaped_two_volumes():
    z = np.zeros((2, 4, 5, 70), np.int32)
    z[0, :2, :2, :3] = 1                                        # covers the corner (0,0,0)
    z[0, 2:, :2, :3] = 2                                        # meets 1 axially ...
    z[0, :2, 2:, :3] = 2                                        # ... and laterally along h
    z[0, :2, :2, 3:5] = 2                                       # ... and along w
    z[0, :, :, 10] = 3                                          # zone 0 between 2 and 3: no pair
    z[0, 3, 4, 69] = 4                                          # one corner voxel: 1 voxel, 1 face voxel
    z[0, 0, 2, 64:] = 4                                         # an edge run
    z[1, :2, :2, :3] = 1                                        # the same (1,2) in a second volume
    z[1, 2:, :2, :3] = 2
    z[1, 0, 0, 60:] = -7                                        # out of range either way: counts as 0
    z[1, 1, 0, 60:] = 5
    return ("l_shape_two_volumes", z, 4)


def five_pairs():
    z = np.zeros((1, 2, 3, 12), np.int32)
    z[0] = np.repeat(np.arange(1, 7), 2)[None, None]            # six slabs: five pairs, lateral only
    return ("five_pairs", z, 6)


def own_labels():
    D, H, W = 3, 9, 65
    return ("own_labels", np.arange(1, D * H * W + 1, dtype=np.int32).reshape(1, D, H, W), D * H * W)


def random_zones(seed, N, D, H, W, max_label):
    z, _ = zones3d_ref(random_volume(seed, N, D, H, W, max_label, 0.02), max_label)
    return ("zones_%dx%dx%dx%d" % (N, D, H, W), z, max_label)


def graph_cases():
    return plane_borders() + [l_shaped_two_volumes(), five_pairs(), own_labels(), random_zones(1, 3, 5, 9, 130, 9),
                              random_zones(2, 1, 1, 1, 200, 5), random_zones(3, 2, 33, 2, 1, 5), random_zones(4, 1, 2, 1, 63, 3)]


# ---- neighbour cases --------------------------------------------------------------------------------------------------
def object_volumes(seed=3, N=2, D=12, H=40, W=70, count=12, classes=2):
    """3-D blobs of `classes` classes -> (mask, labels int32 in table order, cls, centroid (k,3), volume): what
    measure_objects reports, from scipy (the object table itself is pinned in tests/test_gpu_objects.py)"""
    from tests import objects_cases as oc
    mask = oc.blobs3d(seed, N, D, H, W, count, classes=classes, rmax=5)
    ref = oc.objects_ref(mask)
    return mask, ref['labels'], ref['cls'], ref['centroid'], ref['frame']


def shared_seed_volume():
    """two objects whose centres round to one voxel: a shell of class 1 around a dot of class 2, and a third object"""
    mask = np.zeros((1, 13, 20, 40), np.uint8)
    zz, yy, xx = np.mgrid[0:13, 0:20, 0:40]
    r2 = (zz - 6) ** 2 + (yy - 10) ** 2 + (xx - 10) ** 2
    mask[0][(r2 <= 25) & (r2 >= 9)] = 1
    mask[0][r2 <= 1] = 2
    mask[0][(zz - 6) ** 2 + (yy - 10) ** 2 + (xx - 30) ** 2 <= 9] = 1
    return mask
