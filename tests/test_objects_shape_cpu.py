"""Shape columns without a GPU: the scipy restatement of tests/objects_shape_cases.py against a pure-Python brute force
(flood fill, loops over voxels and neighbours, the code table written out), the derived columns of ObjectTable against
independent definitions, and the table's plumbing with and without shape_i."""
import math

import numpy as np
import pytest

from sequitr_amd.objects import ObjectTable
from tests import objects_shape_cases as sc

# code = 1 + 2 n4 + 10 n8 -> column; every other code counts nowhere
CODE_COLUMN = {5: 13, 7: 13, 15: 13, 17: 13, 25: 13, 27: 13, 21: 14, 33: 14, 13: 15, 23: 15}
EDGES3 = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))
DIAGONALS = ((-1, -1), (-1, 1), (1, -1), (1, 1))


def brute(mask):
    """rows (frame, class, key, area) and the 16 columns, by flood fill and loops; sorted by (frame, class, key)"""
    mask = np.asarray(mask)
    m4 = mask if mask.ndim == 4 else mask[:, None]
    N, P, H, W = m4.shape
    inside = lambda p, r, c: 0 <= p < P and 0 <= r < H and 0 <= c < W
    out = []
    for f in range(N):
        owner = -np.ones((P, H, W), np.int64)                   # object number of every voxel
        objects = []
        for p in range(P):
            for r in range(H):
                for c in range(W):
                    v = int(m4[f, p, r, c])
                    if v == 0 or owner[p, r, c] >= 0:
                        continue
                    owner[p, r, c] = len(objects)
                    stack, cells = [(p, r, c)], []
                    while stack:
                        cell = stack.pop()
                        cells.append(cell)
                        for d in EDGES3:
                            q = tuple(a + b for a, b in zip(cell, d))
                            if inside(*q) and owner[q] < 0 and int(m4[(f,) + q]) == v:
                                owner[q] = len(objects)
                                stack.append(q)
                    objects.append((v, (p * H + r) * W + c, cells))
        exposed = lambda cell, d: not inside(*[a + b for a, b in zip(cell, d)]) or \
            int(m4[(f,) + tuple(a + b for a, b in zip(cell, d))]) != int(m4[(f,) + cell])
        edges = EDGES3[2:] if P == 1 else EDGES3
        is_boundary = lambda cell: any(exposed(cell, d) for d in edges)
        for k, (v, key, cells) in enumerate(objects):
            row = [0] * 16
            for (p, r, c) in cells:
                for i, x in enumerate((p, r, c, p * p, r * r, c * c, p * r, p * c, r * c)):
                    row[i] += x
                for d in edges:
                    if exposed((p, r, c), d):
                        row[9 + [abs(x) for x in d].index(1)] += 1
                if not is_boundary((p, r, c)):
                    continue
                row[12] += 1
                if P > 1:
                    continue
                mine = lambda dr, dc: inside(0, r + dr, c + dc) and owner[0, r + dr, c + dc] == k and is_boundary((0, r + dr, c + dc))
                n4 = sum(mine(d[1], d[2]) for d in EDGES3[2:])
                n8 = sum(mine(dr, dc) for dr, dc in DIAGONALS)
                code = 1 + 2 * n4 + 10 * n8
                if code in CODE_COLUMN:
                    row[CODE_COLUMN[code]] += 1
            out.append(((f, v, key, len(cells)), row))
    out.sort(key=lambda t: t[0])
    return np.array([t[0] for t in out], np.int64).reshape(-1, 4), np.array([t[1] for t in out], np.int64).reshape(-1, 16)


def same_as_brute(mask):
    ref = sc.shape_ref(mask)
    head, rows = brute(mask)
    assert np.array_equal(np.stack([ref['frame'], ref['cls'], ref['key'], ref['area']], 1), head)
    bad = np.argwhere(ref['shape'] != rows)
    assert len(bad) == 0, [(int(i), sc.NAMES[j], int(ref['shape'][i, j]), int(rows[i, j])) for i, j in bad[:5]]
    return ref


def test_anchors():
    d = sc.shape_ref(sc.disk(20))['shape'][0]
    assert list(d[13:]) == [32, 16, 64]
    assert abs(32 + 16 * math.sqrt(2.0) + 64 * (1.0 + math.sqrt(2.0)) / 2.0 - 131.88) < 0.005
    assert list(sc.shape_ref(np.ones((1, 1, 1), np.uint8))['shape'][0, 9:]) == [0, 2, 2, 1, 0, 0, 0]
    full = sc.shape_ref(np.ones((1, 4, 6), np.uint8))['shape'][0]
    assert list(full[9:]) == [0, 12, 8, 16, 16, 0, 0]


@pytest.mark.parametrize("seed", range(4))
def test_restatement_equals_brute_force_on_frames(seed):
    same_as_brute(sc.noise(seed, (2, 12, 13), 2))
    same_as_brute(sc.noise(seed + 10, (1, 11, 12), 1, fill=0.6))
    same_as_brute(sc.noise(seed + 20, (1, 1 + seed, 13), 3))


def test_restatement_equals_brute_force_on_built_cases():
    same_as_brute(sc.diagonal_strangers())
    same_as_brute(sc.checkerboard(6, 7))
    same_as_brute(sc.walls()[:, :, :13])
    same_as_brute(sc.spiral(9, 12))
    same_as_brute(sc.comb(7, 11))
    same_as_brute(sc.disk(4))
    same_as_brute(sc.stacked_frames(3, 4, 6))


@pytest.mark.parametrize("planes", [1, 2, 4])
def test_restatement_equals_brute_force_on_volumes(planes):
    ref = same_as_brute(sc.noise(planes, (2, planes, 5, 6), 2))
    assert np.all(ref['shape'][:, 13:].sum(1) == 0) or planes == 1
    same_as_brute(sc.noise(planes + 5, (1, planes, 5, 6), 1, fill=0.7))
    same_as_brute(sc.stacked_volumes(2, planes, 3, 6))
    if planes == 1:                                             # a volume of one plane is the planar mask, perimeter included
        m = sc.noise(3, (2, 9, 11), 2)
        assert np.array_equal(sc.shape_ref(m)['shape'], sc.shape_ref(m[:, None])['shape'])


# ---- the derived columns -------------------------------------------------------------------------------------------------
def table_of(mask):
    """the ObjectTable of a mask from the restatements alone (rows shuffled, as the device hands them over)"""
    from tests import objects_cases as oc
    base, ref = oc.objects_ref(mask), sc.shape_ref(mask)
    assert np.array_equal(base['key'], ref['key'])
    k = len(ref['key'])
    ri, rf = np.zeros((k, 12), np.int64), np.zeros((k, 7))
    ri[:, 0], ri[:, 1], ri[:, 2], ri[:, 3], ri[:, 4:10] = base['frame'], base['cls'], base['key'], base['area'], base['bbox']
    rf[:, :3] = base['centroid']
    perm = np.random.default_rng(k).permutation(k)
    return ObjectTable(ri[perm], rf[perm], mask.shape[0], mask.ndim == 4, shape_i=ref['shape'][perm]), ref


def coords_of(mask, t, k):
    """the (n, 3) voxel coordinates of row k of table t, by scipy's labelling"""
    from scipy import ndimage
    m4 = mask if mask.ndim == 4 else mask[:, None]
    lab, _ = ndimage.label(m4[t.frame[k]] == t.cls[k])
    return np.argwhere(lab == lab.flat[t.key[k]])


@pytest.mark.parametrize("mask,dz", [(sc.disks(3, 2, 40, 70, 8, classes=2), 1.0), (sc.blobs3d(2, 1, 9, 20, 30, 6), 1.0),
                                     (sc.blobs3d(4, 1, 7, 20, 30, 5), 2.5)])
def test_covariance_and_axes_against_numpy(mask, dz):
    t, ref = table_of(mask)
    assert np.array_equal(t._shape_rows(), ref['shape'])
    cov, axes = t.covariance(dz), t.axis_lengths((dz, 1, 1))
    scale = np.array([dz, 1.0, 1.0])
    for k in range(len(t)):
        xyz = coords_of(mask, t, k)
        assert len(xyz) == t.area[k]
        rel = (xyz - t.bbox[k, :3]) * scale                     # box-relative: small numbers, np.cov has nothing to cancel
        want = np.cov(rel.T, bias=True).reshape(3, 3)
        if mask.ndim == 3:
            want = want[1:, 1:]
        # both sides are a few roundings from the exact rational
        assert np.abs(cov[k] - want).max() <= 1e-12 * (np.trace(want) + 1.0), k
        lam = np.clip(np.linalg.eigvalsh(want)[::-1], 0.0, None)
        assert np.abs(axes[k] - 4.0 * np.sqrt(lam)).max() <= 1e-9 * (4.0 * np.sqrt(lam[0]) + 1.0), k
        assert np.all(np.diff(axes[k]) <= 0.0)


def test_covariance_is_exact_far_from_the_origin():
    m = np.zeros((1, 40, 30000), np.uint8)
    m[0, 30:33, 29990:29997] = 1                                # a 3 x 7 rectangle at column 29990
    t, _ = table_of(m)
    assert np.array_equal(t.covariance()[0], [[(9 - 1) / 12.0, 0.0], [0.0, (49 - 1) / 12.0]])   # (n^2 - 1) / 12, exact
    assert t.orientation[0] == math.pi / 2 and t.extent[0] == 1.0
    assert np.allclose(t.axis_lengths()[0], [4 * math.sqrt(4.0), 4 * math.sqrt(8 / 12.0)], rtol=1e-15)
    assert abs(t.eccentricity[0] - math.sqrt(1.0 - (8 / 12.0) / 4.0)) < 1e-15
    assert t.perimeter_counts[0].tolist() == [16, 0, 0] and t.perimeter[0] == 16.0
    assert t.crack_perimeter[0] == 20.0 and t.boundary[0] == 16
    assert t.circularity[0] == 4.0 * math.pi * 21 / 16.0 ** 2
    assert t.equivalent_diameter()[0] == math.sqrt(4.0 * 21 / math.pi)


def test_rasterised_ellipse_approaches_its_parameters():
    a, b, theta = 60.0, 25.0, 0.5                               # semi-axes; the major axis `theta` from the row axis
    yy, xx = np.mgrid[0:200, 0:200] - 100.0
    u, v = yy * math.cos(theta) + xx * math.sin(theta), -yy * math.sin(theta) + xx * math.cos(theta)
    m = ((u / a) ** 2 + (v / b) ** 2 <= 1.0).astype(np.uint8)[None]
    t, _ = table_of(m)
    assert len(t) == 1
    assert np.abs(t.axis_lengths()[0] - [2 * a, 2 * b]).max() < 0.2      # a filled ellipse returns its own axes
    assert abs(t.orientation[0] - theta) < 2e-3
    assert abs(t.eccentricity[0] - math.sqrt(1.0 - (b / a) ** 2)) < 2e-3
    assert abs(t.equivalent_diameter()[0] - 2.0 * math.sqrt(a * b)) < 0.1
    assert t.extent[0] == t.area[0] / float(np.prod(t.bbox[0, 4:6] - t.bbox[0, 1:3]))


def test_orientation_of_bars():
    m = np.zeros((4, 21, 21), np.uint8)
    m[0, 2:19, 10] = 1                                          # along the rows
    m[1, 10, 2:19] = 1                                          # along the columns
    rr, cc = np.mgrid[0:21, 0:21]
    m[2] = (abs(rr - cc) <= 1) & (rr >= 2) & (rr <= 18) & (cc >= 2) & (cc <= 18)   # down-right, its own mirror image
    m[3] = m[2, :, ::-1]                                        # down-left
    t, _ = table_of(m)
    assert len(t) == 4
    assert t.orientation[0] == 0.0 and t.orientation[1] == math.pi / 2
    assert abs(t.orientation[2] - math.pi / 4) < 1e-15 and abs(t.orientation[3] + math.pi / 4) < 1e-15
    assert np.all(t.eccentricity[:2] == 1.0) and np.all(t.axis_lengths()[:2, 1] == 0.0)
    one = np.zeros((1, 3, 3), np.uint8)
    one[0, 1, 1] = 1
    t1, _ = table_of(one)                                       # one pixel: no axes, no perimeter
    assert t1.orientation[0] == 0.0 and t1.eccentricity[0] == 0.0 and t1.perimeter[0] == 0.0 and t1.circularity[0] == 0.0
    assert t1.axis_lengths()[0].tolist() == [0.0, 0.0] and t1.crack_perimeter[0] == 4.0


@pytest.mark.parametrize("dz", [1.0, 2.5])
def test_volume_columns(dz):
    m = np.zeros((1, 8, 9, 10), np.uint8)
    m[0, 1:5, 2:5, 3:9] = 1                                     # a 4 x 3 x 6 cuboid
    t, _ = table_of(m)
    assert t.faces[0].tolist() == [2 * 18, 2 * 24, 2 * 12] and t.boundary[0] == 72 - 2 * 1 * 4
    assert t.perimeter is None and t.eccentricity is None and t.orientation is None and t.circularity is None
    assert t.surface_area(dz)[0] == 36 * 1.0 + (48 + 24) * dz
    assert t.sphericity(dz)[0] == math.pi ** (1.0 / 3.0) * (6.0 * 72 * dz) ** (2.0 / 3.0) / t.surface_area(dz)[0]
    assert t.equivalent_diameter(dz)[0] == np.cbrt(6.0 * 72 * dz / math.pi)
    assert t.extent[0] == 1.0
    want = np.diag([(16 - 1) / 12.0 * dz * dz, (9 - 1) / 12.0, (36 - 1) / 12.0])
    assert np.allclose(t.covariance(dz)[0], want, rtol=1e-15, atol=0.0)
    assert np.allclose(t.axis_lengths(dz)[0], 4.0 * np.sqrt(np.sort(np.diag(want))[::-1]), rtol=1e-14)
    ball, _ = table_of(sc.ball(12))
    assert 0.6 < ball.sphericity()[0] < 0.7                     # voxel faces overstate a sphere's area by about 3/2
    for bad in (0.0, -1.0, float('nan'), (1.0, 2.0, 1.0), (1.0, 1.0), 'x', True):
        with pytest.raises(ValueError):
            t.covariance(bad)


# ---- the table with and without shape_i -----------------------------------------------------------------------------------
OLD_KEYS = ['frame', 'cls', 'key', 'area', 'bbox', 'centroid', 'label']
SHAPE_KEYS = ['coord_sums', 'moments2', 'faces', 'boundary', 'perimeter_counts', 'covariance', 'axis_lengths',
              'equivalent_diameter', 'extent']
PLANAR_KEYS = ['eccentricity', 'orientation', 'perimeter', 'crack_perimeter', 'circularity']
VOLUME_KEYS = ['surface_area', 'sphericity']


def test_table_with_and_without_shape():
    m = sc.disks(5, 3, 30, 40, 6, classes=2)
    t, ref = table_of(m)
    cols = t.columns()
    assert list(cols) == OLD_KEYS + SHAPE_KEYS + PLANAR_KEYS
    assert cols['coord_sums'].shape == (len(t), 3) and cols['moments2'].shape == (len(t), 6) and cols['faces'].shape == (len(t), 3)
    assert cols['boundary'].shape == (len(t),) and cols['perimeter_counts'].shape == (len(t), 3)
    assert all(cols[k].dtype == np.int64 for k in SHAPE_KEYS[:5]) and all(cols[k].dtype == np.float64 for k in SHAPE_KEYS[5:] + PLANAR_KEYS)
    assert cols['covariance'].shape == (len(t), 2, 2)
    ri, rf = t._rows()
    plain = ObjectTable(ri, rf, 3)                              # positional use, as before
    assert list(plain.columns()) == OLD_KEYS and not plain.with_shape and plain._shape_rows() is None
    assert plain.moments2 is None and plain.perimeter is None and plain.covariance() is None and plain.extent is None
    per = t.frames()
    assert sum(len(p) for p in per) == len(t) and all(p.with_shape for p in per)
    assert np.array_equal(np.concatenate([p._shape_rows() for p in per]), ref['shape'])
    assert np.array_equal(np.concatenate([p.perimeter for p in per]), t.perimeter)
    assert all(not p.with_shape for p in plain.frames())
    again = ObjectTable.concatenate(per, [0, 0, 0], 3)     # frames() keeps the stack's numbering
    assert again.with_shape and np.array_equal(again._shape_rows(), ref['shape']) and np.array_equal(again.frame, t.frame)
    for k, v in t.columns().items():
        assert np.array_equal(again.columns()[k], v), k
    shifted = ObjectTable.concatenate([per[2], per[0]], [2, 1], 6)       # batches in any order: rows follow the frames
    assert np.array_equal(shifted._shape_rows(), np.concatenate([per[0]._shape_rows(), per[2]._shape_rows()]))
    mixed = ObjectTable.concatenate([per[0], plain.frames()[1]], [0, 1], 2)
    assert not mixed.with_shape and list(mixed.columns()) == OLD_KEYS
    with pytest.raises(ValueError):
        ObjectTable(ri, rf, 3, shape_i=ref['shape'][:-1])
    empty = ObjectTable(np.zeros((0, 12)), np.zeros((0, 7)), 2, shape_i=np.zeros((0, 16)))
    assert list(empty.columns()) == OLD_KEYS + SHAPE_KEYS + PLANAR_KEYS and empty.columns()['covariance'].shape == (0, 2, 2)
    v, _ = table_of(sc.blobs3d(1, 2, 4, 9, 12, 3))
    assert list(v.columns(spacing=2.0)) == OLD_KEYS + SHAPE_KEYS + VOLUME_KEYS and v.columns()['covariance'].shape == (len(v), 3, 3)
    assert np.array_equal(v.columns(spacing=2.0)['surface_area'], v.surface_area(2.0))


def test_segment_volume_refuses_shape_without_brick_before_any_input_is_opened(tmp_path):
    from sequitr_amd import jobs
    missing = str(tmp_path / "missing.npy")                     # an input that does not even exist
    with pytest.raises(ValueError, match="brick"):
        jobs.SERVER_segment_volume({"input": missing, "output": str(tmp_path)}, {"shape": True})
    for bad in (0, "thick", float("nan")):
        with pytest.raises(ValueError, match="spacing"):
            jobs.SERVER_segment_volume({"input": missing, "output": str(tmp_path), "brick": (8, 8, 4), "spacing": bad},
                                       {"shape": True})
    assert "shape" in jobs.VOLUME_ANALYSIS_OPTIONS and list(tmp_path.iterdir()) == []
