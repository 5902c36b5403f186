"""Mask (+ intensity image) -> one row of measurements per segmented object, on the GPU: what ``CentroidWriter.write``'s
docstring promises beyond the centroid (sequitr/utils.py:492-494, "if the original image data is provided, some image
statistics are calculated") and the reference never built -- area, bounding box, centre of mass, and the sum, sum of
squares, minimum and maximum of the image under every object; a label image; a size filter.

``measure_objects(mask, image)`` is the device path: one C-ABI call (sq_objects_measure: the centroid path's union-find
labelling, then per-object accumulators), the rows sorted on the host into the reference's order -- frame, class ascending,
scipy label order = first pixel in raster order -- and, when a label image or the filtered mask is asked for, a second call
(sq_objects_relabel) that writes them from the labelling the first one left in its workspace.  Integer columns equal
scipy.ndimage's label / sum_labels / find_objects / minimum / maximum exactly, centres equal center_of_mass bit for bit
(tests/test_gpu_objects.py).  There is no CPU path: mask and image must live in GPU memory.

``measure_objects(mask, shape=True)`` makes one more call on that labelling (sq_objects_shape) for the regionprops
columns: second-order coordinate sums, exposed faces, boundary voxels and the counts of the 4-neighbourhood perimeter
estimator, all integers equal to the scipy restatement of tests/objects_shape_cases.py; ObjectTable derives ellipse axes,
orientation, eccentricity, perimeter, circularity, surface area and sphericity from them on the host, in float64.
"""
import numpy as np
import torch

from . import _lib

_MAX_OUT = 1 << 16                                              # room for objects of the first attempt

PIX = {torch.uint8: 0, torch.uint16: 1, torch.float32: 2}

_COLUMNS = ('frame', 'cls', 'key', 'area', 'bbox', 'centroid', 'label')
_INTENSITY = ('intensity_sum', 'intensity_sumsq', 'intensity_min', 'intensity_max')
_SHAPE = ('coord_sums', 'moments2', 'faces', 'boundary', 'perimeter_counts')      # the slices of a shape_i row, in order
_SHAPE_COLS = (slice(0, 3), slice(3, 9), slice(9, 12), 12, slice(13, 16))
_PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))      # moments2's products along (plane, row, column)


class ObjectTable(object):
    """Per-object columns (numpy, host) in the reference's order: frame, then class ascending, then first pixel.

    frame, cls, key (linear index of the first voxel within its frame), area: int64 (k,);  bbox: int64 (k,6)
    [lo_plane, lo_row, lo_col, hi_plane, hi_row, hi_col], hi exclusive (planar masks: plane 0 .. 1);  centroid: float64 (k,3)
    along (plane, row, column);  label: int64, the object's 1-based rank within its frame = its value in ``.labels``.
    With an image: intensity_sum, intensity_sumsq, intensity_min, intensity_max -- int64 for uint8 / uint16 images, float64
    for float32 ones -- and the derived mean_intensity, std_intensity; without one these are None.
    ``.labels`` / ``.mask`` hold the device tensors measure_objects was asked for, ``.found`` the number of components
    before the size filter.

    With ``shape_i`` (the (k,16) int64 rows of sq_objects_shape, in the order of rows_i) the table also holds, int64:
    coord_sums (k,3) = the sums of plane, row, column over the object's voxels;  moments2 (k,6) = the sums of the products
    [pp, rr, cc, pr, pc, rc];  faces (k,3) = the exposed voxel faces along (plane, row, column);  boundary (k,) = the voxels
    with an exposed face;  perimeter_counts (k,3) = [straight, diagonal, mixed] of the 4-neighbourhood perimeter estimator
    (planar masks; 0 for volumes).  From them, in float64 on the host: covariance, axis_lengths, eccentricity, orientation,
    equivalent_diameter, extent, perimeter, crack_perimeter, circularity, surface_area, sphericity -- each docstring is the
    formula.  `spacing` is the depth of a voxel in units of its (square) in-plane side: dz, or (dz, 1, 1).  Without
    shape_i these columns are None and the derived ones return None."""

    def __init__(self, rows_i, rows_f, frames, volumetric=False, image_dtype=None, shape_i=None):
        rows_i = np.asarray(rows_i, np.int64).reshape(-1, 12)
        rows_f = np.asarray(rows_f, np.float64).reshape(-1, 7)
        if len(rows_i) != len(rows_f):
            raise ValueError('rows_i and rows_f hold %d and %d objects' % (len(rows_i), len(rows_f)))
        if shape_i is not None:
            shape_i = np.asarray(shape_i, np.int64).reshape(-1, 16)
            if len(shape_i) != len(rows_i):
                raise ValueError('rows_i and shape_i hold %d and %d objects' % (len(rows_i), len(shape_i)))
        order = np.lexsort((rows_i[:, 2], rows_i[:, 1], rows_i[:, 0]))   # frame, then class, then first pixel
        self.order = order                                      # position of every sorted row in the rows given
        rows_i, rows_f = rows_i[order], rows_f[order]
        self.n_frames, self.volumetric = int(frames), bool(volumetric)
        self.image_dtype = None if image_dtype is None else np.dtype(image_dtype)
        self.frame, self.cls, self.key, self.area = (np.ascontiguousarray(rows_i[:, c]) for c in range(4))
        self.bbox = np.ascontiguousarray(rows_i[:, 4:10])
        self.centroid = np.ascontiguousarray(rows_f[:, 0:3])
        bounds = np.searchsorted(self.frame, np.arange(self.n_frames + 1))
        self._bounds = bounds
        self.label = np.arange(1, len(rows_i) + 1, dtype=np.int64) - bounds[np.clip(self.frame, 0, max(self.n_frames - 1, 0))] \
            if len(rows_i) else np.zeros(0, np.int64)
        if self.image_dtype is None:
            self.intensity_sum = self.intensity_sumsq = self.intensity_min = self.intensity_max = None
        elif self.image_dtype.kind == 'u':
            self.intensity_sum, self.intensity_sumsq = np.ascontiguousarray(rows_i[:, 10]), np.ascontiguousarray(rows_i[:, 11])
            self.intensity_min, self.intensity_max = rows_f[:, 5].astype(np.int64), rows_f[:, 6].astype(np.int64)
        else:
            self.intensity_sum, self.intensity_sumsq, self.intensity_min, self.intensity_max = (
                np.ascontiguousarray(rows_f[:, c]) for c in (3, 4, 5, 6))
        shape_i = None if shape_i is None else shape_i[order]
        for name, cols in zip(_SHAPE, _SHAPE_COLS):
            setattr(self, name, None if shape_i is None else np.ascontiguousarray(shape_i[:, cols]))
        self.labels = self.mask = None
        self.found = len(rows_i)

    def __len__(self):
        return len(self.frame)

    @property
    def with_intensity(self):
        return self.image_dtype is not None

    @property
    def mean_intensity(self):
        """sum / area in float64 (for integer images both are exact in float64: Python's int / int, bit for bit)"""
        if not self.with_intensity:
            return None
        return self.intensity_sum.astype(np.float64) / self.area.astype(np.float64)

    @property
    def var_intensity(self):
        """max(0, (sumsq - sum * sum / area) / area) in float64: the population variance"""
        if not self.with_intensity:
            return None
        s, q, a = (v.astype(np.float64) for v in (self.intensity_sum, self.intensity_sumsq, self.area))
        with np.errstate(invalid='ignore'):
            var = (q - s * s / a) / a
            return np.where(var < 0.0, 0.0, var)                # NaN stays NaN

    @property
    def std_intensity(self):
        """sqrt(var_intensity): the population standard deviation"""
        if not self.with_intensity:
            return None
        return np.sqrt(self.var_intensity)

    def _take(self, lo, hi, frames):
        t = object.__new__(ObjectTable)
        t.n_frames, t.volumetric, t.image_dtype = frames, self.volumetric, self.image_dtype
        for name in _COLUMNS + _INTENSITY + _SHAPE:
            v = getattr(self, name)
            setattr(t, name, None if v is None else v[lo:hi])
        t.order = self.order[lo:hi]
        t._bounds = None
        t.labels = t.mask = None
        t.found = hi - lo
        return t

    def frames(self):
        """a list of n_frames tables, one per frame (the columns are views; `frame` keeps the stack's numbering)"""
        return [self._take(int(self._bounds[i]), int(self._bounds[i + 1]), 1) for i in range(self.n_frames)]

    def coords(self):
        """a list of n_frames (k,5) float32 arrays [frame, x, y, z, class], CentroidWriter's convention and exactly
        mask_centroids' rows: planar x = row centre, y = column centre, z = 0; volumetric the centres along the three axes"""
        rows = np.zeros((len(self), 5), np.float32)
        rows[:, 0] = self.frame
        if self.volumetric:
            rows[:, 1:4] = self.centroid
        else:
            rows[:, 1:3] = self.centroid[:, 1:3]
        rows[:, 4] = self.cls
        b = self._bounds if self._bounds is not None else np.array([0, len(self)])
        return [rows[b[i]:b[i + 1]] for i in range(len(b) - 1)]

    def intensity(self):
        """(k,4) float64 [mean, std, min, max], or None without an image"""
        if not self.with_intensity:
            return None
        return np.stack([self.mean_intensity, self.std_intensity, self.intensity_min.astype(np.float64),
                         self.intensity_max.astype(np.float64)], axis=1).reshape(-1, 4)

    def columns(self, spacing=1.0):
        """the columns as a dict of arrays, for np.savez; with shape columns also the derived ones, the metric ones under
        `spacing` (planar tables: eccentricity, orientation, perimeter, crack_perimeter, circularity; volumes: surface_area,
        sphericity)"""
        d = {name: getattr(self, name) for name in _COLUMNS}
        if self.with_intensity:
            d.update({name: getattr(self, name) for name in _INTENSITY})
            d['mean_intensity'], d['std_intensity'] = self.mean_intensity, self.std_intensity
        if self.with_shape:
            d.update({name: getattr(self, name) for name in _SHAPE})
            d['covariance'], d['axis_lengths'] = self.covariance(spacing), self.axis_lengths(spacing)
            d['equivalent_diameter'], d['extent'] = self.equivalent_diameter(spacing), self.extent
            if self.volumetric:
                d['surface_area'], d['sphericity'] = self.surface_area(spacing), self.sphericity(spacing)
            else:
                for name in ('eccentricity', 'orientation', 'perimeter', 'crack_perimeter', 'circularity'):
                    d[name] = getattr(self, name)
        return d

    @classmethod
    def concatenate(cls, tables, first_frames, frames):
        """one table of `frames` frames out of per-batch tables whose frame 0 is frame first_frames[i] of the stack; the
        shape columns are carried when every table has them"""
        if not tables:
            return cls(np.zeros((0, 12), np.int64), np.zeros((0, 7)), frames)
        ri, rf = [], []
        for t, first in zip(tables, first_frames):
            i, f = t._rows()
            i[:, 0] += int(first)
            ri.append(i)
            rf.append(f)
        shape_i = np.concatenate([t._shape_rows() for t in tables]) if all(t.with_shape for t in tables) else None
        out = cls(np.concatenate(ri), np.concatenate(rf), frames, tables[0].volumetric, tables[0].image_dtype, shape_i=shape_i)
        out.found = int(sum(t.found for t in tables))
        return out

    def _rows(self):
        """the (k,12) int64 and (k,7) float64 rows of include/sequitr_hip.h this table was made from, sorted"""
        ri = np.zeros((len(self), 12), np.int64)
        rf = np.zeros((len(self), 7), np.float64)
        ri[:, 0], ri[:, 1], ri[:, 2], ri[:, 3], ri[:, 4:10] = self.frame, self.cls, self.key, self.area, self.bbox
        rf[:, 0:3] = self.centroid
        if self.with_intensity:
            if self.image_dtype.kind == 'u':
                ri[:, 10], ri[:, 11] = self.intensity_sum, self.intensity_sumsq
            for c, name in zip((3, 4, 5, 6), _INTENSITY):
                rf[:, c] = getattr(self, name)
        return ri, rf

    def _shape_rows(self):
        """the (k,16) int64 rows of sq_objects_shape this table was made from, sorted; None without shape columns"""
        if not self.with_shape:
            return None
        rows = np.zeros((len(self), 16), np.int64)
        for name, cols in zip(_SHAPE, _SHAPE_COLS):
            rows[:, cols] = getattr(self, name)
        return rows

    # ---- shape: derived columns, float64 on the host -----------------------------------------------------------------
    @property
    def with_shape(self):
        return self.moments2 is not None

    def covariance(self, spacing=1.0):
        """(k,3,3) along (plane, row, column) for volumes, the (row, column) (k,2,2) block for planar tables:
        entry ab = float(area * S_ab - S_a * S_b) / float(area)**2 * spacing_a * spacing_b, the numerator formed in exact
        Python integers (S_ab / area - mean_a * mean_b would cancel at coordinates in the thousands)"""
        if not self.with_shape:
            return None
        sp = _spacing(spacing)
        axes = (0, 1, 2) if self.volumetric else (1, 2)
        out = np.zeros((len(self), len(axes), len(axes)), np.float64)
        area = [int(v) for v in self.area]
        S1 = [[int(v) for v in row] for row in self.coord_sums]
        S2 = [[int(v) for v in row] for row in self.moments2]
        for i, a in enumerate(axes):
            for j, b in enumerate(axes):
                col = _PAIRS.index((min(a, b), max(a, b)))
                for k in range(len(self)):
                    num = area[k] * S2[k][col] - S1[k][a] * S1[k][b]
                    out[k, i, j] = float(num) / float(area[k]) ** 2 * sp[a] * sp[b]
        return out

    def _eigenvalues(self, spacing=1.0):
        """eigenvalues of covariance(spacing), clipped at 0, descending: (a + c) / 2 +- sqrt(((a - c) / 2)**2 + b**2) for
        planar tables, np.linalg.eigvalsh for volumes"""
        cov = self.covariance(spacing)
        if self.volumetric:
            lam = np.linalg.eigvalsh(cov)[:, ::-1] if len(self) else np.zeros((0, 3))
        else:
            a, b, c = cov[:, 0, 0], cov[:, 0, 1], cov[:, 1, 1]
            mid, half = (a + c) / 2.0, np.sqrt(((a - c) / 2.0) ** 2 + b ** 2)
            lam = np.stack([mid + half, mid - half], axis=1)
        return np.clip(lam, 0.0, None)

    def axis_lengths(self, spacing=1.0):
        """(k,2) or (k,3), descending: 4 * sqrt(lambda), lambda = the eigenvalues of covariance(spacing) clipped at 0 --
        (a + c) / 2 +- sqrt(((a - c) / 2)**2 + b**2) for planar tables, np.linalg.eigvalsh for volumes.  Regionprops' major /
        minor axis convention: a filled ellipse returns its own axes."""
        if not self.with_shape:
            return None
        return 4.0 * np.sqrt(self._eigenvalues(spacing))

    @property
    def eccentricity(self):
        """sqrt(1 - lambda_2 / lambda_1), 0 when lambda_1 = 0.  Planar tables; None for volumes."""
        if not self.with_shape or self.volumetric:
            return None
        lam = self._eigenvalues()
        safe = np.where(lam[:, 0] > 0.0, lam[:, 0], 1.0)
        return np.where(lam[:, 0] > 0.0, np.sqrt(np.clip(1.0 - lam[:, 1] / safe, 0.0, None)), 0.0)

    @property
    def orientation(self):
        """0.5 * atan2(2 * cov_rc, cov_rr - cov_cc), 0 when both arguments are 0: the angle of the major axis from the row
        axis, in (-pi/2, pi/2].  Planar tables; None for volumes."""
        if not self.with_shape or self.volumetric:
            return None
        cov = self.covariance()
        return 0.5 * np.arctan2(2.0 * cov[:, 0, 1], cov[:, 0, 0] - cov[:, 1, 1]) + 0.0

    def equivalent_diameter(self, spacing=1.0):
        """sqrt(4 * area / pi) for planar tables, cbrt(6 * area * dz / pi) for volumes"""
        if not self.with_shape:
            return None
        area = self.area.astype(np.float64)
        if self.volumetric:
            return np.cbrt(6.0 * area * _spacing(spacing)[0] / np.pi)
        return np.sqrt(4.0 * area / np.pi)

    @property
    def extent(self):
        """area / box volume"""
        if not self.with_shape:
            return None
        box = np.prod(self.bbox[:, 3:6] - self.bbox[:, 0:3], axis=1)
        return self.area.astype(np.float64) / box.astype(np.float64)

    @property
    def perimeter(self):
        """per_straight + per_diag * sqrt(2) + per_mixed * ((1 + sqrt(2)) / 2), evaluated in that order.  Planar tables."""
        if not self.with_shape or self.volumetric:
            return None
        p = self.perimeter_counts.astype(np.float64)
        return p[:, 0] + p[:, 1] * np.sqrt(2.0) + p[:, 2] * ((1.0 + np.sqrt(2.0)) / 2.0)

    @property
    def crack_perimeter(self):
        """faces_r + faces_c: the length of the pixel edges between the object and everything else.  Planar tables."""
        if not self.with_shape or self.volumetric:
            return None
        return (self.faces[:, 1] + self.faces[:, 2]).astype(np.float64)

    @property
    def circularity(self):
        """4 * pi * area / perimeter**2, with inf -> 0 for a one-pixel object whose perimeter is 0.  Planar tables."""
        if not self.with_shape or self.volumetric:
            return None
        per = self.perimeter
        with np.errstate(divide='ignore'):
            c = 4.0 * np.pi * self.area.astype(np.float64) / per ** 2
        return np.where(np.isinf(c), 0.0, c)

    def surface_area(self, spacing=1.0):
        """faces_p * 1 + (faces_r + faces_c) * dz: the exposed voxel faces weighted by their areas.  Volumes."""
        if not self.with_shape or not self.volumetric:
            return None
        dz = _spacing(spacing)[0]
        return self.faces[:, 0].astype(np.float64) * 1.0 + (self.faces[:, 1] + self.faces[:, 2]).astype(np.float64) * dz

    def sphericity(self, spacing=1.0):
        """pi**(1/3) * (6 * area * dz)**(2/3) / surface_area(spacing).  Volumes."""
        if not self.with_shape or not self.volumetric:
            return None
        dz = _spacing(spacing)[0]
        return np.pi ** (1.0 / 3.0) * (6.0 * self.area.astype(np.float64) * dz) ** (2.0 / 3.0) / self.surface_area(spacing)


def _spacing(spacing):
    """(dz, 1.0, 1.0) from dz or (dz, 1, 1); dz finite and > 0, ValueError for anything else"""
    try:
        if isinstance(spacing, bool):
            raise TypeError
        if np.ndim(spacing) == 0:
            sp = (float(spacing), 1.0, 1.0)
        else:
            sp = tuple(float(v) for v in spacing)
    except (TypeError, ValueError):
        raise ValueError("spacing must be dz or (dz, 1, 1) with dz a finite number > 0, got %r" % (spacing,))
    if len(sp) != 3 or sp[1:] != (1.0, 1.0) or not (sp[0] > 0.0 and np.isfinite(sp[0])):
        raise ValueError("spacing must be dz or (dz, 1, 1) with dz a finite number > 0, got %r" % (spacing,))
    return sp


def _check_mask(mask):
    if not isinstance(mask, torch.Tensor):
        raise TypeError("mask must be a torch.Tensor in GPU memory")
    if not mask.is_cuda:
        raise _lib.SequitrHipError("mask must live in GPU memory (no CPU fallback exists)")
    if mask.dtype != torch.uint8 or mask.dim() not in (3, 4) or not mask.is_contiguous():
        raise ValueError("mask must be a contiguous (N,H,W) or (N,D0,D1,D2) uint8 tensor")


def measure_objects(mask, image=None, min_area=1, max_area=None, labels=False, filtered_mask=False, shape=False):
    """Measure every connected component of `mask`: uint8 class labels on the GPU, planar (N,H,W) or volumetric
    (N,D0,D1,D2) -- for volumes in CentroidWriter's sense pass the array after its swapaxes(1,-1), as for mask_centroids.
    `image`: None, or a uint8 / uint16 / float32 tensor of the mask's shape on the same device.  Objects whose area lies
    outside [min_area, max_area] (inclusive, max_area None: no upper bound) are dropped.  labels=True also makes
    ``table.labels``, an int32 tensor of the mask's shape holding each kept object's 1-based rank within its frame (scipy's
    numbering when nothing is dropped and the mask has one class); filtered_mask=True makes ``table.mask``, the mask with
    the dropped objects' pixels set to 0.  shape=True adds the shape columns of ObjectTable with one more call
    (sq_objects_shape) on the labelling the measure call left behind; no extent of a frame may then exceed 65536.
    Returns an ObjectTable."""
    _check_mask(mask)
    if image is not None:
        if not isinstance(image, torch.Tensor):
            raise TypeError("image must be a torch.Tensor in GPU memory")
        if not image.is_cuda or image.device != mask.device:
            raise _lib.SequitrHipError("image must live in GPU memory, on the mask's device (no CPU fallback exists)")
        if image.dtype not in PIX or tuple(image.shape) != tuple(mask.shape) or not image.is_contiguous():
            raise ValueError("image must be a contiguous uint8 / uint16 / float32 tensor of the mask's shape %s"
                             % (tuple(mask.shape),))
    min_area = int(min_area)
    max_area = 0 if max_area is None else int(max_area)
    if min_area < 1:
        raise ValueError("min_area must be at least 1, got %d" % min_area)
    if max_area and max_area < min_area:
        raise ValueError("max_area %d is below min_area %d" % (max_area, min_area))
    volumetric = mask.dim() == 4
    N = int(mask.shape[0])
    planes = int(mask.shape[1]) if volumetric else 1
    H, W = int(mask.shape[-2]), int(mask.shape[-1])
    lib = _lib.load()
    dev = mask.device
    st = torch.cuda.current_stream(dev).cuda_stream
    counters = torch.zeros(2, dtype=torch.int32, device=dev)    # count, found
    max_out = int(_MAX_OUT)
    while True:
        nbytes = lib.sq_objects_workspace(N, planes, H, W, max_out)
        if nbytes < 0:
            raise ValueError("mask %s is too large for one call" % (tuple(mask.shape),))
        ws = torch.empty((nbytes + 15) // 16 * 4, dtype=torch.int32, device=dev)
        rows_i = torch.empty((max_out, 12), dtype=torch.int64, device=dev)
        rows_f = torch.empty((max_out, 7), dtype=torch.float64, device=dev)
        slots = torch.empty((max_out,), dtype=torch.int32, device=dev)
        _lib.check(lib.sq_objects_measure(mask.data_ptr(), N, planes, H, W, image.data_ptr() if image is not None else None,
                                          PIX[image.dtype] if image is not None else 0, min_area, max_area, ws.data_ptr(),
                                          counters.data_ptr(), counters[1:].data_ptr(), rows_i.data_ptr(), rows_f.data_ptr(),
                                          slots.data_ptr(), max_out, st), "sq_objects_measure")
        n, found = (int(v) for v in counters.cpu().numpy())
        if found <= max_out:
            break
        max_out = found                                         # more components than room: once more
    np_dtype = None if image is None else {torch.uint8: np.uint8, torch.uint16: np.uint16, torch.float32: np.float32}[image.dtype]
    shape_i = None
    if shape:
        shape_i = torch.empty((max(n, 1), 16), dtype=torch.int64, device=dev)
        sbytes = lib.sq_objects_shape_workspace(max_out)
        sws = torch.empty((sbytes + 15) // 16 * 4, dtype=torch.int32, device=dev)
        _lib.check(lib.sq_objects_shape(mask.data_ptr(), N, planes, H, W, ws.data_ptr(), max_out, slots.data_ptr(), n,
                                        sws.data_ptr(), shape_i.data_ptr(), st), "sq_objects_shape")
        shape_i = shape_i[:n].cpu().numpy()
    table = ObjectTable(rows_i[:n].cpu().numpy(), rows_f[:n].cpu().numpy(), N, volumetric, np_dtype, shape_i=shape_i)
    table.found = found
    if labels or filtered_mask:
        rank = np.zeros(max_out, np.int32)
        rank[slots[:n].cpu().numpy()[table.order]] = table.label
        rank_d = torch.from_numpy(rank).to(dev)
        if labels:
            table.labels = torch.empty(tuple(mask.shape), dtype=torch.int32, device=dev)
        if filtered_mask:
            table.mask = torch.empty_like(mask)
        _lib.check(lib.sq_objects_relabel(mask.data_ptr(), N, planes, H, W, ws.data_ptr(), rank_d.data_ptr(), max_out,
                                          table.labels.data_ptr() if labels else None,
                                          table.mask.data_ptr() if filtered_mask else None, st), "sq_objects_relabel")
    return table
