"""Label image -> which cells are next to which, on the GPU: the relation sequitr/analysis/neighbors.py computes per cell
and frame (the number of neighbouring winner and loser cells within ``d_thresh``, and a local density).

THIS IS NOT scipy's Delaunay of the centroids, which is what the reference builds.  Two cells are neighbours here when
their ZONES OF INFLUENCE touch: the zone of an object is the set of the frame's pixels that lie nearer to it than to any
other object (exact Euclidean distance, the smaller label at a tie; include/sequitr_hip.h, "Label zones and the zone contact
graph").  With ``seeds='objects'`` every pixel of an object is a seed, which is what microscopy users mean by touching
neighbours (skimage's expand_labels, CellProfiler's MeasureObjectNeighbors).  With ``seeds='centroids'`` every object is
reduced to one seed pixel first, the discrete form of the reference's Voronoi diagram of the points; its zone pairs
approximate the Delaunay edges (DESIGN.md records the agreement: the edges missed lie mostly on the hull, where the Voronoi
edge falls outside the frame).  As in the reference (neighbors.py:144-154) a pair is removed iff the distance of the two
centroids exceeds ``d_thresh``.  The reference's density is the sum of 1 / area over the incident Delaunay triangles; ours
is 1 / zone area, with ``zone_edge > 0`` marking the cells whose zone the frame cuts.

``label_zones`` and ``zone_graph`` are the two device calls (sq_label_zones_i32, sq_zone_graph); the few thousand pairs
per frame are sorted, thresholded and counted on the host in numpy, like ObjectTable's sort.  There is no CPU path: the
label image must live in GPU memory.

Volumes.  ``label_zones3d``, ``zone_graph3d`` and ``neighbors3d`` are the same relation in an (N, D, H, W) z-stack
(sq_label_zones3d_i32, sq_zone_graph3d; the header's "Label zones and the contact graph in volumes"): zones are 3-D, with
``spacing`` = dz, the depth spacing in in-plane pixels, so cells stacked along z are neighbours -- which no slice-by-slice
run shows.  A contact is counted apart as ``border_lateral`` (faces along rows / columns, area dz each) and
``border_axial`` (faces along depth, area 1), ``contact_area`` is their area in in-plane pixels squared, the centroid
distance is sqrt((dz dplane)^2 + drow^2 + dcol^2) and ``d_thresh`` is in in-plane pixels.  ``neighbors_from_objects``
takes planar and volumetric ObjectTables alike.
"""
import numpy as np
import torch

from .. import _lib

SEEDS = ('objects', 'centroids')
MAX_LABEL = (1 << 21) - 1
MAX_REACH = 46340
_MIN_PAIRS = 1024

_COLUMNS = ('frame', 'label', 'cls', 'n_total', 'n_class', 'n_removed', 'zone_area', 'zone_edge', 'local_density',
            'indptr', 'indices', 'border', 'distance')
_COLUMNS3D = _COLUMNS + ('border_lateral', 'border_axial', 'contact_area')   # a volumetric table's further columns


def check_spacing(spacing):
    """the depth spacing dz as a float: finite and > 0; ValueError for anything else"""
    try:
        if isinstance(spacing, bool):
            raise TypeError
        dz = float(spacing)
    except (TypeError, ValueError):
        raise ValueError("spacing must be a finite number > 0, got %r" % (spacing,))
    if not (dz > 0.0 and np.isfinite(dz)):                      # NaN fails too
        raise ValueError("spacing must be a finite number > 0, got %r" % (spacing,))
    return dz


def check_params(d_thresh=100., max_distance=None, seeds='objects', spacing=None):
    """(d_thresh, max_distance, seeds) as float, int-or-None and str; ValueError for anything else.  With `spacing` (the
    volumetric calls' dz) a fourth value, check_spacing's float, follows."""
    if spacing is not None:
        return check_params(d_thresh, max_distance, seeds) + (check_spacing(spacing),)
    try:
        d = float(d_thresh)
    except (TypeError, ValueError):
        raise ValueError("d_thresh must be a number >= 0, got %r" % (d_thresh,))
    if not d >= 0.0:                                            # NaN fails too
        raise ValueError("d_thresh must be a number >= 0, got %r" % (d_thresh,))
    if max_distance is not None:
        if isinstance(max_distance, bool) or not isinstance(max_distance, (int, np.integer)) \
                or not 1 <= int(max_distance) <= MAX_REACH:
            raise ValueError("max_distance must be None or an integer in 1 .. %d, got %r" % (MAX_REACH, max_distance))
        max_distance = int(max_distance)
    if seeds not in SEEDS:
        raise ValueError("seeds must be one of %r, got %r" % (SEEDS, seeds))
    return d, max_distance, seeds


def _rows_cols(centroid, k):
    """the (k,2) [row, column] part of (k,2) or (k,3) centres"""
    return np.asarray(centroid, np.float64).reshape(k, -1)[:, -2:] if k else np.zeros((0, 2))


def _check_image(t, name, dims=3):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor in GPU memory" % name)
    if not t.is_cuda:
        raise _lib.SequitrHipError("%s must live in GPU memory (no CPU fallback exists)" % name)
    if t.dtype != torch.int32 or t.dim() != dims or not t.is_contiguous():
        raise ValueError("%s must be a contiguous %s int32 tensor" % (name, '(N,H,W)' if dims == 3 else '(N,D,H,W)'))


def _workspace(nbytes, dev):
    return torch.empty((nbytes + 15) // 16 * 4, dtype=torch.int32, device=dev)


def label_zones(labels, max_distance=None, return_distance=False, max_label=MAX_LABEL, out=None, distance_out=None,
                workspace=None):
    """The zone of influence of every labelled object: labels (N,H,W) int32 on the GPU, a pixel with 1 <= L <= max_label
    is a seed of object L, everything else is background.  Returns zones (N,H,W) int32 -- per pixel the label of the
    nearest seed of its frame, the smallest label at a tie, 0 beyond ``max_distance`` pixels (None: unbounded) and in a
    frame without a seed -- and, with return_distance, also the exact squared distance (0x7fffffff in a frame without a
    seed).  out / distance_out / workspace: optional preallocated tensors (a captured graph needs them)."""
    _check_image(labels, 'labels')
    _, max_distance, _ = check_params(max_distance=max_distance)
    N, H, W = (int(s) for s in labels.shape)
    lib = _lib.load()
    nbytes = lib.sq_label_zones_workspace(N, H, W)
    if nbytes < 0:
        raise ValueError("labels %s: need 0 < H, W < 30000 and fewer than 2^31 elements" % (tuple(labels.shape),))
    dev = labels.device
    if workspace is None:
        workspace = _workspace(nbytes, dev)
    elif workspace.numel() * workspace.element_size() < nbytes:
        raise ValueError("workspace holds %d bytes, %d are needed" % (workspace.numel() * workspace.element_size(), nbytes))
    zones = torch.empty_like(labels) if out is None else out
    d2 = None
    if return_distance or distance_out is not None:
        d2 = torch.empty_like(labels) if distance_out is None else distance_out
    for t, name in ((zones, 'out'), (d2, 'distance_out')):
        if t is not None and (t.dtype != torch.int32 or tuple(t.shape) != (N, H, W) or not t.is_contiguous() or t.device != dev):
            raise ValueError("%s must be a contiguous int32 tensor of the labels' shape on their device" % name)
    st = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(lib.sq_label_zones_i32(labels.data_ptr(), zones.data_ptr(), d2.data_ptr() if d2 is not None else None,
                                      N, H, W, int(max_label), max_distance or 0, workspace.data_ptr(), st),
               "sq_label_zones_i32")
    return (zones, d2) if return_distance else zones


def zone_graph(zones, max_label, max_pairs=None):
    """Areas and contacts of a zone image (N,H,W) int32 on the GPU.  Returns (stats, pairs): stats (N, max_label+1, 2)
    int64 numpy [area, edge] per label, pairs (k,4) int64 numpy [frame, a, b, border] sorted by (frame, a, b).  Starts with
    room for max_pairs rows (default 1024) and doubles it until nothing is dropped."""
    _check_image(zones, 'zones')
    return _zone_graph(zones, max_label, max_pairs, "sq_zone_graph", 4)


def _zone_graph(zones, max_label, max_pairs, entry, width):
    """zone_graph / zone_graph3d: `entry` and its workspace call over the zones' dimensions, rows of `width` int32"""
    dims = [int(s) for s in zones.shape]
    max_label = int(max_label)
    if not 1 <= max_label <= MAX_LABEL:
        raise ValueError("max_label must lie in 1 .. %d, got %d" % (MAX_LABEL, max_label))
    lib = _lib.load()
    dev = zones.device
    st = torch.cuda.current_stream(dev).cuda_stream
    max_pairs = _MIN_PAIRS if max_pairs is None else int(max_pairs)
    stats = torch.empty((dims[0], max_label + 1, 2), dtype=torch.int64, device=dev)
    counters = torch.empty(2, dtype=torch.int32, device=dev)    # count, dropped
    while True:
        nbytes = getattr(lib, entry + "_workspace")(max_pairs)
        if nbytes < 0:
            raise ValueError("max_pairs %d is outside 1 .. 2^28" % max_pairs)
        ws = _workspace(nbytes, dev)
        pairs = torch.empty((max_pairs, width), dtype=torch.int32, device=dev)
        _lib.check(getattr(lib, entry)(zones.data_ptr(), *dims, max_label, stats.data_ptr(), pairs.data_ptr(), max_pairs,
                                       counters.data_ptr(), counters[1:].data_ptr(), ws.data_ptr(), st), entry)
        n, dropped = (int(v) for v in counters.cpu().numpy())
        if not dropped:
            break
        max_pairs *= 2                                          # rows are missing: once more with twice the room
    rows = pairs[:n].cpu().numpy().astype(np.int64)
    rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
    return stats.cpu().numpy(), rows


def label_zones3d(labels, max_distance=None, spacing=1.0, return_distance=False, max_label=MAX_LABEL, out=None,
                  distance_out=None, workspace=None):
    """label_zones in a volume: labels (N,D,H,W) int32 on the GPU, `spacing` = dz, the depth spacing in in-plane pixels.
    Returns zones (N,D,H,W) int32 -- per voxel the label of the nearest seed of its volume in 3-D, the smallest label at a
    tie (the header pins the tie rule where dz makes the sums round), 0 beyond ``max_distance`` in-plane pixels and in a
    volume without a seed -- and, with return_distance, also the squared distance as float64 (+inf in a volume without a
    seed; elsewhere ops.edt3d_squared of the seed indicator, bit for bit).  out / distance_out (float64) / workspace:
    optional preallocated tensors (a captured graph needs them)."""
    _check_image(labels, 'labels', 4)
    (_, max_distance, _), dz = check_params(max_distance=max_distance), check_spacing(spacing)
    N, D, H, W = (int(s) for s in labels.shape)
    lib = _lib.load()
    nbytes = lib.sq_label_zones3d_workspace(N, D, H, W)
    if nbytes < 0:
        raise ValueError("labels %s: need 0 < D, H, W < 30000 and fewer than 2^31 elements" % (tuple(labels.shape),))
    dev = labels.device
    if workspace is None:
        workspace = _workspace(nbytes, dev)
    elif workspace.numel() * workspace.element_size() < nbytes:
        raise ValueError("workspace holds %d bytes, %d are needed" % (workspace.numel() * workspace.element_size(), nbytes))
    zones = torch.empty_like(labels) if out is None else out
    d2 = None
    if return_distance or distance_out is not None:
        d2 = torch.empty(labels.shape, dtype=torch.float64, device=dev) if distance_out is None else distance_out
    for t, name, dtype in ((zones, 'out', torch.int32), (d2, 'distance_out', torch.float64)):
        if t is not None and (t.dtype != dtype or tuple(t.shape) != (N, D, H, W) or not t.is_contiguous() or t.device != dev):
            raise ValueError("%s must be a contiguous %s tensor of the labels' shape on their device"
                             % (name, str(dtype).split('.')[-1]))
    st = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(lib.sq_label_zones3d_i32(labels.data_ptr(), zones.data_ptr(), d2.data_ptr() if d2 is not None else None,
                                        N, D, H, W, int(max_label), max_distance or 0, dz, workspace.data_ptr(), st),
               "sq_label_zones3d_i32")
    return (zones, d2) if return_distance else zones


def zone_graph3d(zones, max_label, max_pairs=None):
    """Voxel counts and contacts of a zone volume (N,D,H,W) int32 on the GPU.  Returns (stats, pairs): stats
    (N, max_label+1, 2) int64 numpy [voxels, face] per label, pairs (k,5) int64 numpy [volume, a, b, lateral, axial] sorted by
    (volume, a, b).  Starts with room for max_pairs rows (default 1024) and doubles it until nothing is dropped."""
    _check_image(zones, 'zones', 4)
    return _zone_graph(zones, max_label, max_pairs, "sq_zone_graph3d", 5)


class NeighborTable(object):
    """Per-object columns (numpy, host), one row per object in the ObjectTable's order (frame, then label).

    frame, label, cls: int64 (k,);  n_total: neighbours kept;  n_class (k, num_classes) int64: neighbours per class -- with
    GFP as class 1 and RFP as class 2, columns 1 and 2 are the reference's n_winner and n_loser;  n_removed: zone contacts
    removed because the centroids lie further apart than d_thresh;  zone_area, zone_edge: pixels of the zone and those of
    them on the frame's outer border;  local_density = 1 / zone_area in float64 (inf for area 0).
    The adjacency in CSR form: the neighbours of row i are indices[indptr[i]:indptr[i+1]] (rows of this table, ascending),
    with border (contact length in pixel pairs) and distance (of the two centroids, float64) alongside.
    ``zones`` holds the device tensor of the zones when it was asked for.

    A VOLUMETRIC table (``volumetric`` True, made by neighbors3d; ``frame`` is the volume index, ``spacing`` the depth
    spacing dz) is built from zone_graph3d's (k,5) pairs and (k,3) centres: distance = sqrt((dz dplane)^2 + drow^2 + dcol^2);
    zone_area, zone_edge: voxels of the zone and those of them on the volume's faces;  local_density = 1 / (zone_area dz),
    one over the zone's volume in in-plane pixels cubed;  border = border_lateral + border_axial, the two further columns,
    and contact_area = border_lateral dz + border_axial in float64.  A planar table has none of the three."""

    def __init__(self, frame, label, cls, centroid, num_classes, stats, pairs, n_frames, d_thresh=100., max_distance=None,
                 seeds='objects', volumetric=False, spacing=1.0):
        self.frame, self.label, self.cls = (np.ascontiguousarray(v, np.int64) for v in (frame, label, cls))
        k = len(self.frame)
        self.n_frames, self.num_classes = int(n_frames), int(num_classes)
        self.d_thresh, self.max_distance, self.seeds = float(d_thresh), max_distance, seeds
        self.volumetric, self.spacing = bool(volumetric), float(spacing)
        bounds = np.searchsorted(self.frame, np.arange(self.n_frames + 1))
        pairs = np.asarray(pairs, np.int64).reshape(-1, 5 if self.volumetric else 4)
        pairs = pairs[np.lexsort((pairs[:, 2], pairs[:, 1], pairs[:, 0]))]
        i, j = bounds[pairs[:, 0]] + pairs[:, 1] - 1, bounds[pairs[:, 0]] + pairs[:, 2] - 1
        if self.volumetric:
            zyx = np.asarray(centroid, np.float64).reshape(k, 3) if k else np.zeros((0, 3))
            dp, dr, dc = (zyx[i, a] - zyx[j, a] for a in range(3))
            distance = np.sqrt((self.spacing * dp) ** 2 + dr ** 2 + dc ** 2)
        else:
            yx = _rows_cols(centroid, k)
            dy, dx = yx[i, 0] - yx[j, 0], yx[i, 1] - yx[j, 1]
            distance = np.sqrt(dx ** 2 + dy ** 2)
        removed = distance > self.d_thresh
        self.n_pairs, self.n_pairs_removed = int((~removed).sum()), int(removed.sum())
        self.n_removed = np.bincount(np.concatenate([i[removed], j[removed]]), minlength=k).astype(np.int64)
        i, j, b, d = i[~removed], j[~removed], pairs[~removed, 3:], distance[~removed]
        src, dst = np.concatenate([i, j]), np.concatenate([j, i])
        order = np.lexsort((dst, src))
        self.indices = dst[order]
        b = np.concatenate([b, b])[order]
        self.border = np.ascontiguousarray(b.sum(1))
        if self.volumetric:
            self.border_lateral, self.border_axial = np.ascontiguousarray(b[:, 0]), np.ascontiguousarray(b[:, 1])
        self.distance = np.concatenate([d, d])[order]
        self.n_total = np.bincount(src, minlength=k).astype(np.int64)
        self.indptr = np.concatenate([[0], np.cumsum(self.n_total)]).astype(np.int64)
        self.n_class = np.zeros((k, self.num_classes), np.int64)
        np.add.at(self.n_class, (src, self.cls[dst]), 1)
        stats = np.asarray(stats, np.int64)
        self.zone_area = stats[self.frame, self.label, 0] if k else np.zeros(0, np.int64)
        self.zone_edge = stats[self.frame, self.label, 1] if k else np.zeros(0, np.int64)
        self.zones = None

    def __len__(self):
        return len(self.frame)

    @property
    def local_density(self):
        with np.errstate(divide='ignore'):
            if self.volumetric:
                return 1.0 / (self.zone_area.astype(np.float64) * self.spacing)
            return 1.0 / self.zone_area.astype(np.float64)

    @property
    def contact_area(self):
        """a volumetric table's contact areas in in-plane pixels squared: border_lateral dz + border_axial, float64"""
        return self.border_lateral.astype(np.float64) * self.spacing + self.border_axial.astype(np.float64)

    def columns(self):
        """the columns as a dict of arrays, for np.savez"""
        return {name: getattr(self, name) for name in (_COLUMNS3D if self.volumetric else _COLUMNS)}

    @classmethod
    def concatenate(cls, tables, first_frames, frames):
        """one table of `frames` frames out of per-batch tables whose frame 0 is frame first_frames[i] of the stack, given in
        the stack's order; `indices` are offset by the rows in front, so they stay rows of the table returned"""
        out = object.__new__(cls)
        out.n_frames, out.zones = int(frames), None
        first = tables[0] if tables else None
        out.num_classes = first.num_classes if first else 0
        out.d_thresh, out.max_distance, out.seeds = (first.d_thresh, first.max_distance, first.seeds) if first else (100., None, 'objects')
        out.volumetric, out.spacing = (first.volumetric, first.spacing) if first else (False, 1.0)
        if any((t.volumetric, t.spacing) != (out.volumetric, out.spacing) for t in tables):
            raise ValueError("the tables must be all planar or all volumetric with one spacing")
        out.n_pairs = sum(t.n_pairs for t in tables)
        out.n_pairs_removed = sum(t.n_pairs_removed for t in tables)
        rows = np.cumsum([0] + [len(t) for t in tables])
        nnz = np.cumsum([0] + [len(t.indices) for t in tables])

        def cat(parts, dtype, shape=(0,)):
            parts = list(parts)
            return np.concatenate(parts) if parts else np.zeros(shape, dtype)

        out.frame = cat((t.frame + int(f) for t, f in zip(tables, first_frames)), np.int64)
        for name in ('label', 'cls', 'n_total', 'n_removed', 'zone_area', 'zone_edge', 'border') \
                + (('border_lateral', 'border_axial') if out.volumetric else ()):
            setattr(out, name, cat((getattr(t, name) for t in tables), np.int64))
        out.n_class = cat((t.n_class for t in tables), np.int64, (0, out.num_classes))
        out.distance = cat((t.distance for t in tables), np.float64)
        out.indices = cat((t.indices + rows[k] for k, t in enumerate(tables)), np.int64)
        out.indptr = np.concatenate([[0]] + [t.indptr[1:] + nnz[k] for k, t in enumerate(tables)]).astype(np.int64)
        return out


def _centroid_seeds(frame, label, centroid, shape, dev):
    """one seed pixel per object, floor(centre + 0.5) clipped into the frame; the smallest label takes a shared pixel"""
    N, H, W = shape
    yx = _rows_cols(centroid, len(frame))
    sy =np.clip(np.floor(yx[:, 0] + 0.5), 0, H - 1).astype(np.int64)
    sx = np.clip(np.floor(yx[:, 1] + 0.5), 0, W - 1).astype(np.int64)
    flat = torch.full((N * H * W,), 0x7fffffff, dtype=torch.int32, device=dev)   # larger than any label: background
    if len(frame):
        idx = torch.from_numpy((frame * H + sy) * W + sx).to(dev)
        flat.scatter_reduce_(0, idx, torch.from_numpy(label.astype(np.int32)).to(dev), 'amin')
    return flat.view(N, H, W)


def neighbors(labels, cls, centroid, frame, num_classes, d_thresh=100., max_distance=None, seeds='objects',
              return_zones=False):
    """Neighbours of every object of a label image.  labels (N,H,W) int32 on the GPU, each object's pixels holding its
    1-based rank within its frame; cls, centroid, frame: one entry per object in the ObjectTable's order (sorted by frame,
    then by label: object i of frame f has label i + 1) -- centroid (k,2) [row, column] or ObjectTable's (k,3).
    Two objects are neighbours iff their zones touch (see the module's text: not the reference's Delaunay) and their
    centroids lie no further apart than d_thresh.  max_distance bounds the zones (label_zones);  seeds = 'objects' (every
    pixel of an object is a seed) or 'centroids' (one seed pixel per object).  Returns a NeighborTable."""
    _check_image(labels, 'labels')
    d_thresh, max_distance, seeds = check_params(d_thresh, max_distance, seeds)
    N, H, W = (int(s) for s in labels.shape)
    frame = np.ascontiguousarray(frame, np.int64).reshape(-1)
    cls = np.ascontiguousarray(cls, np.int64).reshape(-1)
    k = len(frame)
    num_classes = int(num_classes)
    centroid = np.asarray(centroid, np.float64).reshape(k, -1) if k else np.zeros((0, 2))
    if len(cls) != k or centroid.shape[1] not in (2, 3):
        raise ValueError("cls, centroid (k,2) or (k,3) and frame must hold one entry per object")
    if k and (np.any(np.diff(frame) < 0) or frame[0] < 0 or frame[-1] >= N):
        raise ValueError("frame must be sorted and lie in 0 .. %d" % (N - 1))
    if k and (cls.min() < 0 or cls.max() >= num_classes):
        raise ValueError("cls must lie in 0 .. num_classes - 1 = %d" % (num_classes - 1))
    bounds = np.searchsorted(frame, np.arange(N + 1))
    label = np.arange(1, k + 1, dtype=np.int64) - bounds[frame] if k else np.zeros(0, np.int64)
    max_label = max(1, int(np.diff(bounds).max()))
    if max_label > MAX_LABEL:
        raise ValueError("%d objects in one frame, at most %d are supported" % (max_label, MAX_LABEL))
    source = labels if seeds == 'objects' else _centroid_seeds(frame, label, centroid, (N, H, W), labels.device)
    zones = label_zones(source, max_distance, max_label=max_label)
    stats, pairs = zone_graph(zones, max_label, max(_MIN_PAIRS, 8 * k))
    table = NeighborTable(frame, label, cls, centroid, num_classes, stats, pairs, N, d_thresh, max_distance, seeds)
    if return_zones:
        table.zones = zones
    return table


def _centroid_seeds3d(volume, label, centroid, shape, dev):
    """one seed voxel per object, floor(centre + 0.5) clipped into the volume; the smallest label takes a shared voxel"""
    N, D, H, W = shape
    s = [np.clip(np.floor(centroid[:, a] + 0.5), 0, L - 1).astype(np.int64) for a, L in enumerate((D, H, W))]
    flat = torch.full((N * D * H * W,), 0x7fffffff, dtype=torch.int32, device=dev)   # larger than any label: background
    if len(volume):
        idx = torch.from_numpy(((volume * D + s[0]) * H + s[1]) * W + s[2]).to(dev)
        flat.scatter_reduce_(0, idx, torch.from_numpy(label.astype(np.int32)).to(dev), 'amin')
    return flat.view(N, D, H, W)


def neighbors3d(labels, cls, centroid, volume, num_classes, d_thresh=100., max_distance=None, seeds='objects', spacing=1.0,
                return_zones=False):
    """neighbors() in volumes.  labels (N,D,H,W) int32 on the GPU, each object's voxels holding its 1-based rank within its
    volume; cls, centroid (k,3) [plane, row, column], volume: one entry per object in the ObjectTable's order (sorted by
    volume, then by label).  `spacing` = dz, the depth spacing in in-plane pixels; d_thresh and max_distance are in in-plane
    pixels.  Two objects are neighbours iff their 3-D zones touch and their centroids lie no further apart than d_thresh,
    the plane difference scaled by dz.  seeds = 'objects' (every voxel of an object is a seed) or 'centroids' (one seed
    voxel per object).  Returns a volumetric NeighborTable."""
    _check_image(labels, 'labels', 4)
    (d_thresh, max_distance, seeds), dz = check_params(d_thresh, max_distance, seeds), check_spacing(spacing)
    N, D, H, W = (int(s) for s in labels.shape)
    volume = np.ascontiguousarray(volume, np.int64).reshape(-1)
    cls = np.ascontiguousarray(cls, np.int64).reshape(-1)
    k = len(volume)
    num_classes = int(num_classes)
    centroid = np.asarray(centroid, np.float64).reshape(k, -1) if k else np.zeros((0, 3))
    if len(cls) != k or centroid.shape[1] != 3:
        raise ValueError("cls, centroid (k,3) and volume must hold one entry per object")
    if k and (np.any(np.diff(volume) < 0) or volume[0] < 0 or volume[-1] >= N):
        raise ValueError("volume must be sorted and lie in 0 .. %d" % (N - 1))
    if k and (cls.min() < 0 or cls.max() >= num_classes):
        raise ValueError("cls must lie in 0 .. num_classes - 1 = %d" % (num_classes - 1))
    bounds = np.searchsorted(volume, np.arange(N + 1))
    label = np.arange(1, k + 1, dtype=np.int64) - bounds[volume] if k else np.zeros(0, np.int64)
    max_label = max(1, int(np.diff(bounds).max()))
    if max_label > MAX_LABEL:
        raise ValueError("%d objects in one volume, at most %d are supported" % (max_label, MAX_LABEL))
    source = labels if seeds == 'objects' else _centroid_seeds3d(volume, label, centroid, (N, D, H, W), labels.device)
    zones = label_zones3d(source, max_distance, dz, max_label=max_label)
    stats, pairs = zone_graph3d(zones, max_label, max(_MIN_PAIRS, 8 * k))
    table = NeighborTable(volume, label, cls, centroid, num_classes, stats, pairs, N, d_thresh, max_distance, seeds,
                          volumetric=True, spacing=dz)
    if return_zones:
        table.zones = zones
    return table


def neighbors_from_objects(table, num_classes, d_thresh=100., max_distance=None, seeds='objects', return_zones=False,
                           spacing=1.0):
    """neighbors() -- for a volumetric table neighbors3d() with the depth spacing `spacing` -- of an ObjectTable that
    measure_objects made with labels=True"""
    if getattr(table, 'labels', None) is None:
        raise ValueError("the ObjectTable holds no label image: measure_objects(..., labels=True) makes one")
    if table.volumetric:
        return neighbors3d(table.labels, table.cls, table.centroid, table.frame, num_classes, d_thresh, max_distance, seeds,
                           spacing, return_zones)
    return neighbors(table.labels, table.cls, table.centroid, table.frame, num_classes, d_thresh, max_distance, seeds,
                     return_zones)
