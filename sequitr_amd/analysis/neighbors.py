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


def check_params(d_thresh=100., max_distance=None, seeds='objects'):
    """(d_thresh, max_distance, seeds) as float, int-or-None and str; ValueError for anything else"""
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


def _check_image(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor in GPU memory" % name)
    if not t.is_cuda:
        raise _lib.SequitrHipError("%s must live in GPU memory (no CPU fallback exists)" % name)
    if t.dtype != torch.int32 or t.dim() != 3 or not t.is_contiguous():
        raise ValueError("%s must be a contiguous (N,H,W) int32 tensor" % name)


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
    N, H, W = (int(s) for s in zones.shape)
    max_label = int(max_label)
    if not 1 <= max_label <= MAX_LABEL:
        raise ValueError("max_label must lie in 1 .. %d, got %d" % (MAX_LABEL, max_label))
    lib = _lib.load()
    dev = zones.device
    st = torch.cuda.current_stream(dev).cuda_stream
    max_pairs = _MIN_PAIRS if max_pairs is None else int(max_pairs)
    stats = torch.empty((N, max_label + 1, 2), dtype=torch.int64, device=dev)
    counters = torch.empty(2, dtype=torch.int32, device=dev)    # count, dropped
    while True:
        nbytes = lib.sq_zone_graph_workspace(max_pairs)
        if nbytes < 0:
            raise ValueError("max_pairs %d is outside 1 .. 2^28" % max_pairs)
        ws = _workspace(nbytes, dev)
        pairs = torch.empty((max_pairs, 4), dtype=torch.int32, device=dev)
        _lib.check(lib.sq_zone_graph(zones.data_ptr(), N, H, W, max_label, stats.data_ptr(), pairs.data_ptr(), max_pairs,
                                     counters.data_ptr(), counters[1:].data_ptr(), ws.data_ptr(), st), "sq_zone_graph")
        n, dropped = (int(v) for v in counters.cpu().numpy())
        if not dropped:
            break
        max_pairs *= 2                                          # rows are missing: once more with twice the room
    rows = pairs[:n].cpu().numpy().astype(np.int64)
    rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
    return stats.cpu().numpy(), rows


class NeighborTable(object):
    """Per-object columns (numpy, host), one row per object in the ObjectTable's order (frame, then label).

    frame, label, cls: int64 (k,);  n_total: neighbours kept;  n_class (k, num_classes) int64: neighbours per class -- with
    GFP as class 1 and RFP as class 2, columns 1 and 2 are the reference's n_winner and n_loser;  n_removed: zone contacts
    removed because the centroids lie further apart than d_thresh;  zone_area, zone_edge: pixels of the zone and those of
    them on the frame's outer border;  local_density = 1 / zone_area in float64 (inf for area 0).
    The adjacency in CSR form: the neighbours of row i are indices[indptr[i]:indptr[i+1]] (rows of this table, ascending),
    with border (contact length in pixel pairs) and distance (of the two centroids, float64) alongside.
    ``zones`` holds the device tensor of the zones when it was asked for."""

    def __init__(self, frame, label, cls, centroid, num_classes, stats, pairs, n_frames, d_thresh=100., max_distance=None,
                 seeds='objects'):
        self.frame, self.label, self.cls = (np.ascontiguousarray(v, np.int64) for v in (frame, label, cls))
        k = len(self.frame)
        self.n_frames, self.num_classes = int(n_frames), int(num_classes)
        self.d_thresh, self.max_distance, self.seeds = float(d_thresh), max_distance, seeds
        bounds = np.searchsorted(self.frame, np.arange(self.n_frames + 1))
        pairs = np.asarray(pairs, np.int64).reshape(-1, 4)
        pairs = pairs[np.lexsort((pairs[:, 2], pairs[:, 1], pairs[:, 0]))]
        i, j = bounds[pairs[:, 0]] + pairs[:, 1] - 1, bounds[pairs[:, 0]] + pairs[:, 2] - 1
        yx = _rows_cols(centroid, k)
        dy, dx = yx[i, 0] - yx[j, 0], yx[i, 1] - yx[j, 1]
        distance = np.sqrt(dx ** 2 + dy ** 2)
        removed = distance > self.d_thresh
        self.n_pairs, self.n_pairs_removed = int((~removed).sum()), int(removed.sum())
        self.n_removed = np.bincount(np.concatenate([i[removed], j[removed]]), minlength=k).astype(np.int64)
        i, j, b, d = i[~removed], j[~removed], pairs[~removed, 3], distance[~removed]
        src, dst = np.concatenate([i, j]), np.concatenate([j, i])
        order = np.lexsort((dst, src))
        self.indices = dst[order]
        self.border = np.concatenate([b, b])[order]
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
            return 1.0 / self.zone_area.astype(np.float64)

    def columns(self):
        """the columns as a dict of arrays, for np.savez"""
        return {name: getattr(self, name) for name in _COLUMNS}

    @classmethod
    def concatenate(cls, tables, first_frames, frames):
        """one table of `frames` frames out of per-batch tables whose frame 0 is frame first_frames[i] of the stack, given in
        the stack's order; `indices` are offset by the rows in front, so they stay rows of the table returned"""
        out = object.__new__(cls)
        out.n_frames, out.zones = int(frames), None
        first = tables[0] if tables else None
        out.num_classes = first.num_classes if first else 0
        out.d_thresh, out.max_distance, out.seeds = (first.d_thresh, first.max_distance, first.seeds) if first else (100., None, 'objects')
        out.n_pairs = sum(t.n_pairs for t in tables)
        out.n_pairs_removed = sum(t.n_pairs_removed for t in tables)
        rows = np.cumsum([0] + [len(t) for t in tables])
        nnz = np.cumsum([0] + [len(t.indices) for t in tables])

        def cat(parts, dtype, shape=(0,)):
            parts = list(parts)
            return np.concatenate(parts) if parts else np.zeros(shape, dtype)

        out.frame = cat((t.frame + int(f) for t, f in zip(tables, first_frames)), np.int64)
        for name in ('label', 'cls', 'n_total', 'n_removed', 'zone_area', 'zone_edge', 'border'):
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


def neighbors_from_objects(table, num_classes, d_thresh=100., max_distance=None, seeds='objects', return_zones=False):
    """neighbors() of an ObjectTable that measure_objects made with labels=True"""
    if getattr(table, 'labels', None) is None:
        raise ValueError("the ObjectTable holds no label image: measure_objects(..., labels=True) makes one")
    if table.volumetric:
        raise ValueError("neighbours are planar: volumes are out of scope")
    return neighbors(table.labels, table.cls, table.centroid, table.frame, num_classes, d_thresh, max_distance, seeds,
                     return_zones)
