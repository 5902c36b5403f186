"""Objects linked from frame to frame: which object of frame t + 1 is the same cell as which object of frame t, and which
cells divided.  The reference hands this to an external tracker; its analysis modules only consume tracks
(sequitr/dataio/tracker.py's Track: ID, t, x, y, parent, children).  Here the per-pixel part -- the overlap of every object
of frame t with every object of frame t + 1 -- runs on the GPU over label frames that are already there
(sq_label_overlap, include/sequitr_hip.h "Label overlap and relabelling"), and the rule below runs on the host over the few
thousand rows a step has, in float64 numpy.  This text is the contract; tests/link_cases.py restates it as plain loops.

Input.  Label frames (F, H, W) int32 -- or volumes (F, D, H, W) -- in which each object's positions hold its 1-based rank
within its frame (ObjectTable.label, what measure_objects(..., labels=True) writes), and per object a class.

Footprint.  Frame t's side of the table is ``labels[t]`` itself with ``reach = 0``; with ``reach = R > 0`` it is
``label_zones(labels[t], max_distance=R)``: every object grown by up to R pixels, ties to the smaller label, so that a cell
may move up to R beyond its outline and still meet its successor.  Frame t + 1's side is always ``labels[t + 1]``.
``area_a[la]`` is the number of positions of la's footprint, ``area_b[lb]`` the number of positions of lb, ``overlap`` the
number of positions that lie in both; all three come from the kernel.

Rule for one step t -> t + 1 (link_pairs), all in float64:
  1. Candidates: the rows (la, lb, overlap) with overlap >= min_overlap and, with ``same_class``, cls(la) == cls(lb);
     iou = overlap / (area_a[la] + area_b[lb] - overlap); rows with iou >= min_iou stay.
  2. Continuations: the candidates sorted by (-iou, -overlap, la, lb); going down the list a row is taken if neither its
     la nor its lb is taken.  lb continues la's track.
  3. Divisions (only with ``divisions``): the untaken lb in ascending order.  lb's parent candidate is the la of largest
     overlap among lb's candidates, the smallest la at a tie, provided overlap / area_b[lb] >= min_child_fraction.  If
     that la was continued in step 2 by some lb' and has not divided in this step: la's track ends at t, lb' and lb start
     two new tracks with parent = la's track, and la's track gets children = [ID(lb'), ID(lb)].  Every la divides at most
     once per step (lineage trees are binary): a third claimant becomes a root.
  4. New roots: every other untaken lb starts a root track with parent = its own ID (the convention the reference's
     lineage.py accepts for a root).
  5. Ends: an la that was not continued ends at t.
Track IDs are 1, 2, ... in order of creation.  Frame 0's objects are roots in label order.  In a later frame the new
tracks are created while the untaken lb are gone through in ascending order: a root gets the next ID, a division gives the
next two IDs to the continued child lb' and then to the claimant lb.
Consequences: every object belongs to exactly one track; a track's frames are consecutive; ``children`` is empty or has
two entries; the result does not depend on how the movie was cut into batches (every count is an integer sum).

NOT BUILT: closing gaps (an object missing for a frame ends its track, its reappearance is a root); merges as events (of
two cells that merge the better iou continues, the other simply ends); motion models; ``reach`` for volumes in time;
tracker XML; plotting.

There is no CPU path for the overlap: the label frames must live in GPU memory.  link_pairs, TrackTable and the host state
of FrameLinker need no device.
"""
import numpy as np

from .. import _lib

MAX_LABEL = (1 << 21) - 1
_MIN_PAIRS = 1024
OPTIONS = ('reach', 'min_iou', 'min_overlap', 'divisions', 'min_child_fraction', 'same_class')
DEFAULTS = {'reach': 0, 'min_iou': 0.0, 'min_overlap': 1, 'divisions': True, 'min_child_fraction': 0.5, 'same_class': True}
_TRACK_COLUMNS = ('track', 'ID', 'start', 'end', 'length', 'parent', 'children', 'root', 'generation', 'cls', 'links',
                  'link_overlap', 'link_iou')
KIND_CONTINUATION, KIND_DIVISION = 0, 1
FATE_MITOSIS = 4                                                # index of 'mitosis' in the reference's FATE_LABELS


def check_options(reach=0, min_iou=0.0, min_overlap=1, divisions=True, min_child_fraction=0.5, same_class=True):
    """the linker's options with their types pinned, as a dict; ValueError for anything else"""
    from .neighbors import MAX_REACH

    def integer(v, name, lo, hi):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
            raise ValueError("%s must be an integer in %d .. %d, got %r" % (name, lo, hi, v))
        return int(v)

    def fraction(v, name):
        try:
            if isinstance(v, bool):
                raise TypeError
            f = float(v)
        except (TypeError, ValueError):
            raise ValueError("%s must be a number in 0 .. 1, got %r" % (name, v))
        if not 0.0 <= f <= 1.0:                                 # NaN fails too
            raise ValueError("%s must be a number in 0 .. 1, got %r" % (name, v))
        return f

    def flag(v, name):
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError("%s must be true or false, got %r" % (name, v))
        return bool(v)

    return {'reach': integer(reach, 'reach', 0, MAX_REACH), 'min_iou': fraction(min_iou, 'min_iou'),
            'min_overlap': integer(min_overlap, 'min_overlap', 1, 2 ** 31 - 1), 'divisions': flag(divisions, 'divisions'),
            'min_child_fraction': fraction(min_child_fraction, 'min_child_fraction'),
            'same_class': flag(same_class, 'same_class')}


# ---- the two device calls ---------------------------------------------------------------------------------------------
def _check_stack(t, name):
    import torch
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor in GPU memory" % name)
    if not t.is_cuda:
        raise _lib.SequitrHipError("%s must live in GPU memory (no CPU fallback exists)" % name)
    if t.dtype != torch.int32 or t.dim() < 2 or not t.is_contiguous():
        raise ValueError("%s must be a contiguous (N, ...) int32 tensor" % name)


def overlap_table(a, b, max_label=None, max_pairs=None, areas=True):
    """The contingency table of two label stacks a, b (N, ...) int32 on the GPU, of one shape (sq_label_overlap): returns
    (pairs, area_a, area_b) as numpy -- pairs (k,4) int64 [n, la, lb, overlap] sorted by (n, la, lb), one row per pair of
    labels > 0 that share a position; area_a, area_b (N, max_label + 1) int64, the positions per label (None without
    `areas`).  Values outside 1 .. max_label (default: the larger maximum of a and b, at least 1) count as 0.  Starts with
    room for max_pairs rows (default 1024) and doubles it until nothing is dropped.  ``labels[:-1]`` and ``labels[1:]`` of
    one stack are valid a and b."""
    import torch
    _check_stack(a, 'a')
    _check_stack(b, 'b')
    if tuple(a.shape) != tuple(b.shape) or a.device != b.device:
        raise ValueError("a %s and b %s must have one shape and one device" % (tuple(a.shape), tuple(b.shape)))
    N = int(a.shape[0])
    P = int(a.numel() // N) if N else 0
    if max_label is None:
        max_label = max(1, int(torch.maximum(a.max(), b.max()))) if N and P else 1
    max_label = int(max_label)
    if not 1 <= max_label <= MAX_LABEL:
        raise ValueError("max_label must lie in 1 .. %d, got %d" % (MAX_LABEL, max_label))
    lib = _lib.load()
    dev = a.device
    st = torch.cuda.current_stream(dev).cuda_stream
    max_pairs = _MIN_PAIRS if max_pairs is None else int(max_pairs)
    area = torch.empty((2, N, max_label + 1), dtype=torch.int64, device=dev) if areas else None
    counters = torch.empty(2, dtype=torch.int32, device=dev)    # count, dropped
    while True:
        nbytes = lib.sq_label_overlap_workspace(max_pairs)
        if nbytes < 0:
            raise ValueError("max_pairs %d is outside 1 .. 2^28" % max_pairs)
        ws = torch.empty((nbytes + 15) // 16 * 4, dtype=torch.int32, device=dev)
        pairs = torch.empty((max_pairs, 4), dtype=torch.int32, device=dev)
        _lib.check(lib.sq_label_overlap(a.data_ptr(), b.data_ptr(), N, P, max_label,
                                        area[0].data_ptr() if areas else None, area[1].data_ptr() if areas else None,
                                        pairs.data_ptr(), max_pairs, counters.data_ptr(), counters[1:].data_ptr(),
                                        ws.data_ptr(), st), "sq_label_overlap")
        n, dropped = (int(v) for v in counters.cpu().numpy())
        if not dropped:
            break
        max_pairs *= 2                                          # rows are missing: once more with twice the room
    rows = pairs[:n].cpu().numpy().astype(np.int64)
    rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
    if not areas:
        return rows, None, None
    area = area.cpu().numpy()
    return rows, area[0], area[1]


def relabel(labels, offsets, lut, out=None):
    """labels (N, ...) int32 on the GPU rewritten through a per-frame slice of one table (sq_relabel_lut_i32):
    out[n,p] = lut[offsets[n] + L - 1] for 1 <= L = labels[n,p] <= offsets[n+1] - offsets[n], 0 otherwise.  offsets (N + 1)
    and lut: numpy arrays or tensors (moved to the labels' device as int64 / int32).  ``out`` may be ``labels`` itself (in
    place) or a tensor of its shape; returns out.  With TrackTable.lut() every object's positions get its track ID."""
    import torch
    _check_stack(labels, 'labels')
    dev = labels.device
    N = int(labels.shape[0])
    P = int(labels.numel() // N) if N else 0
    off = torch.as_tensor(np.asarray(offsets, np.int64) if not isinstance(offsets, torch.Tensor) else offsets)
    off = off.to(device=dev, dtype=torch.int64).contiguous()
    tab = torch.as_tensor(np.asarray(lut, np.int32) if not isinstance(lut, torch.Tensor) else lut)
    tab = tab.to(device=dev, dtype=torch.int32).contiguous()
    if off.dim() != 1 or off.numel() != N + 1 or tab.dim() != 1:
        raise ValueError("offsets must hold N + 1 = %d entries and lut must be one-dimensional" % (N + 1))
    if out is None:
        out = torch.empty_like(labels)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.int32 or tuple(out.shape) != tuple(labels.shape)
          or not out.is_contiguous() or out.device != dev):
        raise ValueError("out must be a contiguous int32 tensor of the labels' shape on their device")
    lib = _lib.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(lib.sq_relabel_lut_i32(labels.data_ptr(), out.data_ptr(), N, P, off.data_ptr(),
                                      tab.data_ptr() if tab.numel() else None, int(tab.numel()), st), "sq_relabel_lut_i32")
    return out


# ---- the rule for one step --------------------------------------------------------------------------------------------
class StepLinks(object):
    """link_pairs' result for the n_b objects of frame t + 1, indexed by lb - 1: ``source`` (the la whose track lb continues
    or whose division made it; 0 for a root), ``kind`` (0 continuation, 1 division child, -1 root), ``overlap`` and ``iou``
    of that row (0 for a root); ``created``: the lb that start a new track, in the order their IDs are given out."""

    def __init__(self, n_b):
        self.source = np.zeros(n_b, np.int64)
        self.kind = np.full(n_b, -1, np.int64)
        self.overlap = np.zeros(n_b, np.int64)
        self.iou = np.zeros(n_b, np.float64)
        self.created = np.zeros(0, np.int64)


def link_pairs(pairs, area_a, area_b, cls_a, cls_b, min_iou=0.0, min_overlap=1, divisions=True, min_child_fraction=0.5,
               same_class=True):
    """The rule of the module's text for ONE step t -> t + 1, on the host, no device.  pairs (m,3) [la, lb, overlap] (or
    overlap_table's (m,4) rows of one n) sorted by (la, lb); area_a, area_b indexed by label (one row of overlap_table's
    areas); cls_a (n_a,), cls_b (n_b,) the classes of the objects 1 .. n_a of frame t and 1 .. n_b of frame t + 1.
    Returns a StepLinks."""
    pairs = np.asarray(pairs, np.int64)
    pairs = pairs.reshape(-1, pairs.shape[-1] if pairs.ndim == 2 and pairs.shape[-1] in (3, 4) else 3)[:, -3:]
    cls_a, cls_b = np.asarray(cls_a, np.int64).reshape(-1), np.asarray(cls_b, np.int64).reshape(-1)
    area_a, area_b = np.asarray(area_a, np.int64).reshape(-1), np.asarray(area_b, np.int64).reshape(-1)
    n_a, n_b = len(cls_a), len(cls_b)
    out = StepLinks(n_b)
    la, lb, ov = pairs[:, 0], pairs[:, 1], pairs[:, 2]
    keep = (la >= 1) & (la <= n_a) & (lb >= 1) & (lb <= n_b) & (ov >= int(min_overlap))
    la, lb, ov = la[keep], lb[keep], ov[keep]
    if same_class:
        keep = cls_a[la - 1] == cls_b[lb - 1]
        la, lb, ov = la[keep], lb[keep], ov[keep]
    iou = ov.astype(np.float64) / (area_a[la] + area_b[lb] - ov).astype(np.float64)
    keep = iou >= float(min_iou)
    la, lb, ov, iou = la[keep], lb[keep], ov[keep], iou[keep]
    # 2. continuations.  Going down the sorted list one row at a time is the definition; the rounds below give the same set:
    # a row that is the first of the rows still alive for both its la and its lb cannot be blocked by an earlier row, so it
    # is taken, and every row that shares an end with a taken one is dead.  The first row alive is always such a row.
    order = np.lexsort((lb, la, -ov, -iou))
    la, lb, ov, iou = la[order], lb[order], ov[order], iou[order]
    taken_a, taken_b = np.zeros(n_a + 1, np.int64), np.zeros(n_b + 1, bool)    # taken_a[la] = the lb that continues it
    alive = np.arange(len(la))
    while len(alive):
        a, b = la[alive], lb[alive]
        first = np.zeros((2, len(alive)), bool)
        first[0, np.unique(a, return_index=True)[1]] = True
        first[1, np.unique(b, return_index=True)[1]] = True
        take = alive[first[0] & first[1]]
        taken_a[la[take]], taken_b[lb[take]] = lb[take], True
        i = lb[take] - 1
        out.source[i], out.kind[i], out.overlap[i], out.iou[i] = la[take], KIND_CONTINUATION, ov[take], iou[take]
        alive = alive[(taken_a[a] == 0) & ~taken_b[b]]
    # 3. divisions and 4. roots, the untaken lb in ascending order
    created = []
    divided = np.zeros(n_a + 1, bool)
    by_b = np.lexsort((la, -ov, lb))                            # per lb: the largest overlap first, the smaller la at a tie
    first = np.searchsorted(lb[by_b], np.arange(1, n_b + 2))
    for b in (np.nonzero(~taken_b[1:])[0] + 1).tolist():
        if divisions and first[b - 1] < first[b]:
            i = by_b[first[b - 1]]
            a = int(la[i])
            if float(ov[i]) / float(area_b[b]) >= float(min_child_fraction) and taken_a[a] and not divided[a]:
                divided[a] = True
                other = int(taken_a[a])
                out.kind[other - 1] = KIND_DIVISION
                out.source[b - 1], out.kind[b - 1], out.overlap[b - 1], out.iou[b - 1] = a, KIND_DIVISION, ov[i], iou[i]
                created += [other, b]
                continue
        created.append(b)
    out.created = np.asarray(created, np.int64)
    return out


# ---- tracks -----------------------------------------------------------------------------------------------------------
class TrackTable(object):
    """What linking leaves, all host numpy.
    Per object, aligned with the rows of the movie's ObjectTable (frame, then label): ``track``, the object's track ID.
    Per track, row ID - 1: ``ID``, ``start`` and ``end`` (first and last frame), ``length`` = end - start + 1, ``parent``
    (the dividing track's ID; a root's own ID), ``children`` (k,2) with 0 for none, ``root`` (the ID of the tree's root),
    ``generation`` (0 for a root), ``cls`` (the class of the track's first object).
    Per link, sorted by (t, lb): ``links`` (m,4) [t, la, lb, kind] -- object lb of frame t + 1 follows object la of frame t,
    kind 0 = continuation, 1 = division (both children of a division have one) -- with ``link_overlap`` (int64) and
    ``link_iou`` (float64).  ``counts`` (F,) holds the objects per frame, ``options`` the linker's options."""

    def __init__(self, counts, track, start, end, parent, children, cls, links, link_overlap, link_iou, options=None):
        self.counts = np.asarray(counts, np.int64).reshape(-1)
        self.n_frames = len(self.counts)
        self.track = np.asarray(track, np.int64).reshape(-1)
        self.start, self.end, self.parent, self.cls = (np.asarray(v, np.int64).reshape(-1) for v in (start, end, parent, cls))
        k = len(self.start)
        self.ID = np.arange(1, k + 1, dtype=np.int64)
        self.length = self.end - self.start + 1
        self.children = np.asarray(children, np.int64).reshape(k, 2)
        self.root, self.generation = self.ID.copy(), np.zeros(k, np.int64)
        for i in range(k):                                      # a parent is created before its children: one pass
            p = int(self.parent[i])
            if p != i + 1:
                self.root[i], self.generation[i] = self.root[p - 1], self.generation[p - 1] + 1
        self.links = np.asarray(links, np.int64).reshape(-1, 4)
        self.link_overlap = np.asarray(link_overlap, np.int64).reshape(-1)
        self.link_iou = np.asarray(link_iou, np.float64).reshape(-1)
        self.options = dict(options or DEFAULTS)

    def __len__(self):
        return len(self.ID)

    def columns(self):
        """the columns as a dict of arrays, for np.savez"""
        return {name: getattr(self, name) for name in _TRACK_COLUMNS}

    def lut(self):
        """(offsets, lut) for relabel(): offsets (F + 1) int64, the first row of every frame; lut int32, the track ID per row"""
        return np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64), self.track.astype(np.int32)

    def to_tracks(self, table, cell_type=None):
        """a list of dataio.tracker.Track, one per track in ID order, from the movie's ObjectTable (rows aligned with
        ``track``): t the frames, x / y / z the centres in CentroidWriter's convention (planar: x = row centre, y = column
        centre, z = 0), label the object's class at every frame, parent / children as above, fate = 4 ('mitosis' in the
        reference's list) for a track that divided and 0 otherwise"""
        from ..dataio.tracker import Track
        if len(table) != len(self.track):
            raise ValueError("the ObjectTable holds %d objects, the TrackTable %d" % (len(table), len(self.track)))
        c = np.asarray(table.centroid, np.float64).reshape(len(self.track), -1)
        if getattr(table, 'volumetric', False):
            xyz = c[:, :3]
        else:
            xyz = np.concatenate([c[:, -2:], np.zeros((len(c), 1))], axis=1)
        order = np.lexsort((np.asarray(table.frame), self.track))
        bounds = np.searchsorted(self.track[order], np.arange(1, len(self) + 2))
        tracks = []
        for i in range(len(self)):
            rows = order[bounds[i]:bounds[i + 1]]
            T = Track(int(self.ID[i]))
            T.t = [int(v) for v in np.asarray(table.frame)[rows]]
            T.x, T.y, T.z = ([float(v) for v in xyz[rows, a]] for a in range(3))
            T.label = [int(v) for v in np.asarray(table.cls)[rows]]
            T.length = len(rows)
            T.parent = int(self.parent[i])
            T.children = [int(v) for v in self.children[i] if v]
            T.fate = FATE_MITOSIS if T.children else 0
            T.cell_type = cell_type
            tracks.append(T)
        return tracks


class FrameLinker(object):
    """The streaming linker: push() the batches of a movie in the stack's order, finish() gives the TrackTable.  It keeps
    the previous batch's last label frame (with ``reach`` > 0 that frame's zones) on the device, so the result does not
    depend on how the movie was cut into batches.  Options: the module's text; check_options pins their types.
    ``overlap`` / ``zones``: the two device calls, overlap_table(a, b, max_label) and label_zones(labels, reach, max_label)
    by default -- a test may pass host restatements, the frames are then whatever those take."""

    def __init__(self, reach=0, min_iou=0.0, min_overlap=1, divisions=True, min_child_fraction=0.5, same_class=True,
                 overlap=None, zones=None):
        self.options = check_options(reach, min_iou, min_overlap, divisions, min_child_fraction, same_class)
        self.reach = self.options['reach']
        self._rule = {k: v for k, v in self.options.items() if k != 'reach'}
        if overlap is None:                                     # room for four successors per object before the first doubling
            def overlap(a, b, max_label):
                return overlap_table(a, b, max_label, max(_MIN_PAIRS, 4 * int(a.shape[0]) * max_label))
        self._overlap = overlap
        if zones is None:
            def zones(labels, reach, max_label):
                from .neighbors import label_zones
                return label_zones(labels, reach, max_label=max_label)
        self._zones = zones
        self._frames = 0
        self._prev = None                                       # (footprint (1, ...) on the device, its objects' classes)
        self._prev_track = None                                 # track ID per label of the last frame
        self._counts, self._track = [], []
        self._start, self._end, self._parent, self._children, self._cls = [], [], [], [], []
        self._links, self._link_overlap, self._link_iou = [], [], []

    # -- host state
    def _new_track(self, t, cls, parent=0):
        self._start.append(t)
        self._end.append(t)
        self._cls.append(int(cls))
        self._children.append([0, 0])
        ID = len(self._start)
        self._parent.append(parent or ID)
        return ID

    def _first_frame(self, cls):
        self._prev_track = np.array([0] + [self._new_track(self._frames, c) for c in cls], np.int64)
        self._track.append(self._prev_track[1:])

    def _step(self, pairs, area_a, area_b, cls_a, cls_b):
        """frame self._frames - 1 -> frame self._frames"""
        t = self._frames - 1
        s = link_pairs(pairs, area_a, area_b, cls_a, cls_b, **self._rule)
        track = np.zeros(len(cls_b) + 1, np.int64)
        cont = np.nonzero(s.kind == KIND_CONTINUATION)[0]
        track[cont + 1] = self._prev_track[s.source[cont]]
        for ID in track[cont + 1].tolist():
            self._end[ID - 1] = t + 1
        for b in s.created:
            a = int(s.source[b - 1])
            parent = int(self._prev_track[a]) if s.kind[b - 1] == KIND_DIVISION else 0
            track[b] = self._new_track(t + 1, cls_b[b - 1], parent)
            if parent:
                ch = self._children[parent - 1]
                ch[1 if ch[0] else 0] = int(track[b])
        linked = np.nonzero(s.kind >= 0)[0]
        self._links.append(np.stack([np.full(len(linked), t, np.int64), s.source[linked], linked + 1, s.kind[linked]], axis=1))
        self._link_overlap.append(s.overlap[linked])
        self._link_iou.append(s.iou[linked])
        self._prev_track = track
        self._track.append(track[1:])

    # -- frames
    def push_frames(self, labels, cls):
        """the next n frames of the movie: labels (n, ...) int32 on the device, cls a list of n class vectors (cls[i][l - 1]
        is the class of label l of frame i; the frame holds len(cls[i]) objects)"""
        n = int(labels.shape[0])
        cls = [np.asarray(c, np.int64).reshape(-1) for c in cls]
        if len(cls) != n:
            raise ValueError("%d class vectors for %d frames" % (len(cls), n))
        if n == 0:
            return
        if any(len(c) > MAX_LABEL for c in cls):
            raise ValueError("more than %d objects in one frame" % MAX_LABEL)
        if self.reach and len(labels.shape) != 3:
            raise ValueError("reach > 0 for volumes in time is not built: (F, D, H, W) stacks link with reach = 0")
        kmax = max(1, max(len(c) for c in cls))
        foot = self._zones(labels, self.reach, kmax) if self.reach else labels
        if self._prev is not None:                              # the step across the cut
            pa, ca = self._prev
            m = max(kmax, len(ca), 1)
            pairs, area_a, area_b = self._overlap(pa, labels[0:1], m)
            self._step(pairs, area_a[0], area_b[0], ca, cls[0])
        else:
            self._first_frame(cls[0])
        self._counts.append(len(cls[0]))
        self._frames += 1
        if n > 1:
            pairs, area_a, area_b = self._overlap(foot[:-1], labels[1:], kmax)
            bounds = np.searchsorted(pairs[:, 0], np.arange(n))
            for i in range(n - 1):
                self._step(pairs[bounds[i]:bounds[i + 1]], area_a[i], area_b[i], cls[i], cls[i + 1])
                self._counts.append(len(cls[i + 1]))
                self._frames += 1
        last = foot[n - 1:n]
        self._prev = (last.clone() if hasattr(last, 'clone') else last.copy(), cls[-1])

    def push(self, first, labels, table):
        """a batch as segment_frames' on_batch delivers it: `first` the stack index of its frame 0 (batches come in the
        stack's order), labels (n, H, W) int32 on the device, table the batch's ObjectTable (frame counted from 0 within
        the batch; object l of frame f is row bounds[f] + l - 1)"""
        if int(first) != self._frames:
            raise ValueError("batches must be pushed in the stack's order: frame %d expected, got %d" % (self._frames, first))
        n = int(labels.shape[0])
        frame = np.asarray(table.frame, np.int64).reshape(-1)
        c = np.asarray(table.cls, np.int64).reshape(-1)
        bounds = np.searchsorted(frame, np.arange(n + 1))
        self.push_frames(labels, [c[bounds[i]:bounds[i + 1]] for i in range(n)])

    def finish(self):
        def cat(parts, dtype, shape=(0,)):
            return np.concatenate(parts) if parts else np.zeros(shape, dtype)
        return TrackTable(self._counts, cat(self._track, np.int64), self._start, self._end, self._parent,
                          np.asarray(self._children, np.int64).reshape(-1, 2), self._cls, cat(self._links, np.int64, (0, 4)),
                          cat(self._link_overlap, np.int64), cat(self._link_iou, np.float64), self.options)


def link_labels(labels, cls=None, **options):
    """The one-call form on a resident stack: labels (F, H, W) int32 on the GPU -- or (F, D, H, W), with reach = 0 only --
    each object's positions holding its 1-based rank within its frame (ranks 1 .. k_t, every one present).  cls: a list of F
    class vectors (cls[t][l - 1]), or None for one class.  options: FrameLinker's.  Returns the TrackTable."""
    _check_stack(labels, 'labels')
    if labels.dim() not in (3, 4):
        raise ValueError("labels must be (F, H, W) or (F, D, H, W), got %s" % (tuple(labels.shape),))
    linker = FrameLinker(**options)
    if linker.reach and labels.dim() == 4:
        raise ValueError("reach > 0 for volumes in time is not built: (F, D, H, W) stacks link with reach = 0")
    F = int(labels.shape[0])
    if cls is None:
        counts = labels.reshape(F, -1).amax(dim=1).clamp_(min=0).cpu().numpy() if F else []
        cls = [np.zeros(int(k), np.int64) for k in counts]
    linker.push_frames(labels, cls)
    return linker.finish()
