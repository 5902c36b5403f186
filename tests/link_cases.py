"""Linking objects from frame to frame: the numpy restatements of include/sequitr_hip.h, "Label overlap and relabelling",
that the GPU path is pinned against, a pure-Python brute force that checks the restatement on tiny stacks, the rule of
sequitr_amd/analysis/linking.py's module text written as plain loops over dicts (independent of link_pairs), and the cases
the CPU and GPU tests share.
"""
import numpy as np

WIDTHS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 130, 255, 256, 257, 1000)
TRACK_COLUMNS = ('track', 'ID', 'start', 'end', 'length', 'parent', 'children', 'root', 'generation', 'cls', 'links',
                 'link_overlap', 'link_iou')
DEFAULTS = {'reach': 0, 'min_iou': 0.0, 'min_overlap': 1, 'divisions': True, 'min_child_fraction': 0.5, 'same_class': True}


# ---- the two device calls ---------------------------------------------------------------------------------------------
def in_range(x, max_label):
    x = np.asarray(x).astype(np.int64)
    return np.where((x >= 1) & (x <= max_label), x, 0)


def overlap_ref(a, b, max_label):
    """a, b (N, ...) -> (pairs (k,4) int64 [n, la, lb, overlap] sorted by (n, la, lb), area_a, area_b (N, max_label+1) int64)"""
    a, b = in_range(a, max_label), in_range(b, max_label)
    N = a.shape[0]
    a, b = a.reshape(N, -1), b.reshape(N, -1)
    n = np.broadcast_to(np.arange(N)[:, None], a.shape)
    both = (a > 0) & (b > 0)
    trip = np.stack([n[both], a[both], b[both]], axis=1).reshape(-1, 3)
    if len(trip):
        rows, counts = np.unique(trip, axis=0, return_counts=True)
        pairs = np.concatenate([rows, counts[:, None]], axis=1).astype(np.int64)
    else:
        pairs = np.zeros((0, 4), np.int64)
    area_a = np.stack([np.bincount(a[i], minlength=max_label + 1) for i in range(N)]).astype(np.int64)
    area_b = np.stack([np.bincount(b[i], minlength=max_label + 1) for i in range(N)]).astype(np.int64)
    area_a[:, 0] = 0
    area_b[:, 0] = 0
    return pairs, area_a, area_b


def brute_overlap(a, b, max_label):
    """the definition, position by position (pure Python; tiny stacks only)"""
    a, b = np.asarray(a), np.asarray(b)
    N = a.shape[0]
    fa, fb = a.reshape(N, -1).tolist(), b.reshape(N, -1).tolist()
    table = {}
    area_a = [[0] * (max_label + 1) for _ in range(N)]
    area_b = [[0] * (max_label + 1) for _ in range(N)]
    for n in range(N):
        for p in range(len(fa[n])):
            la = fa[n][p] if 1 <= fa[n][p] <= max_label else 0
            lb = fb[n][p] if 1 <= fb[n][p] <= max_label else 0
            if la:
                area_a[n][la] += 1
            if lb:
                area_b[n][lb] += 1
            if la and lb:
                table[(n, la, lb)] = table.get((n, la, lb), 0) + 1
    pairs = np.array([list(k) + [v] for k, v in sorted(table.items())], np.int64).reshape(-1, 4)
    return pairs, np.array(area_a, np.int64), np.array(area_b, np.int64)


def relabel_ref(labels, offsets, lut):
    """out[n,p] = lut[offsets[n] + L - 1] if 1 <= L <= offsets[n+1] - offsets[n] (and the entry lies in the table), else 0"""
    labels = np.asarray(labels)
    offsets, lut = np.asarray(offsets, np.int64), np.asarray(lut, np.int32)
    out = np.zeros(labels.shape, np.int32)
    for n in range(labels.shape[0]):
        L = labels[n].astype(np.int64)
        idx = offsets[n] + L - 1
        ok = (L >= 1) & (L <= offsets[n + 1] - offsets[n]) & (idx >= 0) & (idx < len(lut))
        out[n][ok] = lut[idx[ok]]
    return out


# ---- the rule ---------------------------------------------------------------------------------------------------------
def link_ref(counts, cls, tables, min_iou=0.0, min_overlap=1, divisions=True, min_child_fraction=0.5, same_class=True):
    """The module text of sequitr_amd/analysis/linking.py as plain loops.  counts[t]: objects of frame t; cls[t][l - 1]: the
    class of label l; tables[t] = (pairs, area_a, area_b) of the step t -> t + 1: rows [la, lb, overlap] and the areas
    indexed by label.  Returns a dict of the TrackTable's columns."""
    tracks, per_frame, links = [], [], []

    def new(t, c, parent=0):
        tracks.append({'start': t, 'end': t, 'cls': int(c), 'children': [0, 0]})
        tracks[-1]['parent'] = parent or len(tracks)
        return len(tracks)

    F = len(counts)
    cur = {}
    if F:
        cur = {l: new(0, cls[0][l - 1]) for l in range(1, counts[0] + 1)}
        per_frame.append([cur[l] for l in range(1, counts[0] + 1)])
    for t in range(F - 1):
        pairs, aa, ab = tables[t]
        cand = []
        for la, lb, o in (tuple(int(v) for v in r[-3:]) for r in pairs):
            if o < min_overlap:
                continue
            if same_class and int(cls[t][la - 1]) != int(cls[t + 1][lb - 1]):
                continue
            iou = o / (int(aa[la]) + int(ab[lb]) - o)           # Python's int / int: correctly rounded
            if iou >= min_iou:
                cand.append((la, lb, o, iou))
        cand.sort(key=lambda r: (-r[3], -r[2], r[0], r[1]))
        cont, src = {}, {}
        for la, lb, o, iou in cand:
            if la not in cont and lb not in src:
                cont[la], src[lb] = lb, (la, o, iou)
        kind = {lb: 0 for lb in src}
        nxt, divided = {}, set()
        for lb in range(1, counts[t + 1] + 1):
            if lb in src:
                continue
            mine = [r for r in cand if r[1] == lb]
            if divisions and mine:
                la, _, o, iou = min(mine, key=lambda r: (-r[2], r[0]))
                if o / int(ab[lb]) >= min_child_fraction and la in cont and la not in divided:
                    divided.add(la)
                    other, parent = cont[la], cur[la]
                    nxt[other] = new(t + 1, cls[t + 1][other - 1], parent)
                    nxt[lb] = new(t + 1, cls[t + 1][lb - 1], parent)
                    tracks[parent - 1]['children'] = [nxt[other], nxt[lb]]
                    kind[other] = kind[lb] = 1
                    src[lb] = (la, o, iou)
                    continue
            nxt[lb] = new(t + 1, cls[t + 1][lb - 1])
        for lb, k in kind.items():
            if k == 0:
                nxt[lb] = cur[src[lb][0]]
                tracks[nxt[lb] - 1]['end'] = t + 1
        for lb in sorted(kind):
            links.append((t, src[lb][0], lb, kind[lb], src[lb][1], src[lb][2]))
        cur = nxt
        per_frame.append([cur[l] for l in range(1, counts[t + 1] + 1)])
    k = len(tracks)
    root, gen = list(range(1, k + 1)), [0] * k
    for i, tr in enumerate(tracks):
        if tr['parent'] != i + 1:
            root[i], gen[i] = root[tr['parent'] - 1], gen[tr['parent'] - 1] + 1
    col = lambda name: np.array([tr[name] for tr in tracks], np.int64).reshape(-1)   # noqa: E731
    return {'track': np.array([v for f in per_frame for v in f], np.int64).reshape(-1),
            'ID': np.arange(1, k + 1, dtype=np.int64), 'start': col('start'), 'end': col('end'),
            'length': col('end') - col('start') + 1, 'parent': col('parent'),
            'children': np.array([tr['children'] for tr in tracks], np.int64).reshape(k, 2),
            'root': np.array(root, np.int64).reshape(-1), 'generation': np.array(gen, np.int64).reshape(-1), 'cls': col('cls'),
            'links': np.array([r[:4] for r in links], np.int64).reshape(-1, 4),
            'link_overlap': np.array([r[4] for r in links], np.int64).reshape(-1),
            'link_iou': np.array([r[5] for r in links], np.float64).reshape(-1)}


def counts_of(labels):
    labels = np.asarray(labels)
    return [int(max(0, labels[t].max())) if labels[t].size else 0 for t in range(labels.shape[0])]


def link_ref_labels(labels, cls=None, reach=0, **opts):
    """link_ref on the restated tables of a label movie (F, ...): frame t's side is labels[t], or with reach > 0 its zones
    within reach (tests/neighbors_cases.zones_ref)"""
    labels = np.asarray(labels)
    F = labels.shape[0]
    counts = counts_of(labels)
    if cls is None:
        cls = [np.zeros(k, np.int64) for k in counts]
    tables = []
    for t in range(F - 1):
        ml = max(1, counts[t], counts[t + 1])
        foot = labels[t:t + 1]
        if reach:
            from tests import neighbors_cases as nc
            foot = nc.zones_ref(foot, ml, reach)[0]
        p, aa, ab = overlap_ref(foot, labels[t + 1:t + 2], ml)
        tables.append((p[:, 1:], aa[0], ab[0]))
    return link_ref(counts, cls, tables, **opts)


def assert_tracks(got, want, what=''):
    """every column of a TrackTable (its .columns(), or an npz of them) equals link_ref's, floats bit for bit"""
    for name in TRACK_COLUMNS:
        g, w = np.asarray(got[name]), want[name]
        assert g.dtype == w.dtype and g.shape == w.shape, "%s %s: %s %s, want %s %s" % (what, name, g.dtype, g.shape, w.dtype,
                                                                                        w.shape)
        assert g.tobytes() == w.tobytes(), "%s %s differs:\n%s\nwant\n%s" % (what, name, g, w)


def check_consequences(t, counts):
    """what the module text states as consequences, on a dict of columns"""
    k = len(t['ID'])
    assert len(t['track']) == sum(counts) and (k == 0 or (t['track'].min() >= 1 and t['track'].max() <= k))
    frame = np.repeat(np.arange(len(counts)), counts)
    for i in range(k):                                          # a track's frames are consecutive, one object per frame
        f = frame[t['track'] == i + 1]
        assert f.tolist() == list(range(int(t['start'][i]), int(t['end'][i]) + 1)), (i + 1, f)
        assert t['length'][i] == len(f)
        ch = t['children'][i]
        assert (ch == 0).all() or ((ch > 0).all() and ch[0] != ch[1])
        for c in ch[ch > 0]:
            assert t['parent'][c - 1] == i + 1 and t['start'][c - 1] == t['end'][i] + 1
        p = int(t['parent'][i])
        if p == i + 1:
            assert t['root'][i] == i + 1 and t['generation'][i] == 0
        else:
            assert p < i + 1 and i + 1 in t['children'][p - 1]
            assert t['root'][i] == t['root'][p - 1] and t['generation'][i] == t['generation'][p - 1] + 1


# ---- movies -----------------------------------------------------------------------------------------------------------
def boxes(shape, frames):
    """frames: per frame a list of (label, y0, y1, x0, x1) boxes, hi exclusive -> (F, H, W) int32"""
    out = np.zeros((len(frames),) + tuple(shape), np.int32)
    for t, fr in enumerate(frames):
        for l, y0, y1, x0, x1 in fr:
            out[t, y0:y1, x0:x1] = l
    return out


def scenarios():
    """(name, labels (F,H,W), cls or None, options) of the hand-made movies; the CPU test states what each must give"""
    S = (8, 24)
    third = 6 / 18                                              # iou of two 2 x 6 boxes shifted by 3: 6 / (12 + 12 - 6)
    half = 6 / 12                                               # the child fraction of a 2 x 6 box half inside its parent
    out = [
        ("stationary", boxes(S, [[(1, 2, 4, 2, 8)]] * 3), None, {}),
        ("moving_with_overlap", boxes(S, [[(1, 2, 4, 2, 8)], [(1, 2, 4, 5, 11)], [(1, 2, 4, 8, 14)]]), None, {}),
        ("moving_without_overlap", boxes(S, [[(1, 2, 4, 2, 8)], [(1, 2, 4, 8, 14)]]), None, {}),
        # a 4 x 8 mother, then two 4 x 3 daughters: the left one (label 1) has the larger iou only by the tie rule
        ("division", boxes(S, [[(1, 2, 6, 4, 12)], [(1, 2, 6, 4, 7), (2, 2, 6, 9, 12)], [(1, 2, 6, 3, 6), (2, 2, 6, 10, 13)]]),
         None, {}),
        # the larger daughter carries the larger label: the continued child comes first, so it gets the smaller ID
        ("division_continued_child_first", boxes(S, [[(1, 2, 6, 4, 12)], [(1, 2, 6, 4, 6), (2, 2, 6, 7, 12)]]), None, {}),
        # two objects of frame 0 overlap one of frame 1 alike: equal iou and overlap, the smaller la wins
        ("tie", boxes(S, [[(1, 2, 4, 2, 6), (2, 2, 4, 10, 14)], [(1, 2, 4, 4, 12)]]), None, {}),
        ("three_claimants", boxes(S, [[(1, 1, 7, 3, 15)], [(1, 1, 7, 3, 6), (2, 1, 7, 7, 10), (3, 1, 7, 11, 14)]]), None, {}),
        ("merge", boxes(S, [[(1, 2, 4, 2, 8), (2, 2, 4, 9, 12)], [(1, 2, 4, 3, 12)]]), None, {}),
        ("class_change_same_class", boxes(S, [[(1, 2, 4, 2, 8)], [(1, 2, 4, 3, 9)]]), [[0], [1]], {}),
        ("class_change_any_class", boxes(S, [[(1, 2, 4, 2, 8)], [(1, 2, 4, 3, 9)]]), [[0], [1]], {"same_class": False}),
        ("no_divisions", boxes(S, [[(1, 2, 6, 4, 12)], [(1, 2, 6, 4, 7), (2, 2, 6, 9, 12)]]), None, {"divisions": False}),
        ("empty_frame_in_the_middle", boxes(S, [[(1, 2, 4, 2, 8)], [], [(1, 2, 4, 2, 8)]]), None, {}),
        ("one_frame", boxes(S, [[(1, 2, 4, 2, 8), (2, 5, 7, 2, 8)]]), [[1, 0]], {}),
        ("min_overlap", boxes(S, [[(1, 2, 4, 2, 8)], [(1, 2, 4, 7, 13)]]), None, {"min_overlap": 3}),
    ]
    iou_movie = boxes(S, [[(1, 2, 4, 2, 8)], [(1, 2, 4, 5, 11)]])
    for name, v in (("at", third), ("below", np.nextafter(third, 0.0)), ("above", np.nextafter(third, 1.0))):
        out.append(("min_iou_" + name, iou_movie, None, {"min_iou": float(v)}))
    # a 2 x 8 mother; daughter 1 inside it, daughter 2 (2 x 6) half outside: fraction 6 / 12
    frac_movie = boxes(S, [[(1, 2, 4, 2, 10)], [(1, 2, 4, 2, 6), (2, 2, 4, 7, 13)]])
    for name, v in (("at", half), ("below", np.nextafter(half, 0.0)), ("above", np.nextafter(half, 1.0))):
        out.append(("min_child_fraction_" + name, frac_movie, None, {"min_child_fraction": float(v)}))
    return out


def disk(img, cy, cx, r, value):
    H, W = img.shape
    yy, xx = np.mgrid[0:H, 0:W]
    img[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = value


def rank_labels(ids):
    """(F, ...) cell identities, 0 = background -> each object's 1-based rank within its frame by first position in memory,
    and per frame the identity of every rank"""
    out = np.zeros(ids.shape, np.int32)
    who = []
    for t in range(ids.shape[0]):
        vals, first = np.unique(ids[t].reshape(-1), return_index=True)
        keep = vals > 0
        vals, first = vals[keep], first[keep]
        order = vals[np.argsort(first)]
        for r, v in enumerate(order):
            out[t][ids[t] == v] = r + 1
        who.append([int(v) for v in order])
    return out, who


def disk_movie(F=6, H=96, W=130):
    """drifting, dividing and vanishing disks -> (labels (F,H,W) int32, cls list, who): cell 1 drifts; cell 2 divides into 21
    and 22 at frame 3; cell 3 vanishes after frame 2; cell 4 (radius 4) jumps 10 pixels per frame, so it never overlaps
    itself and only a reach rescues it; cell 5 appears at frame 4; cell 6 is of class 1 and stays"""
    ids = np.zeros((F, H, W), np.int32)
    for t in range(F):
        disk(ids[t], 20 + 2 * t, 20 + 3 * t, 9, 1)
        if t < 3:
            disk(ids[t], 60, 45 + t, 10, 2)
            disk(ids[t], 30, 100, 7, 3)
        else:
            disk(ids[t], 60, 41 - 2 * (t - 3), 6, 21)
            disk(ids[t], 60, 55 + 2 * (t - 3), 6, 22)
        disk(ids[t], 85, 12 + 10 * t, 4, 4)
        if t >= 4:
            disk(ids[t], 25, 70, 6, 5)
        disk(ids[t], 80 - t, 110, 8, 6)
    labels, who = rank_labels(ids)
    cls = [np.array([1 if v == 6 else 0 for v in w], np.int64) for w in who]
    return labels, cls, who


def volume_movie(F=4, D=3, H=20, W=33):
    """(F, D, H, W): a ball that drifts, one that divides at frame 2, one that vanishes"""
    ids = np.zeros((F, D, H, W), np.int32)
    for t in range(F):
        for z in range(D):
            disk(ids[t, z], 5 + t, 6 + t, 3, 1)
            if t < 2:
                disk(ids[t, z], 13, 20, 5, 2)
            else:
                disk(ids[t, z], 13, 17 - (t - 2), 2, 21)
                disk(ids[t, z], 13, 23 + (t - 2), 2, 22)
        if t < 3:
            disk(ids[t, 1], 4, 27, 2, 3)
    labels, who = rank_labels(ids)
    return labels, who


def random_stack(seed, N, P, max_label, density=0.5, run=6):
    """(N, P) int32 of runs of equal labels with background between them, values 0 .. max_label"""
    rng = np.random.default_rng(seed)
    out = np.zeros((N, P), np.int32)
    for n in range(N):
        p = 0
        while p < P:
            length = int(rng.integers(1, run + 1))
            out[n, p:p + length] = int(rng.integers(1, max_label + 1)) if rng.random() < density else 0
            p += length
    return out
