"""Shared by tests/test_weightmap_definitions.py (CPU) and tests/test_gpu_weightmap_sweep.py (GPU): the case tables of the
planar weight-map kernels (sequitr_amd/csrc/sq_weightmap.hip: edt_rows_kernel, edt_cols_weight_kernel, edt_rows_v2_kernel,
edt_cols_weight_v2_kernel, wm2_raster_kernel, wm2_gauss0_kernel, wm2_gauss1_weight_kernel) and of wm2_points_kernel
(sq_delaunay.hip), the launch arithmetic restated from those sources, a replay of the v2 column search with branch counters,
and the references.  No HIP call, no import of the library.

References, never the code under test: oracle.weightmap_ref (the reference's own scipy calls) and a brute-force O(n^2)
squared distance for the tiny cases.

The numpy rule behind the map (ImageWeightMap.pipe, sequitr/pipeline.py:475-479): ImagePipe.__call__ casts a 2-D image to
float32 and w0 is a Python scalar, so `w0 * (1. - image)` is the FLOAT32 product fl32(fl32(w0) * fl32(1 - image)); it is
widened only where it meets the float64 exp(...).  ImageWeightMap2 does the same with mask.astype('float32').  map_expr_f32
restates that, map_expr_f64 is the all-double reading the kernels had before."""
import functools

import numpy as np

from oracle import weightmap_ref

# ---- launch constants of sq_weightmap.hip / sq_delaunay.hip ------------------------------------------------------------------
ROW_SEGS = 16                                                   # edt_rows_v2_kernel: 64-pixel segments held in registers
CS, RSPLIT = 32, 8                                              # edt_cols_weight_v2_kernel: strip width, blocks sharing a strip
G_INF = 30000
GRID_CAP = 16384                                                # wm_grid: blocks of 256
POINTS_GRID_CAP = 8192                                          # sq_wm2_boundary_points_u8
LDS_DEFAULT = 48 * 1024                                         # above this the launch has to ask for its dynamic LDS

# (w0, sigma).  10 and 30 are float32 numbers; 12.3, 0.1 and 1/3 are not
PARAMS = ((10., 5.), (30., 3.), (12.3, 3.), (0.1, 5.), (1. / 3., 2.5))
PARAMS_ALL = ((10., 5.), (12.3, 3.))                            # run on every case; PARAMS on the cases up to SMALL pixels
NEW_W0 = (12.3, 0.1, 1. / 3.)
SMALL = 20000


def _cdiv(a, b):
    return -(-a // b)


def shape_of(name):
    """(N, H, W) from the NxHxW at the end of a case's name"""
    return tuple(int(v) for v in name.rsplit("_", 1)[1].split("x"))


def params_of(shape):
    return PARAMS if int(np.prod(shape)) <= SMALL else PARAMS_ALL


def regime(N, H, W):
    """how sq_edt_sq_f32 / sq_weightmap_edt_f32 launch on (N, H, W), restated from edt_v2_fits, edt_v2, edt_common, wm_grid"""
    total, rows = N * H * W, N * H
    rows_per = _cdiv(H, RSPLIT)
    nblk8 = _cdiv(H, 8)
    lds = (H + (H + 7) // 8) * 64                               # (H + nblk8) * CS * sizeof(u16)
    grid = min(max(_cdiv(total, 256), 1), GRID_CAP)
    return {
        "form": "v2" if (W <= 64 * ROW_SEGS and H <= 2048) else "v1",
        "nseg": _cdiv(W, 64),                                   # row segments of one wave
        "last_seg_partial": W % 64 != 0,
        "row_blocks": _cdiv(rows, 4),
        "idle_row_waves": rows % 4 != 0,                        # the last row block has waves with r >= rows
        "strips": _cdiv(W, CS),
        "last_strip_padded": W % CS != 0,                       # filled with G_INF
        "rows_per": rows_per,
        "empty_parts": tuple(p for p in range(RSPLIT) if p * rows_per >= H),
        "nblk8": nblk8,
        "last_block_partial": H % 8 != 0,                       # the scalar tail of scan
        "lds_bytes": lds,
        "lds_above_48k": lds > LDS_DEFAULT,
        "v1_trips": _cdiv(total, grid * 256),                   # grid-stride trips of edt_cols_weight_kernel
        "flag_ints": ((N + 3) // 4) * 4,                        # g starts this many ints into the workspace
        "flags_padded": N % 4 != 0,
    }


def stream_trips(total, cap=GRID_CAP):
    """grid-stride trips of a 256-thread kernel over `total` items with its grid capped at `cap` blocks"""
    return _cdiv(total, min(max(_cdiv(total, 256), 1), cap) * 256)


# ---- squared distances --------------------------------------------------------------------------------------------------------
def is_feature(img):
    return np.asarray(img, np.float32) == np.float32(1.0)       # (1 - image) == 0 holds for exactly this value


def brute_force_sq(img):
    """O(n^2): squared distance of every pixel of one (H,W) image to the nearest feature; scipy's artefact, the distance to
    index (-1, 0), where there is none"""
    H, W = img.shape
    y, x = np.mgrid[0:H, 0:W]
    fy, fx = np.nonzero(is_feature(img))
    if len(fy) == 0:
        return ((y + 1) ** 2 + x ** 2).astype(np.int64)
    d = (y.reshape(-1, 1) - fy[None]) ** 2 + (x.reshape(-1, 1) - fx[None]) ** 2
    return d.min(1).reshape(H, W).astype(np.int64)


def row_distances(img):
    """g of the row pass: distance along the row to the nearest feature, G_INF in a row without one; (H,W) int64"""
    H, W = img.shape
    g = np.full((H, W), G_INF, np.int64)
    f = is_feature(img)
    cols = np.arange(W)
    for r in range(H):
        c = np.nonzero(f[r])[0]
        if len(c):
            g[r] = np.abs(cols[:, None] - c[None]).min(1)
    return g


COUNTERS = ("scan_full", "scan_tail", "up_stop_distance", "down_stop_distance", "up_off_image", "down_off_image",
            "skip_block_minimum", "scan_neighbour")
# literal flips of the two comparisons: each only makes the search look at MORE blocks, so neither can change the minimum
BENIGN_MUTATIONS = ("block_minimum_le", "stop_gt")
# the same two tests and the tail, wrong in the direction that leaves candidates out
LOSING_MUTATIONS = ("block_minimum_one_row_off", "stop_one_row_off", "no_tail")


def column_search_replay(g, mutate=None, cols=None):
    """The control flow of edt_cols_weight_v2_kernel's search on the row distances g (H,W) of one image that has a feature,
    every pixel at once: scan of the pixel's own 8-row block, then outwards block by block, the up side before the down side
    at each step as in the kernel.  Returns (D2 (H, len(cols)) int64, {counter: pixels that took the branch}).
    mutate: one of BENIGN_MUTATIONS / LOSING_MUTATIONS."""
    g = np.asarray(g, np.int64)
    if cols is not None:
        g = g[:, list(cols)]
    H, W = g.shape
    nblk8 = _cdiv(H, 8)
    m8 = np.stack([g[8 * b:min(H, 8 * b + 8)].min(0) for b in range(nblk8)])       # block minima
    ys = np.arange(H)[:, None]
    cnt = dict.fromkeys(COUNTERS, 0)
    best = g * g

    def scan(b, mask):
        nonlocal best
        full = 8 * b + 8 <= H
        cnt["scan_full"] += int((mask & full).sum())
        cnt["scan_tail"] += int((mask & ~full).sum())
        if mutate == "no_tail":
            mask = mask & full
        for k in range(8):
            r = 8 * b + k
            ok = mask & (r < H)
            v = g[np.clip(r, 0, H - 1)[:, 0], :]
            c = v * v + (ys - r) ** 2
            best = np.where(ok & (c < best), c, best)

    b0 = ys >> 3
    scan(b0, np.ones((H, W), bool))
    up, dn = np.ones((H, W), bool), np.ones((H, W), bool)
    db = 1
    while up.any() or dn.any():
        for side in ("up", "down"):
            live = up if side == "up" else dn
            if not live.any():
                continue
            blk = b0 - db if side == "up" else b0 + db
            dist = ys - (8 * blk + 7) if side == "up" else 8 * blk - ys           # to the nearest row of that block
            off = (blk < 0) if side == "up" else (blk >= nblk8)
            ds = dist + 1 if mutate == "stop_one_row_off" else dist
            far = (ds * ds > best) if mutate == "stop_gt" else (ds * ds >= best)
            cnt[side + "_off_image"] += int((live & off).sum())
            cnt[side + "_stop_distance"] += int((live & ~off & far).sum())
            live = live & ~off & ~far
            m = m8[np.clip(blk, 0, nblk8 - 1)[:, 0], :]
            dm = dist + 1 if mutate == "block_minimum_one_row_off" else dist
            t = dm * dm + m * m
            go = live & ((t <= best) if mutate == "block_minimum_le" else (t < best))
            cnt["skip_block_minimum"] += int((live & ~go).sum())
            cnt["scan_neighbour"] += int(go.sum())
            scan(blk, go)
            if side == "up":
                up = live
            else:
                dn = live
        db += 1
    return best, cnt


# ---- the map expression -------------------------------------------------------------------------------------------------------
def map_expr_f32(img, d2, w0, sigma):
    """pipeline.py:477-479 on exact squared distances with numpy's types: float32 product, float64 from the exp on"""
    image = np.asarray(img, np.float32)
    d = np.sqrt(np.asarray(d2, np.float64))
    wb = np.float32(w0) * (np.float32(1.) - image)
    assert wb.dtype == np.float32
    return wb.astype(np.float64) * np.exp(-(d * d) / (2. * sigma ** 2 + 1e-99)) + image.astype(np.float64) + 1.


def map_expr_f64(img, d2, w0, sigma):
    """the same expression with the product in double: what the kernels computed before"""
    image = np.asarray(img, np.float32).astype(np.float64)
    d = np.sqrt(np.asarray(d2, np.float64))
    return w0 * (1. - image) * np.exp(-(d * d) / (2. * sigma ** 2 + 1e-99)) + image + 1.


def ordered64(a):
    """float64 -> int64 that orders like the numbers (either sign): differences are distances in units in the last place"""
    i = np.ascontiguousarray(a, np.float64).view(np.int64)
    return np.where(i < 0, np.int64(-2 ** 63) - i, i)


def ulps64(a, b):
    return int(np.abs(ordered64(a) - ordered64(b)).max())


def near_f32_midpoint(v, margin):
    """bool array: v (float64) lies within `margin` (absolute, array or scalar) of the midpoint between two adjacent float32
    numbers -- where rounding a slightly different float64 value to float32 could give the other neighbour"""
    v = np.asarray(v, np.float64)
    f = v.astype(np.float32)
    bad = np.zeros(v.shape, bool)
    for nb in (np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))):
        mid = (f.astype(np.float64) + nb.astype(np.float64)) / 2.
        bad |= np.abs(v - mid) <= margin
    return bad


# ---- planar EDT cases ---------------------------------------------------------------------------------------------------------
def _random(seed, shape, p):
    """random binary labels with at least one feature in every image"""
    rng = np.random.default_rng(seed)
    v = (rng.random(shape) < p).astype(np.float32)
    for i in range(shape[0]):
        if not v[i].any():
            v[i, shape[1] // 2, shape[2] // 2] = 1
    return v


def _rows_wide(W, H):
    """the carries of the row pass: only column 0 (`last` carried over every later segment), only the last column (`nxt`
    carried), columns 63 and 64 (both sides of a segment edge), a featureless row between featured ones"""
    v = np.zeros((1, H, W), np.float32)
    v[0, 0, 0] = 1
    if H == 3:
        v[0, 2, W - 1] = 1                                      # row 1 stays featureless
    else:
        v[0, 1, W - 1] = 1
        v[0, 2, 63] = v[0, 2, 64] = 1
        v[0, 4] = _random(W, (1, 1, W), 0.01)[0, 0]             # row 3 stays featureless
    return v


def _one_bg_one_feature():
    v = np.zeros((1, 2, 1), np.float32)
    v[0, 1, 0] = 1
    return v


def _corner(shape, where):
    v = np.zeros(shape, np.float32)
    v[(0,) + where] = 1
    return v


def _dense_row_far_from_sparse():
    v = np.zeros((1, 2048, 40), np.float32)
    v[0, :400] = _random(21, (1, 400, 40), 0.0008)[0]           # sparse rows at the top
    v[0, 1500] = 1                                              # one dense row far below
    return v


def _middle_empty(seed, shape, p):
    v = _random(seed, shape, p)
    v[shape[0] // 2] = 0
    return v


NONBINARY_VALUES = (0.3, 0.5, 2.0, -0.0, 1. + 2. ** -23, float(np.nextafter(np.float32(1), np.float32(0))))


def _nonbinary(seed, shape):
    """only == 1.0f is a feature: every other value is background with its own 1 - image"""
    rng = np.random.default_rng(seed)
    v = (rng.random(shape) < 0.12).astype(np.float32)           # dense: far from every feature exp() vanishes and 1 + image is
                                                                # exactly a float32 midpoint for the two neighbours of 1
    pick = rng.integers(0, len(NONBINARY_VALUES) + 3, shape)
    for k, val in enumerate(NONBINARY_VALUES):
        v[(pick == k) & (v == 0)] = np.float32(val)
    v[0, 0, 0], v[0, -1, -1] = 1, np.float32(NONBINARY_VALUES[-1])
    return v


_EDT = {
    # v2 row pass: W at the segment edges, N * H rows with rows % 4 != 0
    "rows_1x2x1": _one_bg_one_feature,
    "rows_1x3x63": lambda: _random(31, (1, 3, 63), 0.04),
    "rows_1x5x64": lambda: _random(32, (1, 5, 64), 0.04),
    "rows_1x2x65": lambda: _random(33, (1, 2, 65), 0.04),
    "rows_1x3x1023": lambda: _rows_wide(1023, 3),
    "rows_1x5x1024": lambda: _rows_wide(1024, 5),
    # v2 column pass: 683 rows is the first LDS request above 48 KiB, 2048 rows the largest (147456 B)
    "lds_1x682x33": lambda: _random(41, (1, 682, 33), 0.002),
    "lds_1x683x33": lambda: _random(42, (1, 683, 33), 0.002),
    "tall_corner_1x2048x40": lambda: _corner((1, 2048, 40), (0, 0)),
    "tall_dense_row_1x2048x40": _dense_row_far_from_sparse,
    "batch_empty_middle_3x9x70": lambda: _middle_empty(43, (3, 9, 70), 0.02),
    # v1, reached by shape
    "v1_wide_1x3x1025": lambda: _random(51, (1, 3, 1025), 0.004),
    "v1_wide_2x5x1100": lambda: _random(52, (2, 5, 1100), 0.003),
    "v1_tall_1x2049x3": lambda: _random(53, (1, 2049, 3), 0.004),
    "v1_tall_1x2050x33": lambda: _random(54, (1, 2050, 33), 0.003),
    "v1_flags_5x3x1026": lambda: _middle_empty(55, (5, 3, 1026), 0.004),
    "v1_corner_1x2049x3": lambda: _corner((1, 2049, 3), (2048, 2)),
    "v1_stride_1x2049x2050": lambda: _random(56, (1, 2049, 2050), 0.01),
    # values other than 0 and 1, both forms
    "nonbinary_1x6x70": lambda: _nonbinary(61, (1, 6, 70)),
    "nonbinary_v1_1x2x1030": lambda: _nonbinary(60, (1, 2, 1030)),
}
for _h in (1, 5, 8, 9, 17):
    for _w in (9, 32, 33, 70):
        _EDT["cols_1x%dx%d" % (_h, _w)] = functools.partial(_random, 100 * _h + _w, (1, _h, _w), 0.06)
EDT_CASES = tuple(_EDT)
ROW_PASS_CASES = tuple(n for n in EDT_CASES if n.startswith("rows_"))
TINY = 3000                                                     # pixels per image up to which the brute force runs
REPLAY_COLUMNS = {"tall_corner_1x2048x40": (0, 1, 31, 32, 39), "tall_dense_row_1x2048x40": (0, 17, 32, 39)}


@functools.lru_cache(maxsize=None)
def edt_labels(name):
    v = _EDT[name]()
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def edt_reference_sq(name):
    """weightmap_ref.edt_squared of every image of a case, computed once and shared (read-only)"""
    r = np.stack([weightmap_ref.edt_squared(v) for v in edt_labels(name)])
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def edt_reference_map(name, w0, sigma):
    """weightmap_ref.image_weight_map of every image of a case, called with Python floats; (N,H,W) float64, read-only"""
    r = np.stack([weightmap_ref.image_weight_map(v, float(w0), float(sigma))[..., 0] for v in edt_labels(name)])
    assert r.dtype == np.float64
    r.setflags(write=False)
    return r


# ---- ImageWeightMap2 cases: hand-made simplices ---------------------------------------------------------------------------------
def longest_edges(V):
    """max of edist over the three edges (pipeline.py:545), as oracle.weightmap_ref computes it"""
    V = np.asarray(V, np.int64)
    e = (V - np.roll(V, -1, axis=1)).astype(np.float64)
    return np.sqrt((e ** 2).sum(-1)).max(-1)


def raster_clipped(b, V, w0, sigma):
    """weightmap_ref.image_weight_map2_raster(vertices=) for simplices that may stick out of the tile: the same rule, each
    bounding box clipped to the tile first.  b (H,W) bool, V (S,3,2) int (row, column).  Returns (map (H,W,1), count)."""
    V = np.asarray(V, np.int64).reshape(-1, 3, 2)
    longest = longest_edges(V) if len(V) else np.zeros(0)
    H, W = b.shape
    best = np.zeros((H, W))
    count = np.zeros((H, W), np.int32)
    for k in range(len(V)):
        (x0, y0), (x1, y1), (x2, y2) = V[k]
        xa, xb = max(min(x0, x1, x2), 0), min(max(x0, x1, x2), H - 1)
        ya, yb = max(min(y0, y1, y2), 0), min(max(y0, y1, y2), W - 1)
        if xa > xb or ya > yb:
            continue
        X, Y = np.mgrid[xa:xb + 1, ya:yb + 1]
        e0 = (x1 - x0) * (Y - y0) - (y1 - y0) * (X - x0)
        e1 = (x2 - x1) * (Y - y1) - (y2 - y1) * (X - x1)
        e2 = (x0 - x2) * (Y - y2) - (y0 - y2) * (X - x2)
        ins = ((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))
        sub = best[xa:xb + 1, ya:yb + 1]
        np.maximum(sub, np.where(ins, longest[k], 0.0), out=sub)
        count[xa:xb + 1, ya:yb + 1] += ins
    d = np.where(count > 0, best, 1024.)
    return weightmap_ref._finish2(b, d, w0, sigma), count


def in_tile(V, H, W):
    """bool (S): every vertex of the simplex lies on the tile"""
    V = np.asarray(V, np.int64).reshape(-1, 3, 2)
    return ((V[..., 0] >= 0) & (V[..., 0] < H) & (V[..., 1] >= 0) & (V[..., 1] < W)).all(1)


def reflect(i, n):
    """scipy's 'reflect' border (d c b a | a b c d | d c b a), bouncing as often as a tile narrower than the window needs"""
    if n == 1:
        return 0
    while i < 0 or i >= n:
        i = -i - 1 if i < 0 else 2 * n - 1 - i
    return i


def gauss9_reflect(wm):
    """gaussian_filter(sigma = 1) of an (H,W) map as the two Gaussian kernels apply it: 9 taps, axis 0 then axis 1, centre first
    then the pairs k = 4 .. 1, and the factor of the pass over the length-1 channel axis"""
    w = np.exp(-0.5 * np.arange(-4, 5, dtype=np.float64) ** 2)
    w = (w / w.sum())[4:]
    wsum = w[0] + 2 * (w[1] + w[2] + w[3] + w[4])
    out = np.asarray(wm, np.float64)
    for axis in (0, 1):
        src = np.moveaxis(out, axis, 0)
        n = src.shape[0]
        acc = src * w[0]
        for k in (4, 3, 2, 1):
            lo = src[[reflect(i - k, n) for i in range(n)]]
            hi = src[[reflect(i + k, n) for i in range(n)]]
            acc = acc + (lo + hi) * w[k]
        out = np.moveaxis(acc, 0, axis)
    return out * wsum


PAD = (-1, 0, 0, 0, 0, 0, 0)                                    # a padding row of sq_delaunay2d_batch_i32


def _tri(tile, a, b, c):
    return (tile,) + tuple(a) + tuple(b) + tuple(c)


# (row, column) vertices on a 37 x 90 tile
_BIG_TRIS = (
    ((-5, 10), (8, 4), (6, 30)),                                # sticks out at the top
    ((30, 50), (45, 60), (33, 80)),                             # ... at the bottom
    ((10, -7), (20, 5), (14, 12)),                              # ... on the left
    ((5, 70), (15, 95), (25, 75)),                              # ... on the right; bounding box 21 x 26 > 64 pixels
    ((20, 20), (22, 24), (24, 28)),                             # collinear: covers only its own line
    ((10, 40), (20, 40), (15, 55)),                             # these two share the edge (10,40)-(20,40): tie pixels
    ((10, 40), (20, 40), (14, 30)),
)


def _wide_tiles(transpose):
    N = 3 if transpose else 2
    img = np.zeros((N, 37, 90), np.float32)
    img[0, 0:4, 20:30] = 1                                      # foreground objects crossing the border
    img[0, 12:18, 86:90] = 1
    img[N - 1, 33:37, 0:6] = 1
    img[N - 1, 15:19, 42:50] = 1                                # foreground under the shared edge
    rows = [PAD]
    for t in range(N):
        for k, tri in enumerate(_BIG_TRIS):
            if (k + t) % N == 0 or t == N - 1:
                rows.append(_tri(t, *tri))
        if t < N - 1:
            rows.append(PAD)
    simp = np.array(rows, np.int32)                             # 13 / 15 rows: the last block of four waves is not full
    if transpose:
        img = np.ascontiguousarray(img.transpose(0, 2, 1))
        simp[:, 1:] = simp[:, 1:].reshape(-1, 3, 2)[:, :, ::-1].reshape(-1, 6)
    return img, simp


def _narrow_3x40():
    img = np.zeros((1, 3, 40), np.float32)
    img[0, :, 10:13] = 1
    return img, np.array([_tri(0, (-2, 5), (4, 20), (1, 35))], np.int32)                 # nsimp = 1


def _narrow_40x3():
    img = np.zeros((1, 40, 3), np.float32)
    img[0, 30:34, :] = 1
    img[0, 0, 0] = 1
    return img, np.array([_tri(0, (2, 0), (12, 2), (20, 1)), _tri(0, (12, 2), (20, 1), (28, 2)), PAD,
                          _tri(0, (35, -3), (39, 1), (36, 6)), _tri(0, (3, 0), (3, 1), (3, 2))], np.int32)   # nsimp = 5


def _narrow_2x9():
    img = np.zeros((1, 2, 9), np.float32)
    img[0, 1, 4] = 1
    return img, np.array([PAD, _tri(0, (0, 0), (1, 8), (0, 8)), _tri(0, (0, 0), (1, 0), (1, 3)), PAD,
                          _tri(0, (0, 2), (1, 2), (1, 6))], np.int32)                    # nsimp = 5


def _stride_tile():
    """4.2 M pixels: more than GRID_CAP blocks of 256, so both Gaussian kernels take a second grid-stride trip"""
    img = np.zeros((1, 2049, 2050), np.float32)
    img[0, 1000:1010, 1500:1520] = 1
    img[0, 2045:2049, 2040:2050] = 1                            # foreground in the last rows, the second trip's pixels
    simp = np.array([_tri(0, (0, 0), (6, 2), (2, 7)), _tri(0, (2040, 2030), (2048, 2049), (2046, 2035)),
                     _tri(0, (995, 1490), (1003, 1498), (1001, 1488)), _tri(0, (2044, 3), (2051, 6), (2047, -2)),
                     _tri(0, (1024, 1020), (1030, 1029), (1021, 1027))], np.int32)
    return img, simp


_WM2 = {
    "narrow_1x3x40": _narrow_3x40,
    "narrow_1x40x3": _narrow_40x3,
    "narrow_1x2x9": _narrow_2x9,
    "wide_2x37x90": lambda: _wide_tiles(False),
    "tall_3x90x37": lambda: _wide_tiles(True),
    "stride_1x2049x2050": _stride_tile,
}
WM2_CASES = tuple(_WM2)
# (w0, sigma).  Uncovered pixels are 1024 and the 9-tap Gaussian spreads them 4 pixels into every simplex, so at sigma = 5
# exp(-(wm * wm) / 50) is 0 on most of a small tile and the map says little about the raster; a sigma of a few hundred
# keeps every pixel's value a function of its wm (exp(-1024^2 / (2 * 300^2)) = 3e-3)
WM2_PARAMS = ((10., 5.), (10., 300.), (12.3, 150.))
WM2_PARAMS_STRIDE = ((10., 300.), (12.3, 150.))                 # the 4.2 M pixel tile: its reference takes 0.7 s a run


def wm2_params_of(name):
    return WM2_PARAMS_STRIDE if name.startswith("stride") else WM2_PARAMS


@functools.lru_cache(maxsize=None)
def wm2_case(name):
    """(img (N,H,W) float32, simplices (S,7) int32, longest (S) float64), read-only"""
    img, simp = _WM2[name]()
    lng = longest_edges(simp[:, 1:].reshape(-1, 3, 2))
    for a in (img, simp, lng):
        a.setflags(write=False)
    return img, simp, lng


@functools.lru_cache(maxsize=None)
def wm2_reference(name, w0, sigma):
    """the raster definition tile by tile; the oracle's own where every simplex lies on the tile.  (N,H,W) float64"""
    img, simp, _ = wm2_case(name)
    N, H, W = img.shape
    out = []
    for n in range(N):
        V = simp[simp[:, 0] == n, 1:].reshape(-1, 3, 2)
        if len(V) and in_tile(V, H, W).all():
            m = weightmap_ref.image_weight_map2_raster(img[n], float(w0), float(sigma), vertices=V)[0]
        else:
            m = raster_clipped(img[n] != 0, V, float(w0), float(sigma))[0]
        out.append(m[..., 0])
    r = np.stack(out)
    r.setflags(write=False)
    return r


def _discs(H, W, discs):
    y, x = np.mgrid[0:H, 0:W]
    lab = np.zeros((H, W), np.float32)
    for cy, cx, r in discs:
        lab[(y - cy) ** 2 + (x - cx) ** 2 <= r * r] = 1
    return lab


# the reference path (scipy morphology + Qhull): one wide and one tall tile, objects on the borders
SCIPY_TILES = {
    "scipy_48x96": lambda: _discs(48, 96, ((3, 12, 6), (30, 40, 8), (47, 70, 7), (20, 95, 5), (8, 60, 4), (25, 0, 4))),
    "scipy_96x48": lambda: _discs(96, 48, ((12, 3, 6), (40, 30, 8), (70, 47, 7), (95, 20, 5), (60, 8, 4), (0, 25, 4))),
}


# ---- boundary-point cases -----------------------------------------------------------------------------------------------------
def _points_2x5x70():
    v = np.zeros((2, 5, 70), np.float32)
    v[0, 0, 3:9] = v[0, 4, 20:40] = 1                           # top and bottom border
    v[0, :, 0] = v[0, 1:4, 69] = 1                              # left and right border
    v[0, 4, :] = 1                                              # image 0's last row and image 1's first row both filled:
    v[1, 0, :] = 1                                              # nothing may leak across the batch boundary
    v[1, 3, 30:33] = 1
    return v


def _points_3x6x6():
    v = np.zeros((3, 6, 6), np.float32)
    v[0, 0, 0] = v[0, 5, 5] = v[0, 0, 5] = v[0, 5, 0] = 1       # the four corners
    v[1, 5, :] = 1
    v[2, 0, :] = 1
    v[2, 2:4, 2:4] = 1
    return v


def _points_1x1x20():
    v = np.zeros((1, 1, 20), np.float32)
    v[0, 0, 0] = v[0, 0, 8:11] = v[0, 0, 19] = 1
    return v


_POINTS = {
    "points_2x5x70": _points_2x5x70,
    "points_2x70x5": lambda: np.ascontiguousarray(_points_2x5x70().transpose(0, 2, 1)),
    "points_3x6x6": _points_3x6x6,
    "points_1x1x20": _points_1x1x20,
    "points_stride_1x2049x2050": lambda: _stride_tile()[0],     # more than POINTS_GRID_CAP blocks of 256
}
POINTS_CASES = tuple(_POINTS)


@functools.lru_cache(maxsize=None)
def points_labels(name):
    v = _POINTS[name]()
    v.setflags(write=False)
    return v


def boundary_points_2d(label):
    """weightmap_ref.boundary_points without its np.squeeze, which turns a one-row tile into a 1-D array that scipy's 2-D
    structuring element refuses; the same calls otherwise (tests/test_weightmap_definitions.py shows them equal)"""
    from scipy.ndimage import binary_dilation, binary_erosion
    s = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    b = np.asarray(label).astype('bool')
    assert b.ndim == 2
    out = lambda m: np.logical_xor(binary_erosion(m, iterations=1, structure=s), m)
    return np.logical_xor(out(b), out(binary_dilation(b, iterations=3, structure=s)))


@functools.lru_cache(maxsize=None)
def points_reference(name):
    lab = points_labels(name)
    r = np.stack([boundary_points_2d(v) if 1 in v.shape else weightmap_ref.boundary_points(v) for v in lab])
    r.setflags(write=False)
    return r
