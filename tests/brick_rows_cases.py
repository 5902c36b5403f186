"""The row kernels of the volume front end (sq_volume_frontend.hip) and the volume sampler (sq_volume_sampler.hip) at every
regime of their launch arithmetic: the constants those regimes hang on, the arithmetic restated, the tables of cases, and
what the CPU plan test (tests/test_brick_rows_plan.py) and the GPU test (tests/test_gpu_brick_rows_sweep.py) share.

Both files stream rows the same way.  row_block(row_bytes) picks TX in {4, 8, 16, 32, 64} lanes along a row and 256 / TX
rows per block; a row of n units is written as a scalar head up to the first 16-byte boundary of its destination, a body
of nvec 16-byte stores in a `for (j = tx; j < nvec; j += TX)` lane loop, and a scalar tail.  A regime is a value of TX, of
the number of x groups, of the head, of the tail, of the number of trips a lane takes through the body.  Every function
below that names regimes returns a set of tags; the plan test holds each table to the set it must reach, and holds the
tables of the feature tests (tests/volume_frontend_cases.py, tests/volume_sampler_cases.py) to reaching none of them.

The references are the feature tests' own: volume_frontend_cases.np_bricks / np_scatter, volume_sampler_cases.np_images /
np_copy / np_onehot.  The kernels copy, cast, or evaluate (r - m) / s once, so every comparison is equality.
"""
import functools

import numpy as np

from sequitr_amd.frontend import volume_bricks
from tests import volume_frontend_cases as vc
from tests import volume_sampler_cases as sc

FE, SM, PY = 'sequitr_amd/csrc/sq_volume_frontend.hip', 'sequitr_amd/csrc/sq_volume_sampler.hip', 'sequitr_amd/frontend.py'
_ROW_BLOCK = {'TX_MIN': (r'unsigned tx = (\d+);', 4), 'TX_MAX': (r'while \(tx < (\d+) && tx < pieces\) tx \*= 2;', 64),
              'PIECE': (r'const int64_t pieces = \(row_bytes \+ 15\) / (\d+) \+ 1;', 16),
              'PIECE_ROUND': (r'const int64_t pieces = \(row_bytes \+ (\d+)\) / 16 \+ 1;', 15),
              'BLOCK': (r'return dim3\(tx, (\d+) / tx\);', 256)}
# name -> (file, regular expression whose group 1 is the value as the source writes it, value, places it stands in).  The
# plan test holds each to its source lines.
CONSTANTS = {}
for _tag, _path in (('FE', FE), ('SM', SM)):
    for _k, (_re, _v) in _ROW_BLOCK.items():
        CONSTANTS['%s_%s' % (_tag, _k)] = (_path, _re, _v, 1)
    CONSTANTS['%s_SLOT' % _tag] = (_path, r'\(\(\((\d+)u - \(unsigned\)\(\(uintptr_t\)p & 15u\)\) & 15u\) / sizeof\(E\)\)', 16, 1)
    CONSTANTS['%s_SLOT_MASK' % _tag] = (_path, r'\(\(\(16u - \(unsigned\)\(\(uintptr_t\)p & (\d+)u\)\) & 15u\) / sizeof\(E\)\)', 15, 1)
    CONSTANTS['%s_MAX_COUNT' % _tag] = (_path, r'SQ_REQUIRE\(count > 0 && count <= (\d+),', 65535, 1)
CONSTANTS.update({
    'FE_VECTOR': (FE, r'constexpr int VE = (\d+) / sizeof\(E\);', 16, 1),
    'SM_VECTOR': (SM, r'constexpr int VE = (\d+) / sizeof\(U\);', 16, 1),
    'TILE': (SM, r'constexpr int TILE = (\d+);', 64, 1),
    'TILE_ROWS': (SM, r'dim3\(nt \* nt, g\.BZ, count\), dim3\(TILE, (\d+)\)', 4, 1),
    'PY_CAST_STEP': (PY, r'for lo in range\(0, F, (\d+)\):', 65535, 1),
    'PY_CAST_TAKE': (PY, r'n = min\((\d+), F - lo\)', 65535, 1),
    'PY_BRICK_STEP': (PY, r'for lo in range\(0, count, (\d+)\):', 65535, 2),          # VolumeTiler.bricks and .scatter
    'PY_BRICK_TAKE': (PY, r'n = min\((\d+), count - lo\)', 65535, 2),
})
TX_MIN, TX_MAX, PIECE, BLOCK = (CONSTANTS['FE_' + k][2] for k in ('TX_MIN', 'TX_MAX', 'PIECE', 'BLOCK'))
TILE, TILE_ROWS, MAX_COUNT = CONSTANTS['TILE'][2], CONSTANTS['TILE_ROWS'][2], CONSTANTS['FE_MAX_COUNT'][2]
TXS = (4, 8, 16, 32, 64)

DTYPES = (np.uint8, np.uint16, np.float32)


def _name(dtype):
    return np.dtype(dtype).name


# ---- the launch arithmetic, restated ----------------------------------------------------------------------------------
def row_block(row_bytes):
    """(TX lanes along a row, rows per block): TX the power of two that covers the row's 16-byte pieces and one more"""
    pieces = (row_bytes + PIECE - 1) // PIECE + 1
    tx = TX_MIN
    while tx < TX_MAX and tx < pieces:
        tx *= 2
    return tx, BLOCK // tx


def row_split(dst_byte, unit, n):
    """(head, nvec, tail) of a row of n units of `unit` bytes whose destination starts dst_byte bytes behind a 16-byte
    boundary: head_elems / head_units, the 16-byte body, the rest"""
    head = min(((PIECE - dst_byte % PIECE) % PIECE) // unit, n)
    nvec = (n - head) // (PIECE // unit)
    return head, nvec, n - head - nvec * (PIECE // unit)


def lane_trips(nvec, tx):
    """trips of the busiest lane through `for (j = tx; j < nvec; j += TX)`"""
    return -(-nvec // tx)


def x_groups(rows_wanted, rows_per_block):
    """(x groups that hold a row, rows of the last one)"""
    groups = -(-rows_wanted // rows_per_block)
    return groups, rows_wanted - (groups - 1) * rows_per_block


def tile_grid(B):
    """(LDS tiles along an axis of a B x B plane, width of the last one)"""
    nt = -(-B // TILE)
    return nt, B - (nt - 1) * TILE


def split_tags(dst_bytes, n, unit, tx):
    """the regimes of rows whose destinations start at dst_bytes (an array) and hold n units each (an array or one number)"""
    d = np.asarray(dst_bytes, np.int64).ravel()
    ns = np.broadcast_to(np.asarray(n, np.int64).ravel(), d.shape)
    tags = set()
    for db, nn in set(zip((d % PIECE).tolist(), ns.tolist())):
        head, nvec, tail = row_split(db, unit, nn)
        assert nvec == 0 or (db + head * unit) % PIECE == 0     # the body's stores are aligned
        tags |= {'head=%d' % head, 'trips=%d' % lane_trips(nvec, tx), 'nvec=%d' % nvec}
        if nvec:
            tags |= {'head=%d+body' % head, 'tail=%d+body' % tail}
            if tail:
                tags.add('tail>0+body')
    return tags


def group_tags(rows_wanted, rows_per_block):
    groups, last = x_groups(rows_wanted, rows_per_block)
    tags = {'groups=1' if groups == 1 else 'groups>=2'}
    if groups >= 2 and last < rows_per_block:
        tags.add('last_group=partial')
    return tags


HEADS_WITH_BODY = {unit: {'head=%d+body' % h for h in range(PIECE // unit)} for unit in (1, 2, 4, 8)}


# ---- volume_to_bricks_kernel ------------------------------------------------------------------------------------------
# rows of BY floats.  Every brick runs on two volume shapes: `rows`, with X shorter than the brick (rows of pure fill), two
# bricks along z and at least two along y (a source row is read from oy > 0); `tail`, with Y shorter than the brick, so that
# a row inside the volume ends in fill -- in the second and third lane trip of the wide bricks.
TO_BRICKS_BRICKS = [(2, 70, 5), (2, 20, 27), (2, 10, 61), (2, 5, 131), (1, 5, 263), (1, 3, 519), (2, 20, 45)]
TO_BRICKS_MARGIN = (0, 1, 2)


def to_bricks_volumes(brick):
    BZ, BX, BY = brick
    return {'rows': (2, BZ + 1, BX - 1, BY + 7), 'tail': (1, BZ, BX + 1, BY - BY // 3)}


TO_BRICKS_CASES = [(brick, kind, shape) for brick in TO_BRICKS_BRICKS for kind, shape in sorted(to_bricks_volumes(brick).items())]
TO_BRICKS_IDS = ['%dx%dx%d-%s' % (b + (k,)) for b, k, _ in TO_BRICKS_CASES]


def to_bricks_tags(shape, brick, margin, first=0, count=None):
    """regimes of one launch of volume_to_bricks_kernel: bricks first .. first+count-1 into a fresh, 16-byte aligned out"""
    V, (Z, X, Y), (BZ, BX, BY) = shape[0], shape[1:], brick
    g = volume_bricks(shape[1:], brick, margin)
    count = V * g.per_volume - first if count is None else count
    tx, rows = row_block(BY * 4)
    tags = {'TX=%d' % tx} | group_tags(BX, rows)
    tags |= split_tags(np.arange(count * BZ * BX, dtype=np.int64) * BY * 4, BY, 4, tx)
    ve_reach = 4 + 4 * tx                                       # past any head and one whole trip of the body
    for bl in range(count):
        (oz, ox, oy), _, _ = g.box((first + bl) % g.per_volume)
        if oz + BZ > Z or ox + BX > X:
            tags.add('fill_row')
        if oy > 0:
            tags.add('oy>0')
        if oy + BY > Y and oz < Z and ox < X:
            tags.add('row_fill')
            if BY > ve_reach:                                   # the fill runs to the end of the row
                tags.add('row_fill@trip>=2')
    return tags


TO_BRICKS_NEW = ({'TX=%d' % t for t in (4, 16, 32, 64)} | {'groups>=2', 'last_group=partial', 'trips=2', 'trips=3',
                 'tail>0+body', 'row_fill', 'row_fill@trip>=2'} | (HEADS_WITH_BODY[4] - {'head=0+body'}))
TO_BRICKS_NEEDED = ({'TX=%d' % t for t in TXS} | {'groups=1', 'groups>=2', 'last_group=partial', 'trips=1', 'trips=2', 'trips=3',
                    'tail>0+body', 'fill_row', 'row_fill', 'row_fill@trip>=2', 'oy>0'} | HEADS_WITH_BODY[4])


# ---- bricks_scatter_kernel --------------------------------------------------------------------------------------------
# (volume (Z, X, Y), brick, margin, C); two volumes each.  `offsets`: out is also a contiguous view that many BYTES into a
# larger buffer.
SCATTER_V = 2
SCATTER_U8_CASES = [((3, 9, 150), (2, 4, 131), (0, 1, 3), 1), ((3, 9, 2300), (2, 4, 1100), (0, 1, 8), 1),
                    ((2, 70, 23), (2, 66, 9), (0, 1, 2), 1)]
SCATTER_U8_OFFSETS = (0, 1, 7, 13)
SCATTER_F32_CASES = [((3, 6, 300), (2, 4, 270), (0, 1, 2), 1), ((3, 6, 100), (2, 4, 90), (0, 1, 2), 3),
                     ((2, 5, 700), (2, 3, 530), (0, 0, 1), 1), ((2, 70, 23), (2, 66, 9), (0, 1, 2), 1),
                     ((3, 6, 21), (2, 4, 9), (0, 1, 2), 2), ((3, 6, 21), (2, 4, 9), (0, 1, 2), 5),
                     ((3, 6, 21), (2, 4, 9), (0, 1, 2), 8), ((3, 6, 21), (2, 4, 9), (0, 1, 2), 64)]
SCATTER_F32_OFFSETS = (0, 4, 8, 12)
SCATTER_MAX_C = 64


def _scatter_id(case):
    shape, brick, _, C = case
    return '%dx%dx%d-brick%dx%dx%d-C%d' % (shape + brick + (C,))


def scatter_tags(shape, brick, margin, C, unit, offset=0, V=SCATTER_V):
    """regimes of bricks_scatter_kernel over every brick of V volumes of `shape`; out starts `offset` bytes behind a
    16-byte boundary"""
    Z, X, Y = shape
    g = volume_bricks(shape, brick, margin)
    tx, rows = row_block(brick[2] * C * unit)
    tags = {'TX=%d' % tx}
    for v in range(V):
        for k in range(g.per_volume):
            _, (lz, lx, ly), (hz, hx, hy) = g.box(k)
            tags |= group_tags(hx - lx, rows)
            gz, gx = np.meshgrid(np.arange(lz, hz), np.arange(lx, hx), indexing='ij')
            dst = ((((v * Z + gz) * X + gx) * Y + ly) * C) * unit + offset
            tags |= split_tags(dst, (hy - ly) * C, unit, tx)
    return tags


def interior_bricks(shape, brick, margin, V=SCATTER_V):
    """the first, the last and one interior brick of the stack"""
    total = V * volume_bricks(shape, brick, margin).per_volume
    return sorted({0, total // 2, total - 1})


SCATTER_U8_NEW = ({'TX=16', 'TX=64', 'groups>=2', 'trips=2', 'tail>0+body'} | (HEADS_WITH_BODY[1] - {'head=0+body'}))
SCATTER_U8_NEEDED = {'TX=4', 'TX=16', 'TX=64', 'groups=1', 'groups>=2', 'last_group=partial', 'trips=0', 'trips=1', 'trips=2',
                     'tail>0+body'} | HEADS_WITH_BODY[1]
SCATTER_F32_NEW = {'TX=4', 'TX=32', 'TX=64', 'groups>=2', 'trips=2', 'trips=3'}
SCATTER_F32_NEEDED = {'TX=4', 'TX=32', 'TX=64', 'groups=1', 'groups>=2', 'last_group=partial', 'trips=1', 'trips=2', 'trips=3',
                      'tail>0+body', 'nvec=67', 'nvec=66', 'nvec=132'} | HEADS_WITH_BODY[4]


# ---- sample_rows_kernel -----------------------------------------------------------------------------------------------
# (kind, parameter, brick): kind 'images' with a voxel type, 'copy' with the voxel's bytes, 'onehot' with the class count.
# The bricks are not square in the plane, so the Python layer sends allow_transpose = 0 and every op is a flip on the row
# path.  The row's bytes decide TX: <= 48 is 4, <= 112 is 8, <= 240 is 16, <= 496 is 32, above is 64; two trips of the body
# take more than 64 + 1 stores.  An odd row length walks the rows through every head; the out= views add the rest.
SAMPLER_V, SAMPLER_Z = 2, 3
COPY_SOURCES = {1: (np.uint8, ()), 2: (np.uint16, ()), 3: (np.uint8, (3,)), 4: (np.float32, (1,)), 8: (np.uint8, (8,))}
SAMPLER_ROW_CASES = [
    ('images', np.uint8, (2, 70, 5)), ('images', np.uint16, (2, 33, 27)), ('images', np.float32, (2, 17, 45)),
    ('images', np.uint8, (2, 10, 61)), ('images', np.uint16, (2, 5, 131)), ('images', np.float32, (2, 5, 263)),
    ('copy', 4, (2, 33, 27)), ('copy', 4, (2, 5, 263)),
    ('copy', 1, (2, 70, 37)), ('copy', 1, (2, 33, 99)), ('copy', 1, (2, 17, 201)), ('copy', 1, (2, 10, 301)),
    ('copy', 1, (2, 5, 1061)),
    ('copy', 3, (2, 70, 13)), ('copy', 3, (2, 5, 355)),
    ('copy', 2, (2, 5, 531)),
    ('copy', 8, (2, 70, 5)), ('copy', 8, (2, 33, 13)), ('copy', 8, (2, 17, 29)), ('copy', 8, (2, 10, 61)), ('copy', 8, (2, 5, 131)),
    ('onehot', 1, (2, 33, 99)), ('onehot', 5, (2, 5, 213)), ('onehot', 7, (2, 10, 43)), ('onehot', 16, (2, 17, 13)),
    ('onehot', 16, (2, 5, 67)),
]
SAMPLER_ROW_IDS = ['%s-%s-%dx%dx%d' % ((k, _name(p) if k == 'images' else p) + b) for k, p, b in SAMPLER_ROW_CASES]
ONEHOT_LABELS = 18                                              # labels 0 .. 17: labels >= C are present for every C <= 16


def sampler_unit(kind, param):
    """(bytes of an output unit, units per voxel)"""
    if kind == 'images':
        return 4, 1
    if kind == 'onehot':
        return 1, param
    return (1, 3) if param == 3 else (param, 1)


def sampler_offsets(kind, param):
    """where the out= views start, in UNITS behind a 16-byte boundary: with the rows' own walk, every head of the unit size"""
    unit = sampler_unit(kind, param)[0]
    return {1: (0, 1, 7, 13), 2: (0, 1, 3, 7), 4: (0, 1, 2, 3), 8: (0, 1)}[unit]


def sampler_volume(brick):
    return (SAMPLER_V, SAMPLER_Z, brick[1] + 2, brick[2] + 3)


def carry_positions(start, K):
    """the positions u of a 16-unit vector that starts at unit `start` of a row at which `++sub == K` carries"""
    return {u for u in range(PIECE) if (start + u + 1) % K == 0}


def sampler_row_tags(kind, param, brick, count, offset=0):
    """regimes of sample_rows_kernel over `count` bricks; out starts `offset` units behind a 16-byte boundary"""
    unit, K = sampler_unit(kind, param)
    BZ, BX, BY = brick
    n = BY * K
    tx, rows = row_block(n * unit)
    tags = {'TX=%d' % tx, 'unit=%d' % unit} | group_tags(BX, rows)
    dst = (np.arange(count * BZ * BX, dtype=np.int64) * n + offset) * unit
    tags |= split_tags(dst, n, unit, tx)
    if kind == 'onehot':
        tags.add('C=%d' % K)
        voxels = set()
        for db in set((dst % PIECE).tolist()):
            head, nvec, _ = row_split(db, 1, n)
            for j in range(nvec):
                start = head + PIECE * j
                tags |= {'C=%d,carry@%d' % (K, u) for u in carry_positions(start, K)}
                voxels.add(len({(start + u) // K for u in range(PIECE)}))
        tags |= {'C=%d,voxels/vector=%d' % (K, v) for v in voxels}
    return tags


def sampler_plan(vol_shape, brick, ops=sc.FLIPS, seed=0, random_rows=2):
    """volume_sampler_cases.case_plan's rows -- both extreme origins under every op, plus random rows -- and, under every
    op, a box that straddles the y end of the volume from half its width on and one that straddles the x and y starts: on
    the wide bricks the fill inside a row meets the second lane trip (the first, under a y flip)"""
    plan = sc.case_plan(vol_shape, brick, ops, seed)
    if random_rows < 2:
        keep = np.concatenate([np.arange(5 * i, 5 * i + 3 + random_rows) for i in range(len(ops))])
        plan = plan[keep]
    V, (Z, X, Y) = vol_shape[0], vol_shape[1:]
    extra = []
    for op in ops:
        extra.append([V - 1, 0, 0, Y - brick[2] // 2 - 1, op])
        extra.append([0, max(Z - brick[0], 0), -1, -(brick[2] // 2), op])
    return np.concatenate([plan, np.asarray(extra, np.int32)])


def plan_fill_tags(plan, vol_shape, brick, unit, K, opmask):
    """'row_fill' when a row that lies inside the volume holds fill, 'row_fill@trip>=2' when some of it lies past any head
    and one whole trip of the body"""
    Z, X, Y = vol_shape[1:]
    BZ, BX, BY = brick
    tx = row_block(BY * K * unit)[0]
    reach = (PIECE // unit) * (tx + 1)                          # units: a head is shorter than one vector
    tags = set()
    for v, oz, ox, oy, op in plan.tolist():
        op &= opmask
        if op & 8 or not (0 <= v < vol_shape[0] and oz < Z and oz + BZ > 0 and ox < X and ox + BX > 0):
            continue
        y = np.arange(BY)
        src = oy + (BY - 1 - y if op & 4 else y)
        fill = (src < 0) | (src >= Y)
        if fill.any() and not fill.all():
            tags.add('row_fill')
            if fill[-(-reach // K):].any():
                tags.add('row_fill@trip>=2')
    return tags


SAMPLER_UNITS = (1, 4, 8)
# what the feature tests run (tests/test_gpu_volume_sampler.py): images on every IMAGE_CASES brick and on BIG_TILE_CASE, copies
# and one-hot on three of them.  The 70-float rows of BIG_TILE_CASE are TX = 32, but under transposed ops only: rows of the
# direct gather.  No plain or flipped row is that long.
OLD_SAMPLER_CASES = ([('images', np.uint16, b, ops) for b, ops in sc.IMAGE_CASES + [sc.BIG_TILE_CASE]]
                     + [('copy', 3, sc.BIG_TILE_CASE[0], sc.BIG_TILE_CASE[1]), ('onehot', 2, sc.BIG_TILE_CASE[0], sc.BIG_TILE_CASE[1])]
                     + [('copy', n, b, ops) for n in COPY_SOURCES for b, ops in (sc.IMAGE_CASES[i] for i in (0, 1, 4))]
                     + [('onehot', C, b, ops) for C in (1, 2, 3) for b, ops in (sc.IMAGE_CASES[i] for i in (0, 1, 4))])
SAMPLER_NEW = {'TX=64', 'trips=2', 'C=16', 'C=5', 'C=7'}
SAMPLER_NEW_ON_PLAIN_ROWS = {'TX=32'}
SAMPLER_PER_UNIT = {'TX=%d' % t for t in TXS} | {'groups>=2', 'last_group=partial', 'trips=1', 'trips=2', 'tail>0+body'}
SAMPLER_ONEHOT_NEEDED = ({'C=%d' % c for c in (1, 5, 7, 16)} | {'C=%d,carry@%d' % (c, u) for c in (1, 5, 7) for u in range(16)}
                         | {'C=16,voxels/vector=1', 'C=16,voxels/vector=2', 'C=16,carry@15'})

# the transposed ops through the direct gather (SQ_SAMPLE_LDS=0): float32 rows of 263 voxels read Y apart, two lane trips;
# the same bricks through the LDS tiles are a 5 x 5 grid whose last tiles are 7 wide
GATHER_BRICK, GATHER_VOLUME, GATHER_DTYPE = (1, 263, 263), (1, 2, 270, 266), np.float32

# ---- sample_tiles_kernel ----------------------------------------------------------------------------------------------
TILE_SIDES = (64, 65, 128)
TILE_KINDS = [('images', np.uint16), ('copy', 8), ('onehot', 16)]
TILE_CASES = [(kind, param, B) for B in TILE_SIDES for kind, param in TILE_KINDS]
TILE_IDS = ['%s-%s-B%d' % (k, _name(p) if k == 'images' else p, B) for k, p, B in TILE_CASES]


def tile_volume(B):
    return (2, 2, B + 3, B + 2)


def tile_tags(B, K):
    nt, last = tile_grid(B)
    tags = {'grid=%dx%d,last=%s' % (nt, nt, 'whole' if last == TILE else last), 'last=%s' % ('whole' if last == TILE else last)}
    tags.add('unit_trips=%d' % -(-min(TILE, B) * K // TILE))    # trips of the `k += TILE` loop over a whole tile's row
    return tags


TILE_NEW = {'last=whole', 'last=1', 'unit_trips=16'}
TILE_NEEDED = {'grid=1x1,last=whole', 'grid=2x2,last=whole', 'grid=2x2,last=1', 'unit_trips=1', 'unit_trips=16'}

# ---- the host's launch splitting --------------------------------------------------------------------------------------
# 2 x 33792 bricks of (1, 2, 3): the second launch starts at brick 65535, inside the second volume
SPLIT_VOLUME, SPLIT_BRICK, SPLIT_MARGIN, SPLIT_V, SPLIT_FIRST = (48, 64, 66), (1, 2, 3), 0, 2, 5
SPLIT_FRAMES, SPLIT_FRAME = MAX_COUNT + 2 + 3, (2, 3)


def launches(count):
    """[(lo, n)] of the host loops: `for lo in range(0, count, 65535)`, n = min(65535, count - lo)"""
    return [(lo, min(MAX_COUNT, count - lo)) for lo in range(0, count, MAX_COUNT)]


# ---- inputs: made once, read only -------------------------------------------------------------------------------------
def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def volume(shape, dtype, seed=3):
    """(V, Z, X, Y) raw volumes of volume_frontend_cases.random_volume's kind"""
    return _frozen(vc.random_volume(shape, np.dtype(dtype), seed))


@functools.lru_cache(maxsize=None)
def normalised(shape, dtype, normalise, seed=3):
    return _frozen(sc.np_normalised(volume(shape, dtype, seed), normalise))


@functools.lru_cache(maxsize=None)
def copy_source(shape, nbytes, seed=0):
    """(V, Z, X, Y[, C]) voxels of nbytes bytes, no byte pattern favoured: a zero voxel is as rare as any other"""
    dtype, tail = COPY_SOURCES[nbytes]
    rng = np.random.default_rng(100 + nbytes + seed)
    if dtype == np.float32:
        return _frozen(rng.standard_normal(shape + tail).astype(np.float32))
    return _frozen(rng.integers(1, np.iinfo(dtype).max, shape + tail, endpoint=True).astype(dtype))


@functools.lru_cache(maxsize=None)
def labels(shape, seed=0):
    return _frozen(np.random.default_rng(200 + seed).integers(0, ONEHOT_LABELS, shape).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def masks(shape, seed=0):
    """uint8 brick values 0 .. 199: the sentinel 255 is none of them"""
    return _frozen(np.random.default_rng(300 + seed).integers(0, 200, shape).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def logits(shape, seed=0):
    return _frozen(np.random.default_rng(400 + seed).standard_normal(shape).astype(np.float32))


def sampler_reference(kind, param, vol_shape, brick, plan):
    """(source array, reference bricks) of one sampler case, by volume_sampler_cases' restatement; images normalised"""
    if kind == 'images':
        vols = volume(vol_shape, param)
        return vols, sc.np_images(vols, plan, brick, normalised=normalised(vol_shape, param, True))
    if kind == 'copy':
        src = copy_source(vol_shape, param)
        return src, sc.np_copy(src, plan, brick)
    lab = labels(vol_shape)
    return lab, sc.np_onehot(lab, param, plan, brick)


# ---- brute force: the definitions voxel by voxel, for the smallest cases ----------------------------------------------
def loop_bricks(vols, geometry, normalise):
    BZ, BX, BY = geometry.brick
    V, Z, X, Y = vols.shape
    out = np.zeros((V * geometry.per_volume, BZ, BX, BY, 1), np.float32)
    for v in range(V):
        f = vc.reference_cast(vols[v])
        mean, std = vc.np_stats(vols[v])
        for k in range(geometry.per_volume):
            oz, ox, oy = geometry.box(k)[0]
            for z in range(BZ):
                for x in range(BX):
                    for y in range(BY):
                        if oz + z < Z and ox + x < X and oy + y < Y:
                            r = f[oz + z, ox + x, oy + y]
                            out[v * geometry.per_volume + k, z, x, y, 0] = (r - mean) / (1e-99 + std) if normalise else r
    return out


def loop_scatter(values, out, geometry, first=0):
    for j in range(len(values)):
        v, k = divmod(first + j, geometry.per_volume)
        (oz, ox, oy), lo, hi = geometry.box(k)
        for gz in range(lo[0], hi[0]):
            for gx in range(lo[1], hi[1]):
                for gy in range(lo[2], hi[2]):
                    out[v, gz, gx, gy] = values[j, gz - oz, gx - ox, gy - oy]
    return out


def loop_sample(arr, plan, brick, fill=0):
    """out voxel (z, x, y) of a row is box voxel (fz(z), a, b), (a, b) = (fx(x), fy(y)) or, transposed, (fy(y), fx(x))"""
    BZ, BX, BY = brick
    V, Z, X, Y = arr.shape[:4]
    out = np.full((len(plan), BZ, BX, BY) + arr.shape[4:], fill, arr.dtype)
    for r, (v, oz, ox, oy, op) in enumerate(plan.tolist()):
        for z in range(BZ):
            for x in range(BX):
                for y in range(BY):
                    fz, fx, fy = (BZ - 1 - z if op & 1 else z), (BX - 1 - x if op & 2 else x), (BY - 1 - y if op & 4 else y)
                    a, b = (fy, fx) if op & 8 else (fx, fy)
                    gz, gx, gy = oz + fz, ox + a, oy + b
                    if 0 <= v < V and 0 <= gz < Z and 0 <= gx < X and 0 <= gy < Y:
                        out[r, z, x, y] = arr[v, gz, gx, gy]
    return out
