"""GPU: the row kernels of the volume front end and the volume sampler at the regimes of tests/brick_rows_cases.py (the
plan: tests/test_brick_rows_plan.py).  Everything is BIT-EXACT against the feature tests' own numpy references: the kernels
copy, cast, or evaluate (r - m) / s once.  Whatever a kernel writes into a buffer of the caller's is written into a
sentinel-filled buffer with guard bands, at every offset from a 16-byte boundary the unit size allows, and the whole
buffer is compared: a 16-byte store that runs over into a neighbour's row or out of the array shows as a lost sentinel."""
import numpy as np
import pytest
import torch

from sequitr_amd.frontend import FrameTiler, VolumeSampler, VolumeTiler, volume_stats
from tests import brick_rows_cases as br
from tests import volume_frontend_cases as vc
from tests import volume_sampler_cases as sc
from tests.util import assert_bit_exact

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 64                                                      # elements on either side: whole 16-byte slots of any type
SENTINEL = {np.dtype(np.uint8): 255, np.dtype(np.uint16): 0xA5A5, np.dtype(np.float32): float('nan')}


def dev(a):
    return torch.from_numpy(np.array(a, order='C')).to(DEV)      # a copy: the shared inputs are read-only


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


class Guarded(object):
    """A sentinel-filled flat buffer and a contiguous view of `shape` that starts `lead` elements behind a 16-byte boundary,
    `guard` elements (a multiple of 16) from either end."""

    def __init__(self, shape, dtype, lead, guard=GUARD):
        self.dtype, self.shape, self.lead = np.dtype(dtype), tuple(shape), lead
        self.n, self.guard = int(np.prod(shape)), -(-guard // 16) * 16
        self.buf = dev(np.full(self.guard + lead + self.n + self.guard, SENTINEL[self.dtype], self.dtype))
        self.view = self.buf[self.guard + lead:self.guard + lead + self.n].view(self.shape)
        assert self.buf.data_ptr() % 16 == 0 and self.view.data_ptr() % 16 == (lead * self.dtype.itemsize) % 16
        assert self.view.is_contiguous()

    def blank(self):
        """the view's content before anything is written, on the host"""
        return np.full(self.shape, SENTINEL[self.dtype], self.dtype)

    def check(self, want, what):
        """the guards still hold the sentinel and the view holds `want`, bit for bit; returns the view's content"""
        host = self.buf.cpu().numpy()
        lo = self.guard + self.lead
        guards = bits(np.concatenate([host[:lo], host[lo + self.n:]]))
        sentinel = bits(np.full(1, SENTINEL[self.dtype], self.dtype))[0]
        if not (guards == sentinel).all():
            raise AssertionError("%s: %d guard elements were written" % (what, int((guards != sentinel).sum())))
        got = host[lo:lo + self.n].reshape(self.shape)
        same = bits(got) == bits(np.asarray(want, self.dtype))
        if not same.all():
            raise AssertionError("%s: %d of %d elements differ, first at %s" % (what, int((~same).sum()), same.size,
                                                                                  tuple(int(i) for i in np.argwhere(~same)[0])))
        return got


# ---- volume_to_bricks_kernel ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", br.DTYPES, ids=br._name)
@pytest.mark.parametrize("case", range(len(br.TO_BRICKS_CASES)), ids=br.TO_BRICKS_IDS)
def test_bricks_bit_exact_at_every_row_regime(case, dtype):
    brick, kind, shape = br.TO_BRICKS_CASES[case]
    vols = br.volume(shape, dtype)
    tl = VolumeTiler(shape[1:], brick, br.TO_BRICKS_MARGIN, device=DEV)
    total = shape[0] * tl.bricks_per_volume
    d = dev(vols)
    for normalise in (True, False):
        ref = vc.np_bricks(vols, tl.geometry, normalise)
        got = tl.bricks(d, normalise=normalise)
        assert tuple(got.shape) == (total,) + brick + (1,) and got.dtype == torch.float32
        assert_bit_exact(got.cpu().numpy(), ref, "%s, all bricks, normalise=%s" % (br.TO_BRICKS_IDS[case], normalise))
        stats = tl.stats(d) if normalise else None
        for first, count in ((0, 1), (1, max(total - 2, 1)), (total - 1, 1)):   # a ragged split: other rows meet other heads
            got = tl.bricks(d, first, count, normalise=normalise, stats=stats)
            assert_bit_exact(got.cpu().numpy(), ref[first:first + count], "bricks %d..+%d, normalise=%s" % (first, count, normalise))
        if kind == 'tail':                                      # the fill inside a row is exactly 0.0 in both modes
            assert not bits(ref)[..., shape[3]:, :].any() and not bits(got.cpu().numpy())[..., shape[3]:, :].any()


# ---- bricks_scatter_kernel --------------------------------------------------------------------------------------------
def check_scatter(case, dtype, offsets):
    shape, brick, margin, C = case
    tl = VolumeTiler(shape, brick, margin, device=DEV)
    g = tl.geometry
    total = br.SCATTER_V * g.per_volume
    tail = () if dtype == np.uint8 else (C,)
    values = br.masks((total,) + brick) if dtype == np.uint8 else br.logits((total,) + brick + tail)
    dvalues = dev(values)
    unit = np.dtype(dtype).itemsize
    vol_shape = (br.SCATTER_V,) + shape + tail
    for off in offsets:
        assert off % unit == 0
        # one brick alone: what lies outside its owned box, the guards included, keeps the sentinel
        for k in br.interior_bricks(shape, brick, margin):
            out = Guarded(vol_shape, dtype, off // unit)
            assert tl.scatter(dvalues[k:k + 1], out.view, first=k) is out.view
            want = vc.np_scatter(values[k:k + 1], out.blank(), g, first=k)
            _, lo, hi = g.box(k % g.per_volume)
            owned = np.zeros(vol_shape, bool)
            owned[k // g.per_volume, lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
            assert (bits(want)[~owned] == bits(out.blank())[~owned]).all() and owned.any() and not owned.all()
            out.check(want, "brick %d alone, out %d bytes behind a boundary" % (k, off))
        # all of them, batches forward and reversed
        batches = [(first, min(5, total - first)) for first in range(0, total, 5)]
        want = vc.np_scatter(values, np.full(vol_shape, SENTINEL[np.dtype(dtype)], dtype), g)
        assert not (bits(want) == bits(np.full(1, SENTINEL[np.dtype(dtype)], dtype))[0]).any()     # the boxes partition the volumes
        for order in (batches, batches[::-1]):
            out = Guarded(vol_shape, dtype, off // unit)
            for first, count in order:
                tl.scatter(dvalues[first:first + count], out.view, first)
            out.check(want, "all bricks, out %d bytes behind a boundary" % off)


@pytest.mark.parametrize("case", br.SCATTER_U8_CASES, ids=br._scatter_id)
def test_scatter_masks_into_a_guarded_volume(case):
    check_scatter(case, np.uint8, br.SCATTER_U8_OFFSETS)


@pytest.mark.parametrize("case", br.SCATTER_F32_CASES, ids=br._scatter_id)
def test_scatter_logits_into_a_guarded_volume(case):
    check_scatter(case, np.float32, br.SCATTER_F32_OFFSETS)


# ---- the sampler ------------------------------------------------------------------------------------------------------
def sampler_call(sm, kind, param, src, plan, stats=None):
    """out -> the sampler's call for this kind, writing into out"""
    if kind == 'images':
        return lambda out: sm.images(src, plan, stats=stats, out=out)
    if kind == 'copy':
        return lambda out: sm.copy(src, plan, out=out)
    return lambda out: sm.onehot(src, param, plan, out=out)


def check_sampler(kind, param, vol_shape, brick, plan, monkeypatch, offsets):
    """Every launch writes into a guarded buffer.  Its guards are as wide as the widest overrun a wrong row or tile bound
    could make -- a row, or for the square bricks a tile's 64 rows -- so that such a kernel fails here and nowhere else.
    The transposed ops of a square brick run on both paths: the LDS tiles (default) and, with SQ_SAMPLE_LDS=0 (read per
    launch), the direct gather."""
    src, ref = br.sampler_reference(kind, param, vol_shape, brick, plan)
    sm = VolumeSampler(vol_shape[1:], brick, DEV)
    dsrc, dplan = dev(src), dev(plan)
    call = sampler_call(sm, kind, param, dsrc, dplan, volume_stats(dsrc) if kind == 'images' else None)
    unit, K = br.sampler_unit(kind, param)
    per_elem = unit // ref.dtype.itemsize                       # 8-byte voxels are eight uint8 elements
    row = brick[2] * K * per_elem
    guard = (br.TILE if sm.square else 1) * row + GUARD
    for off in offsets:
        got = {}
        for path in ('lds', 'direct') if sm.square else ('rows',):
            out = Guarded(ref.shape, ref.dtype, off * per_elem, guard)
            if path == 'direct':
                monkeypatch.setenv('SQ_SAMPLE_LDS', '0')
            else:
                monkeypatch.delenv('SQ_SAMPLE_LDS', raising=False)
            try:
                assert call(out.view) is out.view
            finally:
                monkeypatch.delenv('SQ_SAMPLE_LDS', raising=False)
            got[path] = out.check(ref, "%s %s %s, out= %d units behind a boundary, %s" % (kind, param, brick, off, path))
        if sm.square:
            assert got['lds'].tobytes() == got['direct'].tobytes()
    return ref


@pytest.mark.parametrize("case", range(len(br.SAMPLER_ROW_CASES)), ids=br.SAMPLER_ROW_IDS)
def test_sampler_rows_into_guarded_buffers(case, monkeypatch):
    kind, param, brick = br.SAMPLER_ROW_CASES[case]
    shape = br.sampler_volume(brick)
    ref = check_sampler(kind, param, shape, brick, br.sampler_plan(shape, brick), monkeypatch, br.sampler_offsets(kind, param))
    if kind == 'onehot':                                        # labels >= C gave all-zero voxels inside the volume
        assert set(np.unique(ref)) == {0, 1} and ref.sum(-1).max() == 1
        assert (ref[0].sum(-1) == 0).any()                      # row 0: origin 0, no fill


def test_transposed_rows_of_two_lane_trips_through_the_direct_gather(monkeypatch):
    brick, shape = br.GATHER_BRICK, br.GATHER_VOLUME
    plan = br.sampler_plan(shape, brick, sc.TRANSPOSED, seed=1, random_rows=0)
    check_sampler('images', br.GATHER_DTYPE, shape, brick, plan, monkeypatch, (0, 1))


@pytest.mark.parametrize("case", range(len(br.TILE_CASES)), ids=br.TILE_IDS)
def test_sampler_tiles_exact_and_one_wide(case, monkeypatch):
    kind, param, B = br.TILE_CASES[case]
    shape, brick = br.tile_volume(B), (1, B, B)
    plan = br.sampler_plan(shape, brick, sc.TRANSPOSED, seed=B, random_rows=0)
    check_sampler(kind, param, shape, brick, plan, monkeypatch, br.sampler_offsets(kind, param)[:2])


# ---- the host's launch splitting --------------------------------------------------------------------------------------
_split = {}


def split_case():
    if not _split:
        shape = (br.SPLIT_V,) + br.SPLIT_VOLUME
        vols = br.volume(shape, np.uint8)
        tl = VolumeTiler(br.SPLIT_VOLUME, br.SPLIT_BRICK, br.SPLIT_MARGIN, device=DEV)
        total = br.SPLIT_V * tl.bricks_per_volume
        assert br.launches(total) == [(0, 65535), (65535, total - 65535)]
        _split.update(vols=vols, tl=tl, total=total, ref=vc.np_bricks(vols, tl.geometry, True))
    return _split


def test_bricks_of_more_than_one_launch():
    c = split_case()
    tl, d = c['tl'], dev(c['vols'])
    got = tl.bricks(d)
    assert tuple(got.shape) == (c['total'],) + br.SPLIT_BRICK + (1,)
    assert_bit_exact(got.cpu().numpy(), c['ref'], "%d bricks" % c['total'])
    got = tl.bricks(d, first=br.SPLIT_FIRST)
    assert_bit_exact(got.cpu().numpy(), c['ref'][br.SPLIT_FIRST:], "bricks from %d on" % br.SPLIT_FIRST)


@pytest.mark.parametrize("dtype,C", [(np.uint8, 1), (np.float32, 2)], ids=['uint8', 'float32-C2'])
def test_scatter_of_more_than_one_launch(dtype, C):
    c = split_case()
    tl, total = c['tl'], c['total']
    tail = () if dtype == np.uint8 else (C,)
    values = br.masks((total,) + br.SPLIT_BRICK) if dtype == np.uint8 else br.logits((total,) + br.SPLIT_BRICK + tail)
    vol_shape = (br.SPLIT_V,) + br.SPLIT_VOLUME + tail
    out = Guarded(vol_shape, dtype, 0)
    tl.scatter(dev(values), out.view)
    out.check(vc.np_scatter(values, out.blank(), tl.geometry), "%d bricks scattered" % total)
    out = Guarded(vol_shape, dtype, 0)                          # from brick 5 on: the first five boxes keep the sentinel
    tl.scatter(dev(values[br.SPLIT_FIRST:]), out.view, first=br.SPLIT_FIRST)
    out.check(vc.np_scatter(values[br.SPLIT_FIRST:], out.blank(), tl.geometry, first=br.SPLIT_FIRST), "from brick 5 on")


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=br._name)
def test_cast_of_more_than_one_launch(dtype):
    H, W = br.SPLIT_FRAME
    frames = br.volume((1, br.SPLIT_FRAMES, H, W), dtype, seed=9)[0]
    tiler = FrameTiler((H, W), tile=2, margin=0, device=DEV)
    got = tiler.to_f32(dev(frames))
    assert tuple(got.shape) == (br.SPLIT_FRAMES, H, W) and got.dtype == torch.float32
    assert_bit_exact(got.cpu().numpy(), frames.astype(np.float32), "%d frames cast" % br.SPLIT_FRAMES)
    out = Guarded((br.SPLIT_FRAMES, H, W), np.float32, 0)
    assert tiler.to_f32(dev(frames), out=out.view) is out.view
    out.check(frames.astype(np.float32), "cast into a guarded buffer")
