"""GPU: sq_mask_morph_u8, sq_mask_fill_holes_u8, sq_mask_clear_border_u8 and MaskCleanup against the scipy restatement of
include/sequitr_hip.h (tests/mask_cleanup_cases.py).  Every comparison is exact."""
import numpy as np
import pytest
import torch

from sequitr_amd import maskops, volumeops
from tests import mask_cleanup_cases as mc
from tests import objects_cases as oc

pytestmark = pytest.mark.gpu
TILE = maskops.MORPH_TILE
RMAX = maskops.MORPH_MAX_ITER
ALL = [(op, st) for op in mc.OPS for st in mc.STRUCTURES]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_morph(mask, C, radii=(1, 2, 3), pairs=ALL):
    d = dev(mask)
    for op, st in pairs:
        for r in radii:
            got = maskops.morph(d, op, r, st, classes=C).cpu().numpy()
            want = mc.morph_ref(mask, op, r, st, C)
            assert np.array_equal(got, want), "%s %s r=%d C=%d %s: %d pixels differ" % (op, st, r, C, mask.shape,
                                                                                      int((got != want).sum()))
    assert np.array_equal(d.cpu().numpy(), mask)                # the input is not written


@pytest.mark.parametrize("shape", mc.morph_shapes(TILE), ids=lambda s: "%dx%dx%d" % s)
def test_morph_shapes(shape):
    N, H, W = shape
    C = (2, 3, 5)[(H + W) % 3]
    check_morph(mc.random_mask(H * 1000 + W, N, H, W, C, (0.3, 0.5, 0.9)[(H * 7 + W) % 3]), C)


@pytest.mark.parametrize("C", [2, 3, 5])
@pytest.mark.parametrize("density", [0.3, 0.5, 0.9])
def test_morph_random_masks_over_several_tiles(C, density):
    check_morph(mc.random_mask(C * 10 + int(density * 10), 3, TILE[0] + 9, TILE[1] + 13, C, density), C)
    check_morph(mc.random_mask(C, 1, 2 * TILE[0] + 1, 130, C, density, unknown=False), C, radii=(2,))


@pytest.mark.parametrize("op,st", ALL)
def test_morph_largest_radius_over_two_tiles_each_way(op, st):
    m = np.concatenate([mc.random_mask(1, 1, TILE[0] + 36, TILE[1] + 108, 3, 0.97),
                        mc.random_mask(2, 1, TILE[0] + 36, TILE[1] + 108, 3, 0.03),
                        oc.disks(3, 1, TILE[0] + 36, TILE[1] + 108, 14, classes=2, rmax=40)])
    check_morph(m, 3, radii=(RMAX,), pairs=[(op, st)])


def test_morph_structures_on_the_tile_seams():
    check_morph(mc.seams(TILE), 2, radii=(1, 2, 3, 5))
    check_morph(np.concatenate([mc.seams(TILE, 2), mc.seams(TILE, 1)]), 3, radii=(4,))
    check_morph(mc.seams(TILE), 2, radii=(RMAX,), pairs=[("open", "cross"), ("close", "square")])


def test_morph_frame_edges_and_uniform_frames():
    check_morph(mc.flush(), 2, radii=(1, 3, 7))
    check_morph(np.zeros((2, 40, 70), np.uint8), 2, radii=(1, RMAX))
    check_morph(np.ones((2, 40, 70), np.uint8), 2, radii=(1, 4, RMAX))
    check_morph(np.ones((1, TILE[0] + 3, TILE[1] + 5), np.uint8), 2, radii=(2, RMAX))
    check_morph(np.full((1, 9, 10), 4, np.uint8), 5, radii=(1, 5))
    check_morph(np.full((1, 9, 10), 200, np.uint8), 3, radii=(1,))       # no class at all: copied through


def test_morph_frames_smaller_than_the_halo():
    for h, w in ((5, 7), (1, 9), (3, 3), (6, 1)):
        check_morph(mc.random_mask(h * w, 2, h, w, 3, 0.8), 3, radii=(3, 8, RMAX))


def test_morph_refuses_views_and_leaves_the_guard_alone():
    mask = mc.random_mask(9, 2, 37, 66, 3, 0.6)
    d = dev(mask)
    with pytest.raises(ValueError, match="contiguous"):
        maskops.morph(d[:, :, :50], "open", classes=3)           # the binding refuses a view: pass a packed copy
    packed = d[:, :, :50].contiguous()
    assert np.array_equal(maskops.morph(packed, "open", classes=3).cpu().numpy(), mc.morph_ref(mask[:, :, :50], "open", 1, "cross", 3))
    with pytest.raises(ValueError, match="planar"):
        maskops.morph(d[None], "open", classes=3)
    n = mask.size
    for off in (16, 13):                                        # 13: out is not 4-byte aligned, the byte path
        for src, ref in ((d, mask), (packed, mask[:, :, :50])):
            k = ref.size
            buf = torch.full((k + 64,), 0xAB, dtype=torch.uint8, device="cuda")
            out = buf[off:off + k].view(ref.shape)
            got = maskops.morph(src, "close", 2, "square", classes=3, out=out)
            assert got is out and np.array_equal(out.cpu().numpy(), mc.morph_ref(ref, "close", 2, "square", 3))
            guard = buf.cpu().numpy()
            assert np.all(guard[:off] == 0xAB) and np.all(guard[off + k:] == 0xAB)
    assert n == d.numel()
    buf = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
    buf[:n] = d.reshape(-1)
    with pytest.raises(maskops._lib.SequitrHipError, match="overlap"):
        maskops.morph(buf[:n].view(mask.shape), "erode", classes=3, out=buf[8:8 + n].view(mask.shape))


@pytest.mark.parametrize("case", mc.fill_cases(), ids=lambda c: c[0])
def test_fill_holes(case):
    name, mask, C, areas = case
    d = dev(mask)
    for a in areas:
        got = maskops.fill_holes(d, a, classes=C)
        want = mc.fill_holes_ref(mask, a, C)
        assert np.array_equal(got.cpu().numpy(), want), "%s max_area=%r: %d pixels differ" % (name, a, int((got.cpu().numpy() != want).sum()))
        again = maskops.fill_holes(d, a, classes=C)
        assert torch.equal(got, again)
    assert np.array_equal(d.cpu().numpy(), mask)


@pytest.mark.parametrize("case", mc.border_cases(), ids=lambda c: c[0])
def test_clear_border(case):
    name, mask, C = case
    d = dev(mask)
    got = maskops.clear_border(d, classes=C)
    want = mc.clear_border_ref(mask, C)
    assert np.array_equal(got.cpu().numpy(), want), "%s: %d pixels differ" % (name, int((got.cpu().numpy() != want).sum()))
    assert torch.equal(got, maskops.clear_border(d, classes=C)) and np.array_equal(d.cpu().numpy(), mask)
    # a frame is a volume of one plane whose border is its four lateral faces
    assert torch.equal(got, volumeops.clear_border3d(d[:, None].contiguous(), "lateral", classes=C)[:, 0])
    if name == "one row":
        assert not got.any()                                    # every pixel of a one-row frame is on the edge


def test_component_ops_guard_and_default_classes():
    mask = np.concatenate([oc.disks(8, 2, 45, 67, 12, classes=2), mc.random_mask(3, 1, 45, 67, 3, 0.7, unknown=False)])
    d = dev(mask)
    k = mask.size
    for fn, ref in ((lambda o: maskops.fill_holes(d, 6, out=o), mc.fill_holes_ref(mask, 6, 3)),
                    (lambda o: maskops.clear_border(d, out=o), mc.clear_border_ref(mask, 3))):
        buf = torch.full((k + 64,), 0xAB, dtype=torch.uint8, device="cuda")
        out = buf[13:13 + k].view(mask.shape)                   # unaligned: the kernel that copies the mask stays inside k bytes
        assert fn(out) is out and np.array_equal(out.cpu().numpy(), ref)   # classes default to the largest byte + 1
        guard = buf.cpu().numpy()
        assert np.all(guard[:13] == 0xAB) and np.all(guard[13 + k:] == 0xAB)
    zero = torch.zeros((1, 5, 6), dtype=torch.uint8, device="cuda")
    assert not maskops.fill_holes(zero).any() and not maskops.clear_border(zero).any() and not maskops.morph(zero, "dilate").any()


def test_morph_twice_is_bit_identical():
    d = dev(mc.random_mask(77, 3, TILE[0] + 9, TILE[1] + 13, 5, 0.6))
    for op, st in ALL:
        assert torch.equal(maskops.morph(d, op, 3, st, classes=5), maskops.morph(d, op, 3, st, classes=5))


def test_mask_cleanup_apply_is_the_steps_in_sequence():
    steps = [{"op": "open", "iterations": 2, "structure": "cross"}, {"op": "fill_holes", "max_area": 40}, {"op": "clear_border"}]
    mcl = maskops.MaskCleanup(steps)
    mask = np.concatenate([oc.disks(11, 2, 90, 200, 40, classes=2, rmax=14), mc.random_mask(12, 1, 90, 200, 3, 0.75)])
    mask[:2][mc.random_mask(13, 2, 90, 200, 2, 0.04, unknown=False) > 0] = 0        # pepper the disks with holes
    d = dev(mask)
    got = mcl.apply(d, 3)
    want = mc.steps_ref(mask, steps, 3)
    assert np.array_equal(got.cpu().numpy(), want) and (want != mask).any() and np.array_equal(d.cpu().numpy(), mask)
    buffers = {k: tuple(t.data_ptr() for t in v if t is not None) for k, v in mcl._cache.items()}
    again = mcl.apply(d, 3)
    assert again.data_ptr() == got.data_ptr() and np.array_equal(again.cpu().numpy(), want)
    assert {k: tuple(t.data_ptr() for t in v if t is not None) for k, v in mcl._cache.items()} == buffers   # nothing new
    one = maskops.MaskCleanup([{"op": "dilate", "structure": "square"}])
    assert np.array_equal(one.apply(d, 3).cpu().numpy(), mc.morph_ref(mask, "dilate", 1, "square", 3))
    with pytest.raises(ValueError, match="planar"):
        mcl.apply(d[None], 3)
