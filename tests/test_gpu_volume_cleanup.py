"""GPU: sq_volume_morph_u8, sq_volume_fill_holes_u8, sq_volume_clear_border_u8 and VolumeCleanup against the scipy
restatement of include/sequitr_hip.h (tests/volume_cleanup_cases.py).  Every comparison is exact."""
import numpy as np
import pytest
import torch

from sequitr_amd import maskops, volumeops
from tests import mask_cleanup_cases as mc
from tests import volume_cleanup_cases as vc

pytestmark = pytest.mark.gpu
TILE = volumeops.MORPH3D_TILE
TD, TH, TW = TILE
RMAX = volumeops.MORPH3D_MAX_ITER
ALL = [(op, st) for op in vc.OPS for st in vc.STRUCTURES]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_morph(mask, C, radii=(1, 2, 3, 4), pairs=ALL):
    d = dev(mask)
    for op, st in pairs:
        for r in radii:
            got = volumeops.morph3d(d, op, r, st, classes=C).cpu().numpy()
            want = vc.morph_ref(mask, op, r, st, C)
            assert np.array_equal(got, want), "%s %s r=%d C=%d %s: %d voxels differ" % (op, st, r, C, mask.shape,
                                                                                      int((got != want).sum()))
    assert np.array_equal(d.cpu().numpy(), mask)                # the input is not written


@pytest.mark.parametrize("shape", vc.morph_shapes(TILE), ids=lambda s: "%dx%dx%dx%d" % s)
def test_morph_shapes(shape):
    N, D, H, W = shape
    C = (2, 3, 5)[(D + H + W) % 3]
    check_morph(vc.random_volume(D * 10000 + H * 100 + W, N, D, H, W, C, (0.3, 0.6, 0.9)[(D * 5 + H * 7 + W) % 3]), C)


@pytest.mark.parametrize("C", [2, 3, 5])
@pytest.mark.parametrize("density", [0.3, 0.6, 0.9])
def test_morph_random_volumes_over_several_bricks(C, density):
    check_morph(vc.random_volume(C * 10 + int(density * 10), 2, TD + 3, TH + 5, TW + 9, C, density), C)


@pytest.mark.parametrize("op,st", ALL)
def test_morph_largest_radius_over_two_bricks_each_way(op, st):
    shape = (1, TD + 11, TH + 13, TW + 36)
    zz, yy, xx = np.mgrid[0:shape[1], 0:shape[2], 0:shape[3]]
    balls = np.zeros(shape, np.uint8)
    rng = np.random.default_rng(3)
    for _ in range(14):
        cz, cy, cx, r = rng.integers(0, shape[1]), rng.integers(0, shape[2]), rng.integers(0, shape[3]), rng.integers(3, 12)
        balls[0][(zz - cz) ** 2 + (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = rng.integers(1, 3)
    m = np.concatenate([vc.random_volume(1, *shape, 3, 0.995), vc.random_volume(2, *shape, 3, 0.005), balls])
    check_morph(m, 3, radii=(RMAX,), pairs=[(op, st)])


def test_morph_nothing_leaks_between_volumes():
    m = np.zeros((2, TD + 1, 9, 70), np.uint8)
    m[0, -3:] = 1                                               # stacked against the end of volume 0
    m[1, -1, 2:5, 2:9] = 2
    m = np.concatenate([m, m[::-1]])                            # and against the start of a volume, from the one before it
    d = dev(m)
    for st in vc.STRUCTURES:
        got = volumeops.morph3d(d, "dilate", RMAX, st, classes=3).cpu().numpy()
        assert np.array_equal(got, vc.morph_ref(m, "dilate", RMAX, st, 3))
        assert not got[1, :TD - 4].any() and not (got[1] == 1).any() and not (got[3] == 2).any()
    check_morph(m, 3, radii=(1, RMAX))


def test_morph_structures_on_the_brick_seams():
    check_morph(vc.seams(TILE), 2, radii=(1, 2, 3, 4))
    check_morph(np.concatenate([vc.seams(TILE, 2), vc.seams(TILE, 1)]), 3, radii=(2,))


def test_morph_faces_and_uniform_volumes():
    f = vc.flush()
    check_morph(f, 2, radii=(1, 3, 4))
    d = dev(f)
    assert not volumeops.morph3d(d, "erode", 1, "cross", classes=2)[0, 0].any()          # erosion eats in from every face
    closed = volumeops.morph3d(dev(1 - f), "close", 2, "cube", classes=2).cpu().numpy()
    assert np.array_equal(closed, vc.morph_ref(1 - f, "close", 2, "cube", 2))
    check_morph(np.zeros((2, 9, 12, 70), np.uint8), 2, radii=(1, RMAX))
    check_morph(np.ones((2, 9, 12, 70), np.uint8), 2, radii=(1, RMAX))
    check_morph(np.ones((1, TD + 3, TH + 3, TW + 5), np.uint8), 2, radii=(2, RMAX))
    check_morph(np.full((1, 5, 9, 10), 4, np.uint8), 5, radii=(1, 3))
    check_morph(np.full((1, 5, 9, 10), 200, np.uint8), 3, radii=(1,))    # no class at all: copied through


def test_morph_volumes_smaller_than_the_halo():
    for d, h, w in ((3, 40, 70), (20, 5, 70), (20, 40, 5), (3, 5, 70), (3, 40, 6), (20, 4, 7), (5, 6, 7), (1, 1, 9)):
        check_morph(vc.random_volume(d * h * w, 2, d, h, w, 3, 0.85), 3, radii=(2, RMAX))


def test_morph_refuses_views_and_leaves_the_guard_alone():
    mask = vc.random_volume(9, 2, 9, 11, 66, 3, 0.6)
    d = dev(mask)
    with pytest.raises(ValueError, match="contiguous"):
        volumeops.morph3d(d[:, :, :, :50], "open", classes=3)    # the binding refuses a view: pass a packed copy
    packed = d[:, :, :, :50].contiguous()
    assert np.array_equal(volumeops.morph3d(packed, "open", classes=3).cpu().numpy(),
                          vc.morph_ref(mask[:, :, :, :50], "open", 1, "cross", 3))
    with pytest.raises(ValueError, match="maskops"):
        volumeops.morph3d(d[0], "open", classes=3)
    with pytest.raises(ValueError, match="planar"):
        maskops.morph(d, "open", classes=3)                      # and maskops keeps refusing volumes
    n = mask.size
    for off in (16, 13):                                        # 13: out is not 4-byte aligned, the byte path
        for src, ref in ((d, mask), (packed, mask[:, :, :, :50])):   # W = 66 and 50: W % 4 != 0, the byte path as well
            k = ref.size
            buf = torch.full((k + 64,), 0xAB, dtype=torch.uint8, device="cuda")
            out = buf[off:off + k].view(ref.shape)
            got = volumeops.morph3d(src, "close", 2, "cube", classes=3, out=out)
            assert got is out and np.array_equal(out.cpu().numpy(), vc.morph_ref(ref, "close", 2, "cube", 3))
            guard = buf.cpu().numpy()
            assert np.all(guard[:off] == 0xAB) and np.all(guard[off + k:] == 0xAB)
    wide = vc.random_volume(10, 1, 9, 11, 68, 3, 0.6)           # W % 4 == 0: the dword path, and the byte path at offset 13
    for off in (16, 13):
        buf = torch.full((wide.size + 64,), 0xAB, dtype=torch.uint8, device="cuda")
        out = buf[off:off + wide.size].view(wide.shape)
        volumeops.morph3d(dev(wide), "open", 1, "cross", classes=3, out=out)
        assert np.array_equal(out.cpu().numpy(), vc.morph_ref(wide, "open", 1, "cross", 3))
        guard = buf.cpu().numpy()
        assert np.all(guard[:off] == 0xAB) and np.all(guard[off + wide.size:] == 0xAB)
    buf = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
    buf[:n] = d.reshape(-1)
    target = buf[8:8 + n].view(mask.shape)
    before = target.clone()
    with pytest.raises(maskops._lib.SequitrHipError, match="overlap"):
        volumeops.morph3d(buf[:n].view(mask.shape), "erode", classes=3, out=target)
    assert torch.equal(target, before)                          # refused before any launch: out is untouched


@pytest.mark.parametrize("case", vc.fill_cases(), ids=lambda c: c[0])
def test_fill_cavities(case):
    name, mask, C, limits = case
    d = dev(mask)
    for a in limits:
        got = volumeops.fill_cavities(d, a, classes=C)
        want = vc.fill_ref(mask, a, C)
        assert np.array_equal(got.cpu().numpy(), want), "%s max_voxels=%r: %d voxels differ" % (
            name, a, int((got.cpu().numpy() != want).sum()))
        assert torch.equal(got, volumeops.fill_cavities(d, a, classes=C))
    planar = volumeops.fill_cavities(d, None, planar=True, classes=C).cpu().numpy()
    assert np.array_equal(planar, vc.fill_ref(mask, None, C, planar=True))
    assert np.array_equal(d.cpu().numpy(), mask)
    if name in ("open to the first plane", "tunnel to a face", "pierced shell", "one plane"):
        assert np.array_equal(vc.fill_ref(mask, None, C), mask)                  # nothing to fill in 3-D
    if name in ("open to the first plane", "one plane"):
        assert (planar != mask).any()                           # closed in every slice: filled slice by slice only


@pytest.mark.parametrize("case", vc.border_cases(), ids=lambda c: c[0])
def test_clear_border(case):
    name, mask, C = case
    d = dev(mask)
    for faces in vc.FACES:
        got = volumeops.clear_border3d(d, faces, classes=C)
        want = vc.clear_border_ref(mask, C, faces)
        assert np.array_equal(got.cpu().numpy(), want), "%s %s: %d voxels differ" % (name, faces, int((got.cpu().numpy() != want).sum()))
        assert torch.equal(got, volumeops.clear_border3d(d, faces, classes=C))
        if name == "one plane" and faces == "all":
            assert not got.any()                                # D = 1: every voxel is on a face
    assert np.array_equal(d.cpu().numpy(), mask)


def test_component_ops_guards_and_default_classes():
    mask = np.concatenate([vc.seams((4, 8, 20), 2), vc.random_volume(3, 1, 11, 21, 47, 3, 0.7, unknown=False)])
    d = dev(mask)
    k = mask.size
    lib = maskops._lib.load()
    fills, clears = lib.sq_volume_fill_holes_workspace(*mask.shape), lib.sq_volume_clear_border_workspace(*mask.shape)
    assert fills == (9 * k + 15) // 16 * 16 and clears == (8 * k + 15) // 16 * 16
    for fn, nbytes, ref in ((lambda o, w: volumeops.fill_cavities(d, 6, out=o, workspace=w), fills, vc.fill_ref(mask, 6, 3)),
                            (lambda o, w: volumeops.clear_border3d(d, "lateral", out=o, workspace=w), clears,
                             vc.clear_border_ref(mask, 3, "lateral"))):
        buf = torch.full((k + 64,), 0xAB, dtype=torch.uint8, device="cuda")
        out = buf[13:13 + k].view(mask.shape)
        wsbuf = torch.full((nbytes + 64,), 0xCD, dtype=torch.uint8, device="cuda")   # torch's allocations are 16-B aligned
        ws = wsbuf[32:32 + nbytes]
        assert ws.data_ptr() % 16 == 0
        assert fn(out, ws) is out and np.array_equal(out.cpu().numpy(), ref)   # classes default to the largest byte + 1
        guard, wguard = buf.cpu().numpy(), wsbuf.cpu().numpy()
        assert np.all(guard[:13] == 0xAB) and np.all(guard[13 + k:] == 0xAB)
        assert np.all(wguard[:32] == 0xCD) and np.all(wguard[32 + nbytes:] == 0xCD)
    with pytest.raises(ValueError, match="workspace holds"):
        volumeops.fill_cavities(d, workspace=torch.empty(16, dtype=torch.int32, device="cuda"))
    zero = torch.zeros((1, 3, 5, 6), dtype=torch.uint8, device="cuda")
    assert not volumeops.fill_cavities(zero).any() and not volumeops.clear_border3d(zero).any()
    assert not volumeops.morph3d(zero, "dilate").any()


def test_morph_twice_is_bit_identical():
    d = dev(vc.random_volume(77, 2, TD + 3, TH + 5, TW + 9, 5, 0.6))
    for op, st in ALL:
        assert torch.equal(volumeops.morph3d(d, op, 3, st, classes=5), volumeops.morph3d(d, op, 3, st, classes=5))


def test_plane_structures_are_maskops_on_the_view():
    mask = vc.random_volume(21, 2, 5, 40, 70, 3, 0.7)
    d = dev(mask)
    for op, r, st3, st2 in (("open", 2, "plane_cross", "cross"), ("erode", 3, "plane_square", "square"),
                            ("close", 6, "plane_cross", "cross")):
        got = volumeops.morph3d(d, op, r, st3, classes=3)
        assert torch.equal(got.view(10, 40, 70), maskops.morph(d.view(10, 40, 70), op, r, st2, classes=3))
        assert np.array_equal(got.cpu().numpy(), vc.morph_ref(mask, op, r, st3, 3))


def _cleanup_volume():
    mask = np.concatenate([vc.seams((4, 8, 20), 2), vc.seams((4, 8, 20), 1), vc.random_volume(12, 1, 11, 21, 47, 3, 0.75)])
    mask[:2][vc.random_volume(13, 2, 11, 21, 47, 2, 0.04, unknown=False) > 0] = 0      # pepper the objects with cavities
    return mask


STEPS = [{"op": "open", "iterations": 1, "structure": "cross"}, {"op": "fill_holes", "max_voxels": 40},
         {"op": "close", "iterations": 2, "structure": "plane_square"}, {"op": "clear_border", "faces": "lateral"}]


def test_volume_cleanup_apply_is_the_steps_in_sequence():
    vcl = volumeops.VolumeCleanup(STEPS)
    mask = _cleanup_volume()
    d = dev(mask)
    got = vcl.apply(d, 3)
    want = vc.steps_ref(mask, STEPS, 3)
    assert np.array_equal(got.cpu().numpy(), want) and (want != mask).any() and np.array_equal(d.cpu().numpy(), mask)
    buffers = {k: tuple(t.data_ptr() for t in v if t is not None) for k, v in vcl._cache.items()}
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_allocated()
    again = vcl.apply(d, 3)
    assert torch.cuda.memory_allocated() == allocated           # nothing is allocated on the second call
    assert again.data_ptr() == got.data_ptr() and np.array_equal(again.cpu().numpy(), want)
    assert {k: tuple(t.data_ptr() for t in v if t is not None) for k, v in vcl._cache.items()} == buffers
    one = volumeops.VolumeCleanup([{"op": "dilate", "structure": "cube"}, {"op": "fill_holes", "planar": True}])
    assert np.array_equal(one.apply(d, 3).cpu().numpy(), vc.steps_ref(mask, one.record(), 3))
    with pytest.raises(ValueError, match="maskops"):
        vcl.apply(d[0], 3)


def test_graph_replay_equals_eager():
    mask = _cleanup_volume()
    d = dev(mask)
    steps = STEPS + [{"op": "fill_holes", "planar": True}]
    vcl = volumeops.VolumeCleanup(steps)
    frames = mask.reshape((-1,) + mask.shape[2:])               # 33 frames of 21 x 47: W no multiple of 4 or of 64
    dframes = d.view(frames.shape)
    planar_steps = [{"op": "open", "iterations": 1, "structure": "cross"}, {"op": "fill_holes", "max_area": 6},
                    {"op": "clear_border"}]
    mcl = maskops.MaskCleanup(planar_steps)
    eager_morph = volumeops.morph3d(d, "open", 2, "cube", classes=3).clone()
    eager_steps = vcl.apply(d, 3).clone()
    eager_planar = mcl.apply(dframes, 3).clone()
    out = torch.empty_like(d)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        volumeops.morph3d(d, "open", 2, "cube", classes=3, out=out)   # warm up on the side stream
        vcl.apply(d, 3)
        mcl.apply(dframes, 3)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    g1, g2, g3 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g1):
        volumeops.morph3d(d, "open", 2, "cube", classes=3, out=out)
    with torch.cuda.graph(g2):
        res = vcl.apply(d, 3)
    with torch.cuda.graph(g3):
        pres = mcl.apply(dframes, 3)
    for _ in range(2):
        out.zero_()
        res.zero_()
        pres.zero_()
        g1.replay()
        g2.replay()
        g3.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager_morph) and torch.equal(res, eager_steps) and torch.equal(pres, eager_planar)
    assert np.array_equal(eager_steps.cpu().numpy(), vc.steps_ref(mask, steps, 3))
    assert np.array_equal(eager_planar.cpu().numpy(), mc.steps_ref(frames, planar_steps, 3))
