"""GAN sampler without a GPU: the numpy restatement of include/sequitr_hip.h "GAN sampler" (tests/gan_sampler_cases.py)
against torch's bilinear resize with align_corners=True on the CPU, the float32 form against the float64 one within the
bound the coordinate rounding gives, the identity, gan_sample_plan, and the library's host-side refusals."""
import numpy as np
import pytest
import torch

from sequitr_amd import _lib
from sequitr_amd.frontend import GanSampler, gan_sample_plan
from tests import gan_sampler_cases as gc

# (stack shape (N, H, W), C, dtype, crop, sizes): the GPU test's small shapes, the level schedule, and the reference's
# 512 x 512 crop halved
RESIZE_CASES = [(gc.STACK_SHAPE, 2, np.uint8, gc.CROP, gc.SIZES),
                (gc.STACK_SHAPE, 3, np.uint16, gc.CROP, gc.SIZES),
                (gc.LEVEL_SHAPE, 2, np.uint16, gc.LEVEL_CROP, gc.LEVEL_SIZES),
                ((1, 512, 512), 2, np.uint8, (512, 512), [(256, 256)])]


def _case(shape, C, dtype, crop):
    images = gc.random_images(shape + (C,), dtype, seed=C)
    normed = gc.np_normalised(images, *gc.np_stats(images))
    N, H, W = shape
    plan = gc.all_flip_rows(N, H, W, crop, 4 if H < 512 else 1, seed=7)
    if H == 512:
        plan[0, 3] = 3
    return normed, plan


@pytest.mark.parametrize("case", RESIZE_CASES, ids=lambda c: "%dx%dx%d-%s" % (c[0][1], c[0][2], c[1], np.dtype(c[2]).name))
def test_restatement_against_torch_and_float32_against_float64(case):
    shape, C, dtype, crop, sizes = case
    normed, plan = _case(shape, C, dtype, crop)
    for size in sizes:
        ref64 = gc.np_sample(normed, plan, crop, size, np.float64)
        for k, row in enumerate(plan):
            flipped = torch.from_numpy(gc.np_flipped_crop(normed, row, crop).astype(np.float64)).permute(2, 0, 1)[None]
            want = torch.nn.functional.interpolate(flipped, size=size, mode='bilinear', align_corners=True)
            err = float(np.abs(want[0].permute(1, 2, 0).numpy() - ref64[k]).max())
            assert err <= 1e-12, (size, k, err)
        got32 = gc.np_sample(normed, plan, crop, size, np.float32)
        assert got32.dtype == np.float32
        err, bound = float(np.abs(got32.astype(np.float64) - ref64).max()), gc.f32_bound(ref64, crop)
        print("crop %s -> %s: float32 - float64 %.3g, bound %.3g" % (crop, size, err, bound))
        assert err <= bound, (size, err, bound)


def test_identity_size_is_the_normalised_crop_exactly():
    for C, dtype in ((1, np.uint8), (2, np.uint16), (4, np.uint8)):
        images = gc.random_images(gc.STACK_SHAPE + (C,), dtype, seed=11)
        mean, inv = gc.np_stats(images)
        normed = gc.np_normalised(images, mean, inv)
        plan = gc.all_flip_rows(*gc.STACK_SHAPE, gc.CROP, 8, seed=3)
        got = gc.np_sample(normed, plan, gc.CROP, gc.CROP)
        for k, (n, oy, ox, bits) in enumerate(plan):
            want = normed[n, oy:oy + gc.CROP[0], ox:ox + gc.CROP[1]]
            want = want[::-1] if bits & 2 else want
            want = want[:, ::-1] if bits & 1 else want
            assert np.array_equal(got[k], want), (C, k)
        # and the statistics do what they say: every image has mean 0 and deviation 1 per channel
        assert np.abs(normed.mean((1, 2))).max() < 1e-5 and np.abs(normed.std((1, 2)) - 1).max() < 1e-5


def test_statistics_restatement_edge_cases():
    const = np.full((1, 5, 7, 2), 200, np.uint8)
    mean, inv = gc.np_stats(const)
    assert np.all(mean == 200) and np.all(inv == np.float32(1e4))
    assert not gc.np_normalised(const, mean, inv).any()
    near = np.full((1, 300, 300, 1), 65535, np.uint16)
    near[0, 17, 4, 0] = 65534
    mean, inv = gc.np_stats(near)
    assert np.isfinite(inv).all() and inv[0, 0] > 0
    neg = gc.clamp_image()                                      # here the difference is negative before the clamp
    v = neg.astype(np.uint64)
    n, s1, s2 = np.float64(neg.size), np.float64(int(v.sum())), np.float64(int((v * v).sum()))
    assert s2 / n - (s1 / n) * (s1 / n) < 0
    mean, inv = gc.np_stats(neg)
    assert inv[0, 0] == np.float32(1e4) and mean[0, 0] == np.float32(gc.CLAMP_LEVEL)
    images = gc.random_images((2, 9, 11, 3), np.uint16, seed=1)
    mean, inv = gc.np_stats(images)
    x = images.astype(np.float64)
    assert np.allclose(mean, x.mean((1, 2)), rtol=1e-7) and np.allclose(inv, 1 / x.std((1, 2)), rtol=1e-6)


def test_outside_rows_read_zero_where_they_leave_the_stack():
    N, H, W = gc.STACK_SHAPE
    images = gc.random_images(gc.STACK_SHAPE + (2,), np.uint8, seed=2) | 1          # no zero pixel: fill is recognisable
    plan = gc.outside_rows(N, H, W, gc.CROP)
    got = gc.np_sample(gc.np_normalised(images), plan, gc.CROP, gc.CROP)
    assert not got[:4].any() and not got[8:13].any()            # n outside, or the whole crop outside
    assert not got[4, :3].any() and not got[4, :, W - 2:].any() and got[4, 3:, :W - 2].all()   # oy = -3, ox = 2: fill, then image
    assert np.array_equal(got[4, 3:, :W - 2], images[0, :gc.CROP[0] - 3, 2:W].astype(np.float32))
    assert np.array_equal(got[13], gc.np_sample(gc.np_normalised(images), [[2 % N, -2, -2, 3]], gc.CROP, gc.CROP)[0])
    assert np.array_equal(got[15], gc.np_sample(gc.np_normalised(images), [[1 % N, 0, 0, 0]], gc.CROP, gc.CROP)[0])


def test_gan_sample_plan():
    shape, crop, images, count = (40, 48), (32, 32), 5, 23
    plan = gan_sample_plan(shape, crop, images, count, np.random.default_rng(4))
    assert plan.shape == (count, 4) and plan.dtype == np.int32
    for e in range(count // images):                            # every epoch is a permutation
        assert sorted(plan[e * images:(e + 1) * images, 0]) == list(range(images))
    assert len(set(plan[20:, 0])) == 3                          # the partial last epoch repeats no image
    assert not np.array_equal(plan[:5, 0], plan[5:10, 0]) or not np.array_equal(plan[5:10, 0], plan[10:15, 0])
    many = gan_sample_plan(shape, crop, images, 4000, np.random.default_rng(5))
    assert many[:, 1].min() == 0 and many[:, 1].max() == 8 and many[:, 2].min() == 0 and many[:, 2].max() == 16
    assert sorted(set(many[:, 3])) == [0, 1, 2, 3]
    assert np.array_equal(np.bincount(many[:, 0]), [800] * 5)
    short = gan_sample_plan((20, 48), crop, images, 200, np.random.default_rng(6))
    assert not short[:, 1].any() and short[:, 2].max() == 16    # an axis shorter than the crop: origin 0
    exact = gan_sample_plan((32, 32), crop, images, 50, np.random.default_rng(6))
    assert not exact[:, 1:3].any()
    plain = gan_sample_plan(shape, crop, images, 200, np.random.default_rng(7), augment=())
    assert not plain[:, 3].any()
    walk = gan_sample_plan(shape, crop, images, 12, np.random.default_rng(8), shuffle=False)
    assert list(walk[:, 0]) == [k % images for k in range(12)]
    again = gan_sample_plan(shape, crop, images, count, np.random.default_rng(4))
    assert np.array_equal(plan, again)                          # reproducible from the seed
    assert not np.array_equal(plan, gan_sample_plan(shape, crop, images, count, np.random.default_rng(9)))
    assert np.array_equal(gan_sample_plan(shape, crop, images, count, np.random.default_rng(4), augment='flip'), plan)
    for bad in (lambda: gan_sample_plan((40,), crop, images, count, np.random.default_rng(0)),
                lambda: gan_sample_plan(shape, (32, 32, 32), images, count, np.random.default_rng(0)),
                lambda: gan_sample_plan(shape, (0, 32), images, count, np.random.default_rng(0)),
                lambda: gan_sample_plan(shape, crop, 0, count, np.random.default_rng(0)),
                lambda: gan_sample_plan(shape, crop, images, 0, np.random.default_rng(0)),
                lambda: gan_sample_plan(shape, crop, images, count, np.random.default_rng(0), augment=('rotate',))):
        with pytest.raises(ValueError):
            bad()


def test_host_side_validation_needs_no_gpu():
    lib = _lib.load()
    P = 4096                                                    # a stand-in address: every call is refused before any launch
    ok = dict(images=P, dtype=0, mean=P, inv=P, plan=P, out=P, N=3, H=13, W=21, C=2, CH=12, CW=20, SH=4, SW=4, count=5)

    def sample(**kw):
        a = dict(ok, **kw)
        return lib.sq_gan_sample_f32(a['images'], a['dtype'], a['mean'], a['inv'], a['plan'], a['out'], a['N'], a['H'], a['W'],
                                     a['C'], a['CH'], a['CW'], a['SH'], a['SW'], a['count'], None)

    for kw, word in (({'images': None}, b"null"), ({'plan': None}, b"null"), ({'out': None}, b"null"),
                     ({'mean': None}, b"null"), ({'inv': None}, b"null"), ({'C': 0}, b"channels"), ({'C': 5}, b"channels"),
                     ({'count': 0}, b"count"), ({'count': 65536}, b"count"), ({'H': 0}, b"positive"), ({'N': 0}, b"positive"),
                     ({'CW': 0}, b"positive"), ({'SH': -1}, b"positive"), ({'H': 4097, 'W': 4096}, b"2^24"),
                     ({'dtype': 3}, b"pixel type"), ({'images': P + 1}, b"aligned"), ({'out': P + 4}, b"aligned"),
                     ({'SH': 4096, 'SW': 4097}, b"out of range"), ({'SH': 4096, 'SW': 4096, 'count': 128}, b"2^31")):
        assert sample(**kw) == -1 and word in lib.sq_last_error(), (kw, lib.sq_last_error())

    def stats(images=P, dtype=1, mean=P, inv=P, work=P, N=3, H=13, W=21, C=2):
        return lib.sq_gan_image_stats(images, dtype, mean, inv, work, N, H, W, C, None)

    for kw, word in (({'images': None}, b"null"), ({'mean': None}, b"null"), ({'inv': None}, b"null"), ({'work': None}, b"null"),
                     ({'dtype': 2}, b"pixel type"), ({'C': 5}, b"channels"), ({'N': 0}, b"positive"), ({'W': 0}, b"positive"),
                     ({'H': 4096, 'W': 4097}, b"2^24"), ({'images': P + 2}, b"aligned"), ({'work': P + 4}, b"aligned")):
        assert stats(**kw) == -1 and word in lib.sq_last_error(), (kw, lib.sq_last_error())
    assert lib.sq_gan_image_stats_workspace(3, 2) == 3 * 2 * 16 and lib.sq_gan_image_stats_workspace(0, 2) == 0

    with pytest.raises(_lib.SequitrHipError):
        GanSampler((13, 21), 2, (12, 20), 'cpu')
    for bad in (lambda: GanSampler((13,), 2, (12, 20), 'cuda:0'), lambda: GanSampler((13, 21), 5, (12, 20), 'cuda:0'),
                lambda: GanSampler((13, 21), 2, (0, 20), 'cuda:0'), lambda: GanSampler((4097, 4096), 2, (12, 20), 'cuda:0')):
        with pytest.raises(ValueError):
            bad()
    sm = GanSampler((13, 21), 2, (12, 20), 'cuda:0')
    with pytest.raises(_lib.SequitrHipError, match='no CPU fallback'):
        sm.sample(torch.zeros((3, 13, 21, 2), dtype=torch.uint8), torch.zeros((5, 4), dtype=torch.int32), (4, 4))
    with pytest.raises(_lib.SequitrHipError, match='no CPU fallback'):
        sm.stats(torch.zeros((3, 13, 21, 2), dtype=torch.uint8))
