"""GPU GAN sampler vs the numpy restatement of its definition (tests/gan_sampler_cases.py), BIT-EXACT throughout: the
statistics are exact integer sums finished by IEEE float64 divisions and a square root, the sampling is float32 multiplies,
adds and subtractions rounded one by one on floor / ceil of small values, so there is no tolerance to measure.  Then the
network's data path with params['crop'] (one launch per step on the resident stack), graph replay against eager steps, the
unchanged host path without `crop`, and the SERVER_train_gan job."""
import json
import os

import numpy as np
import pytest
import torch

from sequitr_amd import _lib, ops
from sequitr_amd.frontend import GanSampler, gan_sample_plan
from sequitr_amd.networks import gan
from tests import gan_sampler_cases as gc
from tests.util import assert_bit_exact

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_cache = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def stack(shape, C, dtype, seed=3):
    """(raw images, float32 mean, float32 inv, normalised images) of a random stack -- restated once per shape and type"""
    key = (shape, C, np.dtype(dtype).name, seed)
    if key not in _cache:
        images = gc.random_images(shape + (C,), dtype, seed)
        if np.dtype(dtype) == np.float32:                       # float32 pixels come with the caller's own statistics
            mean = images.mean((1, 2)).astype(np.float32)
            inv = (1 / images.std((1, 2))).astype(np.float32)
        else:
            mean, inv = gc.np_stats(images)
        _cache[key] = (images, mean, inv, gc.np_normalised(images, mean, inv))
    return _cache[key]


# ---- statistics -------------------------------------------------------------------------------------------------------

def check_stats(images, what):
    N, H, W, C = images.shape
    sm = GanSampler((H, W), C, (H, W), DEV)
    d = dev(images)
    mean, inv = sm.stats(d)
    again = sm.stats(d)
    want = gc.np_stats(images)
    assert mean.shape == inv.shape == (N, C) and mean.dtype == inv.dtype == torch.float32
    for name, g, a, w in zip(('mean', 'inv'), (mean, inv), again, want):
        print("%s %s: kernel %r, restatement %r" % (what, name, g.cpu().numpy().ravel()[:4], w.ravel()[:4]))
        assert_bit_exact(g.cpu().numpy(), w, "%s: %s" % (what, name))
        assert_bit_exact(a.cpu().numpy(), g.cpu().numpy(), "%s: %s, second run" % (what, name))
    return mean, inv, sm, d


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("C", gc.CHANNELS)
def test_statistics_bit_exact(C, dtype):
    check_stats(stack(gc.STACK_SHAPE, C, dtype)[0], "%s C=%d" % (np.dtype(dtype).name, C))


def test_statistics_constant_image_gives_inv_1e4_and_zero_output():
    images = np.full((2, 13, 21, 2), 200, np.uint8)
    images[1] = 7
    mean, inv, sm, d = check_stats(images, "constant")
    assert torch.all(inv == 1e4) and mean.cpu().numpy().tolist() == [[200, 200], [7, 7]]
    plan = dev(gc.all_flip_rows(2, 13, 21, (13, 21), 4, seed=0))
    assert not sm.sample(d, plan, (4, 4), stats=(mean, inv)).any()
    assert not sm.sample(d, plan, (13, 21)).any()


def test_statistics_clamp_path_and_several_blocks_per_image():
    near = np.full((1, 300, 300, 1), 65535, np.uint16)          # two terms near 2^32 that differ by 1.1e-5: still positive
    near[0, 17, 4, 0] = 65534
    n = np.float64(300 * 300)
    s1, s2 = np.float64(int(near.astype(np.uint64).sum())), np.float64(int((near.astype(np.uint64) ** 2).sum()))
    print("S2/n - mean^2 = %r before the clamp" % (s2 / n - (s1 / n) * (s1 / n),))
    check_stats(near, "nearly constant uint16")
    mean, inv, _, _ = check_stats(gc.clamp_image(), "uint16 image whose variance rounds below zero")
    assert float(inv[0, 0]) == 1e4                              # clamped to 0: without the clamp, the root of a negative number
    check_stats(gc.random_images((1, 300, 300, 2), np.uint16, seed=8), "300 x 300 uint16")     # 22 blocks for one image
    check_stats(gc.random_images((1, 300, 300, 3), np.uint8, seed=9), "300 x 300 uint8")


# ---- sampling ---------------------------------------------------------------------------------------------------------

def run_sample(shape, C, dtype, crop, size, plan, normalise=True, what=""):
    images, mean, inv, normed = stack(shape, C, dtype)
    sm = GanSampler(shape[1:], C, crop, DEV)
    stats = (dev(mean), dev(inv)) if normalise else None
    got = sm.sample(dev(images), dev(plan), size, normalise=normalise, stats=stats)
    assert got.shape == (len(plan),) + tuple(size) + (C,) and got.dtype == torch.float32
    ref = gc.np_sample(normed if normalise else gc.np_normalised(images), plan, crop, size)
    assert_bit_exact(got.cpu().numpy(), ref, "%s %s C=%d crop %s -> %s normalise=%s" % (
        what, np.dtype(dtype).name, C, crop, size, normalise))
    return got, ref


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
@pytest.mark.parametrize("C", gc.CHANNELS)
def test_sampling_bit_exact(C, dtype):
    N, H, W = gc.STACK_SHAPE
    for count in (5, 7):                                        # 5 * 4 * 4 = 80, 7 * 12 * 20 = 1680 pixels: a partial last block
        plan = gc.all_flip_rows(N, H, W, gc.CROP, count, seed=count)
        assert set(plan[:, 3]) == {0, 1, 2, 3}
        for size in gc.SIZES:
            run_sample(gc.STACK_SHAPE, C, dtype, gc.CROP, size, plan, True, "count %d" % count)
    run_sample(gc.STACK_SHAPE, C, dtype, gc.CROP, (8, 8), plan, False, "plain cast")
    run_sample(gc.STACK_SHAPE, C, dtype, gc.CROP, gc.CROP, plan, False, "plain cast, identity")


def test_identity_size_is_the_normalised_crop():
    N, H, W = gc.STACK_SHAPE
    plan = gc.all_flip_rows(N, H, W, gc.CROP, 8, seed=1)
    got, _ = run_sample(gc.STACK_SHAPE, 2, np.uint16, gc.CROP, gc.CROP, plan)
    normed = stack(gc.STACK_SHAPE, 2, np.uint16)[3]
    for k, (n, oy, ox, bits) in enumerate(plan):
        want = normed[n, oy:oy + gc.CROP[0], ox:ox + gc.CROP[1]]
        want = want[::-1] if bits & 2 else want
        want = want[:, ::-1] if bits & 1 else want
        assert_bit_exact(got[k].cpu().numpy(), np.ascontiguousarray(want), "row %d" % k)


def test_kernel_statistics_feed_the_sampler():
    """stats=None: the sampler computes the statistics itself, with the same bits as the caller's"""
    images, mean, inv, normed = stack(gc.STACK_SHAPE, 2, np.uint8)
    sm = GanSampler(gc.STACK_SHAPE[1:], 2, gc.CROP, DEV)
    plan = gc.all_flip_rows(*gc.STACK_SHAPE, gc.CROP, 6, seed=2)
    got = sm.sample(dev(images), dev(plan), (8, 8))
    assert_bit_exact(got.cpu().numpy(), gc.np_sample(normed, plan, gc.CROP, (8, 8)), "stats=None")


def test_level_schedule():
    N, H, W = gc.LEVEL_SHAPE
    plan = gan_sample_plan((H, W), gc.LEVEL_CROP, N, 6, np.random.default_rng(1))
    for dtype in (np.uint8, np.uint16):
        for size in gc.LEVEL_SIZES:
            run_sample(gc.LEVEL_SHAPE, 2, dtype, gc.LEVEL_CROP, size, plan, True, "level")


def test_crop_larger_than_the_image_reads_fill():
    plan = gan_sample_plan(gc.STACK_SHAPE[1:], (16, 32), 3, 6, np.random.default_rng(2))
    assert not plan[:, 1:3].any()
    for size in ((16, 32), (8, 8)):
        got, ref = run_sample(gc.STACK_SHAPE, 2, np.uint8, (16, 32), size, plan, False, "crop beyond the image")
    assert (ref == 0).any() and (ref != 0).any()


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_rows_outside_the_stack_read_zero(dtype):
    N, H, W = gc.STACK_SHAPE
    plan = gc.outside_rows(N, H, W, gc.CROP)
    for size, normalise in ((gc.CROP, False), ((8, 8), True), ((5, 3), False)):
        got, ref = run_sample(gc.STACK_SHAPE, 2, dtype, gc.CROP, size, plan, normalise, "outside rows")
        assert not got[:4].any() and not got[8:13].any()
    assert ref[4:8].any() and ref[13:].any()


def test_out_preallocated_equals_freshly_allocated():
    images, mean, inv, normed = stack(gc.STACK_SHAPE, 4, np.uint16)
    sm = GanSampler(gc.STACK_SHAPE[1:], 4, gc.CROP, DEV)
    plan = dev(gc.all_flip_rows(*gc.STACK_SHAPE, gc.CROP, 5, seed=4))
    d, st = dev(images), (dev(mean), dev(inv))
    fresh = sm.sample(d, plan, (8, 8), stats=st)
    out = torch.full((5, 8, 8, 4), float('nan'), device=DEV)
    got = sm.sample(d, plan, (8, 8), stats=st, out=out)
    assert got is out and torch.equal(out, fresh)
    part = sm.sample(d, plan[2:4], (8, 8), stats=st)            # a slice of the plan: rows 2 and 3
    assert torch.equal(part, fresh[2:4])


def test_many_samples_need_several_blocks():
    N, H, W = gc.LEVEL_SHAPE
    plan = gan_sample_plan((H, W), gc.LEVEL_CROP, N, 64, np.random.default_rng(3))
    run_sample(gc.LEVEL_SHAPE, 2, np.uint8, gc.LEVEL_CROP, (16, 16), plan, True, "64 samples")     # 64 blocks of 256 pixels
    run_sample(gc.LEVEL_SHAPE, 3, np.uint16, gc.LEVEL_CROP, (16, 16), plan, True, "64 samples")


def test_errors_are_loud():
    shape, crop = gc.STACK_SHAPE[1:], gc.CROP
    sm = GanSampler(shape, 2, crop, DEV)
    im = torch.zeros((3,) + shape + (2,), dtype=torch.uint8, device=DEV)
    plan = torch.zeros((5, 4), dtype=torch.int32, device=DEV)
    st = (torch.zeros((3, 2), device=DEV), torch.ones((3, 2), device=DEV))
    for call in (lambda: sm.sample(im.cpu(), plan, (4, 4)), lambda: sm.sample(im, plan.cpu(), (4, 4)),
                 lambda: sm.sample(im, plan, (4, 4), out=torch.zeros((5, 4, 4, 2))), lambda: sm.stats(im.cpu())):
        with pytest.raises(_lib.SequitrHipError, match='no CPU fallback'):
            call()
    bad = [lambda: sm.sample(im.to(torch.float64), plan, (4, 4)),
           lambda: sm.sample(im[..., :1], plan, (4, 4)),                                 # one channel, built for two
           lambda: sm.sample(im[0], plan, (4, 4)),
           lambda: sm.sample(im.permute(0, 2, 1, 3), plan, (4, 4)),
           lambda: sm.sample(im, plan.to(torch.int64), (4, 4)),
           lambda: sm.sample(im, torch.zeros((5, 5), dtype=torch.int32, device=DEV), (4, 4)),
           lambda: sm.sample(im, plan[:0], (4, 4)),
           lambda: sm.sample(im, torch.zeros((65536, 4), dtype=torch.int32, device=DEV), (4, 4)),
           lambda: sm.sample(im, plan, (4,)), lambda: sm.sample(im, plan, (0, 4)), lambda: sm.sample(im, plan, 4),
           lambda: sm.sample(im, plan, (4, 4), out=torch.zeros((5, 4, 4, 1), device=DEV)),
           lambda: sm.sample(im, plan, (4, 4), stats=(st[0][:2], st[1][:2])),
           lambda: sm.sample(im, plan, (4, 4), stats=(st[0], st[1].double())),
           lambda: sm.sample(im.float(), plan, (4, 4)),                                  # float32 pixels without statistics
           lambda: sm.stats(im.float())]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("call %d was accepted" % i)
    assert sm.sample(im.float(), plan, (4, 4), stats=st).shape == (5, 4, 4, 2)
    assert sm.sample(im.float(), plan, (4, 4), normalise=False).shape == (5, 4, 4, 2)


# ---- the network's data path --------------------------------------------------------------------------------------------

PARAMS = {"num_levels": 3, "batch_size": 4, "repeat_batch": 1, "num_epochs_per_level": 1, "learning_rate": 1e-3,
          "device": DEV, "seed": 3}
NET_CROP = (32, 32)


def _net_stack(tmp_path, dtype=np.uint8, channels=2):
    fn = str(tmp_path / ("real_%s_%d.npy" % (np.dtype(dtype).name, channels)))
    images = gc.random_images(gc.NET_STACK[:3] + (channels,), dtype, seed=6)
    np.save(fn, images)
    return fn, images


def make_gan(fn, **kw):
    g = gan.GenerativeAdverserialNetwork(dict(PARAMS, training_data=fn, **kw), mode=gan.TRAIN)
    g.build()
    return g


class LoggedGan(gan.GenerativeAdverserialNetwork):
    """keeps every iteration's losses.  A subclass, not a closure hung on the instance: that would be a reference cycle, and
    a network with captured graphs must be freed when its last reference goes, not by the cycle collector at some later
    time -- which may fall inside another network's capture"""

    def __init__(self, *args, **kw):
        gan.GenerativeAdverserialNetwork.__init__(self, *args, **kw)
        self.log = []

    def iteration(self, X, Z, alpha, r=None):
        losses = gan.GenerativeAdverserialNetwork.iteration(self, X, Z, alpha, r)
        self.log.append(tuple(float(v) for v in losses))        # read now: a replay overwrites the graph's static scalars
        return losses


def test_network_batch_is_the_restated_sample(tmp_path):
    fn, images = _net_stack(tmp_path)
    g = make_gan(fn, crop=NET_CROP)
    N, H, W, C = gc.NET_STACK
    assert g.num_batches_per_epoch == 3 and g.num_iterations_this_level == 3
    plan = gan_sample_plan((H, W), NET_CROP, N, 3 * 4, np.random.default_rng([3, 0]))    # a phase's rows: steps * batch
    normed = gc.np_normalised(images, *gc.np_stats(images))
    for level in (0, 1, 2):                                     # the same plan read at 4 x 4, 8 x 8 and 16 x 16
        g.set_level(level)
        for step in (0, 2):
            x = g._next_real_batch(step)
            want = gc.np_sample(normed, plan[4 * step:4 * step + 4], NET_CROP, g.current_size)
            assert_bit_exact(x.cpu().numpy(), want, "level %d step %d" % (level, step))
    x = g._next_real_batch(3)                                   # past the plan: the next rows of the same generator
    rng = np.random.default_rng([3, 0])
    gan_sample_plan((H, W), NET_CROP, N, 12, rng)
    nxt = gan_sample_plan((H, W), NET_CROP, N, 12, rng)
    assert_bit_exact(x.cpu().numpy(), gc.np_sample(normed, nxt[:4], NET_CROP, g.current_size), "second plan")


def test_network_trains_on_the_resident_stack_graph_equals_eager(tmp_path):
    fn, _ = _net_stack(tmp_path)

    def run(graph):
        g = LoggedGan(dict(PARAMS, training_data=fn, crop=NET_CROP, graph=graph, output=str(tmp_path / ("out_%d" % graph))),
                      mode=gan.TRAIN)
        g.build()
        g.train(max_steps_per_phase=2)
        return g, g.log

    a, la = run(False)
    b, lb = run(True)
    print("losses eager %r\nlosses graph %r" % (la, lb))
    assert a.global_step == b.global_step == 3 * 2 * 2 and len(la) == 12
    assert np.isfinite(la).all() and all(np.isfinite(v) for v in a.last_losses)
    assert la == lb and a.last_losses == b.last_losses          # bit for bit, as for synthetic data (tests/test_gpu_gan.py)
    assert not a._graphs and sorted(k[:2] for k, v in b._graphs.items() if isinstance(v, tuple)) == [("it", 0), ("it", 1), ("it", 2)]
    assert sorted(os.listdir(str(tmp_path / "out_1"))) == ["model_(16x16).npz", "model_(4x4).npz", "model_(8x8).npz"]


def test_network_without_crop_keeps_the_host_path(tmp_path):
    fn, images = _net_stack(tmp_path)
    g = make_gan(fn)
    assert g._sampler is None
    g.set_level(1)
    for step in (0, 2, 4):
        idx = sorted((step * 4 + k) % 12 for k in range(4))
        want = ops.resize_nearest(dev(images[idx].astype(np.float32)), (8, 8))
        assert torch.equal(g._next_real_batch(step), want)


def test_network_refuses_a_stack_that_does_not_fit(tmp_path):
    fn, _ = _net_stack(tmp_path)
    with pytest.raises(MemoryError, match='hbm_budget'):
        make_gan(fn, crop=NET_CROP, hbm_budget=1000)
    with pytest.raises(ValueError, match='channels'):
        make_gan(_net_stack(tmp_path, channels=3)[0], crop=NET_CROP)
    fl = str(tmp_path / "float.npy")
    np.save(fl, np.zeros(gc.NET_STACK, np.float32))
    with pytest.raises(ValueError, match='uint8 or uint16'):
        make_gan(fl, crop=NET_CROP)


# ---- SERVER_train_gan -------------------------------------------------------------------------------------------------

def test_train_gan_job(tmp_path):
    from sequitr_amd import jobs
    fn, images = _net_stack(tmp_path, np.uint16)
    out = str(tmp_path / "job")
    os.mkdir(out)
    params = {"training_data": fn, "num_levels": 2, "batch_size": 4, "repeat_batch": 1, "num_epochs_per_level": 1,
              "seed": 3, "crop": (32, 64), "output": out}
    info = jobs.SERVER_train_gan(params, {"gpu": 0, "max_steps": 1})
    assert sorted(f for f in os.listdir(out) if f.endswith(".npz")) == ["model_(4x4).npz", "model_(8x8).npz"]
    assert os.path.exists(os.path.join(out, "export", "weights.npz")) and info["export_dir"] == os.path.join(out, "export")
    assert info["levels"] == 2 and info["steps"] == 2 * 2 * 1 and info["sizes"] == [[4, 4], [8, 8]]
    assert np.isfinite(info["d_loss"]) and np.isfinite(info["g_loss"])
    assert info["graph"] is True and info["dtype"] == "f32" and info["crop"] == [32, 48] and info["images"] == 12
    assert json.load(open(os.path.join(out, "train.json")))["steps"] == 4
    with pytest.raises(ValueError, match='channels'):
        jobs.SERVER_train_gan(dict(params, num_outputs=3), {"gpu": 0, "max_steps": 1})
    with pytest.raises(ValueError, match='.npy'):
        jobs.SERVER_train_gan(dict(params, training_data="train_GAN.tfrecord"), {"gpu": 0})
