"""GPU tile sampler vs the float32 numpy restatement of its definition (tests/tile_sampler_cases.py), BIT-EXACT throughout:
the arithmetic is IEEE multiplies and adds, a correctly rounded divide, floor and roundf on exactly representable values, so
there is no tolerance to measure.  Random angles in three pixel types with and without ImageNorm, tiles that give partial
32 x 32 patches, the LDS and the direct form against each other, footprints too large for the LDS patch, rows that are out
of range, the tie to FrameTiler, the exact quarter turn, partial calls, and SERVER_train's tile mode closed into
SERVER_segment_frames."""
import json
import os

import numpy as np
import pytest
import torch

from sequitr_amd import _lib
from sequitr_amd.frontend import FrameTiler, TileSampler, covering_tiles, segment_frames, tile_sample_plan
from tests import tile_sampler_cases as tc
from tests.util import assert_bit_exact

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_cache = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def sources(shape, dtype):
    """(raw frames, {normalise: float32 frames}, labels, weights) -- computed once per shape and type"""
    key = (shape, np.dtype(dtype).name)
    if key not in _cache:
        frames = tc.random_frames(shape, dtype, seed=3)
        _cache[key] = (frames, {n: tc.np_normalised(frames, n) for n in (True, False)}, tc.random_labels(shape, 4),
                       tc.random_weights(shape, 5))
    return _cache[key]


def both_forms(monkeypatch, fn):
    """fn() with SQ_ROTATE_LDS=1, the LDS form, and with SQ_ROTATE_LDS=0, the direct gather (also what an unset switch
    selects); the switch is read per launch"""
    monkeypatch.setenv('SQ_ROTATE_LDS', '1')
    a = fn()
    monkeypatch.setenv('SQ_ROTATE_LDS', '0')
    b = fn()
    monkeypatch.delenv('SQ_ROTATE_LDS', raising=False)
    return a, b


def host(t):
    return tuple(None if v is None else v.cpu().numpy() for v in t)


def check_all(got, ref, what):
    for name, g, r in zip(('image', 'onehot', 'weights'), got, ref):
        assert (g is None) == (r is None), (what, name)
        if g is not None:
            assert_bit_exact(g, r.astype(g.dtype), "%s: %s" % (what, name))


def run_case(monkeypatch, shape, dtype, tile, plan, coef, C, normalise, what):
    frames, normed, labels, weights = sources(shape, dtype)
    sm = TileSampler(shape[1:], tile, DEV)
    d = [dev(frames), dev(labels), dev(weights), dev(plan), dev(coef)]
    ref = tc.np_sample(normed[normalise], labels, weights, plan, coef, tile, C)
    lds, direct = both_forms(monkeypatch, lambda: host(sm.sample(*d, C, normalise=normalise)))
    assert lds[0].shape == (len(plan),) + tile + (1,) and lds[1].shape == (len(plan),) + tile + (C,)
    assert lds[2].shape == (len(plan),) + tile + (1,) and lds[1].dtype == np.uint8
    check_all(lds, ref, what)
    check_all(direct, ref, what + ", SQ_ROTATE_LDS=0")
    return ref


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
@pytest.mark.parametrize("tile", tc.TILES, ids=lambda t: '%dx%d' % t)
def test_random_angles_bit_exact(tile, dtype, monkeypatch):
    plan, coef = tc.random_rows(tc.FRAMES_SHAPE, tile, 6, seed=tile[1])
    assert -1 in plan[:, 0] and tc.FRAMES_SHAPE[0] in plan[:, 0] and plan[:, 1].min() == -4
    for C, normalise in zip(tc.CLASSES, (True, False, True, False)):
        run_case(monkeypatch, tc.FRAMES_SHAPE, dtype, tile, plan, coef, C, normalise,
                 "%s %s C=%d normalise=%s" % (tile, np.dtype(dtype).name, C, normalise))
    ref = run_case(monkeypatch, tc.FRAMES_SHAPE, dtype, tile, plan, coef, 2, not normalise, "C=2")
    assert ref[1][-2:, ..., 0].all() and np.all(ref[2][-2:] == 1) and not ref[0][-2:].any()    # f = -1 and f = F: fill


def test_tile_larger_than_the_frame(monkeypatch):
    plan, coef = tc.random_rows(tc.FRAMES_SHAPE, tc.BIG_TILE, 4, seed=9)
    run_case(monkeypatch, tc.FRAMES_SHAPE, np.uint16, tc.BIG_TILE, plan, coef, 5, True, "48x48 on 37x45")


def test_large_footprints_take_the_direct_form_with_the_same_bits(monkeypatch):
    plan, coef = tc.large_footprint_rows()
    for tile in ((40, 40), (16, 40)):
        run_case(monkeypatch, tc.FRAMES_SHAPE, np.uint16, tile, plan, coef, 5, True, "scale and shear rows %s" % (tile,))


def test_bad_coefficients_are_all_fill_and_outputs_are_fully_overwritten(monkeypatch):
    frames, normed, labels, weights = sources(tc.FRAMES_SHAPE, np.float32)
    tile, C = (40, 40), 3
    bad_plan, bad_coef = tc.bad_rows()
    good_plan, good_coef = tc.random_rows(tc.FRAMES_SHAPE, tile, 3, seed=2)
    plan, coef = np.concatenate([bad_plan, good_plan]), np.concatenate([bad_coef, good_coef])
    n, nb = len(plan), len(bad_plan)
    sm = TileSampler(tc.FRAMES_SHAPE[1:], tile, DEV)
    ref = tc.np_sample(normed[True], labels, weights, plan, coef, tile, C)
    assert not ref[0][:nb].any() and np.all(ref[2][:nb] == 1) and ref[1][:nb, ..., 0].all() and not ref[1][:nb, ..., 1:].any()

    def poisoned():
        out = (torch.full((n,) + tile + (1,), float('nan'), device=DEV),
               torch.full((n,) + tile + (C,), 0xA5, dtype=torch.uint8, device=DEV),
               torch.full((n,) + tile + (1,), float('nan'), device=DEV))
        got = sm.sample(dev(frames), dev(labels), dev(weights), dev(plan), dev(coef), C, out=out)
        assert all(g is o for g, o in zip(got, out))
        return host(got)

    lds, direct = both_forms(monkeypatch, poisoned)
    check_all(lds, ref, "bad rows, poisoned outputs")
    check_all(direct, ref, "bad rows, poisoned outputs, SQ_ROTATE_LDS=0")


def test_identity_at_a_tilers_origins_is_the_tilers_tile(monkeypatch):
    T = 24
    for dtype in (np.uint8, np.uint16, np.float32):
        frames = sources(tc.FRAMES_SHAPE, dtype)[0]
        tiler = FrameTiler(tc.FRAMES_SHAPE[1:], T, 2, device=DEV)
        origins = [(int(oy), int(ox)) for oy in tiler.oy for ox in tiler.ox]
        rows = [tc.identity_rows(origins, f) for f in range(tc.FRAMES_SHAPE[0])]
        plan, coef = np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows])
        sm = TileSampler(tc.FRAMES_SHAPE[1:], (T, T), DEV)
        d = dev(frames)
        for normalise in (True, False):
            want = tiler.tiles(d, normalise=normalise).cpu().numpy()
            for got in both_forms(monkeypatch, lambda: sm.sample(d, None, None, dev(plan), dev(coef), 2, normalise=normalise)[0]):
                assert_bit_exact(got.cpu().numpy(), want, "FrameTiler tiles %s normalise=%s" % (np.dtype(dtype).name, normalise))
        stats = tiler.stats(d)
        got = sm.sample(d, None, None, dev(plan), dev(coef), 2, stats=stats)[0]         # with the caller's statistics
        assert_bit_exact(got.cpu().numpy(), tiler.tiles(d).cpu().numpy(), "stats=")


def test_exact_quarter_turn_is_rot90_of_the_normalised_frame(monkeypatch):
    S = 37
    shape = (2, S, S)
    frames, normed, labels, weights = sources(shape, np.uint16)
    plan, coef = tc.quarter_turn_rows(S, f=1)
    sm = TileSampler((S, S), (S, S), DEV)
    for got in both_forms(monkeypatch, lambda: host(sm.sample(dev(frames), dev(labels), dev(weights), dev(plan), dev(coef), 7))):
        assert_bit_exact(got[0][0, ..., 0], np.ascontiguousarray(np.rot90(normed[True][1], 1)), "rot90 image")
        assert_bit_exact(got[2][0, ..., 0], np.ascontiguousarray(np.rot90(weights[1], 1)), "rot90 weights")
        assert np.array_equal(got[1][0].argmax(-1), np.rot90(labels[1], 1)) and np.all(got[1][0].sum(-1) == 1)


def test_partial_calls_give_the_bits_of_the_fused_call(monkeypatch):
    frames, normed, labels, weights = sources(tc.FRAMES_SHAPE, np.uint8)
    tile, C = (16, 40), 5
    plan, coef = tc.random_rows(tc.FRAMES_SHAPE, tile, 5, seed=1)
    sm = TileSampler(tc.FRAMES_SHAPE[1:], tile, DEV)
    f, l, w, p, c = dev(frames), dev(labels), dev(weights[..., None]), dev(plan), dev(coef)   # weights as (F, H, W, 1) too
    for fused in both_forms(monkeypatch, lambda: host(sm.sample(f, l, w, p, c, C))):
        check_all(fused, tc.np_sample(normed[True], labels, weights, plan, coef, tile, C), "fused")
        for parts in both_forms(monkeypatch, lambda: (host(sm.sample(f, None, None, p, c, C)), host(sm.sample(None, l, None, p, c, C)),
                                                      host(sm.sample(None, None, w, p, c, C)))):
            for k, part in enumerate(parts):
                assert [v is not None for v in part] == [k == 0, k == 1, k == 2]
                assert_bit_exact(part[k], fused[k], "partial call %d" % k)


def test_errors_are_loud():
    shape, tile = tc.FRAMES_SHAPE[1:], (24, 24)
    sm = TileSampler(shape, tile, DEV)
    fr = torch.zeros((2,) + shape, dtype=torch.uint16, device=DEV)
    lab = torch.zeros((2,) + shape, dtype=torch.uint8, device=DEV)
    wt = torch.zeros((2,) + shape, dtype=torch.float32, device=DEV)
    plan = torch.zeros((3, 4), dtype=torch.int32, device=DEV)
    coef = torch.zeros((3, 6), dtype=torch.float32, device=DEV)
    with pytest.raises(_lib.SequitrHipError):
        TileSampler(shape, tile, 'cpu')
    with pytest.raises(ValueError):
        TileSampler(shape, (24,), DEV)
    with pytest.raises(ValueError):
        TileSampler((4097, 4096), tile, DEV)
    for call in (lambda: sm.sample(fr.cpu(), lab, wt, plan, coef, 2), lambda: sm.sample(fr, lab.cpu(), wt, plan, coef, 2),
                 lambda: sm.sample(fr, lab, wt.cpu(), plan, coef, 2), lambda: sm.sample(fr, lab, wt, plan.cpu(), coef, 2),
                 lambda: sm.sample(fr, lab, wt, plan, coef.cpu(), 2),
                 lambda: sm.sample(fr, None, None, plan, coef, 2, out=(torch.zeros((3,) + tile + (1,)), None, None))):
        with pytest.raises(_lib.SequitrHipError, match='no CPU fallback'):
            call()
    bad = [lambda: sm.sample(fr.to(torch.float64), lab, wt, plan, coef, 2),            # wrong pixel type
           lambda: sm.sample(fr, fr, wt, plan, coef, 2),                                # labels are uint8
           lambda: sm.sample(fr, lab, lab, plan, coef, 2),                              # weights are float32
           lambda: sm.sample(torch.zeros((2, 45, 37), dtype=torch.uint8, device=DEV).transpose(1, 2), lab, wt, plan, coef, 2),
           lambda: sm.sample(torch.zeros((2, 37, 46), dtype=torch.uint8, device=DEV), None, None, plan, coef, 2),
           lambda: sm.sample(fr[0], None, None, plan, coef, 2),
           lambda: sm.sample(fr, lab[:1], wt, plan, coef, 2),                           # one frame of labels for two frames
           lambda: sm.sample(None, None, None, plan, coef, 2),
           lambda: sm.sample(fr, lab, wt, torch.zeros((3, 5), dtype=torch.int32, device=DEV), coef, 2),
           lambda: sm.sample(fr, lab, wt, plan.to(torch.int64), coef, 2),
           lambda: sm.sample(fr, lab, wt, plan, torch.zeros((3, 4), device=DEV), 2),
           lambda: sm.sample(fr, lab, wt, plan, coef.double(), 2),
           lambda: sm.sample(fr, lab, wt, plan[:2], coef, 2),                           # two plan rows, three coefficient rows
           lambda: sm.sample(fr, lab, wt, plan[:0], coef[:0], 2),
           lambda: sm.sample(fr, lab, wt, torch.zeros((65536, 4), dtype=torch.int32, device=DEV),
                             torch.zeros((65536, 6), device=DEV), 2),                   # more than one launch
           lambda: sm.sample(fr, lab, wt, plan, coef, 0), lambda: sm.sample(fr, lab, wt, plan, coef, 17),
           lambda: sm.sample(fr, None, None, plan, coef, 2, out=(torch.zeros((3,) + tile, device=DEV), None, None)),
           lambda: sm.sample(None, lab, None, plan, coef, 2, out=(None, torch.zeros((3,) + tile + (2,), device=DEV), None)),
           lambda: sm.sample(fr, None, None, plan, coef, 2, stats=(torch.zeros(3, device=DEV), torch.ones(3, device=DEV)))]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("call %d was accepted" % i)


# ---- SERVER_train with params['tile'] --------------------------------------------------------------------------------

TILE = (32, 32)            # the smallest tile the rest of the suite runs the five-level net at (tests/test_gpu_jobs.py)
STACK = (3, 80, 96)


def _stack(tmp_path):
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:STACK[1], 0:STACK[2]]
    lab = np.zeros(STACK, np.uint8)
    lab[0][(yy - 30) ** 2 + (xx - 34) ** 2 < 180] = 1
    lab[0][(yy - 60) ** 2 + (xx - 70) ** 2 < 90] = 1
    lab[1][(yy - 40) ** 2 + (xx - 50) ** 2 < 250] = 1
    lab[2][(yy - 20) ** 2 + (xx - 75) ** 2 < 120] = 1
    imgs = (400 + lab * 900.0 + rng.standard_normal(STACK) * 150).clip(0, 65535).astype(np.uint16)
    np.save(str(tmp_path / "im.npy"), imgs)
    np.save(str(tmp_path / "lab.npy"), lab)
    return imgs, lab


def _job(tmp_path, monkeypatch, out, options, **extra):
    from sequitr_amd import core, jobs
    monkeypatch.setattr(core.TensorflowConfiguration, "MODELDIR", str(tmp_path / "models"))
    for d in ("models", out):
        if not os.path.isdir(str(tmp_path / d)):
            os.mkdir(str(tmp_path / d))
    params = dict({"images": str(tmp_path / "im.npy"), "labels": str(tmp_path / "lab.npy"), "tile": TILE, "batch_size": 4,
                   "dropout": 0.0, "num_outputs": 2, "seed": 5, "num_epochs": 2, "output": str(tmp_path / out)}, **extra)
    info = jobs.SERVER_train(params, dict({"gpu": 0, "max_steps": 3}, **options))
    return info, json.load(open(str(tmp_path / out / "train.json")))


def test_train_job_on_whole_frames_first_loss_outputs_and_segment(tmp_path, monkeypatch):
    """SERVER_train in tile mode on a (3, 80, 96) uint16 stack, then SERVER_segment_frames with the saved model.

    The job's first loss is compared BIT FOR BIT with the loss of one step of a fresh UNetTrainer (the job's network
    parameters and seed) on the first batch restated in numpy: the plan's first four rows from the seeded generator, the
    frames normalised and sampled by tests/tile_sampler_cases, and the weight map the job is specified to use --
    device_weightmaps of the whole frames -- interpolated there.  The first loss involves the forward pass and the loss
    kernel only.  Whether bit-for-bit is the right demand is established first: two fresh trainers on that batch must
    reproduce each other bit for bit (the standard of test_gpu_volume_sampler.py's job test)."""
    from sequitr_amd import jobs, utils
    from sequitr_amd.networks.unet import UNet2D
    from sequitr_amd.train import UNetTrainer
    from sequitr_amd.weightmap import device_weightmaps
    imgs, lab = _stack(tmp_path)
    info, tj = _job(tmp_path, monkeypatch, "out_t", {})
    per = covering_tiles(STACK[1:], TILE)
    assert per == 9
    assert info["steps"] == 3 and len(tj["losses"]) == 3 and np.isfinite(tj["losses"]).all()
    assert tj["tile"] == [32, 32] and tj["augment"] == ["rotate"] and tj["samples_per_epoch"] == 3 * per
    assert tj["seed"] == 5 and tj["frame_shape"] == [80, 96] and tj["batch_size"] == 4 and tj["graph"] is True
    cfg = json.load(open(os.path.join(info["model_dir"], "net.config")))["NetConfiguration"]
    assert tuple(cfg["shape"]) == TILE and cfg["num_inputs"] == 1

    os.mkdir(str(tmp_path / "out_s"))
    np.save(str(tmp_path / "one.npy"), imgs[1:2])
    seg = {"input": str(tmp_path / "one.npy"), "model": info["model_dir"], "shape": TILE, "margin": 4, "num_outputs": 2,
           "output": str(tmp_path / "out_s")}
    sinfo = jobs.SERVER_segment_frames(seg, {"gpu": 0})
    assert sinfo["frames"] == 1 and sinfo["tile"] == 32
    mask = np.load(str(tmp_path / "out_s" / "mask.npy"))
    assert mask.shape == (1, 80, 96) and mask.dtype == np.uint8
    net = UNet2D({"shape": TILE, "num_outputs": 2, "device": DEV}, "infer")
    net.load_state_dict(utils.load_model_weights(info["model_dir"]), strict=True)
    assert np.array_equal(mask, segment_frames(net, imgs[1:2], tile=32, margin=4))

    # the first batch, restated
    plan, coef = tile_sample_plan(STACK[1:], TILE, STACK[0], 3 * per, np.random.default_rng(5), ("rotate",))
    wmap = device_weightmaps(lab, 10., 5., device=DEV).cpu().numpy()
    assert wmap.shape == STACK + (1,)
    batch = [dev(a) for a in tc.np_sample(tc.np_normalised(imgs), lab, wmap[..., 0], plan[:4], coef[:4], TILE, 2)]
    net_p = {"shape": TILE, "num_inputs": 1, "num_outputs": 2, "dropout": 0.0, "seed": 5, "device": DEV}
    fresh = [float(UNetTrainer(net_p).step(*batch).cpu()) for _ in range(2)]
    print("first loss: job %r, fresh trainers %r" % (tj["losses"][0], fresh))
    assert np.float32(fresh[0]).tobytes() == np.float32(fresh[1]).tobytes(), fresh
    assert np.float32(tj["losses"][0]).tobytes() == np.float32(fresh[0]).tobytes(), (tj["losses"][0], fresh)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_train_job_graph_replay_equals_eager(dtype, tmp_path, monkeypatch):
    """options['graph'] True and False: the same losses, bit for bit -- what test_gpu_train.py holds the captured step to
    against the eager one (le.item() == lg.item()); the sampler writes into the capture's static buffers from step 2 on"""
    _stack(tmp_path)
    _, graphed = _job(tmp_path, monkeypatch, "out_g", {"graph": True}, dtype=dtype, augment=("rotate", "flip"))
    _, eager = _job(tmp_path, monkeypatch, "out_e", {"graph": False}, dtype=dtype, augment=("rotate", "flip"))
    print("losses (%s): graph %r, eager %r" % (dtype, graphed["losses"], eager["losses"]))
    assert graphed["graph"] is True and eager["graph"] is False and graphed["dtype"] == dtype
    assert len(graphed["losses"]) == 3 and np.isfinite(graphed["losses"]).all()
    assert graphed["losses"] == eager["losses"]
