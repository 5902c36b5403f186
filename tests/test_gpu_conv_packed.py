"""GPU: the packed form of the 64-channel-block f32 3x3 convolution (conv_mfma_f32_packed_kernel: A operands from the per-model
fragment pack, halo double-buffered, one barrier per item) against the unpacked kernel on the same tensors -- the same call with
SQ_CONV_PACKED=0, which the existing sweeps pin to the oracle and to fp64.  Every comparison is torch.equal: the packed form keeps
every output's fmaf chain.  Each case first asserts, through sq_conv_walk_plan, that the 64-channel-block plan takes its shape
(ntiles x Cout / 64 >= 512) and that the packed kernel would take the call -- a smaller shape falls to narrower blocks and proves
nothing.  The device pack itself is compared bit for bit with the numpy statement of its order (tests/conv_packed_cases.py).
The walk sweep (pc.PACKED_WALKS) compares the packed kernel itself with the C oracle, on outputs between sentinel bands: the two
kernels share the walk and the epilogue text, so a fault common to both shows only there."""
import os
import zlib

import numpy as np
import pytest
import torch

from oracle import c_oracle as co
from sequitr_amd import _lib, ops
from sequitr_amd.networks.unet import UNet2D, init_unet_weights
from tests import conv_packed_cases as pc
from tests import f32_walk_cases as wc

pytestmark = pytest.mark.gpu


class unpacked(object):
    """`with unpacked():` -- SQ_CONV_PACKED=0 (read per call): the same call runs the unpacked kernel"""

    def __enter__(self):
        self.prev = os.environ.get("SQ_CONV_PACKED")
        os.environ["SQ_CONV_PACKED"] = "0"

    def __exit__(self, *exc):
        if self.prev is None:
            del os.environ["SQ_CONV_PACKED"]
        else:
            os.environ["SQ_CONV_PACKED"] = self.prev
        return False


def _inputs(N, H, W, Cin, Cout, seed, weights="normal"):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn((N, H, W, Cin), generator=g)
    x[:, ::7, ::5, ::3] = -0.0                                   # negative zeros in the activations ...
    w = torch.randn((3, 3, Cin, Cout), generator=g) / float(np.sqrt(9 * Cin))
    if weights == "denormal":                                    # ... and a filter at the denormal scale, negative zeros in it:
        w = w * 1e-39                                            # a pack that scaled, rounded or flushed a value would show
        w[:, :, ::3, ::5] = -0.0
    b = torch.randn((Cout,), generator=g) * 0.1
    return x.cuda(), w.cuda(), b.cuda()


def _takes(form, N, H, W, Cin, Cout, act):
    on64, p = pc.on_64_blocks(form, N, H, W, Cin, Cout, act)
    assert on64, "the case does not reach the 64-channel-block plan: %r" % (p,)
    assert ops.conv_packed_takes((N, H, W, Cin), (3, 3, Cin, Cout)), "the packed kernel declines the case"
    return p


# chunks per tile 1, 2, 4, 16; channel blocks 1, 2, 4; one tile per block (ntiles x cblocks exactly 512)
REGIMES = [(2, 256, 256, 16, 64), (2, 256, 256, 32, 64), (4, 128, 128, 64, 128), (2, 128, 128, 256, 256)]


@pytest.mark.parametrize("N,H,W,Cin,Cout", REGIMES)
def test_chunks_and_channel_blocks(N, H, W, Cin, Cout):
    p = _takes(wc.PLAIN, N, H, W, Cin, Cout, "relu")
    assert p["items"] * p["cblocks"] == 512 and p["tmax"] == 1 and p["cblocks"] == Cout // 64
    x, w, b = _inputs(N, H, W, Cin, Cout, Cin * 7 + Cout)
    pk = ops.pack_filter(w)
    y = ops.conv2d(x, w, b, act="relu", pack=pk)
    with unpacked():
        ref = ops.conv2d(x, w, b, act="relu", pack=pk)
    assert torch.equal(y, ref)
    assert torch.equal(ref, ops.conv2d(x, w, b, act="relu"))      # and the switch really is the call without a pack


# (3, 256, 256): 768 tiles, two per block, two chunks per tile -- the ring crosses item AND tile boundaries, the walk crosses
# from one image into the next; (5, 256, 256): 1280 tiles over 427 blocks -- three tiles for most, two for the last (uneven);
# (3, 250, 250): partial tiles on the right and at the bottom, the non-fast epilogue
WALKS = [(3, 256, 256, 2, 2), (5, 256, 256, 2, 3), (3, 250, 250, 2, 2)]


@pytest.mark.parametrize("N,H,W,tmin,tmax", WALKS)
@pytest.mark.parametrize("act,bias", [("relu", True), (None, False), ("leaky", True)])
def test_tiles_per_block_borders_and_epilogues(N, H, W, tmin, tmax, act, bias):
    Cin, Cout = 32, 64
    p = _takes(wc.PLAIN, N, H, W, Cin, Cout, act)
    assert (p["tmin"], p["tmax"]) == (tmin, tmax) and p["G"] < p["items"]
    assert p["G"] % (p["items"] // N) != 0                       # the stride is no whole number of images: the walk crosses them
    x, w, b = _inputs(N, H, W, Cin, Cout, N * 1000 + H, weights="denormal" if act is None else "normal")
    b = b if bias else None
    pk = ops.pack_filter(w)
    y = ops.conv2d(x, w, b, act=act, pack=pk)
    with unpacked():
        ref = ops.conv2d(x, w, b, act=act, pack=pk)
    assert torch.equal(y, ref)


@pytest.mark.parametrize("N,H,W,Cin,Cout", [(2, 256, 256, 32, 64), (3, 256, 256, 32, 64), (4, 128, 128, 64, 128)])
@pytest.mark.parametrize("act", ["relu", "leaky"])
def test_pool_epilogue(N, H, W, Cin, Cout, act):
    _takes(wc.POOL, N, H, W, Cin, Cout, act)
    x, w, b = _inputs(N, H, W, Cin, Cout, 31 * N + Cin)
    pk = ops.pack_filter(w)
    y, pooled = ops.conv3x3_pool(x, w, b, act=act, pack=pk)
    with unpacked():
        ry, rp = ops.conv3x3_pool(x, w, b, act=act, pack=pk)
    assert torch.equal(y, ry) and torch.equal(pooled, rp)
    assert torch.equal(rp, torch.nn.functional.max_pool2d(ry.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1))


# ---- the walk sweep: every case of pc.PACKED_WALKS against the C oracle, on guarded outputs ------------------------------------
def _launch(x, w, wp, b, y, p, act):
    """one call of the packed entry points (the pooled one where `p` is given) into the guarded outputs; asserts their bands"""
    N, H, W, Cin = x.shape
    Cout = w.shape[3]
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    bp = b.data_ptr() if b is not None else None
    if p is not None:
        _lib.check(lib.sq_conv3x3_pool_packed_fwd_f32(x.data_ptr(), w.data_ptr(), wp.data_ptr(), bp, y.t.data_ptr(), p.t.data_ptr(),
                                                      N, H, W, Cin, Cout, ops.ACT[act], st), "sq_conv3x3_pool_packed_fwd_f32")
    else:
        _lib.check(lib.sq_conv2d_packed_nhwc_fwd_f32(x.data_ptr(), w.data_ptr(), wp.data_ptr(), bp, y.t.data_ptr(), N, H, W, Cin,
                                                     Cout, 3, 1.0, ops.ACT[act], st), "sq_conv2d_packed_nhwc_fwd_f32")
    torch.cuda.synchronize()
    assert y.bands_intact(), "a store outside y"
    assert p is None or p.bands_intact(), "a store outside pooled"


def _run_guarded(x, w, wp, b, act, pooled, runs=1):
    """(y, pooled or None): `runs` calls in a row into the same guarded outputs, every one with the first one's bits"""
    N, H, W, _ = x.shape
    Cout = w.shape[3]
    y = pc.Guarded(N, H, W, Cout)
    p = pc.Guarded(N, H // 2, W // 2, Cout) if pooled else None
    _launch(x, w, wp, b, y, p, act)
    assert y.all_stored() and (p is None or p.all_stored()), "an output element never stored"
    if runs > 1:
        first = (y.t.clone(), p.t.clone() if pooled else None)
        for i in range(1, runs):
            _launch(x, w, wp, b, y, p, act)
            assert torch.equal(y.t, first[0]) and (not pooled or torch.equal(p.t, first[1])), "run %d differs from the first" % i
    return y.t, (p.t if pooled else None)


def _seed(c):
    return zlib.crc32(pc.packed_case_id(c).encode())


_shared = {}


def _walk_case(c):
    """inputs on the device and the oracle's output of a case, computed once and left unchanged"""
    if c not in _shared:
        x, w, b = _inputs(c.N, c.H, c.W, c.Cin, c.Cout, _seed(c))
        b = b if c.bias else None
        ref = co.conv2d(x.cpu().numpy(), w.cpu().numpy(), None if b is None else b.cpu().numpy(), act=c.act)
        _shared[c] = (x, w, b, ref)
    return _shared[c]


def _max_pool(y):
    return torch.nn.functional.max_pool2d(y.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)


@pytest.mark.parametrize("c", pc.PACKED_WALKS, ids=pc.packed_case_id)
def test_walks_equal_the_c_oracle(c, monkeypatch):
    """Bit for bit against oracle/sq_oracle.c and against the unpacked kernel, at the walks the table declares (checked on the
    CPU by tests/test_conv_packed_cpu.py): odd chunk counts, channel blocks beyond the first on walks of several tiles, walks of
    four and five tiles, every carry of the stride, ragged last tiles of one and fifteen pixels, single rows and columns of tiles,
    the pooled epilogue on ragged shapes.  The outputs lie between sentinel bands; the call runs twice into the same buffers."""
    monkeypatch.delenv("SQ_CONV_PACKED", raising=False)
    p = _takes(c.form, c.N, c.H, c.W, c.Cin, c.Cout, c.act)
    pooled = c.form == wc.POOL
    x, w, b, ref = _walk_case(c)
    pk = ops.pack_filter(w)
    y, pl = _run_guarded(x, w, pk.wp, b, c.act, pooled, runs=2)
    msg = pc.mismatch(y.cpu().numpy(), ref, p, c.H, c.W)
    assert msg is None, "packed kernel against the oracle [%s]\n%s" % (pc.packed_case_id(c), msg)
    with unpacked():
        assert not ops.conv_packed_takes((c.N, c.H, c.W, c.Cin), (3, 3, c.Cin, c.Cout))
        ry, rp = _run_guarded(x, w, pk.wp, b, c.act, pooled)
    assert torch.equal(y, ry)
    if pooled:
        assert torch.equal(pl, _max_pool(y))
        assert torch.equal(pl, rp)


@pytest.mark.parametrize("pooled", [False, True], ids=["plain", "pool"])
def test_non_finite_activations(pooled, monkeypatch):
    """NaN, +inf and -inf in x (pc.nonfinite_plants: a tile's first and last pixel, halo pixels of the ragged border tiles, image
    corners, the first and the last channel) at 2 x 250 x 278, 32 -> 128, ReLU with a bias, three tiles per block.  The packed and
    the unpacked kernel agree: NaN at the same outputs, the same bits everywhere else.  Both store a NaN pre-activation as +0 under
    ReLU -- fmaxf(v, 0) on whole tiles, v > 0 ? v : 0 on partial ones -- so no NaN is left, and every output whose neighbourhood
    holds a NaN is +0.  Wherever the whole 3x3 x Cin neighbourhood is finite the output equals the oracle bit for bit.
    The oracle itself applies ReLU as v > 0.0f ? v : 0.0f: a NaN or -inf pre-activation gives +0, +inf stays +inf
    (tests/test_conv_packed_cpu.py pins that); its outputs beside non-finite inputs are not relied on here."""
    monkeypatch.delenv("SQ_CONV_PACKED", raising=False)
    c = pc.NONFINITE_CASE
    p = _takes(wc.POOL if pooled else wc.PLAIN, c.N, c.H, c.W, c.Cin, c.Cout, "relu")
    assert p["tmax"] >= 2
    x, w, b = _inputs(c.N, c.H, c.W, c.Cin, c.Cout, _seed(c) + 1)
    xh = x.cpu()
    for (n, yy, xx, ch, v) in pc.nonfinite_plants(c.N, c.H, c.W, c.Cin):
        xh[n, yy, xx, ch] = v
    x = xh.cuda()
    finite, has_nan = pc.neighbourhoods(xh)
    assert 0 < int(has_nan.sum()) < int((~finite).sum()) < 200
    pk = ops.pack_filter(w)
    y, pl = _run_guarded(x, w, pk.wp, b, "relu", pooled, runs=2)
    with unpacked():
        ry, rp = _run_guarded(x, w, pk.wp, b, "relu", pooled)
    nan = torch.isnan(y)
    assert torch.equal(nan, torch.isnan(ry))
    assert torch.equal(y.view(torch.int32)[~nan], ry.view(torch.int32)[~nan])
    assert not bool(nan.any())
    yh = y.cpu()
    assert bool((yh[has_nan].view(torch.int32) == 0).all()), "a NaN pre-activation not stored as +0"
    assert bool(torch.isinf(yh[~finite]).any())                       # the infinities did reach outputs
    ref = co.conv2d(xh.numpy(), w.cpu().numpy(), b.cpu().numpy(), act="relu")
    got = np.where(finite.numpy()[..., None], yh.numpy(), ref)
    msg = pc.mismatch(got, ref, p, c.H, c.W)
    assert msg is None, "outputs with a finite neighbourhood against the oracle\n%s" % msg
    if pooled:
        assert torch.equal(pl, _max_pool(y)) and torch.equal(pl, rp)


@pytest.mark.parametrize("Cin", [16, 48])
@pytest.mark.parametrize("Cout", [64, 192])
def test_device_pack_is_the_numpy_pack_bit_for_bit(Cin, Cout):
    rng = np.random.default_rng(Cin + Cout)
    w = (rng.standard_normal((3, 3, Cin, Cout)) * 0.1).astype(np.float32)
    bits = w.view(np.uint32)
    bits[0, :, ::2, ::3] = 0x80000000                            # -0.0
    bits[1, :, 1::2, ::5] = rng.integers(1, 1 << 23, bits[1, :, 1::2, ::5].shape, dtype=np.uint32)      # denormals
    bits[2, 0, 0, :4] = (0x7FC00001, 0xFFC12345, 0x7F800000, 0x00000001)    # NaN payloads, inf, the smallest denormal
    pk = ops.pack_filter(torch.from_numpy(w).cuda())
    got = pk.wp.cpu().numpy()
    assert got.shape == (9 * Cin * Cout,)
    assert np.array_equal(got.view(np.uint32), pc.pack_numpy(w).view(np.uint32))


def test_fallbacks_run_the_unpacked_kernels():
    N, H, W = 2, 256, 256
    x, w, b = _inputs(N, H, W, 32, 64, 5)
    pk = ops.pack_filter(w)
    # wscale != 1: the pack holds unscaled weights, so the call runs the unpacked kernel on w
    assert torch.equal(ops.conv2d(x, w, b, act="relu", wscale=0.5, pack=pk), ops.conv2d(x, w, b, act="relu", wscale=0.5))
    # Cout = 96 and K = 1 have no pack
    w96 = torch.randn((3, 3, 32, 96), device="cuda") * 0.05
    assert ops.pack_filter(w96) is None
    with pytest.raises(ValueError):
        ops.FilterPackF32(w96)
    b96 = torch.zeros(96, device="cuda")
    y96 = ops.conv2d(x, w96, b96, act="relu", pack=None)
    with unpacked():
        assert torch.equal(y96, ops.conv2d(x, w96, b96, act="relu"))
    w1 = torch.randn((1, 1, 32, 64), device="cuda") * 0.1
    assert ops.pack_filter(w1) is None
    # ... and the entry points themselves decline a pack pointer on such calls (the pointer is never read): K = 1, Cout = 96 and
    # wscale = 0.5 through sq_conv2d_packed_nhwc_fwd_f32 with a non-NULL wp give the unpacked entry's bits
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    for wt, bt, ws in ((w1, b, 1.0), (w96, b96, 1.0), (w, b, 0.5)):
        K, Cout = wt.shape[0], wt.shape[3]
        y = torch.empty((N, H, W, Cout), device="cuda")
        _lib.check(lib.sq_conv2d_packed_nhwc_fwd_f32(x.data_ptr(), wt.data_ptr(), pk.wp.data_ptr(), bt.data_ptr(), y.data_ptr(),
                                                     N, H, W, 32, Cout, K, ws, 1, st), "sq_conv2d_packed_nhwc_fwd_f32")
        assert torch.equal(y, ops.conv2d(x, wt, bt, act="relu", wscale=ws))
    # a pack handed to a call on another filter tensor is refused, never matched by pointer
    with pytest.raises(ValueError):
        ops.conv2d(x, w.clone(), b, act="relu", pack=pk)
    # a shape off the 64-channel-block plan with a pack: the unpacked kernel, same bits
    xs = x[:1, :64, :64].contiguous()
    assert not ops.conv_packed_takes(tuple(xs.shape), tuple(w.shape))
    y = ops.conv2d(xs, w, b, act="relu", pack=pk)
    assert torch.equal(y, ops.conv2d(xs, w, b, act="relu"))


def test_a_tensor_over_2gib_with_a_pack_takes_the_64bit_kernel():
    """The packed kernel addresses with 32-bit buffer offsets, as the unpacked persistent one: a call whose output reaches 2 GiB
    runs what it runs without a pack (the 64-bit-addressed kernel), not an error.  16 -> 64 at 32 x 512 x 512: y is exactly 2 GiB."""
    N, H, W, Cin, Cout = 32, 512, 512, 16, 64
    assert N * H * W * Cout * 4 >= 2 ** 31 and pc.on_64_blocks(wc.PLAIN, N - 1, H, W, Cin, Cout)[0]
    assert not ops.conv_packed_takes((N, H, W, Cin), (3, 3, Cin, Cout)) and ops.conv_packed_takes((N - 1, H, W, Cin), (3, 3, Cin, Cout))
    g = torch.Generator(device="cuda:0").manual_seed(0)
    x = torch.randn((N, H, W, Cin), device="cuda:0", generator=g)
    _, w, b = _inputs(1, 16, 16, Cin, Cout, 9)
    pk = ops.pack_filter(w)
    y = ops.conv2d(x, w, b, act="relu", pack=pk)
    for n in (0, 17, 31):                                        # batch independence: the image on its own runs the packed kernel's plan
        assert torch.equal(y[n:n + 1], ops.conv2d(x[n:n + 1].contiguous(), w, b, act="relu")), n
    del x, y
    torch.cuda.empty_cache()


def _net(filters, bridge="eltwise_mul", seed=0):
    params = {"shape": (256, 256), "num_inputs": 1, "num_outputs": 2, "filters": filters, "bridge": bridge,
              "device": "cuda:0", "seed": seed}
    net = UNet2D(params, "infer")
    net.load_state_dict(init_unet_weights(params, seed=seed))
    return net, params


def _logits_and_mask(net, x):
    mask = net.predict(x)
    return net.logits().clone(), mask.clone()


def test_concat_bridge_gets_no_pack_for_its_two_source_conv():
    net, _ = _net((16, 64), bridge="concat")
    x = torch.randn((8, 256, 256, 1), device="cuda")
    lg, mk = _logits_and_mask(net, x)
    with unpacked():
        rl, rm = _logits_and_mask(net, x)
    assert torch.equal(lg, rl) and torch.equal(mk, rm)


def test_a_pack_is_never_stale():
    """filters (16, 64) on 8 tiles of 256 x 256: level 1 is 16 -> 64 and 64 -> 64 at 8 x 128 x 128 = 512 tiles, packed"""
    net, params = _net((16, 64))
    x = torch.randn((8, 256, 256, 1), device="cuda")
    key = "UNet/down1/conv2/kernel"
    assert ops.conv_packed_takes((8, 128, 128, 64), tuple(net._vars[key].shape))
    assert net._packs[key] is not None and net._packs["UNet/down1/conv1/kernel"] is not None      # made by load_state_dict
    first, _ = _logits_and_mask(net, x)

    def check(changed_from):
        lg, mk = _logits_and_mask(net, x)
        with unpacked():
            rl, rm = _logits_and_mask(net, x)
        assert torch.equal(lg, rl) and torch.equal(mk, rm)
        assert not torch.equal(lg, changed_from)                  # the new weights do show in the output
        return lg

    # an in-place write through the raw pointer, announced as every such write in this code base is
    w = net._vars[key]
    w.copy_(w * 1.25 + 0.01)
    ops.invalidate_packs()
    second = check(first)
    # an Adam wrapper updates the parameter in place and bumps the epoch itself
    g = torch.randn_like(w)
    ops.adam_step(w, g, torch.zeros_like(w), torch.zeros_like(w), 0.05, 0.9, 0.999, 1e-8, 1)
    third = check(second)
    # load_state_dict with other weights rebuilds every pack
    net.load_state_dict(init_unet_weights(params, seed=3))
    check(third)


def test_a_replayed_graph_reads_current_packs():
    """GraphedPredict replays the captured packed kernels without running ops: it refreshes the net's packs before a replay"""
    from sequitr_amd.networks.unet import GraphedPredict
    net, _ = _net((16, 64))
    x = torch.randn((8, 256, 256, 1), device="cuda")
    graphed = GraphedPredict(net, tuple(x.shape))
    mk, lg = graphed(x)
    first = lg.clone()
    with unpacked():
        rl, rm = _logits_and_mask(net, x)
    assert torch.equal(first, rl) and torch.equal(mk, rm)
    w = net._vars["UNet/down1/conv2/kernel"]
    w.copy_(w * 0.75 - 0.02)
    ops.invalidate_packs()
    mk, lg = graphed(x)
    with unpacked():
        rl, rm = _logits_and_mask(net, x)
    assert torch.equal(lg, rl) and torch.equal(mk, rm) and not torch.equal(lg, first)


def test_whole_net_bit_equal_with_the_switch_on_and_off():
    """The workload's filters.  On 2 tiles of 256 x 256 the 64-, 128- and 256-channel levels have 32, 16 and 8 (tile, channel
    block) pairs, far from the 512 the 64-channel-block plan needs, so no layer runs the packed kernel there: that batch checks
    the fall-back of every layer, and 32 tiles (512 tiles of 64 channels at level 2) is the smallest batch at which layers do."""
    filters = (16, 32, 64, 128, 256)
    net, _ = _net(filters)
    g = torch.Generator(device="cpu").manual_seed(11)
    for ntile in (2, 32):
        x = torch.randn((ntile, 256, 256, 1), generator=g).cuda()
        lg, mk = _logits_and_mask(net, x)
        with unpacked():
            rl, rm = _logits_and_mask(net, x)
        assert torch.equal(lg, rl) and torch.equal(mk, rm)
    # encoder conv1 / conv2 and, below the deepest level, the two decoder convs f -> f of every level
    took = [(lvl, ci, f) for lvl, f in enumerate(filters)
            for ci in (((filters[lvl - 1] if lvl else 1), f) + ((f, f) if lvl < len(filters) - 1 else ()))
            if lvl >= 2 and ops.conv_packed_takes((32, 256 >> lvl, 256 >> lvl, ci), (3, 3, ci, f))]
    assert took, "no layer of the 32-tile batch took the packed form"
    assert all(net._packs["UNet/down%d/conv2/kernel" % lvl] is not None for lvl in (2, 3, 4))
