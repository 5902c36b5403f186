"""GPU parity for the whole U-Net forward (sequitr/networks/unet.py:224-322 wiring) through
the operator API: logits, every intermediate layer and the argmax mask are BIT-EXACT
against the C oracle; full-size batches are covered by size-independent properties."""
import numpy as np
import pytest
import torch

from oracle import unet_oracle
from sequitr_amd import ops
from sequitr_amd.networks.unet import UNet2D, init_unet_weights
from tests.util import tiles, rand_weights, assert_bit_exact

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make(params, seed=0, cls=UNet2D):
    net = cls(dict(params, device="cuda:0"), "infer")
    w = init_unet_weights(params, seed)
    net.load_state_dict(w)
    return net, w


@pytest.mark.parametrize("fuse", [False, True])
@pytest.mark.parametrize("bridge", ["eltwise_mul", "eltwise_add", "eltwise_sub", None])
def test_forward_64px_every_layer_bit_exact(bridge, fuse):
    """hook-by-hook graph (fuse=False) and the fused-kernel graph (fuse=True): same bits."""
    params = {"shape": (64, 64), "bridge": bridge, "fuse": fuse}
    net, w = make(params, seed=3)
    x = tiles(0, 2, 64, 64)
    mask = net.predict(x)
    ref_logits, ref_net = unet_oracle.unet_forward(x, w, params, return_net=True)
    assert len(net._net) == len(ref_net) == 10
    for i, (a, b) in enumerate(zip(net._net, ref_net)):
        if a is None:                                   # fused head: up0's activation is not materialised
            assert fuse and i == 8
            continue
        assert_bit_exact(a.cpu().numpy(), b, "layer %d (%s)" % (i, bridge))
    assert_bit_exact(mask.cpu().numpy(), unet_oracle.predict_mask(ref_logits), "mask")


def test_fused_kernels_individually_bit_exact():
    from oracle import c_oracle as co
    from tests.util import rand_weights
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    x1 = tiles(20, 2, 48, 40, 1)                          # ragged vs the 16x16 tile, N = 2
    w1, b1 = rand_weights(21, (3, 3, 1, 16), 0.5), rand_weights(22, (16,), 0.1)
    w2, b2 = rand_weights(23, (3, 3, 16, 16)), rand_weights(24, (16,), 0.1)
    ref = co.conv2d(co.conv2d(x1, w1, b1, act="relu"), w2, b2, act="relu")
    y, p = ops.conv3x3_first_block(dev(x1), dev(w1), dev(b1), dev(w2), dev(b2))
    assert_bit_exact(y.cpu().numpy(), ref, "first block y")
    assert_bit_exact(p.cpu().numpy(), co.maxpool2x2(ref), "first block pooled")
    for cin, cout in ((16, 32), (32, 32), (64, 128)):
        x = tiles(25, 1, 32, 48, cin)
        w, b = rand_weights(26, (3, 3, cin, cout)), rand_weights(27, (cout,), 0.1)
        r = co.conv2d(x, w, b, act="relu")
        y, p = ops.conv3x3_pool(dev(x), dev(w), dev(b))
        assert_bit_exact(y.cpu().numpy(), r, "conv+pool y %d->%d" % (cin, cout))
        assert_bit_exact(p.cpu().numpy(), co.maxpool2x2(r), "conv+pool pooled %d->%d" % (cin, cout))
    x = tiles(28, 2, 40, 24, 16)
    w, b = rand_weights(29, (3, 3, 16, 16)), rand_weights(30, (16,), 0.1)
    for hc in (1, 2, 3):
        hw, hb = rand_weights(31, (1, 1, 16, hc)), rand_weights(32, (hc,), 0.1)
        r = co.conv2d(co.conv2d(x, w, b, act="relu"), hw, hb, act=None)
        logits, mask = ops.conv3x3_head(dev(x), dev(w), dev(b), dev(hw), dev(hb))
        assert_bit_exact(logits.cpu().numpy(), r, "fused head logits C=%d" % hc)
        assert_bit_exact(mask.cpu().numpy(), co.argmax_u8(r), "fused head mask C=%d" % hc)


@pytest.mark.parametrize("shape", [(2, 64, 80), (1, 16, 16), (3, 32, 48), (1, 96, 96)])
def test_level0_kernel_family_bit_exact(shape):
    """sq_conv_f32_l0.hip (16 -> 16 channels, H and W multiples of 16: filter in registers, channel-transposed halo
    image, head from registers, FIRST / UP with two barriers per tile) against the C oracle, bit for bit: tiles on the
    image border and interior tiles (their loads take the unchecked path), one tile and several tiles per image."""
    from oracle import c_oracle as co
    from tests.util import rand_weights
    N, H, W = shape
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    w, b = rand_weights(41, (3, 3, 16, 16)), rand_weights(42, (16,), 0.1)
    x = tiles(43, N, H, W, 16)
    r = co.conv2d(x, w, b, act="relu")
    assert_bit_exact(ops.conv2d(dev(x), dev(w), dev(b), act="relu").cpu().numpy(), r, "plain 16->16")
    w32, b32 = rand_weights(51, (3, 3, 16, 32)), rand_weights(52, (32,), 0.1)
    assert_bit_exact(ops.conv2d(dev(x), dev(w32), dev(b32), act="relu").cpu().numpy(), co.conv2d(x, w32, b32, act="relu"), "plain 16->32")
    y, p = ops.conv3x3_pool(dev(x), dev(w), dev(b))
    assert_bit_exact(y.cpu().numpy(), r, "conv+pool y")
    assert_bit_exact(p.cpu().numpy(), co.maxpool2x2(r), "conv+pool pooled")
    hw, hb = rand_weights(44, (1, 1, 16, 2)), rand_weights(45, (2,), 0.1)
    rl = co.conv2d(r, hw, hb, act=None)
    logits, mask = ops.conv3x3_head(dev(x), dev(w), dev(b), dev(hw), dev(hb))
    assert_bit_exact(logits.cpu().numpy(), rl, "head logits")
    assert_bit_exact(mask.cpu().numpy(), co.argmax_u8(rl), "head mask")
    x1 = tiles(46, N, H, W, 1)
    w1, b1 = rand_weights(47, (3, 3, 1, 16), 0.5), rand_weights(48, (16,), 0.1)
    r1 = co.conv2d(co.conv2d(x1, w1, b1, act="relu"), w, b, act="relu")
    y, p = ops.conv3x3_first_block(dev(x1), dev(w1), dev(b1), dev(w), dev(b))
    assert_bit_exact(y.cpu().numpy(), r1, "first block y")
    assert_bit_exact(p.cpu().numpy(), co.maxpool2x2(r1), "first block pooled")
    y, p = ops.conv3x3_first_block(dev(x1), dev(w1), dev(b1), dev(w), dev(b), want_pool=False)
    assert p is None
    assert_bit_exact(y.cpu().numpy(), r1, "first block y (no pool)")
    rng = np.random.default_rng(H + W)
    xl = rng.standard_normal((N, H // 2, W // 2, 32)).astype(np.float32)
    wt, bt = rand_weights(49, (2, 2, 16, 32), 0.2), rand_weights(50, (16,), 0.1)
    for bridge in ("eltwise_mul", "eltwise_add", "eltwise_sub", None):
        y = ops.convT_conv3x3(dev(xl), dev(wt), dev(bt), dev(x), bridge, dev(w), dev(b), act="relu")
        merged = co.convT2x2s2(xl, wt, bt, skip=x if bridge else None, bridge=bridge)
        assert_bit_exact(y.cpu().numpy(), co.conv2d(merged, w, b, act="relu"), "fused up block (%s)" % bridge)


def test_lazy_init_equals_host_init():
    """variables created lazily during build() draw the same stream as init_unet_weights."""
    params = {"shape": (32, 32), "seed": 7, "device": "cuda:0"}
    net = UNet2D(params, "infer")
    net.build(tiles(1, 1, 32, 32))
    w = init_unet_weights(params, seed=7)
    sd = net.state_dict()
    assert set(sd) == set(w)
    for k in w:
        assert np.array_equal(sd[k], w[k]), k


def test_forward_512px_tile_bit_exact():
    """BASELINE config 1/2 tile size: one 512x512x1 tile, default filters, vs the oracle."""
    params = {"shape": (512, 512)}
    net, w = make(params, seed=0)
    x = tiles(0, 1, 512, 512)
    mask = net.predict(x)
    ref = unet_oracle.unet_forward(x, w, params)
    assert_bit_exact(net.logits().cpu().numpy(), ref, "logits 512")
    assert_bit_exact(mask.cpu().numpy(), unet_oracle.predict_mask(ref), "mask 512")


def test_full_batch_properties():
    """N=32 x 512^2 (BASELINE config 2) without a 5-minute oracle run: (i) two runs are
    bit-identical; (ii) tiles are independent -- tile k of the batch equals the same tile
    run alone; (iii) the fused mask equals argmax of the logits."""
    params = {"shape": (512, 512)}
    net, _ = make(params, seed=0)
    x = torch.from_numpy(tiles(1, 32, 512, 512)).cuda()
    m1 = net.predict(x).clone()
    l1 = net.logits().clone()
    m2 = net.predict(x)
    assert torch.equal(l1, net.logits()) and torch.equal(m1, m2)
    for k in (0, 17, 31):
        mk = net.predict(x[k:k + 1].contiguous())
        assert torch.equal(net.logits()[0], l1[k]) and torch.equal(mk[0], m1[k])
    assert torch.equal(ops.argmax_u8(l1), m1)
    frac = m1.float().mean().item()
    assert 0.0 < frac < 1.0


def test_hook_override_and_unfused_path():
    """Operator API: a subclass may override any leaf hook (unet.py:326-343); overriding
    conv_transpose_layer disables the fused convT+bridge kernel and must give the same bits."""
    class Plain(UNet2D):
        def conv_transpose_layer(self, x, filters):
            return UNet2D.conv_transpose_layer(self, x, filters)

        def max_pool_layer(self, x):              # the name build() calls, unet.py:242
            self.pool_calls = getattr(self, "pool_calls", 0) + 1
            return UNet2D.pool_layer(self, x)

    params = {"shape": (64, 64)}
    a, _ = make(params, seed=5)
    b, _ = make(params, seed=5, cls=Plain)
    x = tiles(2, 1, 64, 64)
    assert torch.equal(a.build(x), b.build(x))
    assert b.pool_calls == 4


@pytest.mark.parametrize("filters,size", [((16, 32, 64), 32), ((16, 32, 64, 128, 256), 64)])
def test_concat_bridge_bit_exact_without_materialising_the_concat(filters, size):
    """bridge = 'concat' (unet.py:196-197): conv1 of every up block reads its input channels from TWO tensors (the
    up-scaled one first, the skip one second; sq_conv2d_concat_nhwc_fwd_f32) -- logits, every layer and the mask are
    bit-identical to the C oracle run on the materialised concatenation, and to the torch.cat graph (fused = same bits)."""
    params = {"shape": (size, size), "bridge": "concat", "filters": filters}
    net, w = make(params, seed=1)
    x = tiles(3, 2, size, size)
    mask = net.predict(x)
    ref_logits, ref_net = unet_oracle.unet_forward(x, w, params, return_net=True)
    assert w["UNet/up0/conv1/kernel"].shape == (3, 3, 2 * filters[0], filters[0])
    for i, (a, b) in enumerate(zip(net._net, ref_net)):
        assert_bit_exact(a.cpu().numpy(), b, "concat net[%d]" % i)
    assert_bit_exact(mask.cpu().numpy(), unet_oracle.predict_mask(ref_logits), "concat mask")
    from oracle import torch_ref
    assert np.max(np.abs(net.logits().cpu().numpy() - torch_ref.unet_forward(x, w, params))) < 1e-4
    # the operator alone against the conv on torch.cat, ragged tile sizes and a 1x1 kernel
    for (n, h, wd, ca, co, k) in ((2, 20, 27, 16, 32, 3), (1, 16, 16, 64, 16, 3), (1, 9, 33, 32, 32, 1)):
        xa, xb = tiles(5, n, h, wd, ca), tiles(6, n, h, wd, ca)
        wt, bs = rand_weights(7, (k, k, 2 * ca, co)), rand_weights(8, (co,), 0.1)
        got = ops.conv2d_concat(dev(xa), dev(xb), dev(wt), dev(bs), act="relu")
        want = ops.conv2d(torch.cat([dev(xa), dev(xb)], -1).contiguous(), dev(wt), dev(bs), act="relu")
        assert torch.equal(got, want), (n, h, wd, ca, co, k)


def test_rejects_cpu_device_and_bad_bridge():
    with pytest.raises(RuntimeError):
        UNet2D({"device": "cpu"}, "infer")
    with pytest.raises(ValueError):
        UNet2D({"bridge": "nope", "device": "cuda:0"}, "infer")


def test_up_kernel_3x3_transpose_conv_bit_exact_and_trainable():
    """SURVEY A.1 alternative conv_transpose_layer: kernel (3,3), stride 2, SAME."""
    from oracle import torch_ref as tr
    from sequitr_amd.train import UNetTrainer
    params = {"shape": (32, 32), "filters": (16, 32, 64), "up_kernel": (3, 3)}
    net, w = make(params, seed=5)
    assert w["UNet/up0/upscale/kernel"].shape == (3, 3, 16, 32)
    x = tiles(2, 2, 32, 32)
    mask = net.predict(x)
    ref_logits, ref_net = unet_oracle.unet_forward(x, w, params, return_net=True)
    for i, (a, b) in enumerate(zip(net._net, ref_net)):
        assert_bit_exact(a.cpu().numpy(), b, "layer %d" % i)
    assert_bit_exact(mask.cpu().numpy(), unet_oracle.predict_mask(ref_logits), "mask")
    # gradients through the zero-insert / gather pair vs the fp64 graph
    rng = np.random.default_rng(1)
    lab = rng.random((2, 32, 32)) < 0.4
    onehot = np.stack([~lab, lab], -1).astype(np.uint8)
    wmap = (1 + rng.random((2, 32, 32, 1))).astype(np.float32)
    t = UNetTrainer(dict(params, device="cuda:0", dropout=0.0, seed=5), learning_rate=0.01)
    w0 = t.state_dict()
    d = lambda a: torch.from_numpy(a).to("cuda:0")
    loss = t.forward_backward(d(x), d(onehot), d(wmap))
    rloss, rgrads, _ = tr.unet_loss_and_grads(x, onehot, wmap, w0, params)
    assert abs(loss.item() - rloss) <= 1e-5 * abs(rloss)
    g = t.grads()
    for k in rgrads:
        assert np.max(np.abs(g[k] - rgrads[k])) <= 1e-3 * np.max(np.abs(rgrads[k])) + 1e-7, k


@pytest.mark.parametrize("bridge", ["eltwise_mul", "eltwise_add", "eltwise_sub", None])
@pytest.mark.parametrize("shape", [(2, 32, 32), (1, 48, 80), (3, 16, 16), (2, 34, 50)])
def test_convT_bridge_conv_fused_kernel_bit_exact(bridge, shape):
    """sq_convT_conv3x3_fwd_f32 (up0: transpose conv + bridge inside the conv's staging) vs the oracle's
    convT -> bridge -> conv, bit for bit, incl. image borders.  The multiples of 16 run the level-0 kernel's UP form; (2, 34, 50),
    even but ragged against the 16 x 16 tile, runs the generic kernel's."""
    from oracle import c_oracle as co
    from tests.util import rand_weights
    N, H, W = shape
    rng = np.random.default_rng(H + W)
    xl = rng.standard_normal((N, H // 2, W // 2, 32)).astype(np.float32)
    skip = rng.standard_normal((N, H, W, 16)).astype(np.float32)
    wt = rand_weights(1, (2, 2, 16, 32), 0.2)
    bt = rand_weights(2, (16,), 0.1)
    w = rand_weights(3, (3, 3, 16, 16))
    b = rand_weights(4, (16,), 0.1)
    d = lambda a: torch.from_numpy(a).to("cuda:0")
    y = ops.convT_conv3x3(d(xl), d(wt), d(bt), d(skip), bridge, d(w), d(b), act="relu")
    merged = co.convT2x2s2(xl, wt, bt, skip=skip if bridge else None, bridge=bridge)
    assert_bit_exact(y.cpu().numpy(), co.conv2d(merged, w, b, act="relu"), "fused up block (%s)" % bridge)


def test_graphed_predict_equals_eager():
    from sequitr_amd.networks.unet import GraphedPredict
    params = {"shape": (64, 64)}
    net, w = make(params, seed=1)
    g = GraphedPredict(net, (3, 64, 64, 1))
    for seed in (0, 1):
        x = tiles(seed, 3, 64, 64)
        mask, logits = g(x)
        ref_mask = net.predict(x).clone()
        assert_bit_exact(logits.cpu().numpy(), net.logits().cpu().numpy(), "graph logits")
        assert torch.equal(mask, ref_mask)
    with pytest.raises(ValueError):
        g(tiles(0, 2, 64, 64))


def test_batches_over_2gib_fall_back_to_the_hook_path_with_the_same_masks():
    """130 tiles of 512x512: the level-0 activation is 2.03 GiB, past the fused kernels' 32-bit offsets."""
    params = {"shape": (512, 512), "filters": (16, 32)}
    net, _ = make(params, seed=2)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(1)
    x = torch.randn((130, 512, 512, 1), device="cuda:0", generator=g)
    assert not net._fits_fused(x) and net._fits_fused(x[:32])
    big = net.predict(x).clone()
    for lo in (0, 96):
        assert torch.equal(net.predict(x[lo:lo + 32].contiguous()), big[lo:lo + 32])
    del x, big
    torch.cuda.empty_cache()


@pytest.mark.parametrize("shape", [(32, 80), (112, 48)])
def test_rectangular_tiles_fused_and_hook_paths_bit_exact(shape):
    for fuse in (True, False):
        params = {"shape": shape, "fuse": fuse}
        net, w = make(params, seed=7)
        x = tiles(3, 2, shape[0], shape[1])
        mask = net.predict(x)
        ref = unet_oracle.unet_forward(x, w, params)
        assert_bit_exact(net.logits().cpu().numpy(), ref, "logits %s fuse=%s" % (shape, fuse))
        assert_bit_exact(mask.cpu().numpy(), unet_oracle.predict_mask(ref), "mask")


@pytest.mark.parametrize("filters", [(32, 64, 128), (8, 16, 32), (16, 64), (48, 96)])
def test_other_filter_schedules_bit_exact(filters):
    """filter counts other than the default: no FIRST / head / UP fusion at 32+, no fused path at all for 8."""
    params = {"shape": (32, 32), "filters": filters, "num_outputs": 3}
    net, w = make(params, seed=9)
    x = tiles(4, 2, 32, 32)
    mask = net.predict(x)
    ref = unet_oracle.unet_forward(x, w, params)
    assert_bit_exact(net.logits().cpu().numpy(), ref, "logits %s" % (filters,))
    assert_bit_exact(mask.cpu().numpy(), unet_oracle.predict_mask(ref), "mask")


@pytest.mark.parametrize("nout", [1, 3, 5, 7])
def test_class_counts_up_to_seven_bit_exact(nout):
    """the reference's label pipeline carries up to 5 classes (weightmap.py:60-61, unet.py:396-398)"""
    params = {"shape": (32, 48), "filters": (16, 32), "num_outputs": nout}
    net, w = make(params, seed=nout)
    x = tiles(nout, 2, 32, 48)
    mask = net.predict(x)
    ref = unet_oracle.unet_forward(x, w, params)
    assert_bit_exact(net.logits().cpu().numpy(), ref, "logits")
    assert_bit_exact(mask.cpu().numpy(), unet_oracle.predict_mask(ref), "mask")


def test_one_by_one_kernel_configuration_bit_exact():
    """`kernel` = (1,1) (base.py hyper-parameter): every conv runs through the 1x1 kernels, hook path only."""
    params = {"shape": (32, 32), "filters": (16, 32), "kernel": (1, 1)}
    net, w = make(params, seed=21)
    assert w["UNet/down0/conv1/kernel"].shape == (1, 1, 1, 16)
    x = tiles(2, 2, 32, 32)
    mask = net.predict(x)
    ref = unet_oracle.unet_forward(x, w, params)
    assert_bit_exact(net.logits().cpu().numpy(), ref, "logits")
    assert_bit_exact(mask.cpu().numpy(), unet_oracle.predict_mask(ref), "mask")


@pytest.mark.parametrize("cin,filters", [(2, (16, 32)), (3, (16, 32)), (4, (32, 64)), (7, (16, 32))])
def test_multi_channel_input_bit_exact(cin, filters):
    """`num_inputs` > 1 (multi-channel microscopy tiles): conv1 of level 0 runs the small-Cin kernels."""
    params = {"shape": (32, 32), "filters": filters, "num_inputs": cin}
    net, w = make(params, seed=cin)
    x = tiles(cin, 3, 32, 32, c=cin)
    mask = net.predict(x)
    ref = unet_oracle.unet_forward(x, w, params)
    assert_bit_exact(net.logits().cpu().numpy(), ref, "logits")
    assert_bit_exact(mask.cpu().numpy(), unet_oracle.predict_mask(ref), "mask")


def test_legacy_wiring_same_bits_flat_variable_names():
    """UNet_LEGACY (unet.py:445-729): identical arithmetic, tf.layers' automatic variable names, max_pool_layer hook."""
    from sequitr_amd.networks.unet import UNet_LEGACY, legacy_state_dict
    params = {"shape": (32, 32), "filters": (16, 32, 64)}
    w = init_unet_weights(params, 4)
    flat, back = legacy_state_dict(w, params)
    assert "conv2d/kernel" in flat and "conv2d_10/kernel" in flat and "conv2d_transpose_1/bias" in flat
    assert back["conv2d_10"] == "UNet/to_image" and back["conv2d_transpose"] == "UNet/up1/upscale"
    calls = []

    class Net(UNet_LEGACY):
        def max_pool_layer(self, x):
            calls.append(tuple(x.shape))
            return UNet_LEGACY.max_pool_layer(self, x)

    net = Net(dict(params, device="cuda:0"), "infer")
    net.load_state_dict(flat)
    x = tiles(5, 2, 32, 32)
    mask = net.predict(x)
    ref = unet_oracle.unet_forward(x, w, params)
    assert_bit_exact(net.logits().cpu().numpy(), ref, "legacy logits")
    assert_bit_exact(mask.cpu().numpy(), unet_oracle.predict_mask(ref), "legacy mask")
    assert sorted(net.state_dict()) == sorted(flat) and len(calls) == 2
    # a fresh legacy net creates the same names on its own
    fresh = UNet_LEGACY(dict(params, device="cuda:0"), "infer")
    fresh.predict(x)
    assert sorted(fresh.state_dict()) == sorted(flat)


def test_o1_logit_fixture_512_tile_bit_exact_and_near_ties_counted():
    """with seeded variance-scaling weights and eltwise_mul bridges the benchmark net's logits are
    ~1e-5, so every tolerance statement was made on near-ties.  bench.o1_weights (3x3 kernels x 1.35, N(0, 0.05)
    biases) gives logits of order one.  On it: a full 512x512 tile is BIT-EXACT against the C oracle (logits, mask),
    the fused and the hook-by-hook graphs agree bit for bit on a 32-tile batch, tile k of the batch equals tile k run
    alone, and the near-tie pixels (|z1 - z0| < 1e-6, where another summation order could flip the argmax) are counted:
    bounded here at 1e-5 of the pixels (SURVEY 7 "Bit-exact argmax")."""
    import bench
    params = {"shape": (512, 512), "filters": (16, 32, 64, 128, 256), "bridge": "eltwise_mul"}
    w = bench.o1_weights(params)
    net = UNet2D(dict(params, device="cuda:0"), "infer")
    net.load_state_dict(w)
    x = tiles(11, 32, 512, 512)
    mask = net.predict(x).cpu().numpy()
    logits = net.logits().cpu().numpy()
    assert 0.3 < logits.std() < 5.0 and np.abs(logits).max() > 3.0, (logits.std(), np.abs(logits).max())   # order one
    ref = unet_oracle.unet_forward(x[:1], w, params)
    assert_bit_exact(logits[:1], ref, "O(1) fixture, 512x512 tile, logits")
    assert_bit_exact(mask[:1], unet_oracle.predict_mask(ref), "O(1) fixture, 512x512 tile, mask")
    gap = np.abs(logits[..., 1] - logits[..., 0])
    assert (gap < 1e-6).mean() <= 1e-5 and 0.05 < mask.mean() < 0.6, ((gap < 1e-6).sum(), mask.mean())
    unfused = UNet2D(dict(params, device="cuda:0", fuse=False), "infer")
    unfused.load_state_dict(w)
    assert np.array_equal(unfused.predict(x).cpu().numpy(), mask) and np.array_equal(unfused.logits().cpu().numpy(), logits)
    for k in (5, 31):
        assert np.array_equal(net.predict(x[k:k + 1]).cpu().numpy()[0], mask[k])
        assert np.array_equal(net.logits().cpu().numpy()[0], logits[k])
    # the torch-oneDNN restatement (bench.py's cpu_baseline leg) on two tiles: logits within north_star's 1e-3 of O(1)
    # logits; masks differ only where the gap is below the logits' disagreement
    from oracle.torch_ref import TorchCpuUNet
    cl = TorchCpuUNet(w, params, threads=8)(x[:2])
    err = float(np.abs(cl - logits[:2]).max())
    assert err <= 1e-3, err
    diff = np.argmax(cl, -1).astype(np.uint8) != mask[:2]
    assert (gap[:2][diff] <= 2 * err).all() and diff.mean() < 1e-4
