"""CPU: the launch plan of the 3-D convolution (sq_conv3d_plan, the host function sq_conv3d_ndhwc_fwd_f32 takes its
kernel, block width, chunk, grid and addressing from).  The plans of the default UNet3D on two volumes are pinned, and the
GPU sweep's case table (tests/conv3d_cases.py) must reach every form."""
import pytest

from sequitr_amd import _lib, ops
from tests import conv3d_cases as cc

FILTERS = (16, 32, 64, 128, 256)


def unet3d_layers(N, D, H, W, cin=1):
    """(name, (N, D, H, W, Cin, Cout)) of every 3x3x3 conv of the default UNet3D (eltwise bridge); level i at >> i"""
    out = []
    for i, fo in enumerate(FILTERS):
        s = (N, D >> i, H >> i, W >> i)
        out += [('down%d/conv1' % i, s + (cin, fo)), ('down%d/conv2' % i, s + (fo, fo))]
        cin = fo
    for i in reversed(range(len(FILTERS) - 1)):
        s = (N, D >> i, H >> i, W >> i)
        out += [('up%d/conv1' % i, s + (FILTERS[i], FILTERS[i])), ('up%d/conv2' % i, s + (FILTERS[i], FILTERS[i]))]
    return out


# (kind, BN, KC, gx, gy, addressing)
PLAN_64x256 = {
    'down0/conv1': ('direct', 16, 3, 4096, 1, 'flat'), 'down0/conv2': ('mfma', 16, 16, 1024, 1, 'flat'),
    'down1/conv1': ('mfma', 32, 16, 683, 1, 'flat'), 'down1/conv2': ('mfma', 32, 32, 512, 1, 'flat'),
    'down2/conv1': ('mfma', 32, 32, 256, 2, 'flat'), 'down2/conv2': ('mfma', 32, 32, 256, 2, 'flat'),
    'down3/conv1': ('mfma', 16, 16, 32, 8, 'flat'), 'down3/conv2': ('mfma', 16, 16, 32, 8, 'flat'),
    'down4/conv1': ('mfma', 16, 16, 4, 16, 'flat'), 'down4/conv2': ('mfma', 16, 16, 4, 16, 'flat'),
    'up3/conv1': ('mfma', 16, 16, 32, 8, 'flat'), 'up3/conv2': ('mfma', 16, 16, 32, 8, 'flat'),
    'up2/conv1': ('mfma', 32, 32, 256, 2, 'flat'), 'up2/conv2': ('mfma', 32, 32, 256, 2, 'flat'),
    'up1/conv1': ('mfma', 32, 32, 512, 1, 'flat'), 'up1/conv2': ('mfma', 32, 32, 512, 1, 'flat'),
    'up0/conv1': ('mfma', 16, 16, 1024, 1, 'flat'), 'up0/conv2': ('mfma', 16, 16, 1024, 1, 'flat'),
}
# 1 x 130 x 512 x 512: level-0 tensors are above 2 GiB (16 channels: 2.18e9 bytes) -> per-slice windows
PLAN_130x512 = {
    'down0/conv1': ('direct', 16, 3, 33792, 1, 'window'), 'down0/conv2': ('mfma', 16, 16, 1024, 1, 'window'),
    'down1/conv1': ('mfma', 32, 16, 757, 1, 'flat'), 'down1/conv2': ('mfma', 32, 32, 505, 1, 'flat'),
    'down2/conv1': ('mfma', 64, 16, 512, 1, 'flat'), 'down2/conv2': ('mfma', 64, 16, 512, 1, 'flat'),
    'down3/conv1': ('mfma', 64, 16, 256, 2, 'flat'), 'down3/conv2': ('mfma', 64, 16, 256, 2, 'flat'),
    'down4/conv1': ('mfma', 16, 16, 32, 16, 'flat'), 'down4/conv2': ('mfma', 16, 16, 32, 16, 'flat'),
    'up3/conv1': ('mfma', 64, 16, 256, 2, 'flat'), 'up3/conv2': ('mfma', 64, 16, 256, 2, 'flat'),
    'up2/conv1': ('mfma', 64, 16, 512, 1, 'flat'), 'up2/conv2': ('mfma', 64, 16, 512, 1, 'flat'),
    'up1/conv1': ('mfma', 32, 32, 505, 1, 'flat'), 'up1/conv2': ('mfma', 32, 32, 505, 1, 'flat'),
    'up0/conv1': ('mfma', 16, 16, 1024, 1, 'window'), 'up0/conv2': ('mfma', 16, 16, 1024, 1, 'window'),
}


def _plan(shape):
    p = ops.conv3d_plan(*shape)
    return (p['kind'], p['bn'], p['kc'], p['gx'], p['gy'], p['addressing'])


@pytest.mark.parametrize("vol,pinned", [((1, 64, 256, 256), PLAN_64x256), ((1, 130, 512, 512), PLAN_130x512)])
def test_unet3d_plans_are_pinned(vol, pinned):
    got = {name: _plan(shape) for name, shape in unet3d_layers(*vol)}
    assert got == pinned


def test_mfma_plan_is_the_planar_plan_of_the_stacked_layer():
    """block width and chunk are those sq_conv_plan gives the planar conv on N*D images of 3*Cin channels (the level-0
    kernel never takes a stacked layer: 3*Cin != 16)"""
    import ctypes
    lib = _lib.load()
    for _, (N, D, H, W, Cin, Cout) in unet3d_layers(1, 64, 256, 256)[1:]:
        out = (ctypes.c_int * 5)()
        _lib.check(lib.sq_conv_plan(2, 0, N * D, H, W, 3 * Cin, Cout, 3, 1, 0, None, 0, out), "sq_conv_plan")
        p = ops.conv3d_plan(N, D, H, W, Cin, Cout)
        assert (p['bn'], p['kc'], p['gy']) == (out[0], out[1], out[2]) and out[4] == 0


def test_sweep_reaches_every_form():
    forms = {}
    for (N, D, H, W, Cin, Cout, act) in cc.SWEEP:
        p = ops.conv3d_plan(N, D, H, W, Cin, Cout)
        key = (p['kind'], p['bn'], p['kc'], p['addressing'])
        forms.setdefault(key, []).append(Cout % p['bn'] != 0)
    want = {('direct', 16, 3, 'flat'), ('direct', 16, 6, 'flat'), ('mfma', 16, 16, 'flat'), ('mfma', 32, 16, 'flat'),
            ('mfma', 32, 32, 'flat'), ('mfma', 64, 16, 'flat')}
    assert set(forms) == want, sorted(forms)
    for bn in (16, 32, 64):                                  # a partial channel block at every block width
        assert any(any(v) for k, v in forms.items() if k[1] == bn), bn
    assert {c[1] for c in cc.SWEEP} >= {1, 2, 3, 8} and {c[4] for c in cc.SWEEP} >= {1, 2, 16, 32, 64}
    assert any(c[2] % 16 or c[3] % 16 for c in cc.SWEEP) and any(c[0] > 1 for c in cc.SWEEP)
    # the large-volume case of the sweep takes the window form
    assert ops.conv3d_plan(1, 130, 512, 512, 16, 16)['addressing'] == 'window'


def test_plan_refuses_what_no_kernel_takes():
    for shape, what in [((1, 4, 16, 16, 3, 16), "Cin=3"), ((1, 4, 16, 16, 24, 16), "Cin=24"),
                        ((1, 4, 16, 16, 16, 18), "Cout=18"), ((1, 2, 8192, 8192, 16, 16), "32-bit"),
                        ((1, 0, 16, 16, 16, 16), "bad shape")]:
        with pytest.raises(_lib.SequitrHipError, match=what):
            ops.conv3d_plan(*shape)
