"""CPU: the launch plan of the 3-D weight gradient (sq_conv3d_wgrad_plan, the host function both
sq_conv3d_ndhwc_wgrad_f32 and its workspace query take their choices from).  The plans of the default UNet3D's conv layers
on one 1 x 32 x 128 x 128 volume are pinned, unsupported shapes are refused, and the GPU sweep's case table
(tests/conv3d_bwd_cases.py) must reach every form the plan can return."""
import pytest

from sequitr_amd import _lib, ops
from tests import conv3d_bwd_cases as bc
from tests.test_conv3d_plan import unet3d_layers

# (kind, stacked input channels per chunk, BN, npairs, gx, tpb, G, workspace floats)
PLAN_32x128 = {
    'down0/conv1': ('small', 3, 16, 1, 2048, 1, 64, 917504),
    'down0/conv2': ('mfma', 16, 16, 3, 171, 12, 64, 1190160),
    'down1/conv1': ('mfma', 16, 32, 3, 128, 2, 64, 1781760),
    'down1/conv2': ('mfma', 16, 32, 6, 86, 3, 64, 2394240),
    'down2/conv1': ('mfma', 16, 32, 12, 32, 1, 32, 1781760),
    'down2/conv2': ('mfma', 16, 32, 24, 16, 2, 16, 1781760),
    'down3/conv1': ('mfma', 16, 32, 48, 4, 1, 4, 890880),
    'down3/conv2': ('mfma', 16, 32, 96, 4, 1, 4, 1781760),
    'down4/conv1': ('mfma', 16, 32, 192, 2, 1, 2, 1781760),
    'down4/conv2': ('mfma', 16, 32, 384, 2, 1, 2, 3563520),
    'up3/conv1': ('mfma', 16, 32, 96, 4, 1, 4, 1781760),
    'up3/conv2': ('mfma', 16, 32, 96, 4, 1, 4, 1781760),
    'up2/conv1': ('mfma', 16, 32, 24, 16, 2, 16, 1781760),
    'up2/conv2': ('mfma', 16, 32, 24, 16, 2, 16, 1781760),
    'up1/conv1': ('mfma', 16, 32, 6, 86, 3, 64, 2394240),
    'up1/conv2': ('mfma', 16, 32, 6, 86, 3, 64, 2394240),
    'up0/conv1': ('mfma', 16, 16, 3, 171, 12, 64, 1190160),
    'up0/conv2': ('mfma', 16, 16, 3, 171, 12, 64, 1190160),
}


def _plan(shape):
    p = ops.conv3d_wgrad_plan(*shape)
    return (p['kind'], p['ni'], p['no'], p['npairs'], p['gx'], p['tpb'], p['g'], p['workspace_floats'])


def test_unet3d_wgrad_plans_are_pinned():
    got = {name: _plan(shape) for name, shape in unet3d_layers(1, 32, 128, 128)}
    assert got == PLAN_32x128


def test_workspace_query_equals_the_plan():
    lib = _lib.load()
    shapes = [s for _, s in unet3d_layers(1, 32, 128, 128)] + list(bc.WGRAD_SWEEP)
    for s in shapes:
        p = ops.conv3d_wgrad_plan(*s)
        assert lib.sq_conv3d_ndhwc_wgrad_workspace_f32(*s) == 4 * p['workspace_floats'], s
        # the plan's own arithmetic: partial images of every block
        N, D, H, W, Cin, Cout = s
        ntiles = -(-W // 16) * -(-H // 16) * N * D
        assert p['gx'] == -(-ntiles // p['tpb']) and (p['gx'] - 1) * p['tpb'] < ntiles
        if p['kind'] == 'small':
            assert p['workspace_floats'] == p['gx'] * (27 * Cin + 1) * Cout and p['ni'] == 3 * Cin
        else:
            assert p['npairs'] == 3 * (Cin // 16) * -(-Cout // p['no'])
            assert p['workspace_floats'] == p['gx'] * p['npairs'] * 145 * p['no']


def test_plan_refuses_what_no_kernel_takes():
    lib = _lib.load()
    for shape, what in [((1, 4, 16, 16, 8, 16), "Cin=8"), ((1, 4, 16, 16, 24, 16), "Cin=24"),
                        ((1, 4, 16, 16, 16, 6), "Cout=6"), ((1, 128, 512, 512, 16, 16), "2 GiB"),
                        ((2, 64, 512, 512, 1, 16), "2 GiB"), ((1, 0, 16, 16, 16, 16), "bad shape")]:
        with pytest.raises(_lib.SequitrHipError, match=what):
            ops.conv3d_wgrad_plan(*shape)
        assert lib.sq_conv3d_ndhwc_wgrad_workspace_f32(*shape) == -1
    # just below the limit is taken (the forward op would switch to window addressing only at 2 GiB)
    assert ops.conv3d_wgrad_plan(1, 127, 512, 512, 16, 16)['kind'] == 'mfma'


def test_weight_transform_refuses_what_the_forward_does_not_take():
    """host-side checks only: the pointers are never dereferenced when the shape is refused"""
    lib = _lib.load()
    for Cin, Cout in [(6, 16), (16, 24), (16, 4), (2, 16)]:
        assert lib.sq_conv3d_weight_transform_f32(16, 16, Cin, Cout, None) == -1, (Cin, Cout)
        assert b"Cin=%d Cout=%d" % (Cin, Cout) in lib.sq_last_error()


def test_sweep_reaches_every_form():
    plans = [(c, ops.conv3d_wgrad_plan(*c)) for c in bc.WGRAD_SWEEP]
    forms = {}
    for c, p in plans:
        forms.setdefault((p['kind'], p['ni'], p['no']), []).append(c[5] % p['no'] != 0)
    # every kernel form and block width the plan can return, both small-Cin forms (3 and 6 stacked channels)
    assert set(forms) == {('small', 3, 16), ('small', 6, 16), ('mfma', 16, 16), ('mfma', 16, 32)}, sorted(forms)
    for key, partial in forms.items():                         # a partial output-channel block at every block width
        assert any(partial), key
    assert any(not v for v in forms[('mfma', 16, 16)]) and any(not v for v in forms[('mfma', 16, 32)])   # and a full one
    assert any(p['kind'] == 'mfma' and c[4] // 16 > 1 for c, p in plans)        # more than one ci chunk per depth tap
    for kind in ('small', 'mfma'):
        assert any(p['kind'] == kind and p['tpb'] >= 2 for c, p in plans), kind     # a block that walks >= 2 tiles
        assert any(p['kind'] == kind and p['gx'] > p['g'] for c, p in plans), kind  # a finish lane that sums serially
        assert any(p['kind'] == kind and p['gx'] > 1 for c, p in plans), kind       # more than one partial per output
    assert any(p['gx'] == 1 for c, p in plans)                                  # ... and the single-partial finish
    for kind in ('small', 'mfma'):                             # both depth borders in one slice, and interior slices
        ds = {c[1] for c, p in plans if p['kind'] == kind}
        assert 1 in ds and any(d >= 3 for d in ds), (kind, ds)
    assert {c[1] for c in bc.WGRAD_SWEEP} >= {1, 2, 3}
    assert any(c[0] > 1 and c[1] == 1 for c in bc.WGRAD_SWEEP)      # D = 1 with neighbour volumes: the batch boundary
    assert any(c[0] > 1 for c, p in plans if p['kind'] == 'small') and any(c[0] > 1 for c, p in plans if p['kind'] == 'mfma')
    assert any(c[2] % 16 and c[3] % 16 for c in bc.WGRAD_SWEEP)


def test_integer_operand_cases_stay_exact():
    """operands in -3..3: every product is at most 9 in magnitude, so every partial sum of an element of dW stays below
    9 * N*D*H*W, which must be below 2^24 for f32 sums to be exact in any order"""
    for (N, D, H, W, Cin, Cout) in bc.WGRAD_SWEEP:
        assert 9 * N * D * H * W < 2 ** 24, (N, D, H, W)


def test_rounding_bounds_follow_the_plans():
    """the per-case tolerance of the GPU sweep is derived from the plan's chain (conv3d_bwd_cases.chain_roundings)"""
    logs = {c: bc.rounding_bound_log2(ops.conv3d_wgrad_plan(*c)) for c in bc.WGRAD_SWEEP}
    assert set(logs.values()) <= {-17, -16}, logs
    assert logs[(1, 8, 64, 64, 16, 16)] == -17 and logs[(1, 5, 48, 48, 64, 64)] == -16
