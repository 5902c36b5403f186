"""Shared by the conv3d tests: the stacked-oracle definitions of the 3-D ops (include/sequitr_hip.h, "Volumes") on top of
the planar C oracle, and the case table of the GPU sweep (tests/test_gpu_conv3d_sweep.py), whose plan coverage
tests/test_conv3d_plan.py checks without a GPU."""
import numpy as np

from oracle import c_oracle

# (N, D, H, W, Cin, Cout, act): every plan form of sq_conv3d_plan on flat addressing (the window form is the large-volume
# check of the sweep), Cin 1, 2, 16, 32, 64, a partial channel block at every block width, D 1, 2, 3, 8, H and W that are
# not multiples of 16, N > 1
SWEEP = [
    (1, 1, 16, 16, 1, 16, 'relu'),            # direct, Cin 1, one slice: both depth taps are border zeros
    (2, 3, 20, 24, 2, 8, None),               # direct, Cin 2, partial 16-channel block
    (2, 6, 18, 16, 1, 4, 'relu'),             # direct, Cin 1: two volumes, a full and a partial group of 4 slices
    (1, 2, 24, 40, 16, 20, 'relu'),           # mfma BN 16 KC 16, partial block (4 of 16)
    (2, 8, 64, 64, 16, 80, 'relu'),           # mfma BN 64 KC 16, partial block (16 of 64)
    (2, 8, 64, 64, 16, 48, None),             # mfma BN 32 KC 16, partial block (16 of 32)
    (2, 8, 64, 64, 32, 40, 'relu'),           # mfma BN 32 KC 32, partial block (8 of 32)
    (2, 8, 40, 36, 64, 64, 'relu'),           # mfma BN 32 KC 32 over two chunks per depth tap, ragged tiles
    (1, 3, 17, 33, 64, 64, 'leaky'),          # mfma BN 16 KC 16, four chunks per depth tap, leaky ReLU
]


def stack_input(x):
    """(N,D,H,W,C) -> the depth-stacked planar input (N*D, H, W, 3C): xs[n,d,h,w, kd*C + c] = x[n, d+kd-1, h, w, c]"""
    N, D, H, W, C = x.shape
    pad = np.zeros((N, D + 2, H, W, C), x.dtype)
    pad[:, 1:D + 1] = x
    xs = np.concatenate([pad[:, kd:kd + D] for kd in range(3)], axis=-1)
    return np.ascontiguousarray(xs.reshape(N * D, H, W, 3 * C))


def stack_weights(w):
    """(3,3,3,Cin,Cout) (kd,kh,kw,in,out) -> (3,3,3*Cin,Cout): ws[kh,kw, kd*Cin + c, o] = w[kd,kh,kw,c,o]"""
    Cin, Cout = w.shape[3], w.shape[4]
    return np.ascontiguousarray(np.transpose(w, (1, 2, 0, 3, 4)).reshape(3, 3, 3 * Cin, Cout))


def conv3d_ref(x, w, bias=None, act=None):
    """conv3d by its definition: the planar oracle on the stacked input and filter"""
    N, D, H, W, _ = x.shape
    y = c_oracle.conv2d(stack_input(x), stack_weights(w), bias, act=act)
    return y.reshape(N, D, H, W, w.shape[4])


def convT3d_ref(x, w, bias=None, skip=None, bridge=None):
    """output slice 2d+a = the planar transpose-conv oracle of input slice d with w[a] (bias and bridge included)"""
    N, D, H, W, Cin = x.shape
    Cout = w.shape[3]
    y = np.empty((N, 2 * D, 2 * H, 2 * W, Cout), np.float32)
    flat = np.ascontiguousarray(x.reshape(N * D, H, W, Cin))
    for a in range(2):
        sk = None if skip is None else np.ascontiguousarray(skip[:, a::2].reshape(N * D, 2 * H, 2 * W, Cout))
        ya = c_oracle.convT2x2s2(flat, np.ascontiguousarray(w[a]), bias, skip=sk, bridge=bridge)
        y[:, a::2] = ya.reshape(N, D, 2 * H, 2 * W, Cout)
    return y


def maxpool3d_ref(x):
    N, D, H, W, C = x.shape
    return x.reshape(N, D // 2, 2, H // 2, 2, W // 2, 2, C).max(axis=(2, 4, 6))
