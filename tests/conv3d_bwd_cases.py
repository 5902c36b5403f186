"""Shared by the conv3d backward tests: fp64 DEFINITIONS of the volumetric gradients, written out in numpy as sums over
shifted views (never another kernel of this project), and the case table of the GPU sweep
(tests/test_gpu_conv3d_bwd_sweep.py), whose plan coverage tests/test_conv3d_bwd_plan.py checks without a GPU.

Layouts: activations NDHWC, conv3d filter (3,3,3,Cin,Cout), transpose-conv filter (2,2,2,Cout,Cin)."""
import numpy as np

# (N, D, H, W, Cin, Cout) of the weight-gradient sweep
WGRAD_SWEEP = [
    (1, 1, 16, 16, 1, 16),            # small Cin, 3 stacked channels, one slice: dw[0], dw[2] are border zeros; one partial
    (2, 3, 20, 24, 2, 8),             # small Cin, 6 stacked channels, partial 16-channel group, two volumes
    (2, 6, 18, 16, 1, 4),             # small Cin, 3 stacked, partial group, two volumes
    (1, 9, 256, 256, 1, 4),           # small Cin: 2304 tiles, every block walks 2 tiles (the register double buffer)
    (2, 1, 20, 18, 16, 8),            # mfma BN 16, partial block (8 of 16), D = 1 with a neighbour volume on either side
    (1, 2, 24, 40, 16, 12),           # mfma BN 16, partial block (12 of 16), D = 2
    (1, 2, 24, 40, 16, 20),           # mfma BN 32, partial block (20 of 32)
    (2, 4, 40, 36, 16, 48),           # mfma BN 32, a full and a partial block, ragged tiles
    (2, 3, 17, 33, 32, 32),           # mfma BN 32, two ci chunks per depth tap, two volumes, odd sides
    (1, 5, 48, 48, 64, 64),           # mfma BN 32, four ci chunks, blocks walk 3 tiles
    (1, 8, 64, 64, 16, 16),           # mfma BN 16 full block, 128 partials per output
]


def _pad_dhw(x):
    N, D, H, W, C = x.shape
    xp = np.zeros((N, D + 2, H + 2, W + 2, C), np.float64)
    xp[:, 1:D + 1, 1:H + 1, 1:W + 1] = x
    return xp


def conv3d64(x, w):
    """y[n,d,h,w,o] = sum_{kd,kh,kw,c} x[n,d+kd-1,h+kh-1,w+kw-1,c] * w[kd,kh,kw,c,o], zeros outside the volume"""
    N, D, H, W, Cin = x.shape
    xp, w = _pad_dhw(x), np.asarray(w, np.float64)
    y = np.zeros((N * D * H * W, w.shape[4]), np.float64)
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                y += xp[:, kd:kd + D, kh:kh + H, kw:kw + W].reshape(-1, Cin) @ w[kd, kh, kw]
    return y.reshape(N, D, H, W, w.shape[4])


def wgrad64(x, dy):
    """dw[kd,kh,kw,c,o] = sum_{n,d,h,w} x[n,d+kd-1,h+kh-1,w+kw-1,c] * dy[n,d,h,w,o] (zeros outside the volume),
    db[o] = sum dy[...,o]"""
    N, D, H, W, Cin = x.shape
    xp = _pad_dhw(x)
    g = np.asarray(dy, np.float64).reshape(-1, dy.shape[4])
    dw = np.empty((3, 3, 3, Cin, dy.shape[4]), np.float64)
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                dw[kd, kh, kw] = xp[:, kd:kd + D, kh:kh + H, kw:kw + W].reshape(-1, Cin).T @ g
    return dw, g.sum(0)


def transform(w):
    """wt[kd][kh][kw][co][ci] = w[2-kd][2-kh][2-kw][ci][co]: the filter whose FORWARD conv3d of dY is the input gradient"""
    return np.ascontiguousarray(np.transpose(np.asarray(w)[::-1, ::-1, ::-1], (0, 1, 2, 4, 3)))


def dgrad64(dy, w):
    return conv3d64(dy, transform(w))


def _windows(x):
    """(N,D,H,W,C) -> (N,D/2,H/2,W/2,C,8), last axis the window in (depth,row,column) raster order"""
    N, D, H, W, C = x.shape
    v = x.reshape(N, D // 2, 2, H // 2, 2, W // 2, 2, C)
    return np.transpose(v, (0, 1, 3, 5, 7, 2, 4, 6)).reshape(N, D // 2, H // 2, W // 2, C, 8)


def maxpool_bwd(x, dy):
    """the gradient goes to the FIRST maximum of each 2x2x2 window in raster order (np.argmax returns the first)"""
    N, D, H, W, C = x.shape
    first = np.argmax(_windows(x), axis=-1)
    dxw = np.zeros((N, D // 2, H // 2, W // 2, C, 8), dy.dtype)
    np.put_along_axis(dxw, first[..., None], np.asarray(dy)[..., None], axis=-1)
    v = dxw.reshape(N, D // 2, H // 2, W // 2, C, 2, 2, 2)
    return np.ascontiguousarray(np.transpose(v, (0, 1, 5, 2, 6, 3, 7, 4)).reshape(N, D, H, W, C))


def space_to_depth(dy):
    """g[n,d,i,j, ((2a+b)*2+e)*C + c] = dy[n, 2d+a, 2i+b, 2j+e, c]"""
    N, D2, H2, W2, C = dy.shape
    v = dy.reshape(N, D2 // 2, 2, H2 // 2, 2, W2 // 2, 2, C)
    return np.ascontiguousarray(np.transpose(v, (0, 1, 3, 5, 2, 4, 6, 7)).reshape(N, D2 // 2, H2 // 2, W2 // 2, 8 * C))


def convT64(x, w, bias=None):
    """y[n,2d+a,2i+b,2j+e,o] = sum_c x[n,d,i,j,c] * w[a,b,e,o,c] + bias[o]"""
    N, D, H, W, Cin = x.shape
    w = np.asarray(w, np.float64)
    Cout = w.shape[3]
    y = np.empty((N, 2 * D, 2 * H, 2 * W, Cout), np.float64)
    xf = np.asarray(x, np.float64).reshape(-1, Cin)
    for a in range(2):
        for b in range(2):
            for e in range(2):
                y[:, a::2, b::2, e::2] = (xf @ w[a, b, e].T).reshape(N, D, H, W, Cout)
    return y if bias is None else y + np.asarray(bias, np.float64)


def convT_bwd64(x, w, G):
    """(dx, dw (2,2,2,Cout,Cin), db) of convT64 from its output gradient G (N,2D,2H,2W,Cout)"""
    N, D, H, W, Cin = x.shape
    w, G = np.asarray(w, np.float64), np.asarray(G, np.float64)
    Cout = w.shape[3]
    xf = np.asarray(x, np.float64).reshape(-1, Cin)
    dx = np.zeros((N * D * H * W, Cin), np.float64)
    dw = np.empty((2, 2, 2, Cout, Cin), np.float64)
    for a in range(2):
        for b in range(2):
            for e in range(2):
                g = G[:, a::2, b::2, e::2].reshape(-1, Cout)
                dx += g @ w[a, b, e]
                dw[a, b, e] = g.T @ xf
    return dx.reshape(N, D, H, W, Cin), dw, G.reshape(-1, Cout).sum(0)


def chain_roundings(plan):
    """Upper count of f32 roundings that can touch one element of dW under `plan` (ops.conv3d_wgrad_plan), each at most
    2^-24 of the absolute sum S = sum |x * dy| of that element: 1 for the products, 4 per MFMA step (four pixels enter
    the accumulator) x 16 steps per wave and tile x tpb tiles, 3 cross-wave adds, ceil(gx / G) serial adds per finish
    lane, log2(G) butterfly adds.
    Four per MFMA step, not one: v_mfma_f32_16x16x4_f32 adds four products to the accumulator and the ISA documents no
    wider intermediate, so the count assumes the worst the instruction may do -- each of the four additions rounded to
    f32 -- where the planar sweep's docstring counted a step as one rounding (an assumption about the hardware, not a
    bound).  A bound has to hold for any conforming evaluation, so the looser count is the one asserted."""
    G = plan['g']
    return 1 + 64 * plan['tpb'] + 3 + -(-plan['gx'] // G) + int(np.log2(G))


def rounding_bound_log2(plan):
    """the power of two p with chain_roundings * 2^-24 <= 2^p"""
    return int(np.ceil(np.log2(chain_roundings(plan)))) - 24
