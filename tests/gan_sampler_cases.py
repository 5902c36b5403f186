"""GAN sampler on the CPU -- the numpy restatement of include/sequitr_hip.h "GAN sampler" that the tests of
sequitr_amd.frontend.gan_sample_plan / GanSampler compare against, and their case tables.

Statistics of images (N, H, W, C), uint8 or uint16, per (image, channel) over the n = H*W pixels:

    S1 = sum v,  S2 = sum v^2                                   # exact integers (uint64)
    mean = S1 / n;  var = max(S2 / n - mean * mean, 0);  inv = 1 / sqrt(var + 1e-8)      # float64, no FMA
    stored as float32(mean), float32(inv)

A sample is one row plan[k] = [n, oy, ox, bits].  The definition, word for word; for output pixel (i, j) and channel c of
sample k, crop (CH, CW), output (SH, SW):

    sy = SH > 1 ? float32(CH-1) / float32(SH-1) : 0.0f      (sx likewise from CW, SW)
    py = float32(i) * sy;  y0 = floor(py);  y1 = min(ceil(py), CH-1);  ly = py - y0     (x likewise)
    crop(r, q) = src(oy + (bits&2 ? CH-1-r : r), ox + (bits&1 ? CW-1-q : q))
    src(Y, X)  = (float32(v[n,Y,X,c]) - mean[n,c]) * inv[n,c]   if 0<=n<N, 0<=Y<H, 0<=X<W   else 0.0f
                 (plain cast when mean == inv == NULL)
    top = tl + (tr - tl) * lx;  bot = bl + (br - bl) * lx;  out = top + (bot - top) * ly

np_sample evaluates this in `dtype`: float32 is the definition (numpy rounds every array operation to the arrays' type, so
every *, + and - is rounded on its own and nothing is fused); float64 is the same formulas on the same float32 pixels,
means and inverse deviations, which is what torch's bilinear resize and the error bound are compared with."""
import numpy as np

STACK_SHAPE = (3, 13, 21)                                       # (N, H, W): odd sizes, no multiple of anything
CROP = (12, 20)
SIZES = [(4, 4), (8, 8), (12, 20), (1, 1), (5, 3)]              # (12, 20): the identity; (1, 1): sy = sx = 0
CHANNELS = (1, 2, 3, 4)
LEVEL_SHAPE, LEVEL_CROP, LEVEL_SIZES = (3, 40, 48), (32, 32), [(4, 4), (8, 8), (16, 16), (32, 32)]
NET_STACK = (12, 40, 48, 2)                                     # the network's and the job's uint8 stack
# the smallest image found (a search over sides and grey levels) whose float64 S2 / n - mean * mean comes out NEGATIVE: one
# pixel below an otherwise constant uint16 image of CLAMP_SIDE^2 pixels -- the true variance, about 1 / n = 2.4e-7, is
# under the rounding of the two terms near 2.6e9
CLAMP_SIDE, CLAMP_LEVEL = 2047, 50666


def clamp_image():
    img = np.full((1, CLAMP_SIDE, CLAMP_SIDE, 1), CLAMP_LEVEL, np.uint16)
    img[0, 1000, 3, 0] = CLAMP_LEVEL - 1
    return img


def random_images(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype) == np.float32:
        return (rng.standard_normal(shape) * 30 + 100).astype(np.float32)
    return rng.integers(0, np.iinfo(dtype).max + 1, shape).astype(dtype)


def np_stats(images):
    """(mean, inv) float32 (N, C) of uint8 / uint16 images (N, H, W, C)"""
    images = np.asarray(images)
    assert images.dtype in (np.uint8, np.uint16) and images.ndim == 4
    N, H, W, C = images.shape
    n = np.float64(H * W)
    v = images.reshape(N, H * W, C).astype(np.uint64)
    s1 = v.sum(1, dtype=np.uint64).astype(np.float64)           # uint64 -> float64 rounds to nearest even
    s2 = (v * v).sum(1, dtype=np.uint64).astype(np.float64)
    mean = s1 / n
    var = np.maximum(s2 / n - mean * mean, 0.0)
    inv = 1.0 / np.sqrt(var + 1e-8)
    return mean.astype(np.float32), inv.astype(np.float32)


def np_normalised(images, mean=None, inv=None):
    """src of every pixel, float32 (N, H, W, C): (float32(v) - mean) * inv, the plain cast without statistics"""
    x = np.asarray(images).astype(np.float32)
    if mean is None:
        return x
    return (x - np.asarray(mean, np.float32)[:, None, None, :]) * np.asarray(inv, np.float32)[:, None, None, :]


def np_axis(T, S, dtype):
    """(lower index, upper index, weight) along one axis of crop length T and output length S"""
    scale = dtype(T - 1) / dtype(S - 1) if S > 1 else dtype(0)   # one division in `dtype`
    p = np.arange(S).astype(dtype) * scale
    lo = np.floor(p)
    hi = np.minimum(np.ceil(p), dtype(T - 1))
    return lo.astype(np.int64), hi.astype(np.int64), (p - lo).astype(dtype)


def np_sample(normed, plan, crop, size, dtype=np.float32):
    """(count, SH, SW, C) in `dtype`; `normed` is np_normalised(images, mean, inv), float32 (N, H, W, C)"""
    N, H, W, C = normed.shape
    (CH, CW), (SH, SW) = crop, size
    y0, y1, ly = np_axis(CH, SH, dtype)
    x0, x1, lx = np_axis(CW, SW, dtype)
    ly, lx = ly[:, None, None], lx[None, :, None]
    src = normed.astype(dtype)
    out = []
    for n, oy, ox, bits in np.asarray(plan).astype(np.int64):
        def corner(r, q):
            Y = oy + (CH - 1 - r if bits & 2 else r)
            X = ox + (CW - 1 - q if bits & 1 else q)
            ok = (0 <= n < N) & ((Y >= 0) & (Y < H))[:, None] & ((X >= 0) & (X < W))[None, :]
            v = src[min(max(n, 0), N - 1)][np.clip(Y, 0, H - 1)[:, None], np.clip(X, 0, W - 1)[None, :]]
            return np.where(ok[..., None], v, dtype(0)).astype(dtype)
        tl, tr, bl, br = corner(y0, x0), corner(y0, x1), corner(y1, x0), corner(y1, x1)
        top = tl + (tr - tl) * lx
        bot = bl + (br - bl) * lx
        out.append((top + (bot - top) * ly).astype(dtype))
    return np.stack(out)


def np_flipped_crop(normed, row, crop):
    """the flipped crop of one plan row, fill 0 where it leaves the image: (CH, CW, C), what the resize is applied to"""
    return np_sample(normed, [row], crop, crop)[0]


def f32_bound(ref64, crop):
    """how far the float32 restatement may be from the float64 one.  The float32 coordinate py = float32(i) * sy carries two
    roundings, the division's and the product's, each relative 2^-24 of a value of at most L - 1: |dpy| <= (L-1) * 2^-23.
    The interpolant is continuous and piecewise linear with a slope of at most (max - min) per pixel, also across a cell
    border (where floor jumps the weight jumps with it), so an axis moves the value by at most (L-1) * 2^-23 * (max - min),
    and the two axes by twice that.  The lerps themselves are six roundings of values within the data's range, under 8 ulp
    of the largest magnitude."""
    L = max(crop)
    spread = float(ref64.max() - ref64.min())
    return 2 * (L - 1) * 2.0 ** -23 * spread + 8 * 2.0 ** -23 * float(np.abs(ref64).max())


def all_flip_rows(N, H, W, crop, count, seed):
    """`count` rows inside the stack that go through all four mirror values, the two extreme origins among them"""
    rng = np.random.default_rng(seed)
    plan = np.zeros((count, 4), np.int32)
    plan[:, 0] = rng.integers(0, N, count)
    plan[:, 1] = rng.integers(0, max(H - crop[0], 0) + 1, count)
    plan[:, 2] = rng.integers(0, max(W - crop[1], 0) + 1, count)
    plan[:, 3] = np.arange(count) % 4
    plan[0, 1:3] = 0
    if count > 1:
        plan[1, 1:3] = max(H - crop[0], 0), max(W - crop[1], 0)
    return plan


def outside_rows(N, H, W, crop):
    """rows that leave the stack: n = -1, n = N and a huge n (all fill), origins negative, beyond the image and at the int32
    extremes, under every mirror value, with bits above bit 1 set (ignored)"""
    CH, CW = crop
    big = 2 ** 31 - 1
    rows = [[-1, 0, 0, 0], [N, 0, 0, 1], [big, 1, 1, 2], [-big - 1, 0, 0, 3],
            [0, -3, 2, 0], [1, 2, -5, 1], [2 % N, H - CH + 4, 0, 2], [0, 0, W - CW + 6, 3],
            [1 % N, -CH, 0, 0], [0, H, W, 1], [0, big, 0, 2], [1 % N, 0, big, 3], [0, -big - 1, -big - 1, 3],
            [2 % N, -2, -2, 4 + 3], [0, 1, 1, -1], [1 % N, 0, 0, 8]]
    return np.asarray(rows, np.int32)
