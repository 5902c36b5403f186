"""GPU: sq_bricks_view_f32 and sq_bricks_scatter_probs against the numpy restatement of the header
(tests/volume_tta_cases.py), the views against the volume sampler's own kernels, and segment_volumes(tta=, probabilities=)
against that restatement around the network's own net.build.  Views are bit-exact (copies by bit pattern, accumulations
against numpy float32 adds), masks byte-equal, probabilities within (K + 4) * 2^-23 of the float64 softmax."""
import numpy as np
import pytest
import torch

from sequitr_amd import _lib
from sequitr_amd.frontend import PIX, VolumeSampler, VolumeTiler, segment_volumes
from sequitr_amd.networks.unet import UNet3D, init_unet3d_weights
from tests import volume_tta_cases as vc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
E_SIZES = (1, 2, 3, 4, 5, 8, 16)
SQUARES = (1, 5, 31, 32, 33, 40)                                # the 32-pixel LDS block (E <= 4): - 1 / exact / + 1
SQUARES_16 = (15, 16, 17)                                       # the 16-pixel block of E > 4
RECTANGLES = ((6, 10), (7, 9))                                  # BY * E % 4 is 0 for some E and not for others


def any_tiler():
    return VolumeTiler((4, 8, 8), (4, 8, 8), 0, device=DEV)     # view() takes any brick shape


def stream():
    return torch.cuda.current_stream().cuda_stream


def run_all_views(x, pre, monkeypatch):
    """every (lds form, op, direction, plain / accumulating) into its own guarded slot of one buffer: (slots, keys, n)"""
    tl, n = any_tiler(), x.numel()
    ops = vc.OPS if x.shape[2] == x.shape[3] else range(8)
    pitch = n + GUARD + (-n) % 4                                # every slot starts 16-byte aligned
    keys = [(lds, op, inv, acc) for op in ops for lds in (("1", "0") if op & 8 else ("1",)) for inv in (False, True)
            for acc in (False, True)]
    slots = torch.empty((len(keys), pitch), dtype=torch.float32, device=DEV)
    slots[:, :n] = pre.reshape(-1)
    slots[:, n:] = -77.0
    for s, (lds, op, inv, acc) in enumerate(keys):
        monkeypatch.setenv("SQ_TTA_LDS", lds)
        tl.view(x, op, inverse=inv, out=slots[s, :n].view(x.shape), accumulate=acc)
    torch.cuda.synchronize()
    return slots.cpu().numpy(), keys, n


@pytest.mark.parametrize("BZ", [1, 2, 3])
@pytest.mark.parametrize("E", E_SIZES)
def test_views_are_bit_exact(monkeypatch, E, BZ):
    N = 3
    shapes = [(s, s) for s in SQUARES + (SQUARES_16 if E > 4 else ())] + list(RECTANGLES)
    for BX, BY in shapes:
        shape = (N, BZ, BX, BY, E)
        rng = np.random.default_rng(1000 * BX + 100 * BY + 10 * E + BZ)
        x_h, pre_h = vc.special_values(shape, rng), vc.special_values(shape, rng)
        got, keys, n = run_all_views(torch.from_numpy(x_h).to(DEV), torch.from_numpy(pre_h).to(DEV), monkeypatch)
        want, by_key = {}, {}
        for s, (lds, op, inv, acc) in enumerate(keys):
            out = got[s, :n].reshape(shape)
            assert (got[s, n:] == -77.0).all(), ("guard", shape, lds, op, inv, acc)
            if (op, inv) not in want:
                want[(op, inv)] = (vc.unview if inv else vc.view)(x_h, op)
            ref = want[(op, inv)]
            if acc:
                with np.errstate(invalid="ignore"):
                    assert vc.same_bits_nan_aware(out, pre_h + ref), ("accumulate", shape, lds, op, inv)
            else:
                assert np.array_equal(vc.bits(out), vc.bits(ref)), ("copy", shape, lds, op, inv)    # NaN payloads included
            by_key[(lds, op, inv, acc)] = out
        for (lds, op, inv, acc), out in by_key.items():         # the two forms give the same bits
            if lds == "0":
                assert np.array_equal(vc.bits(out), vc.bits(by_key[("1", op, inv, acc)])), (shape, op, inv, acc)


def test_views_equal_the_volume_sampler():
    """two independent kernels: view_op of the tiler's bricks is the sampler's brick at the same origin under op"""
    shape, brick, margin = (3, 21, 37), (4, 8, 8), (1, 2, 2)    # shorter than the brick along z: both kernels fill
    vols = torch.from_numpy(np.random.default_rng(7).integers(100, 4000, (2,) + shape).astype(np.uint16)).to(DEV)
    tl, sm = VolumeTiler(shape, brick, margin, device=DEV), VolumeSampler(shape, brick, device=DEV)
    stats = tl.stats(vols)
    bricks = tl.bricks(vols, stats=stats)
    g = tl.geometry
    KZ, KX, KY = g.counts
    org = g.table()
    rows = [[v, org[kz], org[KZ + kx], org[KZ + KX + ky]] for v in range(2) for kz in range(KZ) for kx in range(KX)
            for ky in range(KY)]
    assert len(rows) == bricks.shape[0] > 2 and shape[0] < brick[0]
    for op in vc.OPS:
        plan = torch.tensor([r + [op] for r in rows], dtype=torch.int32, device=DEV)
        want = sm.images(vols, plan, stats=stats)
        got = tl.view(bricks, op)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), op
    assert torch.equal(tl.view(bricks, 0), bricks)


def test_views_past_the_grid_caps(monkeypatch):
    """more than 16384 * 256 units of the row form (one float a unit: BY * E % 4 != 0, and the direct gather of a transposed
    op) and more than 16384 items of the LDS form: the block-stride loops"""
    tl = any_tiler()
    rng = np.random.default_rng(5)
    cases = [((2, 33, 256, 255, 1), "1", 5, False), ((2, 33, 256, 255, 1), "1", 6, True),
             ((2, 33, 256, 256, 1), "0", 11, True),
             ((1400, 3, 33, 33, 1), "1", 9, False), ((1400, 3, 33, 33, 1), "1", 13, True)]
    assert 2 * 33 * 256 * 255 > 16384 * 256 and 1400 * 3 * 4 > 16384
    made = {}
    for shape, lds, op, acc in cases:
        if shape not in made:
            made.clear()
            made[shape] = (rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32))
        x_h, pre_h = made[shape]
        monkeypatch.setenv("SQ_TTA_LDS", lds)
        out = torch.from_numpy(pre_h).to(DEV)
        tl.view(torch.from_numpy(x_h).to(DEV), op, out=out, accumulate=acc)
        ref = vc.view(x_h, op)
        assert np.array_equal(vc.bits(out.cpu().numpy()), vc.bits(pre_h + ref if acc else ref)), (shape, lds, op, acc)


@pytest.mark.parametrize("E", [3, 8])
def test_views_twice_and_graph_replay(monkeypatch, E):
    shape = (3, 3, 33, 33, E)
    rng = np.random.default_rng(E)
    x = torch.from_numpy(vc.special_values(shape, rng)).to(DEV)
    pre = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(DEV)
    tl = any_tiler()
    for lds in ("1", "0"):
        monkeypatch.setenv("SQ_TTA_LDS", lds)

        def chain(buf):                                         # the merge of the dihedral set, as segment_volumes runs it
            for op in vc.OPS:
                tl.view(x, op, inverse=True, out=buf, accumulate=op != 0)

        a, b, c = pre.clone(), pre.clone(), pre.clone()
        chain(a)
        chain(b)
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            chain(c)
        for _ in range(2):
            c.copy_(pre)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(a.view(torch.int32), c.view(torch.int32)), lds


def test_view_refusals_leave_dst_untouched():
    lib = _lib.load()
    N, BZ, BX, BY, E = 2, 2, 8, 8, 4
    n = N * BZ * BX * BY * E
    buf = torch.arange(3 * n + 8, dtype=torch.float32, device=DEV)
    before = buf.clone()
    src, dst = buf[:n], buf[2 * n:3 * n]

    def call(s, d, N=N, BZ=BZ, BX=BX, BY=BY, E=E, op=3):
        return lib.sq_bricks_view_f32(s, d, N, BZ, BX, BY, E, op, 0, 0, stream())

    cases = {
        "same": call(src.data_ptr(), src.data_ptr()),
        "overlap ahead": call(src.data_ptr(), buf[n // 2:].data_ptr()),
        "overlap behind": call(buf[n // 2:].data_ptr(), src.data_ptr()),
        "op 16": call(src.data_ptr(), dst.data_ptr(), op=16),
        "op -1": call(src.data_ptr(), dst.data_ptr(), op=-1),
        "transpose of a rectangle": call(src.data_ptr(), dst.data_ptr(), BX=4, BY=16, op=8),
        "E 0": call(src.data_ptr(), dst.data_ptr(), E=0),
        "E 17": call(src.data_ptr(), dst.data_ptr(), E=17),
        "BZ 0": call(src.data_ptr(), dst.data_ptr(), BZ=0),
        "BX 0": call(src.data_ptr(), dst.data_ptr(), BX=0),
        "BY 0": call(src.data_ptr(), dst.data_ptr(), BY=0),
        "BX 65536": call(src.data_ptr(), dst.data_ptr(), BX=65536),
        "BY 65536": call(src.data_ptr(), dst.data_ptr(), BY=65536),
        "N 0": call(src.data_ptr(), dst.data_ptr(), N=0),
        "rows past 2^31": call(src.data_ptr(), dst.data_ptr(), N=32768, BZ=65536, BX=1),
        "null": call(None, dst.data_ptr()),
        "src misaligned": call(buf[1:].data_ptr(), dst.data_ptr()),
        "dst misaligned": call(src.data_ptr(), buf[2 * n + 1:].data_ptr()),
    }
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in cases.values()), cases
    assert cases["src misaligned"] == cases["dst misaligned"] == -3          # SQ_EALIGN
    assert torch.equal(buf, before)
    assert call(src.data_ptr(), buf[n:2 * n].data_ptr()) == 0                # adjacent ranges do not overlap
    assert call(src.data_ptr(), dst.data_ptr(), BX=4, BY=16, op=7) == 0      # the mirrors take a rectangle
    tl = any_tiler()
    x = src.view(N, BZ, BX, BY, E)
    for bad in (lambda: tl.view(x, 16), lambda: tl.view(x, True), lambda: tl.view(x, 1, accumulate=True),
                lambda: tl.view(x, 1, out=torch.empty(n, device=DEV)), lambda: tl.view(x[:, :, :, :4], 1),
                lambda: tl.view(x.double(), 1), lambda: tl.view(x.view(N, BZ, 4, 16, E), 8), lambda: tl.view(x[0], 1)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(_lib.SequitrHipError):
        tl.view(x, 1, out=x)
    with pytest.raises(_lib.SequitrHipError):
        tl.view(x.cpu(), 1)


# ---- scatter -----------------------------------------------------------------------------------------------------------
def guarded(n, dtype, fill):
    """a flat buffer with GUARD elements before and after its n: (whole, the middle)"""
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return whole, whole[GUARD:GUARD + n]


def guards_hold(whole, n, fill):
    return bool((whole[:GUARD] == fill).all() and (whole[GUARD + n:] == fill).all())


@pytest.mark.parametrize("K", vc.SCATTER_K)
@pytest.mark.parametrize("which", [0, 1])
def test_scatter_probs_matches_the_restatement(which, K):
    shape, brick, margin = vc.SCATTER_VOLUMES[which]
    V = 2
    tl = VolumeTiler(shape, brick, margin, device=DEV)
    nb, nvox = tl.bricks_per_volume, int(np.prod(shape))
    total = V * nb
    rng = np.random.default_rng(K)
    batches = [(f, min(5, total - f)) for f in range(0, total, 5)]
    order = [batches[i] for i in rng.permutation(len(batches))]
    left_out = order.pop() if len(order) > 1 else None          # one batch is never scattered: its voxels keep the fill
    touched = np.zeros((V,) + shape, bool)
    for f, c in order:
        vc.scatter(np.ones((c,) + brick, bool), touched, shape, brick, margin, f)
    assert touched.any() and (left_out is None or not touched.all())
    worst = 0.0
    for n in vc.SCATTER_N:
        acc_h = vc.scatter_case(shape, brick, margin, V, K, 1.0 / n, vc.scatter_seed(K, n, which), specials=which == 0)
        acc = torch.from_numpy(acc_h).to(DEV)
        want_mask, want_p = np.full((V,) + shape, 201, np.uint8), np.full((V, K) + shape, np.nan)
        for f, c in order:
            vc.scatter_probs(acc_h[f:f + c], 1.0 / n, shape, brick, margin, want_mask, want_p, f)
        tk = np.broadcast_to(touched[:, None], want_p.shape)
        what = "%s K=%d n=%d" % (shape, K, n)
        mw, mask = guarded(V * nvox, torch.uint8, 201)
        fw, p32 = guarded(V * K * nvox, torch.float32, -5.0)
        bw, p8 = guarded(V * K * nvox, torch.uint8, 202)
        mw2, mask_only = guarded(V * nvox, torch.uint8, 201)
        mask, mask_only = mask.view((V,) + shape), mask_only.view((V,) + shape)
        p32, p8 = p32.view((V, K) + shape), p8.view((V, K) + shape)
        for f, c in order:
            tl.scatter_probs(acc[f:f + c], mask, p32, first=f, n=n)             # both
            tl.scatter_probs(acc[f:f + c], None, p8, first=f, n=n)              # probabilities only
            tl.scatter_probs(acc[f:f + c], mask_only, None, first=f, n=n)       # the mask only
        torch.cuda.synchronize()
        assert guards_hold(mw, V * nvox, 201) and guards_hold(mw2, V * nvox, 201), what
        assert guards_hold(fw, V * K * nvox, -5.0) and guards_hold(bw, V * K * nvox, 202), what
        got_mask, got32, got8 = mask.cpu().numpy(), p32.cpu().numpy(), p8.cpu().numpy()
        assert np.array_equal(got_mask, want_mask) and torch.equal(mask, mask_only), what      # 201 where nothing was scattered
        assert (got32[~tk] == -5.0).all() and (got8[~tk] == 202).all(), what
        worst = max(worst, vc.check_probs(got32[tk], want_p[tk], K, what))
        vc.check_probs_u8(got8[tk], want_p[tk], K, what)
    print("K=%d %s: worst |p - p64| = %.3g of %.3g allowed" % (K, shape, worst, vc.prob_bound(K)))


def raw_scatter(tl, acc, inv_n, mask, prob, V, K, first=0, count=None):
    dtype = PIX[prob.dtype] if prob is not None else 0
    return _lib.load().sq_bricks_scatter_probs(acc.data_ptr(), tl._geom.data_ptr(), mask.data_ptr() if mask is not None else None,
                                               prob.data_ptr() if prob is not None else None, dtype, inv_n,
                                               *(tl._dims(V) + (K, first, acc.shape[0] if count is None else count, stream())))


def test_scatter_probs_twice_graph_and_refusals():
    shape, brick, margin = vc.SCATTER_VOLUMES[0]
    V, K = 2, 3
    tl = VolumeTiler(shape, brick, margin, device=DEV)
    acc = torch.from_numpy(vc.scatter_case(shape, brick, margin, V, K, 0.125, 1)).to(DEV)
    mask = torch.full((V,) + shape, 201, dtype=torch.uint8, device=DEV)
    p32 = torch.full((V, K) + shape, -5.0, dtype=torch.float32, device=DEV)
    want_mask, want_p = tl.scatter_probs(acc, mask.clone(), p32.clone(), n=8)
    assert raw_scatter(tl, acc, 0.125, mask, p32, V, K) == 0
    torch.cuda.synchronize()
    assert torch.equal(mask, want_mask) and torch.equal(p32.view(torch.int32), want_p.view(torch.int32))   # run to run
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        raw_scatter(tl, acc, 0.125, mask, p32, V, K)
    for _ in range(2):
        mask.fill_(0), p32.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(mask, want_mask) and torch.equal(p32.view(torch.int32), want_p.view(torch.int32))
    # refusals: nothing is written
    mask.fill_(201), p32.fill_(-5.0)
    lib = _lib.load()
    assert raw_scatter(tl, acc, 0.125, None, None, V, K) != 0 and b"mask_out, prob_out" in lib.sq_last_error()
    total = acc.shape[0]
    rcs = {"inv_n 0": raw_scatter(tl, acc, 0.0, mask, p32, V, K), "inv_n 2": raw_scatter(tl, acc, 2.0, mask, p32, V, K),
           "K 17": raw_scatter(tl, acc, 0.125, mask, p32, V, 17), "K 0": raw_scatter(tl, acc, 0.125, mask, p32, V, 0),
           "count 0": raw_scatter(tl, acc, 0.125, mask, p32, V, K, count=0),
           "past the end": raw_scatter(tl, acc, 0.125, mask, p32, V, K, first=1),
           "first -1": raw_scatter(tl, acc, 0.125, mask, p32, V, K, first=-1, count=1),
           "V 0": raw_scatter(tl, acc, 0.125, mask, p32, 0, K),
           "null logits": lib.sq_bricks_scatter_probs(None, tl._geom.data_ptr(), mask.data_ptr(), p32.data_ptr(), 2, 0.125,
                                                      *(tl._dims(V) + (K, 0, total, stream()))),
           "null geom": lib.sq_bricks_scatter_probs(acc.data_ptr(), None, mask.data_ptr(), p32.data_ptr(), 2, 0.125,
                                                    *(tl._dims(V) + (K, 0, total, stream()))),
           "u16 probabilities": lib.sq_bricks_scatter_probs(acc.data_ptr(), tl._geom.data_ptr(), mask.data_ptr(), p32.data_ptr(),
                                                            1, 0.125, *(tl._dims(V) + (K, 0, total, stream()))),
           "logits misaligned": raw_scatter(tl, acc.view(-1)[1:], 0.125, mask, p32, V, K, count=1)}
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in rcs.values()), rcs
    assert rcs["logits misaligned"] == -3                       # SQ_EALIGN
    assert (mask == 201).all() and (p32 == -5.0).all()
    for bad in (lambda: tl.scatter_probs(acc, mask, p32, n=4), lambda: tl.scatter_probs(acc, None, None),
                lambda: tl.scatter_probs(acc, mask, p32.half()), lambda: tl.scatter_probs(acc, mask, p32, first=1),
                lambda: tl.scatter_probs(acc[:, :2], mask, p32), lambda: tl.scatter_probs(acc, mask[:, :4], p32),
                lambda: tl.scatter_probs(acc, mask, p32[:, :2].contiguous()), lambda: tl.scatter_probs(acc, mask.int(), None)):
        with pytest.raises(ValueError):
            bad()
    assert (mask == 201).all() and (p32 == -5.0).all()


# ---- the network -------------------------------------------------------------------------------------------------------
NET = {"shape": (16, 16, 8), "filters": (16, 32), "num_outputs": 2}     # the job's order: (X, Y, Z)
BRICK, MARGIN, STACK = (8, 16, 16), (2, 4, 4), (2, 11, 40, 24)
BATCH = 5


@pytest.fixture(scope="module")
def net3():
    params = dict(NET, device=DEV)
    net = UNet3D(params, "infer")
    net.load_state_dict(init_unet3d_weights(params, 4))
    return net


def make_stack(seed=3):
    rng = np.random.default_rng(seed)
    zz, xx, yy = np.mgrid[:STACK[1], :STACK[2], :STACK[3]]
    v = 400 + 40 * zz[None] + 3 * xx[None] + 2 * yy[None] + rng.integers(0, 300, STACK)
    for k in range(8):                                          # blobs on a ramp: nothing a symmetry maps onto itself
        cz, cx, cy, r = rng.integers(1, 10), rng.integers(4, 36), rng.integers(4, 20), rng.integers(3, 6)
        v = v + 1500 * ((2 * (zz - cz)) ** 2 + (xx - cx) ** 2 + (yy - cy) ** 2 < r * r)[None] * (np.arange(2)[:, None, None, None] + 1)
    return v.astype(np.uint16)


_restated = {}


def restate(net, vols, tta):
    """(masks, float64 probabilities, mean logits) of the header's text around net.build, batched as segment_volumes
    batches; computed once per view set and shared"""
    if tta not in _restated:
        N, shape = vols.shape[0], vols.shape[1:]
        tl = VolumeTiler(shape, BRICK, MARGIN, device=DEV)
        ops_, nb = vc.SETS[tta], tl.bricks_per_volume
        assert nb % BATCH != 0, "the last batch of a volume must be a partial one"
        masks, probs = np.full((N,) + shape, 255, np.uint8), np.full((N, 2) + shape, np.nan)
        means = np.full((N,) + shape + (2,), np.nan, np.float32)
        for i in range(N):
            raw = torch.from_numpy(vols[i:i + 1]).to(DEV)
            stats = tl.stats(raw)
            for first in range(0, nb, BATCH):
                bricks = tl.bricks(raw, first, min(BATCH, nb - first), stats=stats)
                by_op = {op: net.build(tl.view(bricks, op)).cpu().numpy().copy() for op in ops_}
                acc = vc.merge(by_op, ops_)
                inv_n = 1.0 / len(ops_)
                vc.scatter_probs(acc, inv_n, shape, BRICK, MARGIN, masks[i:i + 1], probs[i:i + 1], first)
                vc.scatter(acc * np.float32(inv_n), means[i:i + 1], shape, BRICK, MARGIN, first)
        _restated[tta] = (masks, probs, means)
    return _restated[tta]


def test_scatter_probs_of_one_pass_is_todays_mask(net3):
    vols = torch.from_numpy(make_stack()).to(DEV)
    tl = VolumeTiler(STACK[1:], BRICK, MARGIN, device=DEV)
    bricks = tl.bricks(vols)
    today = tl.scatter(net3.predict(bricks), torch.full(STACK, 255, dtype=torch.uint8, device=DEV)).clone()
    mask = torch.full(STACK, 254, dtype=torch.uint8, device=DEV)
    tl.scatter_probs(net3.build(bricks), mask, None)
    assert torch.equal(mask, today) and 0 < float(mask.float().mean()) < 1


@pytest.mark.parametrize("tta", ["flips", "dihedral"])
def test_segment_volumes_tta_matches_the_restatement(net3, tta):
    vols = make_stack()
    want_mask, want_p, want_mean = restate(net3, vols, tta)
    kw = dict(brick=BRICK, margin=MARGIN, bricks_per_batch=BATCH)
    masks, logits = segment_volumes(net3, vols, tta=tta, want_logits=True, **kw)
    assert masks.dtype == np.uint8 and np.array_equal(masks, want_mask)
    assert np.array_equal(vc.bits(logits), vc.bits(want_mean))                  # the mean logits, bit for bit
    plain, plain_logits = segment_volumes(net3, vols, want_logits=True, **kw)
    print("tta=%s changes %d of %d voxels; foreground %.3f" % (tta, int((masks != plain).sum()), masks.size, masks.mean()))
    assert 0 < masks.mean() < 1 and not np.array_equal(masks, plain)
    for kind, check in (("float32", vc.check_probs), ("uint8", vc.check_probs_u8)):
        m, none, p = segment_volumes(net3, vols, tta=tta, probabilities=kind, **kw)
        assert none is None and np.array_equal(m, want_mask) and p.shape == (2, 2) + STACK[1:] and p.dtype == np.dtype(kind)
        check(p, want_p, 2, "%s %s" % (tta, kind))


def test_probabilities_alone_keep_the_plain_masks_and_logits(net3):
    vols = make_stack()
    kw = dict(brick=BRICK, margin=MARGIN, bricks_per_batch=BATCH)
    plain, plain_logits = segment_volumes(net3, vols, want_logits=True, **kw)
    m, logits, p = segment_volumes(net3, vols, want_logits=True, probabilities="float32", **kw)
    assert np.array_equal(m, plain) and np.array_equal(vc.bits(logits), vc.bits(plain_logits))
    want_mask, want_p, want_mean = restate(net3, vols, None)
    assert np.array_equal(plain, want_mask) and np.array_equal(vc.bits(plain_logits), vc.bits(want_mean))
    vc.check_probs(p, want_p, 2, "tta=None")
    again = segment_volumes(net3, vols, want_logits=True, tta=None, probabilities=None, on_probs=None, **kw)
    assert len(again) == 2 and np.array_equal(again[0], plain) and np.array_equal(vc.bits(again[1]), vc.bits(plain_logits))


def test_sinks_see_probabilities_first_and_postprocess_only_the_masks(net3):
    vols = make_stack()
    want_mask, want_p, _ = restate(net3, vols, "flips")
    kw = dict(brick=BRICK, margin=MARGIN, bricks_per_batch=BATCH, tta="flips", probabilities="float32")
    for sink in ("on_masks", "on_volume"):
        seen = []
        on_probs = lambda i, p: seen.append(("probs", i, p.cpu().numpy(), tuple(p.shape)))
        on_masks = lambda i, m: seen.append(("masks", i, m.cpu().numpy()))
        on_volume = lambda i, raw, m: seen.append(("masks", i, m.cpu().numpy(), tuple(raw.shape)))
        res = segment_volumes(net3, vols, on_probs=on_probs, **dict(kw, **({"on_masks": on_masks} if sink == "on_masks"
                                                                           else {"on_volume": on_volume})))
        assert res == (None, None, None)
        assert [(s[0], s[1]) for s in seen] == [("probs", 0), ("masks", 0), ("probs", 1), ("masks", 1)]
        assert all(s[3] == (1, 2) + STACK[1:] for s in seen if s[0] == "probs")
        assert np.array_equal(np.concatenate([s[2] for s in seen if s[0] == "masks"]), want_mask)
        vc.check_probs(np.concatenate([s[2] for s in seen if s[0] == "probs"]), want_p, 2, sink)
    steps = [{"op": "open", "structure": "cross"}, {"op": "clear_border", "faces": "lateral"}]
    m, _, p = segment_volumes(net3, vols, postprocess=steps, **kw)
    m0, _, p0 = segment_volumes(net3, vols, **kw)
    assert np.array_equal(m0, want_mask) and not np.array_equal(m, m0) and (m <= m0).all()
    assert np.array_equal(p.view(np.uint32), p0.view(np.uint32))        # the probabilities are the network's own


def test_bad_values_raise_before_a_voxel_is_read(net3):
    class Untouchable(object):
        shape, dtype, ndim = STACK, np.dtype("uint16"), 4

        def __getitem__(self, key):
            raise AssertionError("a voxel was read")

    v = Untouchable()
    kw = dict(brick=BRICK, margin=MARGIN)
    for bad in ({"tta": "rot90"}, {"tta": 8}, {"tta": True}, {"tta": ("flips",)}, {"probabilities": "float16"},
                {"probabilities": True}, {"probabilities": np.float32}, {"on_probs": print},
                {"probabilities": "uint8", "on_probs": print}, {"probabilities": "uint8", "on_masks": print},
                {"probabilities": "uint8", "on_volume": print}, {"tta": "flips", "on_probs": print, "on_masks": print},
                {"tta": "dihedral", "brick": (8, 16, 32)}):
        with pytest.raises(ValueError):
            segment_volumes(net3, v, **dict(kw, **bad))

    class Wide(object):
        n_outputs, device = 17, torch.device(DEV)

    with pytest.raises(ValueError, match="classes"):
        segment_volumes(Wide(), v, tta="flips", **kw)
    with pytest.raises(AssertionError, match="a voxel was read"):      # good values do get as far as the voxels
        segment_volumes(net3, v, tta="flips", **kw)
