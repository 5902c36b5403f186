"""GPU confusion counts (sq_confusion) against the numpy restatement of their definition (tests/confusion_cases.py).  Every
quantity is an integer count: every comparison below is exact equality, and no tolerance appears.  The library has one
counting scheme (an LDS histogram per block), so there is no scheme switch to compare."""
import numpy as np
import pytest
import torch

from sequitr_amd import _lib, confusion, ops
from tests import confusion_cases as cc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def big_n(items):
    """an n at which one item spans several blocks, from the kernel's own chunk: two whole chunks and an odd tail"""
    chunk = ops.confusion_chunk(items, 1)
    n = 2 * chunk + 17
    assert ops.confusion_chunk(items, n) == chunk and n > 2 * chunk
    return n


def sizes(items):
    return cc.SIZES + (big_n(items),)


def count(pred, truth, C):
    """fresh buffers, one call through the operator layer; host int64 (counts, ignored)"""
    items = pred.shape[0]
    counts = torch.zeros((items, C, C), dtype=torch.int64, device=DEV)
    ignored = torch.zeros((items,), dtype=torch.int64, device=DEV)
    ops.confusion_(counts, ignored, pred, truth, C)
    return counts.cpu().numpy(), ignored.cpu().numpy()


def check(pred_h, truth_h, C, what, pred_d=None, truth_d=None):
    want_c, want_i = cc.confusion_ref(pred_h, truth_h, C)
    got_c, got_i = count(dev(pred_h) if pred_d is None else pred_d, dev(truth_h) if truth_d is None else truth_d, C)
    assert got_c.dtype == np.int64 and got_i.dtype == np.int64
    assert np.array_equal(got_c, want_c), (what, got_c, want_c)
    assert np.array_equal(got_i, want_i), (what, got_i, want_i)
    n = int(np.prod(pred_h.shape[1:2]))
    assert np.array_equal(got_c.sum((1, 2)) + got_i, np.full(pred_h.shape[0], n)), what
    return want_c, want_i


@pytest.mark.parametrize("C", cc.CLASSES)
def test_masks_against_index_labels(C):
    rng = np.random.default_rng(C)
    seen_ignored = 0
    for items in cc.ITEMS:
        for n in sizes(items):                                  # with odd n, rows 1 and 2 start unaligned
            p, t = cc.class_bytes(rng, (items, n), C), cc.class_bytes(rng, (items, n), C)
            _, ig = check(p, t, C, "mask x index C=%d items=%d n=%d" % (C, items, n))
            seen_ignored += int(ig.sum())
    assert seen_ignored > 0                                     # bytes >= C and 255 were among them
    # both bases at every byte offset of a 4-byte word from an allocation, the same and different for the two
    for n in (17, 4099, big_n(3)):
        p, t = cc.class_bytes(rng, (3, n), C), cc.class_bytes(rng, (3, n), C)
        for op, ot in ((1, 1), (2, 2), (3, 3), (1, 2), (3, 0), (0, 3), (2, 13)):
            pd, td = cc.offset_view(torch, p, op, DEV), cc.offset_view(torch, t, ot, DEV)
            assert pd.data_ptr() % 16 == op % 16 and td.data_ptr() % 16 == ot % 16
            check(p, t, C, "offsets %d / %d, n=%d" % (op, ot, n), pd, td)


@pytest.mark.parametrize("C", cc.CLASSES)
def test_onehot_truth_with_empty_and_double_rows(C):
    rng = np.random.default_rng(100 + C)
    for items in cc.ITEMS:
        for n in sizes(items):
            y = cc.onehot_labels(rng, (items, n), C)
            if n >= 63:
                assert (y.sum(-1) == 0).any() and (C == 1 or ((y != 0).sum(-1) == 2).any())
            check(cc.class_bytes(rng, (items, n), C), y, C, "mask x one-hot C=%d items=%d n=%d" % (C, items, n))
            check(cc.logits_cases(rng, (items, n), C), y, C, "logits x one-hot C=%d items=%d n=%d" % (C, items, n))
    for off in (1, 2, 3):                                       # one-hot rows read as 4-, 2- and 1-byte words
        p, y = cc.class_bytes(rng, (3, 63), C), cc.onehot_labels(rng, (3, 63), C)
        check(p, y, C, "one-hot at byte offset %d" % off, cc.offset_view(torch, p, 3 - off, DEV), cc.offset_view(torch, y, off, DEV))


@pytest.mark.parametrize("C", cc.CLASSES)
def test_logits_give_the_class_argmax_u8_writes(C):
    rng = np.random.default_rng(200 + C)
    for items in cc.ITEMS:
        for n in sizes(items):
            z, t = cc.logits_cases(rng, (items, n), C), cc.class_bytes(rng, (items, n), C)
            if n >= 4099:
                assert np.isnan(z).any() and np.isposinf(z).any() and np.isneginf(z).any() and (z == 0).any()
            zd, td = dev(z), dev(t)
            want_c, want_i = check(z, t, C, "logits x index C=%d items=%d n=%d" % (C, items, n), zd, td)
            mask = ops.argmax_u8(zd)                             # the materialised mask gives the same counts, exactly
            assert np.array_equal(mask.cpu().numpy(), cc.argmax_lowest(z))
            via_c, via_i = confusion.confusion_counts(mask, td, C, per_item=True)
            assert np.array_equal(via_c.cpu().numpy(), want_c) and np.array_equal(via_i.cpu().numpy(), want_i)
    for off in (1, 2, 3):                                       # logits at 4, 8 and 12 bytes: float, float2 and float4 reads
        z, t = cc.logits_cases(rng, (3, 63), C), cc.class_bytes(rng, (3, 63), C)
        check(z, t, C, "logits at float offset %d" % off, cc.offset_view(torch, z, off, DEV), cc.offset_view(torch, t, off, DEV))


def test_calls_accumulate_with_64_bit_adds():
    C, items, n = 3, 3, big_n(3)
    rng = np.random.default_rng(7)
    p1, t1 = cc.class_bytes(rng, (items, n), C), cc.class_bytes(rng, (items, n), C)
    z2, y2 = cc.logits_cases(rng, (items, n), C), cc.onehot_labels(rng, (items, n), C)
    (c1, i1), (c2, i2) = cc.confusion_ref(p1, t1, C), cc.confusion_ref(z2, y2, C)
    counts = torch.zeros((items, C, C), dtype=torch.int64, device=DEV)
    ignored = torch.zeros((items,), dtype=torch.int64, device=DEV)
    ops.confusion_(counts, ignored, dev(p1), dev(t1), C)
    ops.confusion_(counts, ignored, dev(z2), dev(y2), C)       # a second batch of the stream, another pair of kinds
    assert np.array_equal(counts.cpu().numpy(), c1 + c2) and np.array_equal(ignored.cpu().numpy(), i1 + i2)
    # prefilled with 2^32 - 1 in every cell: a 32-bit add would wrap
    full = 2 ** 32 - 1
    counts.fill_(full), ignored.fill_(full)
    ops.confusion_(counts, ignored, dev(p1), dev(t1), C)
    assert (c1 > 0).all() and (i1 > 0).all()
    assert np.array_equal(counts.cpu().numpy(), c1 + full) and np.array_equal(ignored.cpu().numpy(), i1 + full)


def test_confusion_counts_meter_and_confusion_matrix():
    from sklearn.metrics import confusion_matrix as sk
    C = 5
    rng = np.random.default_rng(11)
    p, t = cc.class_bytes(rng, (4, 37, 41), C), cc.class_bytes(rng, (4, 37, 41), C)
    want_c, want_i = cc.confusion_ref(p.reshape(4, -1), t.reshape(4, -1), C)
    pd, td = dev(p), dev(t)
    c, i = confusion.confusion_counts(pd, td, C, per_item=True)
    assert c.is_cuda and c.dtype == torch.int64 and tuple(c.shape) == (4, C, C) and tuple(i.shape) == (4,)
    assert np.array_equal(c.cpu().numpy(), want_c) and np.array_equal(i.cpu().numpy(), want_i)
    c, i = confusion.confusion_counts(pd, td, C)               # everything as one item
    assert tuple(c.shape) == (C, C) and i.dim() == 0
    assert np.array_equal(c.cpu().numpy(), want_c.sum(0)) and int(i) == want_i.sum()
    meter = confusion.ConfusionMeter(C, DEV)
    z, y = cc.logits_cases(rng, (2, 37, 41), C), cc.onehot_labels(rng, (2, 37, 41), C)
    zc, zi = cc.confusion_ref(z.reshape(2, -1, C), y.reshape(2, -1, C), C)
    meter.update(pd[:2], td[:2]).update(pd[2:], td[2:]).update(dev(z), dev(y))
    assert np.array_equal(meter.counts(), want_c.sum(0) + zc.sum(0)) and meter.ignored() == want_i.sum() + zi.sum()
    assert meter.counts().dtype == np.int64
    s = meter.scores()
    assert np.array_equal(s['support'], meter.counts().sum(1)) and 0 < s['mean_iou'] < 1
    assert not meter.reset().counts().any() and meter.ignored() == 0
    # the reference's function: scikit-learn's matrix, compressed to the classes present, from numpy or device inputs
    yt, yp = rng.choice([0, 3, 9, 15], 5000), rng.choice([3, 9], 5000)
    want = sk(yt, yp)
    got = confusion.confusion_matrix(yt, yp)
    assert got.dtype == np.int64 and np.array_equal(got, want) and got.shape == (4, 4)
    assert np.array_equal(confusion.confusion_matrix(dev(yt.astype(np.uint8)), dev(yp.astype(np.int64))), want)
    with pytest.raises(_lib.SequitrHipError):
        confusion.confusion_counts(pd, td, 17)                 # the library's own refusal, with its message
    with pytest.raises(ValueError):
        confusion.confusion_counts(pd, td[:, :, :40], C)


def test_captured_graph_replays_the_call():
    C, items, n = 2, 3, big_n(3)
    rng = np.random.default_rng(13)
    p, t = dev(cc.class_bytes(rng, (items, n), C)), dev(cc.class_bytes(rng, (items, n), C))
    z = dev(cc.logits_cases(rng, (items, n), C))
    eager_c, eager_i = count(p, t, C)
    eager_zc, eager_zi = count(z, t, C)
    counts = torch.zeros((items, C, C), dtype=torch.int64, device=DEV)
    ignored = torch.zeros((items,), dtype=torch.int64, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.confusion_(counts, ignored, p, t, C)               # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.confusion_(counts, ignored, p, t, C)
        ops.confusion_(counts, ignored, z, t, C)
    counts.zero_(), ignored.zero_()
    graph.replay()
    assert np.array_equal(counts.cpu().numpy(), eager_c + eager_zc) and np.array_equal(ignored.cpu().numpy(), eager_i + eager_zi)
    graph.replay()                                              # the call adds: a second replay doubles every cell
    assert np.array_equal(counts.cpu().numpy(), 2 * (eager_c + eager_zc))
    assert np.array_equal(ignored.cpu().numpy(), 2 * (eager_i + eager_zi))
