"""Scoring without a GPU: the numpy restatement of sq_confusion (tests/confusion_cases.py) against scikit-learn and against
the C oracle's arg-max, scores() against sklearn.metrics, the 0 / 0 -> NaN -> null rule, the compression rule of
confusion_matrix, the library's host-side refusals, and the jobs' checks that come before any GPU work."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from oracle import c_oracle
from sequitr_amd import _lib, confusion, jobs, ops
from tests import confusion_cases as cc


def test_argmax_rule_is_the_oracles_not_numpys():
    rng = np.random.default_rng(0)
    for C in cc.CLASSES:
        z = cc.logits_cases(rng, (257,), C)
        assert np.array_equal(cc.argmax_lowest(z), c_oracle.argmax_u8(z)), C
    z = np.array([[np.nan, 5.0, 1.0], [1.0, np.nan, 0.5], [0.0, -0.0, -0.0], [-0.0, 0.0, 0.0], [2.0, 2.0, 2.0],
                  [-np.inf, -np.inf, -np.inf], [1.0, np.inf, np.inf]], np.float32)
    assert cc.argmax_lowest(z).tolist() == [0, 0, 0, 0, 0, 0, 1]
    assert np.argmax(z[1]) == 1                                  # numpy would have returned the NaN


def test_restatement_against_sklearn_and_the_ignore_rule():
    from sklearn.metrics import confusion_matrix as sk
    rng = np.random.default_rng(1)
    for C in cc.CLASSES:
        p, t = cc.class_bytes(rng, (3, 4099), C), cc.class_bytes(rng, (3, 4099), C)
        counts, ignored = cc.confusion_ref(p, t, C)
        for i in range(3):
            ok = (p[i] < C) & (t[i] < C)
            assert np.array_equal(counts[i], sk(t[i][ok], p[i][ok], labels=list(range(C)))), (C, i)
            assert ignored[i] == int((~ok).sum()) and ignored[i] > 0
            assert counts[i].sum() + ignored[i] == 4099
    # one-hot truth: the lowest non-zero channel, none for an all-zero row; logits: the arg-max above
    y = np.array([[[0, 0, 0], [0, 9, 1], [1, 1, 1], [0, 0, 2]]], np.uint8)
    assert cc.onehot_class(y).tolist() == [[255, 1, 0, 2]]
    z = np.array([[[0.0, 1.0, 1.0], [3.0, 1.0, 1.0], [np.nan, 1.0, 9.0], [0.0, 0.0, 0.5]]], np.float32)
    counts, ignored = cc.confusion_ref(z, y, 3)
    want = np.zeros((3, 3), np.int64)
    want[1, 0] = want[0, 0] = want[2, 2] = 1
    assert np.array_equal(counts[0], want) and ignored.tolist() == [1]


def test_scores_against_sklearn_metrics():
    from sklearn import metrics
    rng = np.random.default_rng(2)
    for C in (2, 3, 5, 16):
        t = np.concatenate([np.arange(C), rng.integers(0, C, 5000)]).astype(np.uint8)   # every class in both arguments
        p = np.concatenate([np.arange(C), np.where(rng.random(5000) < 0.7, t[C:], rng.integers(0, C, 5000))]).astype(np.uint8)
        labels = list(range(C))
        counts, ignored = cc.confusion_ref(p[None], t[None], C)
        assert ignored[0] == 0 and np.array_equal(counts[0], metrics.confusion_matrix(t, p, labels=labels))
        s = confusion.scores(counts[0])
        np.testing.assert_allclose(s['iou'], metrics.jaccard_score(t, p, labels=labels, average=None), rtol=1e-12)
        np.testing.assert_allclose(s['dice'], metrics.f1_score(t, p, labels=labels, average=None), rtol=1e-12)
        np.testing.assert_allclose(s['precision'], metrics.precision_score(t, p, labels=labels, average=None), rtol=1e-12)
        np.testing.assert_allclose(s['recall'], metrics.recall_score(t, p, labels=labels, average=None), rtol=1e-12)
        np.testing.assert_allclose(s['accuracy'], metrics.accuracy_score(t, p), rtol=1e-12)
        np.testing.assert_allclose(s['mean_iou'], np.mean(s['iou']), rtol=1e-12)
        assert np.array_equal(s['support'], counts[0].sum(1)) and s['iou'].dtype == np.float64


def test_zero_over_zero_is_nan_and_json_null():
    c = np.array([[5, 0, 1], [0, 0, 0], [2, 0, 7]], np.int64)   # class 1 occurs on neither side
    s = confusion.scores(c)
    for k in ('iou', 'dice', 'precision', 'recall'):
        assert np.isnan(s[k][1]) and not np.isnan(s[k][[0, 2]]).any(), k
    assert s['mean_iou'] == pytest.approx((5 / 8 + 7 / 10) / 2, rel=1e-15) and s['accuracy'] == 12 / 15
    text = json.dumps(confusion.json_ready(s))
    assert 'NaN' not in text and json.loads(text)['iou'][1] is None and json.loads(text)['support'] == [6, 0, 9]
    # a class that is predicted but never true: recall 0 / 0, precision 0
    s = confusion.scores(np.array([[3, 2], [0, 0]]))
    assert np.isnan(s['recall'][1]) and s['precision'][1] == 0.0 and s['iou'][1] == 0.0
    empty = confusion.scores(np.zeros((2, 2), np.int64))
    assert np.isnan(empty['accuracy']) and np.isnan(empty['mean_iou'])
    assert confusion.json_ready(empty)['accuracy'] is None
    with pytest.raises(ValueError):
        confusion.scores(np.zeros((2, 3)))


def test_compression_rule_of_confusion_matrix():
    from sklearn.metrics import confusion_matrix as sk
    rng = np.random.default_rng(3)
    for present_t, present_p in (([0, 3, 9], [3, 9]), ([2], [2]), ([1, 15], [0, 7]), (list(range(16)), [4])):
        t = rng.choice(present_t, 300).astype(np.uint8)
        p = rng.choice(present_p, 300).astype(np.uint8)
        t[:len(present_t)], p[:len(present_p)] = present_t, present_p
        full, ignored = cc.confusion_ref(p[None], t[None], 16)
        got = confusion.compress_present(full[0])
        assert ignored[0] == 0 and got.dtype == np.int64 and np.array_equal(got, sk(t, p))


def test_host_side_refusals_need_no_gpu():
    lib = _lib.load()
    buf = (ctypes.c_int64 * 512)()
    a = ctypes.addressof(buf)

    def call(pred=a, pk=0, truth=a, tk=0, counts=a, ignored=a, items=1, n=8, C=2):
        return lib.sq_confusion(pred, pk, truth, tk, counts, ignored, items, n, C, None)

    for C in (0, 17, -1):
        assert call(C=C) == -1 and b"classes" in lib.sq_last_error(), C
    for k in ('pred', 'truth', 'counts', 'ignored'):
        assert call(**{k: None}) == -1 and b"null" in lib.sq_last_error(), k
    assert call(n=-1) == -1 and b"negative" in lib.sq_last_error()
    assert call(items=-1) == -1 and b"negative" in lib.sq_last_error()
    assert call(pk=2) == -1 and b"pred_kind" in lib.sq_last_error()
    assert call(tk=2) == -1 and b"truth_kind" in lib.sq_last_error()
    assert call(counts=a + 4) == -1 and b"aligned" in lib.sq_last_error()
    assert call(pred=a + 2, pk=1) == -1 and b"aligned" in lib.sq_last_error()
    # zero of either is a no-op that returns 0, before any launch
    assert call(items=0) == 0 and call(n=0) == 0 and call(items=0, n=0, pk=1, tk=1, C=16) == 0
    assert not any(buf)
    # the chunk a block counts: 16384 pixels, doubled while a call would have more than 2^22 of them, at most 2^30
    assert lib.sq_confusion_chunk(1, 1) == 16384 and lib.sq_confusion_chunk(0, 5) == 0 and lib.sq_confusion_chunk(3, 0) == 0
    assert lib.sq_confusion_chunk(1, 16384 << 22) == 16384 and lib.sq_confusion_chunk(1, (16384 << 22) + 1) == 32768
    assert lib.sq_confusion_chunk(2, 16384 << 22) == 32768 and lib.sq_confusion_chunk(1, 1 << 44) == 1 << 22
    assert ops.confusion_chunk(3, 4099) == 16384


def test_cpu_tensors_raise():
    p, t = torch.zeros(4, 16, dtype=torch.uint8), torch.zeros(4, 16, dtype=torch.uint8)
    with pytest.raises(_lib.SequitrHipError):
        confusion.confusion_counts(p, t, 2)
    with pytest.raises(_lib.SequitrHipError):
        confusion.confusion_counts(torch.zeros(4, 16, 2), t, 2, per_item=True)
    with pytest.raises(_lib.SequitrHipError):
        ops.confusion_(torch.zeros(4, 2, 2, dtype=torch.int64), torch.zeros(4, dtype=torch.int64), p, t, 2)
    with pytest.raises(_lib.SequitrHipError):
        confusion.ConfusionMeter(2, 'cpu')
    with pytest.raises(_lib.SequitrHipError):
        confusion.confusion_matrix(t, p)                         # host tensors are refused; numpy arrays are uploaded
    with pytest.raises(ValueError):
        confusion.confusion_matrix(np.array([0, 16]), np.array([0, 1]))
    with pytest.raises(ValueError):
        confusion.ConfusionMeter(17)


def test_evaluate_refuses_a_label_shape_mismatch_before_any_gpu_work(tmp_path):
    frames = np.zeros((3, 80, 72), np.uint8)
    np.save(tmp_path / 'frames.npy', frames)
    np.save(tmp_path / 'labels.npy', np.zeros((3, 80, 70), np.uint8))
    params = {'input': str(tmp_path / 'frames.npy'), 'labels': str(tmp_path / 'labels.npy'), 'output': str(tmp_path),
              'shape': (64, 64), 'filters': (16, 32), 'margin': 8, 'num_outputs': 2}
    with pytest.raises(ValueError, match='do not match the frames'):
        jobs.SERVER_evaluate(params, {})
    with pytest.raises(ValueError, match='do not match the frames'):   # both as ndarrays
        jobs.SERVER_evaluate(dict(params, input=frames, labels=np.zeros((2, 80, 72), np.uint8)), {})
    with pytest.raises(TypeError, match='uint8'):
        jobs.SERVER_evaluate(dict(params, labels=np.zeros((3, 80, 72), np.int32)), {})
    vol = {'input': np.zeros((1, 8, 24, 24), np.uint8), 'labels': np.zeros((1, 8, 24, 20), np.uint8), 'brick': (16, 16, 8),
           'output': str(tmp_path), 'filters': (16, 32), 'num_outputs': 2}
    with pytest.raises(ValueError, match='do not match the volumes'):
        jobs.SERVER_evaluate(vol, {})
    assert not os.path.exists(tmp_path / 'evaluate.json') and not os.path.exists(tmp_path / 'confusion.npy')


def test_train_refuses_half_a_validation_pair_and_ranks(tmp_path, monkeypatch):
    params = {'images': 'unused.npy', 'labels': 'unused.npy', 'val_images': 'v.npy', 'output': str(tmp_path)}
    with pytest.raises(ValueError, match='go together'):
        jobs.SERVER_train(params, {})
    with pytest.raises(ValueError, match='validate_every'):
        jobs._validation_keys({'val_images': 'a', 'val_labels': 'b', 'validate_every': 0})
    assert jobs._validation_keys({}) == (False, None)
    assert jobs._validation_keys({'val_images': 'a', 'val_labels': 'b', 'validate_every': 2}) == (True, 2)
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(RuntimeError, match='single process'):
        jobs._validation_keys({'val_images': 'a', 'val_labels': 'b'})
    assert jobs._validation_keys({}) == (False, None)            # without the keys nothing changes under torchrun


def test_plot_confusion_matrix_saves_a_figure(tmp_path):
    pytest.importorskip('matplotlib')
    import matplotlib
    matplotlib.use('Agg')
    c = np.array([[50, 2, 0], [3, 40, 1], [0, 0, 9]], np.int64)
    out = tmp_path / 'cm.png'
    confusion.plot_confusion_matrix(c, labels=['background', 'cell', 'debris'], save=str(out))
    assert out.stat().st_size > 1000
    confusion.plot_confusion_matrix(c, scores=False, normalise=False, fmt='%.1f', save=str(tmp_path / 'raw.png'))
    assert (tmp_path / 'raw.png').exists()
    import matplotlib.pyplot as plt
    assert not plt.get_fignums()                                 # the figures are closed after saving
    with pytest.raises(TypeError):
        confusion.plot_confusion_matrix(c, save=3)
