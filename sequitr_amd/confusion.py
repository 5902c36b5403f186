"""Scoring masks against labels on the GPU: the counterpart of the reference's sequitr/confusion.py.

The reference's confusion_matrix hands host arrays to scikit-learn.  Here the counting is one streaming HIP pass over the
prediction and the labels where they already are, in HBM (sq_confusion, include/sequitr_hip.h "Scoring"), and what comes
back to the host is C x C integers:

    confusion_counts(pred, truth, C)       device tensors in, device int64 counts out
    ConfusionMeter(C, device)              accumulates over the batches of a stream without synchronising
    scores(counts)                         IoU, Dice, precision, recall, accuracy from the integer matrix (numpy, float64)
    confusion_matrix / plot_confusion_matrix   the reference's two functions

Rows are the truth and columns the prediction, scikit-learn's convention.  A pixel whose label is >= C (255 is the usual
"unlabelled" value), whose one-hot row is all zero, or whose mask byte is >= C is counted in `ignored` and in no cell.
There is no host fallback: a CPU tensor is an error.
"""
import numpy as np
import torch

from . import _lib, ops

DEFAULT_LABELS = []
MAX_CLASSES = 16


def _device_pair(pred, truth):
    for t, name in ((pred, "pred"), (truth, "truth")):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor" % name)
        if not t.is_cuda:
            raise _lib.SequitrHipError("%s must live in GPU memory (no CPU fallback exists)" % name)


def _kinds(pred, truth, C):
    """(space, onehot): the shape the classes live on, and whether truth carries a trailing one-hot axis"""
    if pred.dtype == torch.uint8:
        space = tuple(pred.shape)
    elif pred.dtype == torch.float32:
        if pred.dim() < 1 or pred.shape[-1] != C:
            raise ValueError("float32 logits must end in %d classes, got %s" % (C, tuple(pred.shape)))
        space = tuple(pred.shape[:-1])
    else:
        raise TypeError("pred must be uint8 masks or float32 logits, got %s" % pred.dtype)
    if truth.dtype != torch.uint8:
        raise TypeError("truth must be uint8, got %s" % truth.dtype)
    if tuple(truth.shape) == space:
        return space, False
    if tuple(truth.shape) == space + (C,):
        return space, True
    raise ValueError("truth has shape %s; expected %s (class indices) or %s (one-hot)"
                     % (tuple(truth.shape), space, space + (C,)))


def _rows(pred, truth, C, per_item):
    """pred and truth as (items, n[, C]) views: one row per leading index, or one row for everything"""
    space, onehot = _kinds(pred, truth, C)
    if per_item and not space:
        raise ValueError("per_item needs a leading items axis")
    items = space[0] if per_item else 1
    lead = (items, -1)
    p = pred.reshape(lead if pred.dtype == torch.uint8 else lead + (C,))
    t = truth.reshape(lead + (C,) if onehot else lead)
    return p, t, items


def confusion_counts(pred, truth, num_classes, per_item=False):
    """Confusion counts of `pred` against `truth`, counted on the device.

    pred:  uint8 class masks of any shape, or float32 logits with a trailing axis of num_classes (arg-max with ties to
           the lowest index, the class ops.argmax_u8 writes; no mask is materialised).
    truth: uint8 class indices of the mask's shape, or the trainer's one-hot uint8 format with a trailing num_classes.
    Returns (counts, ignored), device int64: (C, C) and () over everything, or (items, C, C) and (items,) with one row per
    index of the leading axis when per_item is set.  No synchronisation.
    """
    _device_pair(pred, truth)
    C = int(num_classes)
    if not pred.is_contiguous() or not truth.is_contiguous():
        raise ValueError("pred and truth must be contiguous")
    p, t, items = _rows(pred, truth, C, per_item)
    counts = torch.zeros((items, C, C), dtype=torch.int64, device=pred.device)
    ignored = torch.zeros((items,), dtype=torch.int64, device=pred.device)
    ops.confusion_(counts, ignored, p, t, C)
    return (counts, ignored) if per_item else (counts[0], ignored[0])


class ConfusionMeter(object):
    """Running confusion counts in HBM: update() per batch adds into the same C x C integers and never synchronises;
    counts() / scores() download them."""

    def __init__(self, num_classes, device=None):
        self.num_classes = int(num_classes)
        if not 1 <= self.num_classes <= MAX_CLASSES:
            raise ValueError("num_classes %d not in 1 .. %d" % (self.num_classes, MAX_CLASSES))
        self.device = torch.device("cuda" if device is None else device)
        if self.device.type != "cuda":
            raise _lib.SequitrHipError("ConfusionMeter counts in GPU memory (no CPU fallback exists)")
        C = self.num_classes
        self._counts = torch.zeros((1, C, C), dtype=torch.int64, device=self.device)
        self._ignored = torch.zeros((1,), dtype=torch.int64, device=self.device)

    def update(self, pred, truth):
        _device_pair(pred, truth)
        if not pred.is_contiguous() or not truth.is_contiguous():
            raise ValueError("pred and truth must be contiguous")
        p, t, _ = _rows(pred, truth, self.num_classes, False)
        ops.confusion_(self._counts, self._ignored, p, t, self.num_classes)
        return self

    def reset(self):
        self._counts.zero_()
        self._ignored.zero_()
        return self

    def counts(self):
        return self._counts[0].cpu().numpy()

    def ignored(self):
        return int(self._ignored[0].item())

    def scores(self):
        return scores(self.counts())


def _ratio(num, den):
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    out = np.full(np.broadcast(num, den).shape, np.nan)
    np.divide(num, den, out=out, where=den != 0)
    return out


def scores(counts):
    """Scores of an integer confusion matrix (C, C), row = truth, column = prediction, in float64:
    tp = diag, fp = column sum - tp, fn = row sum - tp;  iou = tp / (tp + fp + fn), dice = 2tp / (2tp + fp + fn),
    precision = tp / (tp + fp), recall = tp / (tp + fn), accuracy = sum(tp) / sum(counts), mean_iou = nanmean(iou),
    support = the row sums.  A 0 / 0 is NaN (json_ready writes it as null)."""
    c = np.asarray(counts)
    if c.ndim != 2 or c.shape[0] != c.shape[1]:
        raise ValueError("counts must be a square matrix, got %s" % (c.shape,))
    c = c.astype(np.int64)
    tp = np.diag(c)
    support = c.sum(1)
    fp, fn = c.sum(0) - tp, support - tp
    iou = _ratio(tp, tp + fp + fn)
    return {"iou": iou,
            "dice": _ratio(2 * tp, 2 * tp + fp + fn),
            "precision": _ratio(tp, tp + fp),
            "recall": _ratio(tp, tp + fn),
            "accuracy": float(_ratio(tp.sum(), c.sum())),
            "mean_iou": float(np.mean(iou[~np.isnan(iou)])) if (~np.isnan(iou)).any() else float("nan"),
            "support": support}


def json_ready(obj):
    """arrays -> lists, numpy scalars -> Python numbers, NaN -> None (JSON null), through dicts and lists"""
    if isinstance(obj, dict):
        return {k: json_ready(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [json_ready(v) for v in obj]
    if isinstance(obj, np.ndarray):
        return json_ready(obj.tolist())
    if isinstance(obj, (float, np.floating)):
        return None if np.isnan(obj) else float(obj)
    if isinstance(obj, np.integer):
        return int(obj)
    return obj


def compress_present(counts):
    """The rows and columns of the classes that occur in either argument, in sorted order: what scikit-learn's
    confusion_matrix returns when it is given no labels."""
    c = np.asarray(counts)
    keep = np.flatnonzero((c.sum(0) + c.sum(1)) > 0)
    return c[np.ix_(keep, keep)]


def _class_indices(y, name, device):
    if isinstance(y, torch.Tensor):
        if not y.is_cuda:
            raise _lib.SequitrHipError("%s must live in GPU memory, or be a numpy array to upload" % name)
        if y.dtype != torch.uint8:
            if y.numel() and (int(y.min()) < 0 or int(y.max()) >= MAX_CLASSES):
                raise ValueError("%s holds classes outside 0 .. %d" % (name, MAX_CLASSES - 1))
            y = y.to(torch.uint8)
        return y.contiguous().reshape(-1)
    a = np.asarray(y)
    if a.dtype.kind not in "iub":
        raise TypeError("%s must hold integer class indices, got %s" % (name, a.dtype))
    if a.size and (a.min() < 0 or a.max() >= MAX_CLASSES):
        raise ValueError("%s holds classes outside 0 .. %d" % (name, MAX_CLASSES - 1))
    return torch.from_numpy(np.ascontiguousarray(a.reshape(-1).astype(np.uint8))).to(device)


def confusion_matrix(y_true, y_pred, labels=DEFAULT_LABELS, display=False):
    """The reference's confusion_matrix: the int64 matrix sklearn.metrics.confusion_matrix(y_true, y_pred) returns, for
    numpy arrays or device tensors of class indices 0 .. 15.  Numpy inputs are uploaded; the counting runs on the device
    over all 16 classes and the matrix is compressed to the classes present in either argument, as scikit-learn does."""
    device = next((y.device for y in (y_true, y_pred) if isinstance(y, torch.Tensor) and y.is_cuda), "cuda")
    t, p = _class_indices(y_true, "y_true", device), _class_indices(y_pred, "y_pred", device)
    if t.numel() != p.numel():
        raise ValueError("y_true and y_pred hold %d and %d samples" % (t.numel(), p.numel()))
    counts, ignored = confusion_counts(p, t, MAX_CLASSES)
    if int(ignored.item()):
        raise ValueError("y_true or y_pred holds classes outside 0 .. %d" % (MAX_CLASSES - 1))
    conf_matrix = compress_present(counts.cpu().numpy())
    if display:
        plot_confusion_matrix(conf_matrix, labels)
    return conf_matrix


def plot_confusion_matrix(c, labels=DEFAULT_LABELS, scores=True, fmt='%.3f', save=None, normalise=True, epsilon=1e-99):
    """Draw a confusion matrix (row = truth, column = prediction) as a heat map with the ground truth along x and the
    prediction along y, each cell coloured by its share of its true class (of the raw count with normalise=False) and,
    with `scores`, annotated with the count and that share formatted by `fmt`.  `save`: a file name to write the figure
    to instead of showing it.  matplotlib is imported here, so that the module works without it."""
    if save is not None and not isinstance(save, str):
        raise TypeError('Filename should be a string')
    import matplotlib.pyplot as plt

    c = np.asarray(c)
    shown = c.T.astype(np.float64)                              # truth along x, prediction along y
    share = shown / (shown.sum(axis=0, keepdims=True) + epsilon)
    cells = share if normalise else shown
    fig, ax = plt.subplots(figsize=(10, 6))
    heatmap = ax.pcolormesh(cells, cmap="viridis", vmin=0., vmax=1. if normalise else max(float(shown.max()), 1.))
    if scores:
        top = 1. if normalise else max(float(shown.max()), 1.)
        for (y, x), count in np.ndenumerate(c.T):
            colour = "black" if cells[y, x] > 0.5 * top else "white"
            ax.text(x + 0.5, y + 0.5, ("%d \n (" + fmt + ")") % (int(count), share[y, x]), ha="center", va="center",
                    color=colour)
    ax.set_xticks(np.arange(cells.shape[1]) + 0.5, minor=False)
    ax.set_yticks(np.arange(cells.shape[0]) + 0.5, minor=False)
    names = [str(l).title() for l in labels] if len(labels) else [str(k) for k in range(c.shape[0])]
    ax.set_xticklabels(names[:cells.shape[1]], minor=False, rotation='vertical')
    ax.set_yticklabels(names[:cells.shape[0]], minor=False)
    ax.set_aspect('equal')
    ax.set_xlabel('Ground truth')
    ax.set_ylabel('Prediction')
    ax.set_title('Confusion matrix (%d examples)' % int(c.sum()))
    fig.colorbar(heatmap).set_label('Normalised class accuracy' if normalise else 'Count')
    fig.subplots_adjust(bottom=.25, left=.25)
    if save is not None:
        fig.savefig(save, dpi=144)
        plt.close(fig)
    else:
        plt.show()
    return None
