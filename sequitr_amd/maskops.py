"""Clean up segmented masks where they lie, in HBM, between "mask" and "objects": binary morphology per class, hole
filling, removal of objects cut by the frame edge.  The reference has no counterpart -- its CentroidWriter
(sequitr/utils.py:492-494) measures the raw argmax mask and users ran scipy.ndimage on a downloaded mask.npy.

``morph``, ``fill_holes``, ``clear_border`` and ``split`` are one C-ABI call each (sq_mask_morph_u8,
sq_mask_fill_holes_u8, sq_mask_clear_border_u8, sq_mask_split_u8; include/sequitr_hip.h, "Mask clean-up" and "Mask
clean-up: splitting", is the contract: classes, merge rules, scipy's definitions).  ``MaskCleanup`` is a validated list of such steps that runs on a batch of device masks between two cached
buffers; the frame jobs take one as ``params['postprocess']``.  Planar (N, H, W) uint8 masks only; there is no CPU path.
The (N, D, H, W) masks of UNet3D are cleaned by sequitr_amd.volumeops (3-D morphology, cavities, faces).
Every result equals the scipy restatement in tests/mask_cleanup_cases.py and tests/mask_split_cases.py exactly
(tests/test_gpu_mask_cleanup.py, tests/test_gpu_mask_split.py).

``split`` separates touching objects: seeds are the components of the eroded class planes, they grow back through
their class for a bounded number of synchronous steps, and a one-pixel line of background is cut where two different
seeds' growths meet.  Deliberately not built: growth until nothing changes (it would need a device-to-host readback
inside the frame stream and could not be captured in a graph; pixels beyond ``reach`` keep their class and may still
bridge two parts), and seeds from the Euclidean distance transform or its h-maxima (the seeds are plain erosions).
Objects whose eroded cores stay connected -- three mutually overlapping disks, say -- are not split.
"""
import json

import torch

from . import _lib

MORPH_TILE = (64, 192)                                          # SQ_MORPH_TILE_ROWS, SQ_MORPH_TILE_COLS: a block's tile
MORPH_MAX_ITER = 16                                             # SQ_MORPH_MAX_ITER
MORPH_OPS = {'erode': 0, 'dilate': 1, 'open': 2, 'close': 3}    # SQ_MORPH_*
STRUCTURES = {'cross': 0, 'square': 1}                          # generate_binary_structure(2, 1) / (2, 2)
SPLIT_MAX_REACH = 64                                            # SQ_SPLIT_MAX_REACH
SPLIT_TILE = (64, 64)                                           # SQ_SPLIT_TILE_ROWS, SQ_SPLIT_TILE_COLS
SPLIT_STEPS = 8                                                 # SQ_SPLIT_STEPS: synchronous steps per launch = halo

# op -> the keys a step may carry besides 'op', with their defaults
_STEP_KEYS = dict({op: {'iterations': 1, 'structure': 'cross'} for op in MORPH_OPS},
                  fill_holes={'max_area': None}, clear_border={},
                  split={'erosions': None, 'structure': 'cross', 'reach': None})


def _check_mask(mask, classes):
    if not isinstance(mask, torch.Tensor):
        raise TypeError("mask must be a torch.Tensor in GPU memory")
    if not mask.is_cuda:
        raise _lib.SequitrHipError("mask must live in GPU memory (no CPU fallback exists)")
    if mask.dtype != torch.uint8:
        raise ValueError("mask must be uint8 class labels, got %s" % mask.dtype)
    if mask.dim() != 3:
        raise ValueError("mask clean-up covers planar (N,H,W) masks only, got shape %s: volumes are out of scope"
                         % (tuple(mask.shape),))
    if not mask.is_contiguous():
        raise ValueError("mask must be contiguous: pass a packed copy of a view")
    if mask.numel() == 0:
        raise ValueError("mask %s is empty" % (tuple(mask.shape),))
    if classes is None:
        return max(int(mask.max()) + 1, 2)                      # an all-background mask still has a class 1
    return int(classes)


def _check_out(out, mask):
    if out is None:
        return torch.empty_like(mask)
    if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != mask.device \
            or tuple(out.shape) != tuple(mask.shape) or not out.is_contiguous():
        raise ValueError("out must be a contiguous uint8 tensor of the mask's shape on its device")
    return out


def _dims(mask):
    return int(mask.shape[0]), int(mask.shape[1]), int(mask.shape[2])


def _stream(mask):
    return torch.cuda.current_stream(mask.device).cuda_stream


def _workspace(fn, mask, workspace):
    nbytes = fn(*_dims(mask))
    if nbytes < 0:
        raise ValueError("mask %s is too large for one call" % (tuple(mask.shape),))
    if workspace is None:
        return torch.empty(nbytes // 4, dtype=torch.int32, device=mask.device)
    if workspace.numel() * workspace.element_size() < nbytes:
        raise ValueError("workspace holds %d bytes, the call needs %d" % (workspace.numel() * workspace.element_size(), nbytes))
    return workspace


def morph(mask, op, iterations=1, structure='cross', classes=None, out=None):
    """scipy.ndimage.binary_{erosion,dilation,opening,closing} of every class plane of `mask` ((N,H,W) uint8 on the GPU),
    `iterations` = 1 .. MORPH_MAX_ITER times with the 'cross' or 'square' structure, merged by the header's rules.
    classes: the number of classes C (default: the largest byte + 1); bytes >= C pass through.  Returns a new tensor, or
    `out` (which must not overlap the mask)."""
    if op not in MORPH_OPS:
        raise ValueError("op must be one of %s, got %r" % (sorted(MORPH_OPS), op))
    if structure not in STRUCTURES:
        raise ValueError("structure must be one of %s, got %r" % (sorted(STRUCTURES), structure))
    iterations = int(iterations)
    if not 1 <= iterations <= MORPH_MAX_ITER:
        raise ValueError("iterations must be 1 .. %d, got %d" % (MORPH_MAX_ITER, iterations))
    classes = _check_mask(mask, classes)
    out = _check_out(out, mask)
    N, H, W = _dims(mask)
    lib = _lib.load()
    _lib.check(lib.sq_mask_morph_u8(mask.data_ptr(), out.data_ptr(), N, H, W, classes, MORPH_OPS[op], STRUCTURES[structure],
                                    iterations, _stream(mask)), "sq_mask_morph_u8")
    return out


def fill_holes(mask, max_area=None, classes=None, out=None, workspace=None):
    """scipy.ndimage.binary_fill_holes per class: background enclosed by class c (4-connected, not reaching the frame's
    outer rows or columns) becomes c, the lowest class first.  max_area: fill only holes of at most that many pixels,
    counting everything inside the hole (None or <= 0: all holes)."""
    classes = _check_mask(mask, classes)
    out = _check_out(out, mask)
    lib = _lib.load()
    ws = _workspace(lib.sq_mask_fill_holes_workspace, mask, workspace)
    N, H, W = _dims(mask)
    _lib.check(lib.sq_mask_fill_holes_u8(mask.data_ptr(), out.data_ptr(), N, H, W, classes,
                                         0 if max_area is None else int(max_area), ws.data_ptr(), _stream(mask)),
               "sq_mask_fill_holes_u8")
    return out


def clear_border(mask, classes=None, out=None, workspace=None):
    """Remove every object (4-connected, one class) that has a pixel in the frame's first or last row or column."""
    classes = _check_mask(mask, classes)
    out = _check_out(out, mask)
    lib = _lib.load()
    ws = _workspace(lib.sq_mask_clear_border_workspace, mask, workspace)
    N, H, W = _dims(mask)
    _lib.check(lib.sq_mask_clear_border_u8(mask.data_ptr(), out.data_ptr(), N, H, W, classes, ws.data_ptr(), _stream(mask)),
               "sq_mask_clear_border_u8")
    return out


def split(mask, erosions, structure='cross', reach=None, classes=None, out=None, workspace=None):
    """Cut a one-pixel line of background between the parts of an object (include/sequitr_hip.h, "Mask clean-up:
    splitting").  Seeds are the 4-connected components of every class plane eroded `erosions` = 1 .. MORPH_MAX_ITER times
    with `structure`; they grow back through their class for `reach` = 1 .. SPLIT_MAX_REACH synchronous steps (None:
    2 * erosions), the smallest label winning where several arrive together, and a labelled pixel with a same-class
    neighbour of a smaller label becomes background.  Everything else is unchanged; bytes >= classes pass through."""
    if structure not in STRUCTURES:
        raise ValueError("structure must be one of %s, got %r" % (sorted(STRUCTURES), structure))
    erosions = int(erosions)
    if not 1 <= erosions <= MORPH_MAX_ITER:
        raise ValueError("erosions must be 1 .. %d, got %d" % (MORPH_MAX_ITER, erosions))
    reach = 2 * erosions if reach is None else int(reach)
    if not 1 <= reach <= SPLIT_MAX_REACH:
        raise ValueError("reach must be 1 .. %d, got %d" % (SPLIT_MAX_REACH, reach))
    classes = _check_mask(mask, classes)
    out = _check_out(out, mask)
    lib = _lib.load()
    ws = _workspace(lib.sq_mask_split_workspace, mask, workspace)
    N, H, W = _dims(mask)
    _lib.check(lib.sq_mask_split_u8(mask.data_ptr(), out.data_ptr(), N, H, W, classes, erosions, STRUCTURES[structure], reach,
                                    ws.data_ptr(), _stream(mask)), "sq_mask_split_u8")
    return out


def load_steps(spec):
    """a step list as the jobs take it: the list itself, or the path of a JSON file that holds one"""
    if isinstance(spec, str):
        with open(spec) as f:
            spec = json.load(f)
    return spec


class MaskCleanup(object):
    """A validated list of clean-up steps, e.g. [{"op": "open", "iterations": 2, "structure": "cross"},
    {"op": "fill_holes", "max_area": 400}, {"op": "split", "erosions": 8}, {"op": "clear_border"}].  Unknown ops, unknown keys and bad values raise a
    ValueError that names them, at construction.  ``apply`` runs the steps in order on a batch of device masks."""

    def __init__(self, steps):
        if isinstance(steps, MaskCleanup):
            steps = steps.record()
        if not isinstance(steps, (list, tuple)) or not steps:
            raise ValueError("postprocess steps must be a non-empty list of {'op': ...} dicts, got %r" % (steps,))
        self.steps = []
        for i, step in enumerate(steps):
            if not isinstance(step, dict) or 'op' not in step:
                raise ValueError("postprocess step %d must be a dict with an 'op', got %r" % (i, step))
            op = step['op']
            if not isinstance(op, str) or op not in _STEP_KEYS:
                raise ValueError("postprocess step %d: unknown op %r (known: %s)" % (i, op, ', '.join(sorted(_STEP_KEYS))))
            unknown = sorted(k for k in step if k != 'op' and k not in _STEP_KEYS[op])
            if unknown:
                raise ValueError("postprocess step %d (%s): unknown key(s) %s (allowed: %s)"
                                 % (i, op, ', '.join(map(repr, unknown)), ', '.join(sorted(_STEP_KEYS[op])) or 'none'))
            full = dict(_STEP_KEYS[op], **step)
            if op in MORPH_OPS:
                r = full['iterations']
                if isinstance(r, bool) or not isinstance(r, int) or not 1 <= r <= MORPH_MAX_ITER:
                    raise ValueError("postprocess step %d (%s): iterations must be an integer 1 .. %d, got %r"
                                     % (i, op, MORPH_MAX_ITER, r))
                if full['structure'] not in STRUCTURES:
                    raise ValueError("postprocess step %d (%s): structure must be one of %s, got %r"
                                     % (i, op, sorted(STRUCTURES), full['structure']))
            elif op == 'fill_holes':
                a = full['max_area']
                if a is not None and (isinstance(a, bool) or not isinstance(a, int) or a < 1):
                    raise ValueError("postprocess step %d (fill_holes): max_area must be a positive integer or null, got %r"
                                     % (i, a))
            elif op == 'split':
                r, t = full['erosions'], full['reach']
                if isinstance(r, bool) or not isinstance(r, int) or not 1 <= r <= MORPH_MAX_ITER:
                    raise ValueError("postprocess step %d (split): erosions must be an integer 1 .. %d, got %r"
                                     % (i, MORPH_MAX_ITER, r))
                if full['structure'] not in STRUCTURES:
                    raise ValueError("postprocess step %d (split): structure must be one of %s, got %r"
                                     % (i, sorted(STRUCTURES), full['structure']))
                if t is not None and (isinstance(t, bool) or not isinstance(t, int) or not 1 <= t <= SPLIT_MAX_REACH):
                    raise ValueError("postprocess step %d (split): reach must be an integer 1 .. %d or null, got %r"
                                     % (i, SPLIT_MAX_REACH, t))
            self.steps.append(full)
        self._cache = {}

    def record(self):
        """the steps with every default written out: a JSON-able list"""
        return [dict(s) for s in self.steps]

    def _buffers(self, mask):
        key = (tuple(mask.shape), str(mask.device))
        if key not in self._cache:
            lib = _lib.load()
            need = 0
            for s in self.steps:
                fn = {'fill_holes': lib.sq_mask_fill_holes_workspace, 'clear_border': lib.sq_mask_clear_border_workspace,
                      'split': lib.sq_mask_split_workspace}.get(s['op'])
                if fn is not None:
                    nbytes = fn(*_dims(mask))
                    if nbytes < 0:
                        raise ValueError("mask %s is too large for one call" % (tuple(mask.shape),))
                    need = max(need, nbytes)
            ws = torch.empty(need // 4, dtype=torch.int32, device=mask.device) if need else None
            self._cache[key] = (torch.empty_like(mask), torch.empty_like(mask), ws)
        return self._cache[key]

    def apply(self, mask, classes):
        """Run the steps on `mask` ((N,H,W) uint8 on the GPU, `classes` classes) on the current stream.  The input is not
        written; the result is one of two buffers this object caches per shape (nothing is allocated after the first call
        for a shape), valid until the next apply()."""
        classes = int(classes)
        if classes < 2:
            raise ValueError("classes must be at least 2, got %d" % classes)
        _check_mask(mask, classes)
        a, b, ws = self._buffers(mask)
        src = mask
        for s in self.steps:
            dst = a if src is not a else b
            if s['op'] in MORPH_OPS:
                morph(src, s['op'], s['iterations'], s['structure'], classes, out=dst)
            elif s['op'] == 'fill_holes':
                fill_holes(src, s['max_area'], classes, out=dst, workspace=ws)
            elif s['op'] == 'split':
                split(src, s['erosions'], s['structure'], s['reach'], classes, out=dst, workspace=ws)
            else:
                clear_border(src, classes, out=dst, workspace=ws)
            src = dst
        return src
