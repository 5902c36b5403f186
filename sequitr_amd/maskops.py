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


def _check_mask(mask, classes, rank=3):
    """rank 3: a planar (N,H,W) mask; 4: the (N,D,H,W) mask of sequitr_amd.volumeops"""
    if not isinstance(mask, torch.Tensor):
        raise TypeError("mask must be a torch.Tensor in GPU memory")
    if not mask.is_cuda:
        raise _lib.SequitrHipError("mask must live in GPU memory (no CPU fallback exists)")
    if mask.dtype != torch.uint8:
        raise ValueError("mask must be uint8 class labels, got %s" % mask.dtype)
    if mask.dim() != rank:
        if rank == 3:
            raise ValueError("mask clean-up covers planar (N,H,W) masks only, got shape %s: volumes are out of scope"
                             % (tuple(mask.shape),))
        if mask.dim() == 3:
            raise ValueError("volume clean-up covers (N,D,H,W) masks, got the planar shape %s: use sequitr_amd.maskops"
                             % (tuple(mask.shape),))
        raise ValueError("volume clean-up covers (N,D,H,W) masks, got shape %s" % (tuple(mask.shape),))
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
    return tuple(int(s) for s in mask.shape)


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
    return _split(mask, erosions, structure, reach, classes, out, workspace, 3, STRUCTURES, MORPH_MAX_ITER, SPLIT_MAX_REACH,
                  lambda r, st: 2 * r, "sq_mask_split_workspace", "sq_mask_split_u8")


def _split(mask, erosions, structure, reach, classes, out, workspace, rank, structures, max_erosions, max_reach,
           default_reach, workspace_fn, split_fn):
    """split and volumeops.split3d: the rank of the mask, `structures` names -> codes, the two caps,
    default_reach(erosions, structure) for reach=None, and the names of the library's two functions"""
    if structure not in structures:
        raise ValueError("structure must be one of %s, got %r" % (sorted(structures), structure))
    erosions = int(erosions)
    if not 1 <= erosions <= max_erosions:
        raise ValueError("erosions must be 1 .. %d, got %d" % (max_erosions, erosions))
    reach = default_reach(erosions, structure) if reach is None else int(reach)
    if not 1 <= reach <= max_reach:
        raise ValueError("reach must be 1 .. %d, got %d" % (max_reach, reach))
    classes = _check_mask(mask, classes, rank)
    out = _check_out(out, mask)
    lib = _lib.load()
    ws = _workspace(getattr(lib, workspace_fn), mask, workspace)
    _lib.check(getattr(lib, split_fn)(mask.data_ptr(), out.data_ptr(), *(_dims(mask) + (
        classes, erosions, structures[structure], reach, ws.data_ptr(), _stream(mask)))), split_fn)
    return out


def load_steps(spec):
    """a step list as the jobs take it: the list itself, or the path of a JSON file that holds one"""
    if isinstance(spec, str):
        with open(spec) as f:
            spec = json.load(f)
    return spec


class _Cleanup(object):
    """What MaskCleanup and VolumeCleanup share: a validated list of steps that runs between two cached buffers.  A
    subclass gives LABEL (the job parameter its messages name), RANK (of its masks), STEP_KEYS (op -> the keys a step may
    carry besides 'op', with their defaults), NOT_BUILT (op -> why it is no step here) and three methods:
    _check_step(where, op, full) raises a ValueError that starts with `where` for a bad value,
    _step_workspace(lib, step, dims) is the bytes of workspace a step needs (0: none, < 0: too large),
    _run(step, src, classes, dst, ws) runs one step."""
    NOT_BUILT = {}

    def __init__(self, steps):
        label, keys = self.LABEL, self.STEP_KEYS
        if isinstance(steps, type(self)):
            steps = steps.record()
        if not isinstance(steps, (list, tuple)) or not steps:
            raise ValueError("%s steps must be a non-empty list of {'op': ...} dicts, got %r" % (label, steps))
        self.steps = []
        for i, step in enumerate(steps):
            if not isinstance(step, dict) or 'op' not in step:
                raise ValueError("%s step %d must be a dict with an 'op', got %r" % (label, i, step))
            op = step['op']
            if not isinstance(op, str) or op not in keys:
                why = self.NOT_BUILT[op] if isinstance(op, str) and op in self.NOT_BUILT else "unknown op %r" % (op,)
                raise ValueError("%s step %d: %s (known: %s)" % (label, i, why, ', '.join(sorted(keys))))
            unknown = sorted(k for k in step if k != 'op' and k not in keys[op])
            if unknown:
                raise ValueError("%s step %d (%s): unknown key(s) %s (allowed: %s)"
                                 % (label, i, op, ', '.join(map(repr, unknown)), ', '.join(sorted(keys[op])) or 'none'))
            full = dict(keys[op], **step)
            self._check_step("%s step %d (%s)" % (label, i, op), op, full)
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
                nbytes = self._step_workspace(lib, s, _dims(mask))
                if nbytes < 0:
                    raise ValueError("mask %s is too large for one call" % (tuple(mask.shape),))
                need = max(need, nbytes)
            ws = torch.empty(need // 4, dtype=torch.int32, device=mask.device) if need else None
            self._cache[key] = (torch.empty_like(mask), torch.empty_like(mask), ws)
        return self._cache[key]

    def apply(self, mask, classes):
        """Run the steps on `mask` (uint8 on the GPU, `classes` classes) on the current stream.  The input is not
        written; the result is one of two buffers this object caches per shape (nothing is allocated after the first call
        for a shape), valid until the next apply()."""
        classes = int(classes)
        if classes < 2:
            raise ValueError("classes must be at least 2, got %d" % classes)
        _check_mask(mask, classes, self.RANK)
        a, b, ws = self._buffers(mask)
        src = mask
        for s in self.steps:
            dst = a if src is not a else b
            self._run(s, src, classes, dst, ws)
            src = dst
        return src


def _is_int(v, lo, hi=None):
    return not isinstance(v, bool) and isinstance(v, int) and v >= lo and (hi is None or v <= hi)


def _check_split_step(where, full, structures, max_erosions, max_reach):
    """the 'split' step of a MaskCleanup list and the 'split3d' step of a VolumeCleanup list"""
    if not _is_int(full['erosions'], 1, max_erosions):
        raise ValueError("%s: erosions must be an integer 1 .. %d, got %r" % (where, max_erosions, full['erosions']))
    if not isinstance(full['structure'], str) or full['structure'] not in structures:
        raise ValueError("%s: structure must be one of %s, got %r" % (where, sorted(structures), full['structure']))
    if full['reach'] is not None and not _is_int(full['reach'], 1, max_reach):
        raise ValueError("%s: reach must be an integer 1 .. %d or null, got %r" % (where, max_reach, full['reach']))


class MaskCleanup(_Cleanup):
    """A validated list of clean-up steps, e.g. [{"op": "open", "iterations": 2, "structure": "cross"},
    {"op": "fill_holes", "max_area": 400}, {"op": "split", "erosions": 8}, {"op": "clear_border"}].  Unknown ops, unknown keys and bad values raise a
    ValueError that names them, at construction.  ``apply`` runs the steps in order on a batch of (N,H,W) device masks."""
    LABEL, RANK, STEP_KEYS = 'postprocess', 3, _STEP_KEYS

    def _check_step(self, where, op, full):
        if op in MORPH_OPS and not _is_int(full['iterations'], 1, MORPH_MAX_ITER):
            raise ValueError("%s: iterations must be an integer 1 .. %d, got %r" % (where, MORPH_MAX_ITER, full['iterations']))
        if op == 'fill_holes' and full['max_area'] is not None and not _is_int(full['max_area'], 1):
            raise ValueError("%s: max_area must be a positive integer or null, got %r" % (where, full['max_area']))
        if op == 'split':
            _check_split_step(where, full, STRUCTURES, MORPH_MAX_ITER, SPLIT_MAX_REACH)
        elif 'structure' in full and full['structure'] not in STRUCTURES:
            raise ValueError("%s: structure must be one of %s, got %r" % (where, sorted(STRUCTURES), full['structure']))

    def _step_workspace(self, lib, s, dims):
        fn = {'fill_holes': lib.sq_mask_fill_holes_workspace, 'clear_border': lib.sq_mask_clear_border_workspace,
              'split': lib.sq_mask_split_workspace}.get(s['op'])
        return fn(*dims) if fn is not None else 0

    def _run(self, s, src, classes, dst, ws):
        if s['op'] in MORPH_OPS:
            morph(src, s['op'], s['iterations'], s['structure'], classes, out=dst)
        elif s['op'] == 'fill_holes':
            fill_holes(src, s['max_area'], classes, out=dst, workspace=ws)
        elif s['op'] == 'split':
            split(src, s['erosions'], s['structure'], s['reach'], classes, out=dst, workspace=ws)
        else:
            clear_border(src, classes, out=dst, workspace=ws)
