"""Clean up segmented volumes where they lie, in HBM: the 3-D counterpart of maskops for the (N, D, H, W) uint8 masks of
UNet3D -- binary morphology per class with the 6- and 26-neighbour structures, filling of enclosed cavities, removal of
objects cut by the volume's faces.  The reference has no counterpart; its users ran scipy.ndimage on a downloaded mask.npy.

``morph3d``, ``fill_cavities`` and ``clear_border3d`` are one C-ABI call each (sq_volume_morph_u8, sq_volume_fill_holes_u8,
sq_volume_clear_border_u8; include/sequitr_hip.h, "Volume clean-up", is the contract: classes, merge rules, scipy's
definitions), or -- for the slice-by-slice variants, ``structure='plane_cross' | 'plane_square'`` and ``planar=True`` -- the
planar call of maskops on the zero-copy (N*D, H, W) view of the mask.  ``VolumeCleanup`` is a validated list of such steps
that runs between two cached buffers; the volume jobs take one as ``params['volume_postprocess']`` and
``frontend.segment_volumes`` as ``postprocess``.  There is no CPU path.  The three volume calls are chains of kernel
launches and can be captured in a graph and replayed; ``planar=True`` runs the planar entry, whose memset and memcpy calls
are not covered under replay.  Every result equals the scipy restatement in
tests/volume_cleanup_cases.py exactly (tests/test_gpu_volume_cleanup.py).

Not built, each on purpose: a 3-D ``split`` (the planar regrowth cut has no volume kernel); the 18-neighbour structure
(generate_binary_structure(3, 2)); more than MORPH3D_MAX_ITER iterations in one launch (use two steps, see the header
for when they compose); anisotropic, spacing-aware structuring elements.  What follows the clean-up -- ``measure`` and
``neighbors`` for volumes -- is SERVER_segment_volume's options of those names with ``brick`` (objects.measure_objects and
analysis/neighbors.py's neighbors3d on each cleaned mask in HBM).
"""
import torch

from . import _lib, maskops
from .maskops import MORPH_OPS, load_steps  # noqa: F401  (load_steps: the jobs' step-list loader)

MORPH3D_TILE = (8, 32, 128)                                     # SQ_MORPH3D_TILE_D, _H, _W: a block's brick
MORPH3D_MAX_ITER = 4                                            # SQ_MORPH3D_MAX_ITER
STRUCTURES3D = {'cross': 0, 'cube': 1}                          # generate_binary_structure(3, 1) / (3, 3)
PLANE_STRUCTURES = {'plane_cross': 'cross', 'plane_square': 'square'}   # generate_binary_structure(2, k)[None]: per slice
FACES = {'all': 0, 'lateral': 1}                                # SQ_FACES_ALL, SQ_FACES_LATERAL

# op -> the keys a step may carry besides 'op', with their defaults
_STEP_KEYS = dict({op: {'iterations': 1, 'structure': 'cross'} for op in MORPH_OPS},
                  fill_holes={'max_voxels': None, 'planar': False}, clear_border={'faces': 'all'})


def _check_mask(mask, classes):
    if not isinstance(mask, torch.Tensor):
        raise TypeError("mask must be a torch.Tensor in GPU memory")
    if not mask.is_cuda:
        raise _lib.SequitrHipError("mask must live in GPU memory (no CPU fallback exists)")
    if mask.dtype != torch.uint8:
        raise ValueError("mask must be uint8 class labels, got %s" % mask.dtype)
    if mask.dim() == 3:
        raise ValueError("volume clean-up covers (N,D,H,W) masks, got the planar shape %s: use sequitr_amd.maskops"
                         % (tuple(mask.shape),))
    if mask.dim() != 4:
        raise ValueError("volume clean-up covers (N,D,H,W) masks, got shape %s" % (tuple(mask.shape),))
    if not mask.is_contiguous():
        raise ValueError("mask must be contiguous: pass a packed copy of a view")
    if mask.numel() == 0:
        raise ValueError("mask %s is empty" % (tuple(mask.shape),))
    if classes is None:
        return max(int(mask.max()) + 1, 2)                      # an all-background mask still has a class 1
    return int(classes)


def _dims(mask):
    return tuple(int(s) for s in mask.shape)


def _slices(t):
    """the zero-copy (N*D, H, W) view of a contiguous (N, D, H, W) tensor"""
    return t.view(t.shape[0] * t.shape[1], t.shape[2], t.shape[3])


def _workspace(fn, mask, workspace):
    nbytes = fn(*_dims(mask))
    if nbytes < 0:
        raise ValueError("mask %s is too large for one call" % (tuple(mask.shape),))
    if workspace is None:
        return torch.empty(nbytes // 4, dtype=torch.int32, device=mask.device)
    if workspace.numel() * workspace.element_size() < nbytes:
        raise ValueError("workspace holds %d bytes, the call needs %d" % (workspace.numel() * workspace.element_size(), nbytes))
    return workspace


def _check_morph(op, iterations, structure):
    if op not in MORPH_OPS:
        raise ValueError("op must be one of %s, got %r" % (sorted(MORPH_OPS), op))
    if structure not in STRUCTURES3D and structure not in PLANE_STRUCTURES:
        raise ValueError("structure must be one of %s, got %r" % (sorted(STRUCTURES3D) + sorted(PLANE_STRUCTURES), structure))
    iterations = int(iterations)
    cap = MORPH3D_MAX_ITER if structure in STRUCTURES3D else maskops.MORPH_MAX_ITER
    if not 1 <= iterations <= cap:
        raise ValueError("iterations must be 1 .. %d for structure %r, got %d" % (cap, structure, iterations))
    return iterations


def morph3d(mask, op, iterations=1, structure='cross', classes=None, out=None):
    """scipy.ndimage.binary_{erosion,dilation,opening,closing} of every class plane of `mask` ((N,D,H,W) uint8 on the GPU),
    merged by the header's rules.  structure 'cross' (6 neighbours) or 'cube' (26): one launch of the 3-D kernel,
    `iterations` = 1 .. MORPH3D_MAX_ITER.  'plane_cross' / 'plane_square' are generate_binary_structure(2, k)[None], the
    planar operation slice by slice: maskops.morph on the (N*D, H, W) view, `iterations` = 1 .. maskops.MORPH_MAX_ITER.
    classes: the number of classes C (default: the largest byte + 1); bytes >= C pass through.  Returns a new tensor, or
    `out` (which must not overlap the mask)."""
    iterations = _check_morph(op, iterations, structure)
    classes = _check_mask(mask, classes)
    out = maskops._check_out(out, mask)
    if structure in PLANE_STRUCTURES:
        maskops.morph(_slices(mask), op, iterations, PLANE_STRUCTURES[structure], classes, out=_slices(out))
        return out
    lib = _lib.load()
    _lib.check(lib.sq_volume_morph_u8(mask.data_ptr(), out.data_ptr(), *(_dims(mask) + (
        classes, MORPH_OPS[op], STRUCTURES3D[structure], iterations, maskops._stream(mask)))), "sq_volume_morph_u8")
    return out


def fill_cavities(mask, max_voxels=None, planar=False, classes=None, out=None, workspace=None):
    """scipy.ndimage.binary_fill_holes per class on 3-D arrays: background enclosed by class c (6-connected, not reaching
    any of the volume's six faces) becomes c, the lowest class first.  max_voxels: fill only cavities of at most that
    many voxels, counting everything inside the cavity (None or <= 0: all).  planar=True fills the holes of every
    (H, W) slice instead -- maskops.fill_holes on the (N*D, H, W) view -- and max_voxels is then the slice hole's area."""
    classes = _check_mask(mask, classes)
    out = maskops._check_out(out, mask)
    if planar:
        maskops.fill_holes(_slices(mask), max_voxels, classes, out=_slices(out), workspace=workspace)
        return out
    lib = _lib.load()
    ws = _workspace(lib.sq_volume_fill_holes_workspace, mask, workspace)
    _lib.check(lib.sq_volume_fill_holes_u8(mask.data_ptr(), out.data_ptr(), *(_dims(mask) + (
        classes, 0 if max_voxels is None else int(max_voxels), ws.data_ptr(), maskops._stream(mask)))),
        "sq_volume_fill_holes_u8")
    return out


def clear_border3d(mask, faces='all', classes=None, out=None, workspace=None):
    """Remove every object (6-connected, one class) that has a voxel on a face of the volume: on any of the six with
    faces='all', on the four faces h = 0, H-1 and w = 0, W-1 only with faces='lateral' (objects cut by the first or last
    slice of a z-stack stay)."""
    if faces not in FACES:
        raise ValueError("faces must be one of %s, got %r" % (sorted(FACES), faces))
    classes = _check_mask(mask, classes)
    out = maskops._check_out(out, mask)
    lib = _lib.load()
    ws = _workspace(lib.sq_volume_clear_border_workspace, mask, workspace)
    _lib.check(lib.sq_volume_clear_border_u8(mask.data_ptr(), out.data_ptr(), *(_dims(mask) + (
        classes, FACES[faces], ws.data_ptr(), maskops._stream(mask)))), "sq_volume_clear_border_u8")
    return out


class VolumeCleanup(object):
    """A validated list of clean-up steps for volumes, e.g. [{"op": "open", "iterations": 1, "structure": "cross"},
    {"op": "fill_holes", "max_voxels": 500}, {"op": "clear_border", "faces": "lateral"}].  Unknown ops, unknown keys and
    bad values raise a ValueError that names them, at construction.  ``apply`` runs the steps in order on a batch of
    device masks."""

    def __init__(self, steps):
        if isinstance(steps, VolumeCleanup):
            steps = steps.record()
        if not isinstance(steps, (list, tuple)) or not steps:
            raise ValueError("volume_postprocess steps must be a non-empty list of {'op': ...} dicts, got %r" % (steps,))
        self.steps = []
        for i, step in enumerate(steps):
            if not isinstance(step, dict) or 'op' not in step:
                raise ValueError("volume_postprocess step %d must be a dict with an 'op', got %r" % (i, step))
            op = step['op']
            if op == 'split':
                raise ValueError("volume_postprocess step %d: 'split' is not a step for volumes: a 3-D split is not built "
                                 "(known: %s)" % (i, ', '.join(sorted(_STEP_KEYS))))
            if not isinstance(op, str) or op not in _STEP_KEYS:
                raise ValueError("volume_postprocess step %d: unknown op %r (known: %s)" % (i, op, ', '.join(sorted(_STEP_KEYS))))
            unknown = sorted(k for k in step if k != 'op' and k not in _STEP_KEYS[op])
            if unknown:
                raise ValueError("volume_postprocess step %d (%s): unknown key(s) %s (allowed: %s)"
                                 % (i, op, ', '.join(map(repr, unknown)), ', '.join(sorted(_STEP_KEYS[op]))))
            full = dict(_STEP_KEYS[op], **step)
            if op in MORPH_OPS:
                st, r = full['structure'], full['iterations']
                if not isinstance(st, str) or (st not in STRUCTURES3D and st not in PLANE_STRUCTURES):
                    raise ValueError("volume_postprocess step %d (%s): structure must be one of %s, got %r"
                                     % (i, op, sorted(STRUCTURES3D) + sorted(PLANE_STRUCTURES), st))
                cap = MORPH3D_MAX_ITER if st in STRUCTURES3D else maskops.MORPH_MAX_ITER
                if isinstance(r, bool) or not isinstance(r, int) or not 1 <= r <= cap:
                    raise ValueError("volume_postprocess step %d (%s): iterations must be an integer 1 .. %d for structure "
                                     "%r, got %r" % (i, op, cap, st, r))
            elif op == 'fill_holes':
                a = full['max_voxels']
                if a is not None and (isinstance(a, bool) or not isinstance(a, int) or a < 1):
                    raise ValueError("volume_postprocess step %d (fill_holes): max_voxels must be a positive integer or "
                                     "null, got %r" % (i, a))
                if not isinstance(full['planar'], bool):
                    raise ValueError("volume_postprocess step %d (fill_holes): planar must be true or false, got %r"
                                     % (i, full['planar']))
            else:
                if not isinstance(full['faces'], str) or full['faces'] not in FACES:
                    raise ValueError("volume_postprocess step %d (clear_border): faces must be one of %s, got %r"
                                     % (i, sorted(FACES), full['faces']))
            self.steps.append(full)
        self._cache = {}

    def record(self):
        """the steps with every default written out: a JSON-able list"""
        return [dict(s) for s in self.steps]

    def _buffers(self, mask):
        key = (tuple(mask.shape), str(mask.device))
        if key not in self._cache:
            lib = _lib.load()
            N, D, H, W = _dims(mask)
            need = 0
            for s in self.steps:
                if s['op'] == 'fill_holes':
                    nbytes = lib.sq_mask_fill_holes_workspace(N * D, H, W) if s['planar'] \
                        else lib.sq_volume_fill_holes_workspace(N, D, H, W)
                elif s['op'] == 'clear_border':
                    nbytes = lib.sq_volume_clear_border_workspace(N, D, H, W)
                else:
                    continue
                if nbytes < 0:
                    raise ValueError("mask %s is too large for one call" % (tuple(mask.shape),))
                need = max(need, nbytes)
            ws = torch.empty(need // 4, dtype=torch.int32, device=mask.device) if need else None
            self._cache[key] = (torch.empty_like(mask), torch.empty_like(mask), ws)
        return self._cache[key]

    def apply(self, mask, classes):
        """Run the steps on `mask` ((N,D,H,W) uint8 on the GPU, `classes` classes) on the current stream.  The input is
        not written; the result is one of two buffers this object caches per shape (nothing is allocated after the first
        call for a shape), valid until the next apply()."""
        classes = int(classes)
        if classes < 2:
            raise ValueError("classes must be at least 2, got %d" % classes)
        _check_mask(mask, classes)
        a, b, ws = self._buffers(mask)
        src = mask
        for s in self.steps:
            dst = a if src is not a else b
            if s['op'] in MORPH_OPS:
                morph3d(src, s['op'], s['iterations'], s['structure'], classes, out=dst)
            elif s['op'] == 'fill_holes':
                fill_cavities(src, s['max_voxels'], s['planar'], classes, out=dst, workspace=ws)
            else:
                clear_border3d(src, s['faces'], classes, out=dst, workspace=ws)
            src = dst
        return src
