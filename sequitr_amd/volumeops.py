"""Clean up segmented volumes where they lie, in HBM: the 3-D counterpart of maskops for the (N, D, H, W) uint8 masks of
UNet3D -- binary morphology per class with the 6- and 26-neighbour structures, filling of enclosed cavities, removal of
objects cut by the volume's faces.  The reference has no counterpart; its users ran scipy.ndimage on a downloaded mask.npy.

``morph3d``, ``fill_cavities``, ``clear_border3d`` and ``split3d`` are one C-ABI call each (sq_volume_morph_u8,
sq_volume_fill_holes_u8, sq_volume_clear_border_u8, sq_volume_split_u8; include/sequitr_hip.h, "Volume clean-up" and "Volume
clean-up: splitting", is the contract: classes, merge rules, scipy's definitions), or -- for the slice-by-slice variants, ``structure='plane_cross' | 'plane_square'`` and ``planar=True`` -- the
planar call of maskops on the zero-copy (N*D, H, W) view of the mask.  ``VolumeCleanup`` is a validated list of such steps
that runs between two cached buffers; the volume jobs take one as ``params['volume_postprocess']`` and
``frontend.segment_volumes`` as ``postprocess``.  There is no CPU path.  Every call, the planar ones included, is a chain
of kernel launches and can be captured in a graph and replayed.  Every result equals the scipy restatement in
tests/volume_cleanup_cases.py and tests/volume_split_cases.py exactly (tests/test_gpu_volume_cleanup.py,
tests/test_gpu_volume_split.py).

``split3d`` separates touching cells: seeds are the 6-connected components of the eroded class planes (3-D erosions, or the
planar ones slice by slice for z-stacks with few, thick slices), they grow back through their class for a bounded number of
synchronous 6-neighbour steps, and a one-voxel sheet of background is cut where two different seeds' growths meet.  The step
of a VolumeCleanup list is called ``split3d``; ``split`` is the planar step's name and stays refused in a volume list.

Not built, each on purpose: growth until nothing changes, EDT or h-maxima seeds and spacing-aware growth for ``split3d``
(voxels beyond ``reach`` keep their class and may still bridge two parts); the 18-neighbour structure
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
SPLIT3D_TILE = (8, 16, 32)                                      # SQ_SPLIT3D_TILE_D, _H, _W: a block's brick
SPLIT3D_STEPS = 2                                               # SQ_SPLIT3D_STEPS: synchronous steps per launch = halo
SPLIT3D_LDS_DEFAULT = 1                                         # SQ_SPLIT3D_LDS_DEFAULT: the form when SQ_SPLIT3D_LDS is unset
SPLIT3D_MAX_REACH = 64                                          # SQ_SPLIT3D_MAX_REACH
SPLIT3D_MAX_EROSIONS = 16                                       # SQ_SPLIT3D_MAX_EROSIONS
SPLIT3D_STRUCTURES = {'cross': 0, 'cube': 1, 'plane_cross': 2, 'plane_square': 3}   # SQ_MORPH3D_*, SQ_SPLIT3D_PLANE_*

# op -> the keys a step may carry besides 'op', with their defaults
_STEP_KEYS = dict({op: {'iterations': 1, 'structure': 'cross'} for op in MORPH_OPS},
                  fill_holes={'max_voxels': None, 'planar': False}, clear_border={'faces': 'all'},
                  split3d={'erosions': None, 'structure': 'cross', 'reach': None})


def _slices(t):
    """the zero-copy (N*D, H, W) view of a contiguous (N, D, H, W) tensor"""
    return t.view(t.shape[0] * t.shape[1], t.shape[2], t.shape[3])


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
    classes = maskops._check_mask(mask, classes, 4)
    out = maskops._check_out(out, mask)
    if structure in PLANE_STRUCTURES:
        maskops.morph(_slices(mask), op, iterations, PLANE_STRUCTURES[structure], classes, out=_slices(out))
        return out
    lib = _lib.load()
    _lib.check(lib.sq_volume_morph_u8(mask.data_ptr(), out.data_ptr(), *(maskops._dims(mask) + (
        classes, MORPH_OPS[op], STRUCTURES3D[structure], iterations, maskops._stream(mask)))), "sq_volume_morph_u8")
    return out


def fill_cavities(mask, max_voxels=None, planar=False, classes=None, out=None, workspace=None):
    """scipy.ndimage.binary_fill_holes per class on 3-D arrays: background enclosed by class c (6-connected, not reaching
    any of the volume's six faces) becomes c, the lowest class first.  max_voxels: fill only cavities of at most that
    many voxels, counting everything inside the cavity (None or <= 0: all).  planar=True fills the holes of every
    (H, W) slice instead -- maskops.fill_holes on the (N*D, H, W) view -- and max_voxels is then the slice hole's area."""
    classes = maskops._check_mask(mask, classes, 4)
    out = maskops._check_out(out, mask)
    if planar:
        maskops.fill_holes(_slices(mask), max_voxels, classes, out=_slices(out), workspace=workspace)
        return out
    lib = _lib.load()
    ws = maskops._workspace(lib.sq_volume_fill_holes_workspace, mask, workspace)
    _lib.check(lib.sq_volume_fill_holes_u8(mask.data_ptr(), out.data_ptr(), *(maskops._dims(mask) + (
        classes, 0 if max_voxels is None else int(max_voxels), ws.data_ptr(), maskops._stream(mask)))),
        "sq_volume_fill_holes_u8")
    return out


def clear_border3d(mask, faces='all', classes=None, out=None, workspace=None):
    """Remove every object (6-connected, one class) that has a voxel on a face of the volume: on any of the six with
    faces='all', on the four faces h = 0, H-1 and w = 0, W-1 only with faces='lateral' (objects cut by the first or last
    slice of a z-stack stay)."""
    if faces not in FACES:
        raise ValueError("faces must be one of %s, got %r" % (sorted(FACES), faces))
    classes = maskops._check_mask(mask, classes, 4)
    out = maskops._check_out(out, mask)
    lib = _lib.load()
    ws = maskops._workspace(lib.sq_volume_clear_border_workspace, mask, workspace)
    _lib.check(lib.sq_volume_clear_border_u8(mask.data_ptr(), out.data_ptr(), *(maskops._dims(mask) + (
        classes, FACES[faces], ws.data_ptr(), maskops._stream(mask)))), "sq_volume_clear_border_u8")
    return out


def default_reach3d(erosions, structure):
    """the reach that None stands for: a cube erosion removes a Chebyshev ball, which the 6-neighbour growth needs up to
    3 r steps to refill; the other structures' balls refill in 2 r"""
    return (3 if structure == 'cube' else 2) * erosions


def split3d(mask, erosions, structure='cross', reach=None, classes=None, out=None, workspace=None):
    """Cut a one-voxel sheet of background between the parts of an object (include/sequitr_hip.h, "Volume clean-up:
    splitting").  Seeds are the 6-connected components of every class plane eroded `erosions` = 1 .. SPLIT3D_MAX_EROSIONS
    times with `structure` ('cross', 'cube', or 'plane_cross' / 'plane_square': the planar erosion slice by slice); they
    grow back through their class for `reach` = 1 .. SPLIT3D_MAX_REACH synchronous 6-neighbour steps (None: 3 * erosions
    for 'cube', 2 * erosions otherwise), the smallest label winning where several arrive together, and a labelled voxel
    with a same-class neighbour of a smaller label becomes background.  Everything else is unchanged; bytes >= classes
    pass through."""
    return maskops._split(mask, erosions, structure, reach, classes, out, workspace, 4, SPLIT3D_STRUCTURES,
                          SPLIT3D_MAX_EROSIONS, SPLIT3D_MAX_REACH, default_reach3d, "sq_volume_split_workspace",
                          "sq_volume_split_u8")


class VolumeCleanup(maskops._Cleanup):
    """A validated list of clean-up steps for volumes, e.g. [{"op": "open", "iterations": 1, "structure": "cross"},
    {"op": "fill_holes", "max_voxels": 500}, {"op": "split3d", "erosions": 4}, {"op": "clear_border", "faces": "lateral"}].  Unknown ops, unknown keys and
    bad values raise a ValueError that names them, at construction.  ``apply`` runs the steps in order on a batch of
    (N,D,H,W) device masks."""
    LABEL, RANK, STEP_KEYS = 'volume_postprocess', 4, _STEP_KEYS
    NOT_BUILT = {'split': "'split' is not a step for volumes: a 3-D split is not built under that name, "
                          "the volume step is called 'split3d'"}

    def _check_step(self, where, op, full):
        if op in MORPH_OPS:
            st, r = full['structure'], full['iterations']
            if not isinstance(st, str) or (st not in STRUCTURES3D and st not in PLANE_STRUCTURES):
                raise ValueError("%s: structure must be one of %s, got %r"
                                 % (where, sorted(STRUCTURES3D) + sorted(PLANE_STRUCTURES), st))
            cap = MORPH3D_MAX_ITER if st in STRUCTURES3D else maskops.MORPH_MAX_ITER
            if not maskops._is_int(r, 1, cap):
                raise ValueError("%s: iterations must be an integer 1 .. %d for structure %r, got %r" % (where, cap, st, r))
        elif op == 'fill_holes':
            if full['max_voxels'] is not None and not maskops._is_int(full['max_voxels'], 1):
                raise ValueError("%s: max_voxels must be a positive integer or null, got %r" % (where, full['max_voxels']))
            if not isinstance(full['planar'], bool):
                raise ValueError("%s: planar must be true or false, got %r" % (where, full['planar']))
        elif op == 'split3d':
            maskops._check_split_step(where, full, SPLIT3D_STRUCTURES, SPLIT3D_MAX_EROSIONS, SPLIT3D_MAX_REACH)
        elif not isinstance(full['faces'], str) or full['faces'] not in FACES:
            raise ValueError("%s: faces must be one of %s, got %r" % (where, sorted(FACES), full['faces']))

    def _step_workspace(self, lib, s, dims):
        if s['op'] == 'fill_holes':
            return lib.sq_mask_fill_holes_workspace(dims[0] * dims[1], *dims[2:]) if s['planar'] \
                else lib.sq_volume_fill_holes_workspace(*dims)
        if s['op'] == 'split3d':
            return lib.sq_volume_split_workspace(*dims)
        return lib.sq_volume_clear_border_workspace(*dims) if s['op'] == 'clear_border' else 0

    def _run(self, s, src, classes, dst, ws):
        if s['op'] in MORPH_OPS:
            morph3d(src, s['op'], s['iterations'], s['structure'], classes, out=dst)
        elif s['op'] == 'fill_holes':
            fill_cavities(src, s['max_voxels'], s['planar'], classes, out=dst, workspace=ws)
        elif s['op'] == 'split3d':
            split3d(src, s['erosions'], s['structure'], s['reach'], classes, out=dst, workspace=ws)
        else:
            clear_border3d(src, s['faces'], classes, out=dst, workspace=ws)
