"""The `jobs` plugin module: job functions with the signature ``func(params, options)`` that
``JobWrapper.__call__`` imports and calls (sequitr/worker.py:56-57, 208-215).  The
reference names this module in its example job file but does not ship it; these
functions are the drop-in bodies that route the per-tile hot path to the MI355X.

Job-file example::

    [job]
    ID = 467e3c03
    user = Alan
    priority = 99
    device = GPU
    module = sequitr_amd.jobs
    func = SERVER_segment
    params = {'input': '/data/tiles.npy', 'shape': (512, 512), 'num_outputs': 2}
    options = {'gpu': 0, 'save_logits': True}

There is no CPU back end: ``device = CPU`` jobs fail loudly (the exception is logged by the
worker's exception_logger, as every job error is).
"""
import json
import logging
import os
import time

import numpy as np

logger = logging.getLogger('worker_process')

NET_KEYS = ('name', 'filters', 'dropout', 'num_inputs', 'num_outputs', 'shape', 'bridge', 'kernel', 'seed', 'dtype',
            'batch_norm', 'up_kernel')


def _resolve_device(params, options):
    """job.device / options['gpu'] / LOCAL_RANK -> torch device string."""
    dev = str(params.get('device', 'GPU'))
    if dev.upper() == 'CPU':
        raise RuntimeError("sequitr_amd has no CPU back end: submit the job with device = GPU")
    if dev.lower().startswith('cuda'):
        return dev
    idx = options.get('gpu', os.environ.get('LOCAL_RANK', 0))
    return 'cuda:%d' % int(idx)


def _load_tiles(params):
    src = params.get('input')
    if isinstance(src, np.ndarray):
        x = src
    elif isinstance(src, str) and src.endswith('.npy'):
        x = np.load(src, mmap_mode='r', allow_pickle=False)
    elif isinstance(src, dict) and src.get('synthetic'):
        s = src
        x = np.random.default_rng(s.get('seed', 0)).standard_normal(
            (s.get('tiles', 1),) + tuple(params.get('shape', (512, 512))) + (params.get('num_inputs', 1),)
        ).astype(np.float32)
    else:
        raise ValueError("params['input'] must be a .npy path, an ndarray or {'synthetic': True, ...}")
    if x.ndim == 2:
        x = x[np.newaxis, ..., np.newaxis]
    elif x.ndim == 3:
        x = x[..., np.newaxis]
    return x


def _net_params(params, device):
    p = {k: params[k] for k in NET_KEYS if k in params}
    p['device'] = device
    return p


def SERVER_segment(params, options):
    """Segment a stack of tiles: writes ``mask.npy`` (uint8 class labels, N x H x W) and,
    with options['save_logits'], ``logits.npy`` into params['output'], plus ``segment.json``
    with timing.  params: input, shape, num_inputs, num_outputs, filters, bridge, model
    (numbered model dir or name to warm-start from; else seeded initial weights), pipeline
    (ImagePipeline JSON applied to every tile on the host), batch (tiles per launch batch).
    options: gpu, save_logits, centroids, io_threads (host staging threads, default 4).

    ``segment.json``: ``seconds`` / ``mpixels_per_s`` cover the stream over the whole stack (host tiles in, host
    masks out, PCIe both ways included); ``setup_seconds`` is what comes before it once per job (weights, pinned
    staging buffers, one warm-up batch) and ``mpixels_per_s_with_setup`` the rate with it counted.
    """
    _refuse_volume_postprocess(params, 'SERVER_segment')
    _refuse_volume_tta(params, options, 'SERVER_segment')
    _refuse_tta(params, options, 'SERVER_segment (the tile job)')
    _refuse_blend(params, 'SERVER_segment (the tile job)')
    import torch
    from .networks.unet import UNet2D
    from .pipeline import ImagePipeline
    from .frontend import TileStreamer

    device = _resolve_device(params, options)
    torch.cuda.set_device(torch.device(device))
    out_dir = params['output']
    x = _load_tiles(params)
    N = x.shape[0]
    net_p = _net_params(params, device)
    net_p.setdefault('shape', tuple(x.shape[1:3]))
    net = UNet2D(net_p, 'infer')
    _load_net_weights(net, params)

    pipe = ImagePipeline.load(params['pipeline']) if params.get('pipeline') else None
    batch = int(params.get('batch', 32))
    want_logits = bool(options.get('save_logits'))
    writer, frames_out = None, {}
    on_batch = None
    if options.get('centroids'):                               # the reference's next step: utils.CentroidWriter
        from .centroids import CentroidWriter, mask_centroids
        writer = CentroidWriter(os.path.join(out_dir, 'tracks.hdf5'))

        def on_batch(first, m):                                # centroids straight from the mask in HBM
            for k, coords in enumerate(mask_centroids(m)):
                coords[:, 0] = first + k                       # frame index within the whole stack
                frames_out[first + k] = coords

    # the streamed data path (frontend.TileStreamer): staging, H2D, the network and D2H of consecutive batches
    # overlap on three streams; set-up (pinned buffers, first-launch costs) is timed apart from the stream itself
    t_setup = time.time()
    streamer = TileStreamer(net, batch=batch, want_logits=want_logits, workers=int(options.get('io_threads', 4)))
    streamer.warm_up(tuple(x.shape[1:]))
    # zeros, not empty: the pages are touched here, in the set-up time -- first-touch faults of a 268 MB array inside the
    # stream are ~15 ms of a 180 ms pass (the download threads write it while the GPU works)
    masks = np.zeros(x.shape[:3], np.uint8)
    logits = np.zeros(x.shape[:3] + (net.n_outputs,), np.float32) if want_logits else None
    t0 = time.time()
    streamer.run(x, out_masks=masks, out_logits=logits, pipe=(lambda t: pipe(t)) if pipe is not None else None,
                 on_batch=on_batch)
    dt = time.time() - t0
    n_objects = 0
    if writer is not None:
        for k in sorted(frames_out):
            writer.add_frame(k, frames_out[k])
            n_objects += len(frames_out[k])
        writer.close()
    np.save(os.path.join(out_dir, 'mask.npy'), masks)
    if logits is not None:
        np.save(os.path.join(out_dir, 'logits.npy'), logits)
    pixels = N * x.shape[1] * x.shape[2]
    info = {'tiles': int(N), 'shape': [int(s) for s in x.shape[1:3]], 'seconds': dt, 'setup_seconds': t0 - t_setup,
            'mpixels_per_s': float(pixels / max(dt, 1e-9) / 1e6),
            'mpixels_per_s_with_setup': float(pixels / max(dt + t0 - t_setup, 1e-9) / 1e6),
            'batch': batch, 'streamed': True, 'device': device}
    if writer is not None:
        info['centroids'] = {'file': os.path.basename(writer.filename), 'objects': int(n_objects)}
    with open(os.path.join(out_dir, 'segment.json'), 'w') as f:
        json.dump(info, f, indent=2)
    logger.info('Segmented {tiles} tiles in {seconds:.3f}s on {device}'.format(**info))
    return info


def _load_volumes(params):
    """(N, Z, X, Y, C) float32 volumes from a .npy path, an ndarray or {'synthetic': True, 'volumes': n, 'seed': s}
    (params['shape'] = (X, Y, Z) as UNet3D takes it); (Z, X, Y) and (N, Z, X, Y) inputs gain the missing axes."""
    src = params.get('input')
    if isinstance(src, np.ndarray):
        x = src
    elif isinstance(src, str) and src.endswith('.npy'):
        x = np.load(src, mmap_mode='r', allow_pickle=False)
    elif isinstance(src, dict) and src.get('synthetic'):
        if len(tuple(params.get('shape', ()))) != 3:
            raise ValueError("synthetic volumes need params['shape'] = (X, Y, Z), got %r" % (params.get('shape'),))
        X, Y, Z = tuple(params['shape'])
        x = np.random.default_rng(src.get('seed', 0)).standard_normal(
            (src.get('volumes', 1), Z, X, Y, params.get('num_inputs', 1))).astype(np.float32)
    else:
        raise ValueError("params['input'] must be a .npy path, an ndarray or {'synthetic': True, ...}")
    if x.ndim == 3:
        x = x[np.newaxis, ..., np.newaxis]
    elif x.ndim == 4:
        x = x[..., np.newaxis]
    if x.ndim != 5:
        raise ValueError('volumes must be (N, Z, X, Y[, C]), got shape %s' % (x.shape,))
    return x


def _load_net_weights(net, params):
    """params['model'] (a numbered model dir, or a name under MODELDIR) into `net`; seeded initial weights without it"""
    from . import utils
    model = params.get('model')
    if not model:
        net.initialize()
        return
    model_dir = model if os.path.isdir(model) else utils.get_latest_model_dir(
        os.path.join(utils.core.TensorflowConfiguration.MODELDIR, model))
    if model_dir is None:
        raise IOError('No saved model found for {0}'.format(model))
    net.load_state_dict(utils.load_model_weights(model_dir))
    logger.info('Loaded weights from {0:s}'.format(model_dir))


def _brick_volumes(params, options):
    """What the brick jobs check before any voxel is read or any GPU work starts: (device, volumes (N, Z, X, Y) raw,
    brick (bz, bx, by), margin in (Z, X, Y) order, geometry)"""
    from .frontend import NP_TORCH, volume_bricks

    device = _resolve_device(params, options)
    x = _load_volumes(params)
    if x.shape[4] != 1 or int(params.get('num_inputs', 1)) != 1:
        raise ValueError("params['brick'] segments single-channel volumes only, got %d channels" % x.shape[4])
    x = x[..., 0]                                              # (N, Z, X, Y), still the raw array or memmap: no host cast
    if np.dtype(x.dtype) not in NP_TORCH:
        raise TypeError("with params['brick'] the volumes must be uint8, uint16 or float32, got %s" % x.dtype)
    N, Z, X, Y = (int(s) for s in x.shape)
    if len(tuple(params['brick'])) != 3:
        raise ValueError("params['brick'] must be (X, Y, Z), got %r" % (params['brick'],))
    bx, by, bz = (int(s) for s in params['brick'])
    margin = params.get('margin', 0)
    if not np.isscalar(margin):
        if len(tuple(margin)) != 3:
            raise ValueError("params['margin'] must be an int or (X, Y, Z), got %r" % (margin,))
        margin = (int(margin[2]), int(margin[0]), int(margin[1]))
    geometry = volume_bricks((Z, X, Y), (bz, bx, by), margin)  # raises on a margin too large for the brick
    return device, x, (bz, bx, by), margin, geometry


VOLUME_ANALYSIS_OPTIONS = ('measure', 'save_labels', 'neighbors', 'save_zones', 'shape')


def _parse_volume_analysis(params, options):
    """options['measure'] / ['save_labels'] / ['neighbors'] / ['save_zones'] / ['shape'] of SERVER_segment_volume, before any input is
    opened: None without them, else a dict of what they ask for with the neighbour parameters checked and their defaults
    filled in.  They need params['brick']; a bad value raises here."""
    asked = [k for k in VOLUME_ANALYSIS_OPTIONS if options.get(k)]
    if not asked:
        return None
    if params.get('brick') is None:
        raise ValueError("options %s measure the volumes while they are in HBM, which the brick front end keeps them in: "
                         "they need params['brick']" % ', '.join(repr(k) for k in asked))
    want_neighbors = bool(options.get('neighbors'))
    a = {'neighbors': want_neighbors, 'save_labels': bool(options.get('save_labels')),
         'save_zones': want_neighbors and bool(options.get('save_zones')),
         'min_area': int(params.get('min_area') or 1), 'max_area': params.get('max_area')}
    if a['min_area'] < 1 or (a['max_area'] is not None and int(a['max_area']) < a['min_area']):
        raise ValueError("params['min_area'] / params['max_area'] must satisfy 1 <= min_area <= max_area, got %r / %r"
                         % (params.get('min_area'), params.get('max_area')))
    if want_neighbors:
        from .analysis.neighbors import check_params, check_spacing
        a['d_thresh'], a['zone_reach'], a['neighbor_seeds'] = check_params(
            params.get('d_thresh', 100.0), params.get('zone_reach'), params.get('neighbor_seeds', 'objects'))
        a['spacing'] = check_spacing(params.get('spacing', 1.0))
    a['shape'] = bool(options.get('shape'))
    if a['shape']:                                              # the metric shape columns read the same depth spacing
        from .analysis.neighbors import check_spacing
        a['spacing'] = check_spacing(params.get('spacing', 1.0))
    return a


def _segment_volume_bricks(params, options, cleanup=None, analysis=None, volume_tta=(None, None)):
    """SERVER_segment_volume with params['brick']: volumes of any size, raw, brick by brick (frontend.segment_volumes)."""
    device, x, (bz, bx, by), margin, geometry = _brick_volumes(params, options)
    out_dir = params['output']
    N, Z, X, Y = (int(s) for s in x.shape)
    tta, probabilities = volume_tta

    import torch
    from .networks.unet import UNet3D
    from .frontend import segment_volumes
    torch.cuda.set_device(torch.device(device))
    net_p = _net_params(params, device)
    net_p['shape'] = (bx, by, bz)
    net_p['num_inputs'] = 1
    t_setup = time.time()
    net = UNet3D(net_p, 'infer')
    _load_net_weights(net, params)
    want_logits = bool(options.get('save_logits'))
    want_centroids = bool(options.get('centroids'))
    batch = int(params.get('bricks_per_batch', 8))
    net.predict(torch.zeros((min(batch, geometry.per_volume), bz, bx, by, 1), device=device))   # first-launch costs
    torch.cuda.synchronize()
    per_volume = {}
    masks = np.zeros((N, Z, X, Y), np.uint8) if want_centroids or analysis else None

    def sink(i, m):                                            # centroids straight from the mask in HBM: no second upload
        from .centroids import mask_centroids
        masks[i] = m[0].cpu().numpy()
        coords = mask_centroids(m.transpose(1, 3).contiguous())[0]    # the axes as CentroidWriter.write swaps them
        coords[:, 0] = i
        per_volume[i] = coords

    tables, neighbor_tables = {}, {}
    num_classes = int(net_p.get('num_outputs', 2))
    if analysis:
        bounded = analysis['min_area'] != 1 or analysis['max_area'] is not None
        label_stack = np.empty((N, Z, X, Y), np.int32) if analysis['save_labels'] else None
        zone_stack = np.empty((N, Z, X, Y), np.int32) if analysis['save_zones'] else None

    def measure_sink(i, raw, m):                               # objects against the raw volume, both in HBM as they lie
        from .objects import measure_objects
        t = measure_objects(m, image=raw, min_area=analysis['min_area'], max_area=analysis['max_area'],
                            labels=label_stack is not None or analysis['neighbors'], filtered_mask=bounded, shape=analysis['shape'])
        if label_stack is not None:
            label_stack[i] = t.labels[0].cpu().numpy()
        if analysis['neighbors']:                               # on the kept objects' labels, while the volume is in HBM
            from .analysis.neighbors import neighbors_from_objects
            nt = neighbors_from_objects(t, num_classes, analysis['d_thresh'], analysis['zone_reach'],
                                        analysis['neighbor_seeds'], return_zones=zone_stack is not None,
                                        spacing=analysis['spacing'])
            if zone_stack is not None:
                zone_stack[i] = nt.zones[0].cpu().numpy()
                nt.zones = None
            neighbor_tables[i] = nt
        kept = t.mask if bounded else m                         # what mask.npy and the centroid path see
        t.labels = t.mask = None
        tables[i] = t
        if want_centroids:
            sink(i, kept)
        else:
            masks[i] = kept[0].cpu().numpy()

    with_sink = bool(want_centroids or analysis)
    prob_stack = np.empty((N, num_classes, Z, X, Y), probabilities) if probabilities and with_sink else None

    def prob_sink(i, p):                                       # with a mask sink the probabilities are visited too
        prob_stack[i] = p[0].cpu().numpy()

    t0 = time.time()
    res = segment_volumes(net, x, (bz, bx, by), margin, bricks_per_batch=batch,
                          normalise=bool(params.get('normalise', True)), want_logits=want_logits,
                          on_masks=sink if want_centroids and not analysis else None,
                          **({'postprocess': cleanup} if cleanup else {}),
                          **({'on_volume': measure_sink} if analysis else {}),
                          **({'tta': tta} if tta is not None else {}),
                          **({'probabilities': probabilities,
                              'on_probs': prob_sink if with_sink else None} if probabilities is not None else {}))
    out, logits = res[0], res[1]
    if probabilities is not None and not with_sink:
        prob_stack = res[2]
    if not with_sink:
        masks = out
    dt = time.time() - t0
    np.save(os.path.join(out_dir, 'mask.npy'), masks)
    if logits is not None:
        np.save(os.path.join(out_dir, 'logits.npy'), logits)
    if probabilities is not None:
        np.save(os.path.join(out_dir, 'probability.npy'), prob_stack)
    voxels = N * Z * X * Y
    info = {'volumes': int(N), 'shape': [Z, X, Y], 'seconds': dt, 'setup_seconds': t0 - t_setup,
            'mvoxels_per_s': float(voxels / max(dt, 1e-9) / 1e6), 'device': device,
            'brick': [bx, by, bz], 'margin': [geometry.margin[1], geometry.margin[2], geometry.margin[0]],
            'bricks_per_volume': int(geometry.per_volume)}
    if cleanup is not None:
        info['volume_postprocess'] = cleanup.record()
    if 'volume_tta' in params:
        info['volume_tta'] = tta
    if 'save_volume_probabilities' in options:
        info['probabilities'] = probabilities
    if want_centroids:
        from .centroids import CentroidWriter
        with CentroidWriter(os.path.join(out_dir, 'tracks.hdf5')) as cw:
            for i in sorted(per_volume):
                cw.add_frame(i, per_volume[i])
        info['centroids'] = {'file': os.path.basename(cw.filename), 'objects': int(sum(len(v) for v in per_volume.values()))}
    if analysis:
        from .objects import ObjectTable
        table = ObjectTable.concatenate([tables[i] for i in range(N)], list(range(N)), N)
        np.savez(os.path.join(out_dir, 'objects.npz'), **table.columns(spacing=analysis.get('spacing', 1.0)))
        if label_stack is not None:
            np.save(os.path.join(out_dir, 'labels.npy'), label_stack)
        info['objects'] = {'count': len(table), 'found': int(table.found), 'min_area': analysis['min_area'],
                           'max_area': None if analysis['max_area'] is None else int(analysis['max_area']),
                           'with_intensity': True}
        if analysis['shape']:                                   # the record's own 'shape' key is the volumes' shape
            info['objects']['shape'] = True
            info['objects']['spacing'] = analysis['spacing']
        if analysis['neighbors']:
            from .analysis.neighbors import NeighborTable
            ntable = NeighborTable.concatenate([neighbor_tables[i] for i in range(N)], list(range(N)), N)
            np.savez(os.path.join(out_dir, 'neighbors.npz'), **ntable.columns())
            if zone_stack is not None:
                np.save(os.path.join(out_dir, 'zones.npy'), zone_stack)
            info['neighbors'] = {'objects': len(ntable), 'pairs': int(ntable.n_pairs),
                                 'pairs_removed': int(ntable.n_pairs_removed), 'num_classes': num_classes,
                                 'd_thresh': analysis['d_thresh'], 'zone_reach': analysis['zone_reach'],
                                 'neighbor_seeds': analysis['neighbor_seeds'], 'spacing': analysis['spacing']}
    with open(os.path.join(out_dir, 'segment_volume.json'), 'w') as f:
        json.dump(info, f, indent=2)
    logger.info('Segmented {volumes} volumes in {seconds:.3f}s on {device}, {bricks_per_volume} bricks each'.format(**info))
    return info


def SERVER_segment_volume(params, options):
    """Segment volumes (z-stacks) with UNet3D, one volume per launch: writes ``mask.npy`` (uint8, N x Z x X x Y),
    with options['save_logits'] ``logits.npy``, with options['centroids'] the centroid file (``tracks.hdf5``, or
    ``.npz`` without h5py) as CentroidWriter.write makes it from the (N,Z,X,Y) mask, and ``segment_volume.json``.
    params: as SERVER_segment (input, num_inputs, num_outputs, filters, bridge, batch_norm, model for a warm start);
    shape defaults to (X, Y, Z) of the input (synthetic input needs it).  options: gpu, save_logits, centroids.

    With params['brick'] = (X, Y, Z), the network's `shape` convention, volumes of any size are segmented brick by brick
    (frontend.segment_volumes): the network is built at the brick shape, the input is raw uint8 / uint16 / float32 single-
    channel volumes that cross PCIe as they are, and ImageNorm per volume (params['normalise'], default True), brick
    cutting and the scatter of masks and logits run on the GPU.  params['margin'] (an int, or (X, Y, Z); default 0) is
    the context every owned voxel keeps to its brick's faces, params['bricks_per_batch'] (default 8) the bricks per
    network launch.  The centroids come from the masks while they are in HBM.  ``segment_volume.json`` gains ``brick``,
    ``margin`` (both (X, Y, Z)) and ``bricks_per_volume``.

    params['volume_postprocess'] (a list of volume clean-up steps, or the path of a JSON file holding one;
    volumeops.VolumeCleanup, with D, H, W = Z, X, Y) cleans every volume's mask in HBM, with and without ``brick``:
    ``mask.npy`` and the centroid file describe the cleaned masks and ``segment_volume.json`` records the steps, defaults
    written out, under ``volume_postprocess``.  A bad step list raises before any input is opened; without the key
    nothing changes.  The steps: 3-D morphology, fill_holes, split3d (touching cells cut apart; ``split`` is the planar
    step's name and is refused here), clear_border.  params['postprocess'], the planar list, stays refused.

    With ``brick``, params['volume_tta'] (null, "flips" or "dihedral") is test-time augmentation (frontend.segment_volumes:
    the network sees every batch of bricks under the 8 mirror states, or under all 16 symmetries the volume sampler trains
    with -- "dihedral" needs a brick with X == Y -- and the float32 logits are merged in HBM); ``mask.npy`` is the argmax of
    the merged logits, ``logits.npy`` (options['save_logits']) their mean, and the clean-up and the analysis see the merged
    mask.  options['save_volume_probabilities'] (true = 'uint8', or 'uint8' / 'float32') writes ``probability.npy``
    (N,K,Z,X,Y) next to ``mask.npy``: the softmax of the (mean) logits per voxel, uint8 as rounded p * 255; the clean-up
    does not touch it.  ``segment_volume.json`` records ``volume_tta`` and ``probabilities`` when the keys are present.
    Both keys are refused before anything is opened without ``brick``, on "dihedral" with a non-square brick and on bad
    values; the planar params['tta'] / options['save_probabilities'] stay refused here.

    With ``brick``, options['measure'] measures every volume's objects in HBM (objects.measure_objects on the cleaned mask as
    it lies, D0, D1, D2 = Z, X, Y, 6-connected, against the RAW volume): ``objects.npz`` holds ObjectTable.columns() with
    ``frame`` the volume index, ``segment_volume.json`` an ``objects`` record, options['save_labels'] adds ``labels.npy``
    (N,Z,X,Y) int32.  params['min_area'] / params['max_area'] (inclusive, in voxels) drop objects outside the range, and
    ``mask.npy`` and the centroid file then describe the mask without them.  options['neighbors'] (implies measure) finds
    every object's neighbours in 3-D (analysis/neighbors.py, neighbors3d: touching zones of influence in the z-stack):
    ``neighbors.npz`` holds the volumetric NeighborTable.columns(), the json a ``neighbors`` record with the defaults filled
    in, options['save_zones'] adds ``zones.npy`` (N,Z,X,Y) int32.  params['d_thresh'] (100.0, in in-plane pixels),
    params['zone_reach'] (none), params['neighbor_seeds'] ('objects') and params['spacing'] (1.0: the slice spacing in
    in-plane pixels, SERVER_train_volume's key); a bad value raises before any input is opened, and so do these four options
    without ``brick``.  Without them every file is what it was.  options['shape'] (implies measure, refused without
    ``brick`` like its siblings) adds the shape columns and the columns derived from them under params['spacing']
    (covariance, axis_lengths, equivalent_diameter, extent, surface_area, sphericity; ObjectTable's docstrings are the
    formulas) to ``objects.npz``, and the json's ``objects`` record gains ``shape: true`` and ``spacing``.

    ``segment_volume.json``: ``seconds`` / ``mvoxels_per_s`` cover the volumes (upload, network, download);
    ``setup_seconds`` is weights plus one warm-up volume."""
    if params.get('postprocess') is not None:
        raise ValueError("params['postprocess'] cleans planar (N,H,W) masks only: volumes are out of scope "
                         "(params['volume_postprocess'] cleans them)")
    _refuse_tta(params, options, 'SERVER_segment_volume')
    _refuse_blend(params, 'SERVER_segment_volume')
    volume_tta = _parse_volume_tta(params, options, 'SERVER_segment_volume')    # before anything is opened
    cleanup = _parse_volume_postprocess(params)                 # likewise
    analysis = _parse_volume_analysis(params, options)          # likewise
    import torch
    from .networks.unet import UNet3D

    if params.get('brick') is not None:
        return _segment_volume_bricks(params, options, cleanup, analysis, volume_tta)
    device = _resolve_device(params, options)
    torch.cuda.set_device(torch.device(device))
    out_dir = params['output']
    x = _load_volumes(params)
    N, Z, X, Y = x.shape[:4]
    net_p = _net_params(params, device)
    net_p.setdefault('shape', (X, Y, Z))
    net_p.setdefault('num_inputs', x.shape[4])
    t_setup = time.time()
    net = UNet3D(net_p, 'infer')
    _load_net_weights(net, params)
    want_logits = bool(options.get('save_logits'))
    net.predict(np.ascontiguousarray(x[:1]))                    # warm-up: first-launch costs stay in the set-up time
    torch.cuda.synchronize()
    masks = np.zeros((N, Z, X, Y), np.uint8)
    logits = np.zeros((N, Z, X, Y, net.n_outputs), np.float32) if want_logits else None
    t0 = time.time()
    for i in range(N):
        m = net.predict(np.ascontiguousarray(x[i:i + 1]))
        if cleanup is not None:
            m = cleanup.apply(m.contiguous(), net.n_outputs)   # on the device mask, before the download
        masks[i] = m[0].cpu().numpy()
        if logits is not None:
            logits[i] = net.logits()[0].cpu().numpy()
    torch.cuda.synchronize()
    dt = time.time() - t0
    np.save(os.path.join(out_dir, 'mask.npy'), masks)
    if logits is not None:
        np.save(os.path.join(out_dir, 'logits.npy'), logits)
    voxels = N * Z * X * Y
    info = {'volumes': int(N), 'shape': [int(Z), int(X), int(Y)], 'seconds': dt, 'setup_seconds': t0 - t_setup,
            'mvoxels_per_s': float(voxels / max(dt, 1e-9) / 1e6), 'device': device}
    if cleanup is not None:
        info['volume_postprocess'] = cleanup.record()
    if options.get('centroids'):
        from .centroids import CentroidWriter
        with CentroidWriter(os.path.join(out_dir, 'tracks.hdf5')) as cw:
            frames = cw.write(masks, device=device)
        info['centroids'] = {'file': os.path.basename(cw.filename), 'objects': int(sum(len(f) for f in frames))}
    with open(os.path.join(out_dir, 'segment_volume.json'), 'w') as f:
        json.dump(info, f, indent=2)
    logger.info('Segmented {volumes} volumes in {seconds:.3f}s on {device}'.format(**info))
    return info


def _open_frames(params):
    """params['input'] of the frame jobs -> (frames, F, H, W): an Octopus stream, a .npy memmap or an ndarray; no pixel is
    read here"""
    src = params.get('input')
    if isinstance(src, str) and not src.endswith('.npy'):
        from .dataio import OctopusData
        frames = OctopusData(src, timeout=params.get('timeout', 60))
        F, (H, W) = len(frames), frames.framesize
    else:
        frames = np.load(src, mmap_mode='r', allow_pickle=False) if isinstance(src, str) else np.asarray(src)
        F, H, W = frames.shape
    return frames, int(F), int(H), int(W)


def _open_channels(params):
    """params['input'] of the frame jobs with more than one channel -> (frames, F, H, W, C), what segment_frames takes: a
    list of C sources (each an Octopus stem, a .npy or an ndarray of (F,H,W) frames; one length, shape and pixel type) or
    one interleaved (F,H,W,C) .npy / ndarray.  A single (F,H,W) source is _open_frames' and gives C = None.  No pixel is
    read here; ragged channels raise."""
    from .frontend import open_channels
    src = params.get('input')

    def one(s):
        if isinstance(s, str) and not s.endswith('.npy'):
            from .dataio import OctopusData
            return OctopusData(s, timeout=params.get('timeout', 60))
        if isinstance(s, str):
            return np.load(s, mmap_mode='r', allow_pickle=False)
        return s if hasattr(s, 'shape') and hasattr(s, 'dtype') else np.asarray(s)

    if isinstance(src, (list, tuple)):
        frames = [one(s) for s in src]
    else:
        if isinstance(src, str) and not src.endswith('.npy'):   # one Octopus stream
            return _open_frames(params) + (None,)
        frames = one(src)                                       # a header or an attribute: no pixel
        if frames.ndim == 3:
            return _open_frames(params) + (None,)               # the single-channel path, as it was
    _, (F, H, W), _, C = open_channels(frames)
    return frames, int(F), int(H), int(W), int(C)


def _parse_pipelines(params):
    """params['pipeline'] through FrameClean.from_pipeline, before any input is opened: None, one (clean, normalise), or a
    list of them with (None, True) -- ImageNorm alone, the default -- for a null entry.  A pipe the device does not run
    raises here."""
    from .frontend import FrameClean
    pipeline = params.get('pipeline')
    if pipeline is None:
        return None
    if isinstance(pipeline, (list, tuple)):
        return [(None, True) if p is None else FrameClean.from_pipeline(p) for p in pipeline]
    return FrameClean.from_pipeline(pipeline)


def _parse_postprocess(params):
    """params['postprocess'] -- a list of mask clean-up steps, or the path of a JSON file that holds one -- as a
    maskops.MaskCleanup, before any input is opened; None without the key.  A bad step list raises here."""
    spec = params.get('postprocess')
    if spec is None:
        return None
    from .maskops import MaskCleanup, load_steps
    if params.get('brick') is not None:
        raise ValueError("params['postprocess'] cleans planar (N,H,W) masks only: volumes (params['brick']) are out of scope")
    return MaskCleanup(load_steps(spec))


def _parse_volume_postprocess(params):
    """params['volume_postprocess'] -- a list of volume clean-up steps, or the path of a JSON file that holds one -- as a
    volumeops.VolumeCleanup, before any input is opened; None without the key.  A bad step list raises here."""
    spec = params.get('volume_postprocess')
    if spec is None:
        return None
    from .volumeops import VolumeCleanup, load_steps
    return VolumeCleanup(load_steps(spec))


def _refuse_volume_postprocess(params, job):
    """the jobs that produce no (N, Z, X, Y) masks from bricks refuse the key before any input is opened"""
    if params.get('volume_postprocess') is not None:
        raise ValueError("params['volume_postprocess'] cleans the masks of SERVER_segment_volume and of SERVER_evaluate with "
                         "params['brick']: %s does not take it" % job)


TTA_SETS = (None, 'flips', 'dihedral')


def _parse_tta(params, options, job):
    """(tta, probabilities) of a whole-frame job: params['tta'] -- null, "flips" or "dihedral" (frontend.segment_frames'
    view sets) -- and options['save_probabilities'] -- true ('uint8'), 'uint8' or 'float32'; false / null: none.  Volumes
    (params['brick']) take neither; a bad value raises here, before anything is opened."""
    tta = params.get('tta')
    if tta is not None and not (isinstance(tta, str) and tta in TTA_SETS):
        raise ValueError("params['tta'] must be null, \"flips\" or \"dihedral\", got %r" % (tta,))
    save = options.get('save_probabilities')
    if save is None or save is False:
        probabilities = None
    elif save is True:
        probabilities = 'uint8'
    elif isinstance(save, str) and save in ('uint8', 'float32'):
        probabilities = save
    else:
        raise ValueError("options['save_probabilities'] must be true, false, 'uint8' or 'float32', got %r" % (save,))
    if (tta is not None or probabilities is not None) and params.get('brick') is not None:
        raise ValueError("params['tta'] / options['save_probabilities'] cover whole frames only: %s with params['brick'] "
                         "segments volumes, and test-time augmentation for UNet3D is not built" % job)
    return tta, probabilities


def _refuse_tta(params, options, job):
    """jobs that do not segment whole frames take neither params['tta'] nor options['save_probabilities']"""
    if params.get('tta') is not None or options.get('save_probabilities'):
        raise ValueError("params['tta'] / options['save_probabilities'] belong to the whole-frame jobs (SERVER_segment_frames, "
                         "SERVER_evaluate on frames): %s does not take them" % job)


def _parse_blend(params, job):
    """params['blend'] of a whole-frame job: null, or the number of pixels to either side of a seam over which
    frontend.segment_frames blends the overlapping tiles (0: none), checked against the job's tile and margin as
    segment_frames checks it.  Volumes (params['brick']) do not take it; a bad value raises here, before anything is
    opened."""
    blend = params.get('blend')
    if blend is None:
        return None
    if params.get('brick') is not None:
        raise ValueError("params['blend'] covers whole frames only: %s with params['brick'] segments volumes, and seam "
                         "blending between bricks is not built" % job)
    from .frontend import check_blend
    try:
        return check_blend(blend, int(params.get('shape', (512, 512))[0]), int(params.get('margin', 32)))
    except ValueError as e:
        raise ValueError("params['blend']: %s" % e)


def _refuse_blend(params, job):
    """jobs that do not segment whole frames do not take params['blend']"""
    if params.get('blend') is not None:
        raise ValueError("params['blend'] belongs to the whole-frame jobs (SERVER_segment_frames, SERVER_evaluate on "
                         "frames): %s does not take it" % job)


def _parse_volume_tta(params, options, job):
    """(volume_tta, probabilities) of a brick job: params['volume_tta'] -- null, "flips" or "dihedral"
    (frontend.segment_volumes' view sets: the 8 mirror states, or the 16 symmetries the volume sampler trains with, which
    need a brick with X == Y) -- and options['save_volume_probabilities'] -- true ('uint8'), 'uint8' or 'float32'; false /
    null: none.  Both need params['brick']; a bad value raises here, before anything is opened."""
    tta = params.get('volume_tta')
    if tta is not None and not (isinstance(tta, str) and tta in TTA_SETS):
        raise ValueError("params['volume_tta'] must be null, \"flips\" or \"dihedral\", got %r" % (tta,))
    save = options.get('save_volume_probabilities')
    if save is None or save is False:
        probabilities = None
    elif save is True:
        probabilities = 'uint8'
    elif isinstance(save, str) and save in ('uint8', 'float32'):
        probabilities = save
    else:
        raise ValueError("options['save_volume_probabilities'] must be true, false, 'uint8' or 'float32', got %r" % (save,))
    if tta is None and probabilities is None:
        return None, None
    brick = params.get('brick')
    if brick is None:
        raise ValueError("params['volume_tta'] / options['save_volume_probabilities'] merge and scatter brick logits: %s "
                         "takes them with params['brick'] only" % job)
    if tta == 'dihedral':
        if len(tuple(brick)) != 3:
            raise ValueError("params['brick'] must be (X, Y, Z), got %r" % (brick,))
        if int(brick[0]) != int(brick[1]):
            raise ValueError("params['volume_tta'] \"dihedral\" transposes x and y: params['brick'] %r is not square in "
                             "(X, Y)" % (tuple(brick),))
    return tta, probabilities


def _refuse_volume_tta(params, options, job):
    """jobs that do not segment volumes brick by brick take neither params['volume_tta'] nor
    options['save_volume_probabilities']"""
    if params.get('volume_tta') is not None or options.get('save_volume_probabilities'):
        raise ValueError("params['volume_tta'] / options['save_volume_probabilities'] belong to the brick jobs "
                         "(SERVER_segment_volume and SERVER_evaluate with params['brick']): %s does not take them" % job)


def _channel_setup(params, C, parsed=None):
    """What the frame jobs derive from params once the number of channels is known, before a pixel is read:
    (clean, normalise, pipeline record or None, num_inputs or None).  params['pipeline'] (`parsed`: what _parse_pipelines
    made of it, when the job has called it already) is one pipeline for every channel or, with C channels, a list of C with
    null entries; the channels must agree on whether ImageNorm closes the chain.  params['num_inputs'] defaults to C and
    must equal it."""
    from .frontend import FrameClean
    pipeline = params.get('pipeline')
    if pipeline is not None and parsed is None:
        parsed = _parse_pipelines(params)
    if C is None:
        clean, normalise = None, True
        if pipeline is not None:
            if isinstance(parsed, list):
                raise ValueError("params['pipeline'] is a list of %d pipelines, the input has one channel" % len(parsed))
            clean, normalise = parsed
        return clean, normalise, None if pipeline is None else (clean or FrameClean()).pipes(normalise), None
    if params.get('num_inputs') is not None and int(params['num_inputs']) != C:
        raise ValueError("params['num_inputs'] is %d, the input has %d channels" % (int(params['num_inputs']), C))
    if pipeline is None:
        return None, True, None, C
    if isinstance(parsed, list):
        if len(parsed) != C:
            raise ValueError("params['pipeline'] holds %d pipelines for %d channels" % (len(parsed), C))
    else:
        parsed = [parsed] * C
    flags = set(n for _, n in parsed)
    if len(flags) != 1:
        raise ValueError("params['pipeline']: the channels must agree on ImageNorm (a null entry is ImageNorm alone); "
                         "per-channel normalisation is not built")
    normalise = flags.pop()
    clean = [c for c, _ in parsed]
    return clean, normalise, [(c or FrameClean()).pipes(normalise) for c in clean], C


def SERVER_segment_frames(params, options):
    """Segment whole camera frames (larger than the network tile): params['input'] = an Octopus stream stem
    (sequitr/dataio/octopus.py), a .npy of (F,H,W) uint8/uint16/float32 frames, or an ndarray.  Raw frames
    cross PCIe; ImageNorm, tiling, the U-Net and stitching run on the GPU (sequitr_amd/frontend.py).  Writes
    ``mask.npy`` (F,H,W) uint8, ``segment.json`` and, with options['centroids'], the centroid file.
    options['measure'] (implies centroids) measures every object per batch in HBM against the RAW frames -- the camera's
    counts, before any cleaning (sequitr_amd/objects.py): the centroid file gains per frame ``area``, ``bbox`` and
    ``intensity`` (mean, std, min, max) next to ``coords``, ``objects.npz`` holds ObjectTable.columns() of the whole
    stack and segment.json an ``objects`` record; options['save_labels'] adds ``labels.npy`` (F,H,W) int32, each object's
    1-based rank within its frame.  params['min_area'] / params['max_area'] (inclusive, in pixels) drop objects outside
    the range from all of these, and ``mask.npy`` is then the mask without them.
    params: shape (tile, default (512,512)), margin, frames_per_batch, model / filters / ... as SERVER_segment;
    pipeline: the JSON ImagePipeline.save wrote (or an ImagePipeline).  It runs on the GPU per whole frame and may hold
    any subsequence of ImageOutliers, ImageBlur, ImageBGSubtract, ImageNorm in that order (frontend.FrameClean.from_pipeline;
    ImageBlur with a finite sigma in (0, 8.125); anything else raises before a frame is read -- there is no host fallback);
    segment.json records it under 'pipeline'.  Without it the frames are normalised with ImageNorm alone.

    Multi-channel frames (bright field + fluorescence): params['input'] may be a list of C sources, each an Octopus stem, a
    .npy or an ndarray of (F,H,W) frames of one length, shape and pixel type, or one interleaved (F,H,W,C) .npy / ndarray.
    num_inputs defaults to C and must equal it; params['pipeline'] may then be a list of C pipelines with null entries (one
    pipeline applies to every channel; each channel gets its own background fit); options['measure'] measures intensity in
    channel params['measure_channel'] (default 0).  segment.json gains 'channels' and 'pipeline' is recorded per channel.
    Ragged sources, a num_inputs other than C, a pipeline list of the wrong length or a measure_channel out of range raise
    before a pixel is read.  With one (F,H,W) source every file is what it was.

    params['postprocess'] (a list of mask clean-up steps, or the path of a JSON file holding one; maskops.MaskCleanup) runs
    on each batch's stitched masks in HBM before any sink sees them: ``mask.npy``, the centroid file, ``objects.npz``,
    ``labels.npy`` and the min_area / max_area filter all describe the cleaned mask, and segment.json records the steps
    under 'postprocess'.  A bad step list raises before a frame is read; without the key nothing changes.  A step
    {"op": "split", "erosions": r, "structure": ..., "reach": ...} (maskops.split) cuts touching cells apart, so the
    centroid file and ``objects.npz`` get one row per cell instead of one per clump.

    options['neighbors'] (implies measure) finds every object's neighbours per batch in HBM (sequitr_amd/analysis/
    neighbors.py: touching zones of influence, NOT the reference's Delaunay of the centroids): ``neighbors.npz`` holds
    NeighborTable.columns() of the whole stack, one row per row of ``objects.npz`` with ``indices`` global, segment.json a
    ``neighbors`` record (objects, pairs, pairs_removed and the parameters with their defaults filled in);
    options['save_zones'] adds ``zones.npy`` (F,H,W) int32.  params['d_thresh'] (default 100.0), params['zone_reach'] (the
    zones' max_distance, default none) and params['neighbor_seeds'] ('objects' or 'centroids'); a bad value raises before a
    frame is opened.  The table describes the mask after `postprocess` and the size filter: dropped objects are no seeds.
    Without the option every file is what it was.

    options['link'] (implies measure) links every object to its successor in the next frame while the batch's labels are
    in HBM (sequitr_amd/analysis/linking.py: overlap tracks and divisions; its module text is the rule): ``lineage.npz``
    holds TrackTable.columns() of the whole stack -- ``track`` has one entry per row of ``objects.npz`` -- and segment.json a
    ``link`` record (objects, tracks, links, divisions, roots and the parameters with their defaults filled in);
    options['save_track_labels'] adds ``track_labels.npy`` (F,H,W) int32, every object's pixels holding its track ID, so
    that a cell keeps one value through the movie.  params['link_reach'] (0), params['link_min_iou'] (0.0),
    params['link_min_overlap'] (1), params['link_divisions'] (true), params['link_min_child_fraction'] (0.5) and
    params['link_same_class'] (true); a bad value raises before a frame is opened.  The result does not depend on
    frames_per_batch.  Without the option every file is what it was.

    options['shape'] (implies measure) adds the shape columns (objects.measure_objects(shape=True): second-order moments,
    exposed faces, boundary pixels, perimeter counts) and the columns derived from them (covariance, axis_lengths,
    eccentricity, orientation, equivalent_diameter, extent, perimeter, crack_perimeter, circularity; ObjectTable's
    docstrings are the formulas) to ``objects.npz``, for the cleaned mask behind `postprocess` and the size filter, as
    `measure` does; segment.json's ``objects`` record gains ``shape: true``.  Without the option every file is what it was.

    params['tta'] (null, "flips" or "dihedral") is test-time augmentation (frontend.segment_frames: the network sees every
    tile under the four flip states or all eight symmetries of the square and the logits are averaged in HBM; 4 or 8 network
    passes).  Every sink sees the merged mask -- ``mask.npy``, the centroid file, `measure`, `shape`, `neighbors`, `link`,
    the size filter and `postprocess`.  options['save_probabilities'] (true = 'uint8', or 'uint8' / 'float32') writes
    ``probability.npy`` (F,K,H,W) next to ``mask.npy``: the softmax of the (mean) logits stitched to whole frames, uint8 as
    rounded p * 255; `postprocess` and the size filter do not touch it.  segment.json records ``tta`` and ``probabilities``
    with the defaults filled in, but only when the keys are present.  A bad value, or either key together with
    params['brick'], raises before anything is opened; SERVER_segment (the tile job) and SERVER_segment_volume refuse both.
    WORLD_SIZE plays no part in this job (every process segments the stack it was given), so the keys add nothing to refuse
    there.  Without them every file is what it was.

    params['blend'] (an integer number of pixels, 0 .. min(margin, (tile - 2 margin) // 2, 255)) blends the seams between
    overlapping tiles (frontend.segment_frames(blend=): within that distance of a seam line the tiles' logits are mixed with
    integer tent weights before the argmax and the softmax).  It goes with `tta` and `save_probabilities`, and every sink
    sees the blended mask as above.  segment.json records ``blend`` when the key is present.  A bad value, or the key
    together with params['brick'], raises before anything is opened; SERVER_segment, SERVER_segment_volume and the training
    jobs refuse it.  Without the key (or with null / 0) every file is what it was."""
    _refuse_volume_postprocess(params, 'SERVER_segment_frames')
    _refuse_volume_tta(params, options, 'SERVER_segment_frames')
    tta, probabilities = _parse_tta(params, options, 'SERVER_segment_frames')
    blend = _parse_blend(params, 'SERVER_segment_frames')
    postprocess = _parse_postprocess(params)                    # before anything is opened
    want_neighbors = bool(options.get('neighbors'))
    want_link = bool(options.get('link'))
    if want_link:                                               # a bad value raises here, before a frame is opened
        from .analysis.linking import DEFAULTS as link_defaults, FrameLinker
        linker = FrameLinker(**{k: params.get('link_' + k, v) for k, v in link_defaults.items()})
    if want_neighbors:                                          # a bad value raises here, before a frame is opened
        from .analysis.neighbors import check_params
        d_thresh, zone_reach, neighbor_seeds = check_params(params.get('d_thresh', 100.0), params.get('zone_reach'),
                                                            params.get('neighbor_seeds', 'objects'))
    import torch
    from .networks.unet import UNet2D
    from .frontend import segment_frames

    device = _resolve_device(params, options)
    out_dir = params['output']
    parsed = _parse_pipelines(params)                           # a pipe the device does not run: before the frames are opened
    frames, F, H, W, C_in = _open_channels(params)
    clean, normalise, pipe_record, num_inputs = _channel_setup(params, C_in, parsed)
    measure_channel = int(params.get('measure_channel', 0))
    if not 0 <= measure_channel < (C_in or 1):
        raise ValueError("params['measure_channel'] is %d, the input has %d channel(s)" % (measure_channel, C_in or 1))
    net_p = _net_params(params, device)
    if num_inputs is not None:
        net_p['num_inputs'] = num_inputs
    net_p.setdefault('shape', (512, 512))
    tile = int(net_p['shape'][0])
    net = UNet2D(net_p, 'infer')
    _load_net_weights(net, params)
    per_frame = {}
    want_shape = bool(options.get('shape'))
    want_measure = bool(options.get('measure')) or want_neighbors or want_link or want_shape
    want_centroids = bool(options.get('centroids')) or want_measure
    masks = np.empty((F, H, W), np.uint8) if want_centroids else None
    min_area, max_area = int(params.get('min_area') or 1), params.get('max_area')
    bounded = min_area != 1 or max_area is not None
    if bounded and not want_measure:
        raise ValueError("params['min_area'] / params['max_area'] need options['measure']")
    label_stack = np.empty((F, H, W), np.int32) if want_measure and options.get('save_labels') else None
    tables, firsts = [], []
    neighbor_tables = []
    zone_stack = np.empty((F, H, W), np.int32) if want_neighbors and options.get('save_zones') else None
    num_classes = int(net_p.get('num_outputs', 2))
    track_stack = np.empty((F, H, W), np.int32) if want_link and options.get('save_track_labels') else None
    prob_stack = np.empty((F, num_classes, H, W), probabilities) if probabilities and want_centroids else None
    kept_labels = []                                            # with save_track_labels: the batches' label frames, in HBM

    def sink(first, m):                                       # centroids need the masks while they are in HBM
        from .centroids import mask_centroids
        masks[first:first + m.shape[0]] = m.cpu().numpy()
        for k, coords in enumerate(mask_centroids(m)):
            coords[:, 0] = first + k
            per_frame[first + k] = coords

    def prob_sink(first, p):                                   # with a mask sink the probabilities are visited too
        prob_stack[first:first + p.shape[0]] = p.cpu().numpy()

    def measure_sink(first, raw, m):                           # objects against the raw frames, both still in HBM
        from .objects import measure_objects
        image = raw if raw.dim() == 3 else raw[measure_channel]   # (C, n, H, W) planes: the channel's slice as it lies
        t = measure_objects(m, image=image, min_area=min_area, max_area=max_area,
                            labels=label_stack is not None or want_neighbors or want_link, filtered_mask=bounded, shape=want_shape)
        masks[first:first + m.shape[0]] = (t.mask if bounded else m).cpu().numpy()
        if label_stack is not None:
            label_stack[first:first + m.shape[0]] = t.labels.cpu().numpy()
        if want_neighbors:                                      # on the kept objects' labels, while the batch is in HBM
            from .analysis.neighbors import neighbors_from_objects
            nt = neighbors_from_objects(t, num_classes, d_thresh, zone_reach, neighbor_seeds,
                                        return_zones=zone_stack is not None)
            if zone_stack is not None:
                zone_stack[first:first + m.shape[0]] = nt.zones.cpu().numpy()
                nt.zones = None
            neighbor_tables.append(nt)
        if want_link:                                           # batches arrive in the stack's order
            linker.push(first, t.labels, t)
            if track_stack is not None:
                kept_labels.append((first, t.labels))
        tables.append(t)
        firsts.append(first)

    t0 = time.time()
    # without centroids the masks come back through segment_frames' own double-buffered download (batch i-1 drains
    # while batch i runs); with them every batch is visited on the device first
    out = segment_frames(net, frames, tile=tile, margin=int(params.get('margin', 32)),
                         frames_per_batch=int(params.get('frames_per_batch', 4)),
                         on_masks=sink if want_centroids and not want_measure else None,
                         on_batch=measure_sink if want_measure else None, normalise=normalise, clean=clean,
                         postprocess=postprocess, tta=tta, probabilities=probabilities, blend=blend,
                         on_probs=prob_sink if prob_stack is not None else None)
    if probabilities is not None and not want_centroids:
        out, prob_stack = out
    if not want_centroids:
        masks = out
    torch.cuda.synchronize()
    dt = time.time() - t0
    np.save(os.path.join(out_dir, 'mask.npy'), masks)
    if probabilities is not None:
        np.save(os.path.join(out_dir, 'probability.npy'), prob_stack)
    info = {'frames': int(F), 'shape': [int(H), int(W)], 'tile': tile, 'seconds': dt,
            'mpixels_per_s': float(F * H * W / max(dt, 1e-9) / 1e6), 'device': device}
    if 'tta' in params:
        info['tta'] = tta
    if 'save_probabilities' in options:
        info['probabilities'] = probabilities
    if 'blend' in params:
        info['blend'] = blend
    if C_in is not None:
        info['channels'] = C_in
        if want_measure:
            info['measure_channel'] = measure_channel
    if pipe_record is not None:
        info['pipeline'] = pipe_record
    if postprocess is not None:
        info['postprocess'] = postprocess.record()
    if want_measure:
        from .centroids import CentroidWriter
        from .objects import ObjectTable
        table = ObjectTable.concatenate(tables, firsts, F)
        with CentroidWriter(os.path.join(out_dir, 'tracks.hdf5')) as cw:
            for k, (coords, t) in enumerate(zip(table.coords(), table.frames())):
                cw.add_frame(k, coords, **cw._extras(t))
        np.savez(os.path.join(out_dir, 'objects.npz'), **table.columns())
        if label_stack is not None:
            np.save(os.path.join(out_dir, 'labels.npy'), label_stack)
        info['centroids'] = {'file': os.path.basename(cw.filename), 'objects': len(table)}
        info['objects'] = {'count': len(table), 'found': int(table.found), 'min_area': min_area,
                           'max_area': None if max_area is None else int(max_area), 'with_intensity': True}
        if want_shape:                                          # the record's own 'shape' key is the frames' shape
            info['objects']['shape'] = True
        if want_neighbors:
            from .analysis.neighbors import NeighborTable
            order = np.argsort(firsts, kind='stable')           # batches in the stack's order: indices become global rows
            ntable = NeighborTable.concatenate([neighbor_tables[i] for i in order], [firsts[i] for i in order], F)
            np.savez(os.path.join(out_dir, 'neighbors.npz'), **ntable.columns())
            if zone_stack is not None:
                np.save(os.path.join(out_dir, 'zones.npy'), zone_stack)
            info['neighbors'] = {'objects': len(ntable), 'pairs': int(ntable.n_pairs),
                                 'pairs_removed': int(ntable.n_pairs_removed), 'num_classes': num_classes,
                                 'd_thresh': d_thresh, 'zone_reach': zone_reach, 'neighbor_seeds': neighbor_seeds}
        if want_link:
            from .analysis.linking import relabel
            tracks = linker.finish()
            np.savez(os.path.join(out_dir, 'lineage.npz'), **tracks.columns())
            if track_stack is not None:                         # ranks -> track IDs on the device, batch by batch
                offsets, lut = tracks.lut()
                lut_d = torch.from_numpy(lut).to(device)
                for first, lab in kept_labels:
                    n = int(lab.shape[0])
                    track_stack[first:first + n] = relabel(lab, offsets[first:first + n + 1], lut_d, out=lab).cpu().numpy()
                np.save(os.path.join(out_dir, 'track_labels.npy'), track_stack)
            info['link'] = dict(tracks.options, objects=len(tracks.track), tracks=len(tracks), links=len(tracks.links),
                                divisions=int((tracks.children[:, 0] > 0).sum()),
                                roots=int((tracks.parent == tracks.ID).sum()))
    elif want_centroids:
        from .centroids import CentroidWriter
        with CentroidWriter(os.path.join(out_dir, 'tracks.hdf5')) as cw:
            for k in sorted(per_frame):
                cw.add_frame(k, per_frame[k])
        info['centroids'] = {'file': os.path.basename(cw.filename), 'objects': int(sum(len(v) for v in per_frame.values()))}
    with open(os.path.join(out_dir, 'segment.json'), 'w') as f:
        json.dump(info, f, indent=2)
    logger.info('Segmented {frames} frames in {seconds:.3f}s on {device}'.format(**info))
    return info


def _load_labels(src, key='labels'):
    """class-index labels: a .npy path (opened as a memmap) or an ndarray, uint8"""
    if isinstance(src, str) and src.endswith('.npy'):
        labels = np.load(src, mmap_mode='r', allow_pickle=False)
    elif isinstance(src, np.ndarray):
        labels = src
    else:
        raise ValueError("params[%r] must be a .npy path or an ndarray of uint8 class indices" % key)
    if labels.dtype != np.uint8:
        raise TypeError("params[%r] must be uint8 class indices, got %s" % (key, labels.dtype))
    return labels


def _upload_rows(arr, shape, np_dtype, device, out=None):
    """host array or memmap -> a device tensor of `shape` and `np_dtype` (`out` when it is given), one leading index at a
    time: the host copies (and casts) one row at a time, never the whole stack -- arr may be a read-only memmap"""
    import torch
    from .frontend import NP_TORCH
    if out is None:
        out = torch.empty(tuple(shape), dtype=NP_TORCH[np.dtype(np_dtype)], device=device)
    for i in range(out.shape[0]):
        out[i].copy_(torch.from_numpy(np.array(arr[i], dtype=np_dtype, order='C')).reshape(out[i].shape))
    return out


class _LabelFeed(object):
    """uint8 labels (N, ...) on their way to the device: the whole stack once when it fits in `resident_bytes`, otherwise
    the rows a batch needs, through two pinned buffers, on the stream the masks are produced on"""

    def __init__(self, labels, device, rows_per_batch, resident_bytes):
        import torch
        from .frontend import _pinned
        self.labels, self.all = labels, None
        if labels.nbytes <= resident_bytes:
            self.all = _upload_rows(labels, labels.shape, np.uint8, device)
            return
        shape = (int(rows_per_batch),) + tuple(labels.shape[1:])
        self.pinned = [_pinned('labels%d' % i, shape, torch.uint8) for i in range(2)]
        self.staged = [torch.empty(shape, dtype=torch.uint8, device=device) for _ in range(2)]
        self.sent = [torch.cuda.Event(), torch.cuda.Event()]
        self.turn = 0

    def get(self, first, n):
        """labels[first:first + n] in HBM; a staged batch stays valid until the second get() after it"""
        if self.all is not None:
            return self.all[first:first + n]
        k, self.turn = self.turn, 1 - self.turn
        self.sent[k].synchronize()                              # the previous upload out of this pinned buffer is done
        self.pinned[k][:n].numpy()[...] = self.labels[first:first + n]
        self.staged[k][:n].copy_(self.pinned[k][:n], non_blocking=True)
        self.sent[k].record()
        return self.staged[k][:n]


def _evaluation_record(counts, ignored):
    """the part of evaluate.json that follows from the per-item counts (F, C, C) and ignored (F), host int64"""
    from .confusion import json_ready, scores
    total = counts.sum(0)
    return {'confusion': total.tolist(), 'ignored': int(ignored.sum()), 'scores': json_ready(scores(total)),
            'per_frame': [dict(json_ready(scores(c)), ignored=int(g)) for c, g in zip(counts, ignored)]}


def _evaluate_volume_bricks(params, options, cleanup=None, tta=None):
    """SERVER_evaluate with params['brick']: volumes brick by brick, each stitched mask scored where segment_volumes
    leaves it (after params['volume_postprocess'], when given)"""
    labels = _load_labels(params.get('labels'))
    device, x, (bz, bx, by), margin, geometry = _brick_volumes(params, options)
    N, Z, X, Y = (int(s) for s in x.shape)
    if tuple(labels.shape) != (N, Z, X, Y):
        raise ValueError('labels %s do not match the volumes %s' % (tuple(labels.shape), (N, Z, X, Y)))
    out_dir = params['output']

    import torch
    from . import ops
    from .networks.unet import UNet3D
    from .frontend import segment_volumes
    torch.cuda.set_device(torch.device(device))
    net_p = _net_params(params, device)
    net_p['shape'], net_p['num_inputs'] = (bx, by, bz), 1
    t_setup = time.time()
    net = UNet3D(net_p, 'infer')
    _load_net_weights(net, params)
    C = int(net.n_outputs)
    batch = int(params.get('bricks_per_batch', 8))
    net.predict(torch.zeros((min(batch, geometry.per_volume), bz, bx, by, 1), device=device))   # first-launch costs
    feed = _LabelFeed(labels, device, 1, float(options.get('resident_label_gib', 4)) * 2 ** 30)
    counts = torch.zeros((N, C, C), dtype=torch.int64, device=device)
    ignored = torch.zeros((N,), dtype=torch.int64, device=device)
    masks = np.zeros((N, Z, X, Y), np.uint8) if options.get('masks') else None
    torch.cuda.synchronize()

    def sink(i, m):                                            # m (1, Z, X, Y) in HBM
        ops.confusion_(counts[i:i + 1], ignored[i:i + 1], m, feed.get(i, 1), C)
        if masks is not None:
            masks[i] = m[0].cpu().numpy()

    t0 = time.time()
    segment_volumes(net, x, (bz, bx, by), margin, bricks_per_batch=batch, normalise=bool(params.get('normalise', True)),
                    on_masks=sink, **({'postprocess': cleanup} if cleanup else {}), **({'tta': tta} if tta is not None else {}))
    counts_h, ignored_h = counts.cpu().numpy(), ignored.cpu().numpy()
    dt = time.time() - t0
    np.save(os.path.join(out_dir, 'confusion.npy'), counts_h)
    if masks is not None:
        np.save(os.path.join(out_dir, 'mask.npy'), masks)
    info = {'volumes': N, 'shape': [Z, X, Y], 'num_classes': C, 'seconds': dt, 'setup_seconds': t0 - t_setup,
            'mpixels_per_s': float(N * Z * X * Y / max(dt, 1e-9) / 1e6), 'device': device, 'brick': [bx, by, bz],
            'margin': [geometry.margin[1], geometry.margin[2], geometry.margin[0]],
            'bricks_per_volume': int(geometry.per_volume)}
    if cleanup is not None:
        info['volume_postprocess'] = cleanup.record()
    if 'volume_tta' in params:
        info['volume_tta'] = tta
    info.update(_evaluation_record(counts_h, ignored_h))
    with open(os.path.join(out_dir, 'evaluate.json'), 'w') as f:
        json.dump(info, f, indent=2)
    logger.info('Scored {volumes} volumes in {seconds:.3f}s on {device}'.format(**info))
    return info


def SERVER_evaluate(params, options):
    """Score a saved model on labelled data: segments as SERVER_segment_frames does (the same params: input, shape,
    margin, frames_per_batch, pipeline, model ...) or, with params['brick'], as SERVER_segment_volume does, and counts
    every stitched mask against params['labels'] -- a .npy (or ndarray) of uint8 class indices, (F, H, W) or
    (V, Z, X, Y) -- while the mask is in HBM (sq_confusion): what comes back per frame is C x C integers, not the mask.
    Labels >= num_outputs (255 is the usual "unlabelled") are counted as ``ignored`` and enter no cell.

    Writes ``confusion.npy``, int64 (F, C, C) with row = truth and column = prediction, and ``evaluate.json``: the total
    matrix ``confusion``, ``ignored``, ``scores`` (iou, dice, precision, recall and support per class, accuracy, mean_iou;
    a class absent from both sides scores null), ``per_frame`` with the same per frame, ``seconds``, ``mpixels_per_s``
    and the ``pipeline`` record as segment.json has it (with a multi-channel input -- a list of C sources or an (F,H,W,C)
    array, as SERVER_segment_frames takes it -- also ``channels``, and ``pipeline`` per channel).  ``mask.npy`` is written
    only with options['masks'].  The labels
    follow the frames to the device batch by batch; a stack up to options['resident_label_gib'] (default 4) is uploaded
    once instead.  A label shape that does not match the frames raises before any frame is read.

    params['postprocess'] (as SERVER_segment_frames takes it, the ``split`` step included) cleans each batch's masks in HBM first: ``confusion.npy``, the
    scores and ``mask.npy`` describe the cleaned masks and evaluate.json records the steps under 'postprocess'.  It covers
    frames only: together with params['brick'] it is refused.  params['volume_postprocess'] (as SERVER_segment_volume takes
    it) does the same for volumes: it needs params['brick'] and is refused without it; evaluate.json records the steps
    under 'volume_postprocess'.

    params['tta'] (null, "flips" or "dihedral", as SERVER_segment_frames takes it) scores the test-time-augmented masks --
    the way to see whether the 4 or 8 network passes pay on a data set; evaluate.json records ``tta`` when the key is
    present.  Frames only: with params['brick'] it is refused, and so is options['save_probabilities'], before anything is
    opened.  With params['brick'], params['volume_tta'] (as SERVER_segment_volume takes it) scores the merged masks of the
    8 or 16 views and evaluate.json records ``volume_tta``; options['save_volume_probabilities'] is refused.

    params['blend'] (as SERVER_segment_frames takes it) scores the masks with the seams between tiles blended;
    evaluate.json records ``blend`` when the key is present.  Frames only: with params['brick'] it is refused before
    anything is opened."""
    if options.get('save_probabilities'):
        raise ValueError("options['save_probabilities'] belongs to SERVER_segment_frames: SERVER_evaluate writes scores")
    tta, _ = _parse_tta(params, {}, 'SERVER_evaluate')          # before anything is opened
    blend = _parse_blend(params, 'SERVER_evaluate')
    postprocess = _parse_postprocess(params)
    cleanup = _parse_volume_postprocess(params)
    if options.get('save_volume_probabilities'):
        raise ValueError("options['save_volume_probabilities'] belongs to SERVER_segment_volume: SERVER_evaluate writes scores")
    if params.get('brick') is not None:
        volume_tta, _ = _parse_volume_tta(params, {}, 'SERVER_evaluate')
        return _evaluate_volume_bricks(params, options, cleanup, volume_tta)
    _refuse_volume_postprocess(params, 'SERVER_evaluate without it')
    _refuse_volume_tta(params, options, 'SERVER_evaluate without it')
    labels = _load_labels(params.get('labels'))
    frames, F, H, W, C_in = _open_channels(params)
    if tuple(labels.shape) != (F, H, W):
        raise ValueError('labels %s do not match the frames %s' % (tuple(labels.shape), (F, H, W)))
    from .frontend import segment_frames
    clean, normalise, pipe_record, num_inputs = _channel_setup(params, C_in)

    import torch
    from . import ops
    from .networks.unet import UNet2D
    device = _resolve_device(params, options)
    torch.cuda.set_device(torch.device(device))
    out_dir = params['output']
    net_p = _net_params(params, device)
    if num_inputs is not None:
        net_p['num_inputs'] = num_inputs
    net_p.setdefault('shape', (512, 512))
    tile = int(net_p['shape'][0])
    net = UNet2D(net_p, 'infer')
    _load_net_weights(net, params)
    C = int(net.n_outputs)
    B = int(params.get('frames_per_batch', 4))
    feed = _LabelFeed(labels, device, B, float(options.get('resident_label_gib', 4)) * 2 ** 30)
    counts = torch.zeros((F, C, C), dtype=torch.int64, device=device)
    ignored = torch.zeros((F,), dtype=torch.int64, device=device)
    masks = np.empty((F, H, W), np.uint8) if options.get('masks') else None

    def sink(first, m):                                        # m (n, H, W) in HBM: one row of counts per frame
        n = m.shape[0]
        ops.confusion_(counts[first:first + n], ignored[first:first + n], m, feed.get(first, n), C)
        if masks is not None:
            masks[first:first + n] = m.cpu().numpy()

    t0 = time.time()
    segment_frames(net, frames, tile=tile, margin=int(params.get('margin', 32)), frames_per_batch=B, on_masks=sink,
                   normalise=normalise, clean=clean, postprocess=postprocess, tta=tta, blend=blend)
    counts_h, ignored_h = counts.cpu().numpy(), ignored.cpu().numpy()
    dt = time.time() - t0
    np.save(os.path.join(out_dir, 'confusion.npy'), counts_h)
    if masks is not None:
        np.save(os.path.join(out_dir, 'mask.npy'), masks)
    info = {'frames': F, 'shape': [H, W], 'tile': tile, 'num_classes': C, 'seconds': dt,
            'mpixels_per_s': float(F * H * W / max(dt, 1e-9) / 1e6), 'device': device}
    if 'tta' in params:
        info['tta'] = tta
    if 'blend' in params:
        info['blend'] = blend
    if C_in is not None:
        info['channels'] = C_in
    if pipe_record is not None:
        info['pipeline'] = pipe_record
    if postprocess is not None:
        info['postprocess'] = postprocess.record()
    info.update(_evaluation_record(counts_h, ignored_h))
    with open(os.path.join(out_dir, 'evaluate.json'), 'w') as f:
        json.dump(info, f, indent=2)
    logger.info('Scored {frames} frames in {seconds:.3f}s on {device}'.format(**info))
    return info


def SERVER_test(params, options):
    """Plumbing check (the reference's commented-out SERVER_test, worker.py:300-302):
    writes the params it was called with into the output folder."""
    with open(os.path.join(params['output'], 'test.json'), 'w') as f:
        json.dump({'params': {k: repr(v) for k, v in params.items()},
                   'options': {k: repr(v) for k, v in options.items()}}, f, indent=2)


def _onehot(labels, num_outputs, spatial=2):
    """class-index labels (N,H,W) -> one-hot uint8 (N,H,W,num_outputs); classes >= num_outputs get an
    all-zero row, as tr_augment's ``concat(...)[..., :outputs]`` does (sequitr/networks/unet.py:396-398).  Labels with
    one more dimension than the `spatial` ones carry a trailing class axis already and are cut to num_outputs; volumes
    (N,Z,X,Y[,C]) are spatial = 3."""
    labels = np.asarray(labels)
    if labels.ndim == spatial + 2:
        return np.ascontiguousarray(labels[..., :num_outputs], dtype=np.uint8)
    return np.stack([(labels == c) for c in range(num_outputs)], -1).astype(np.uint8)


def _validation_keys(params):
    """(wanted, validate_every): the val_* keys come as a pair; validate_every counts epochs, None = after the last step only"""
    have = [k for k in ('val_images', 'val_labels') if params.get(k) is not None]
    if len(have) == 1:
        raise ValueError("params['val_images'] and params['val_labels'] go together, got only %r" % have[0])
    every = params.get('validate_every')
    if every is not None and int(every) < 1:
        raise ValueError('validate_every counts epochs and must be positive, got %r' % (every,))
    if have and int(os.environ.get('WORLD_SIZE', 1)) > 1:
        raise RuntimeError("validation (params['val_images'] / ['val_labels']) runs in a single process: WORLD_SIZE is %s "
                           "(rank 0 validating alone while the others wait is not built)" % os.environ.get('WORLD_SIZE'))
    return bool(have), (None if every is None else int(every))


class _Validator(object):
    """Held-out scoring between training steps, outside the captured graphs.  The net is the inference net the segment
    jobs build for a saved model (UNet2D, mode 'infer': no dropout, the fused f32 kernels), and its variables ARE the
    trainer's: views of the flat parameter bucket plus the trainer's non-trainable state, re-bound on the device before
    every run, so a validation sees the weights of the step before it without a copy.  Nothing the training step reads
    is written: the dropout salt, the samplers' random streams and the trainer's workspace arena are not touched."""

    def __init__(self, trainer, net_p, run, steps_per_epoch, every, total_steps):
        from .confusion import ConfusionMeter
        from .networks.unet import UNet2D
        self.trainer, self.run = trainer, run
        self.net = UNet2D(dict(net_p), 'infer')
        self.meter = ConfusionMeter(self.net.n_outputs, self.net.device)
        self.steps_per_epoch, self.every, self.total_steps = int(steps_per_epoch), every, int(total_steps)
        self.log, self.seconds = [], 0.0

    def _bind(self):
        tr, net = self.trainer, self.net
        for k in tr.pbucket.names:
            net._vars[k] = tr.pbucket.view(k).detach()
        for k, v in tr.net._vars.items():                       # BN moving statistics
            if k not in tr.pbucket.shapes:
                net._vars[k] = v.detach()
        net._loaded, net._creatable = True, set()

    def after_step(self, done):
        """called with the number of optimiser steps done; validates at the end of every `every`-th epoch and after
        the last step"""
        import torch
        from .confusion import json_ready
        last = done == self.total_steps
        due = self.every is not None and done % (self.every * self.steps_per_epoch) == 0
        if not (last or due):
            return
        torch.cuda.synchronize()
        t0 = time.time()
        self._bind()
        self.meter.reset()
        with torch.no_grad():
            self.run(self.net, self.meter)
        counts = self.meter.counts()                            # the one download, and the synchronisation
        dt = time.time() - t0
        self.seconds += dt
        s = json_ready(self.meter.scores())
        self.log.append({'step': int(done), 'epoch': int(-(-done // self.steps_per_epoch)), 'confusion': counts.tolist(),
                         'ignored': self.meter.ignored(), 'iou': s['iou'], 'dice': s['dice'], 'accuracy': s['accuracy'],
                         'mean_iou': s['mean_iou'], 'seconds': dt})


def _make_trainer(params, net_p, config, net_cls=None):
    """The trainer of the four U-Net training jobs: UNetTrainer on net_p (which gains the jobs' dropout default), the
    hyper-parameters it uses recorded in `config`, and params['warm_start'] applied"""
    from . import utils
    from .train import UNetTrainer
    net_p['dropout'] = float(params.get('dropout', 0.4))
    # learning_rate: the job's own value when it gives one; otherwise the trainer's default, NOT NetConfiguration's 0.01
    # (sequitr/utils.py:289), which diverges on the 5-level net under Adam (train.DEFAULT_LEARNING_RATE, HISTORY.md section 8)
    trainer = UNetTrainer(net_p, learning_rate=params.get('learning_rate'), warmup_steps=params.get('warmup_steps'),
                          net_cls=net_cls)
    # net.config must record the hyper-parameters that were USED (it is what a warm start or an audit reads): the
    # trainer's learning rate and warm-up, not NetConfiguration's untouched defaults
    config.learning_rate = trainer.lr
    config.warmup_steps = trainer.warmup_steps
    if config.warm_start:
        latest = config.warm_start_from()
        if latest:
            trainer.load_state_dict(utils.load_model_weights(latest))
            logger.info('Warm start from {0:s}'.format(latest))
    return trainer


def _step_budget(params, options, config, steps_per_epoch):
    """(epochs, total_steps): params['num_epochs'] (else the configuration's) full epochs, cut off at options['max_steps']"""
    epochs = int(params.get('num_epochs', config.num_epochs))
    max_steps = options.get('max_steps')
    total_steps = epochs * steps_per_epoch if not max_steps else min(int(max_steps), epochs * steps_per_epoch)
    return epochs, total_steps


def _run_steps(trainer, bufs, epochs, steps_per_epoch, total_steps, begin_epoch, fill, use_graph, validator, dev):
    """The loop of the four U-Net training jobs -> (losses, steps done, seconds, ms_per_step, steady_steps).

    begin_epoch(epoch) makes an epoch's state (its permutation or sampling plan: the job's one random draw per epoch, never
    made in an epoch that total_steps cuts off) and fill(state, s, bufs) writes step s's batch into the list `bufs` (image,
    one-hot labels, weights).  With use_graph the first step runs eagerly (it warms every kernel up and sizes the
    workspaces), then the step is captured -- (zero, forward, loss, backward) + (Adam), the all-reduce between them -- and
    `bufs` is rebound IN PLACE to the capture's static inputs, so that later batches are written straight into them and
    step() has nothing to copy.  The loss of every step lands in a device-side log that is read back once, at the end (no
    per-step .item(): the host runs ahead of the GPU).  ms_per_step is the steady state: the first step carries the
    first-launch costs (and the capture) and is left out, as are the validator's seconds, all of which fall after it."""
    import torch
    loss_log = torch.zeros(max(total_steps, 1), dtype=torch.float32, device=dev)
    done = 0
    t_start = t_steady = time.time()
    for epoch in range(epochs):
        if done >= total_steps:
            break
        state = begin_epoch(epoch)
        for s in range(steps_per_epoch):
            if done >= total_steps:
                break
            fill(state, s, bufs)
            if use_graph and done == 0:
                trainer.capture(*bufs, warmup=1)
                bufs[:] = trainer.static_inputs
                loss_log[0].copy_(trainer.last_loss)
            else:
                loss_log[done].copy_(trainer.step(*bufs))
            done += 1
            if done == 1:
                torch.cuda.synchronize()
                t_steady = time.time()
            if validator is not None:
                validator.after_step(done)
    torch.cuda.synchronize()
    t_end = time.time()
    losses = [float(v) for v in loss_log[:done].cpu().numpy()]
    steady = max(done - 1, 0)
    val_seconds = validator.seconds if validator is not None else 0.0
    return (losses, done, t_end - t_start, (t_end - t_steady - val_seconds) * 1e3 / steady if steady > 0 else None, steady)


def _finish_training(params, config, trainer, validator, run, batch, path_info, use_graph, dtype, device, message,
                     after=None, world=1, rank=0):
    """What follows the loop in the four U-Net training jobs -> info.  `run` is what _run_steps returned; the job's own
    keys are path_info (they go between batch_size and graph) and `after` (behind device).  Rank 0 saves the model, writes
    train.json (info, losses and the validation log) and logs `message`."""
    from . import utils
    losses, done, seconds, ms_per_step, steady = run
    info = {'steps': done, 'first_loss': losses[0] if losses else None, 'last_loss': losses[-1] if losses else None,
            'seconds': seconds, 'ms_per_step': ms_per_step, 'steady_steps': steady, 'batch_size': batch, **path_info,
            'graph': use_graph, 'dtype': dtype, 'warmup_steps': trainer.warmup_steps, 'learning_rate': trainer.lr,
            'world': world, 'device': device, **(after or {})}
    if rank == 0:
        info['model_dir'] = utils.save_model(trainer.state_dict(), config)
        extra = {'validation': validator.log} if validator is not None else {}
        with open(os.path.join(params['output'], 'train.json'), 'w') as f:
            json.dump(dict(info, losses=losses, **extra), f, indent=2)
        logger.info(message.format(**info))
    return info


def _train_frame_tiles(params, options):
    """SERVER_train with params['tile']: whole raw frames of any size, their class-index labels and weight maps stay in
    HBM, and every step's batch of rotated tiles is cut there by one kernel (frontend.tile_sample_plan, TileSampler) --
    the reference's tr_augment (sequitr/networks/unet.py:348-401) in front of the captured step.  params['images'] (and
    val_images) may be an (F, H, W, C) .npy with C > 1 or a list of C (F, H, W) .npy: the frames are then uploaded plane by
    plane into a resident (C, F, H, W) tensor, ImageNorm's statistics are taken once per channel and frame, the sampler
    writes the step's (batch, th, tw, C) input, and net.config records num_inputs = C, so that the model loads into
    SERVER_segment_frames with the same list of inputs.  params['num_inputs'] (default 1, as everywhere in SERVER_train)
    must be given as C.  A channel count the trainer does not take (the bf16 graph: more
    than 7) raises the trainer's own message before any upload."""
    world = int(os.environ.get('WORLD_SIZE', 1))
    if world > 1:
        raise RuntimeError("params['tile'] samples frames in a single process: WORLD_SIZE is %d (data-parallel frame "
                           "sampling is not built)" % world)
    from .frontend import NP_TORCH, covering_tiles, tile_sample_plan
    tile = tuple(params['tile'])
    if len(tile) != 2:
        raise ValueError("params['tile'] must be (TH, TW), got %r" % (params['tile'],))
    th, tw = (int(s) for s in tile)

    def open_stack(src, key):
        """(stack, planes): the frames as segment_frames takes them, and one (F, H, W) array per channel (views, no pixel
        read).  src is an (F,H,W[,C]) .npy or a list of C (F,H,W) .npy"""
        from .frontend import open_channels
        if isinstance(src, (list, tuple)):
            stack = [np.load(s, mmap_mode='r', allow_pickle=False) for s in src]
        else:
            stack = np.load(src, mmap_mode='r', allow_pickle=False)
            if stack.ndim == 4 and stack.shape[3] == 1:
                stack = stack[..., 0]
            if stack.ndim not in (3, 4):
                raise ValueError("params[%r] with params['tile'] are (F, H, W) or (F, H, W, C) frame stacks, got shape %s"
                                 % (key, stack.shape))
        _, _, dtype, C = open_channels(stack)
        if dtype not in NP_TORCH:
            raise TypeError("with params['tile'] params[%r] must be raw uint8, uint16 or float32 frames, got %s" % (key, dtype))
        if C is None:
            return stack, [stack]
        return stack, list(stack) if isinstance(stack, list) else [stack[..., c] for c in range(C)]

    _, x_planes = open_stack(params['images'], 'images')
    x, CI = x_planes[0], len(x_planes)
    n_in = int(params.get('num_inputs', 1))                    # SERVER_train's default, a single-channel model
    if n_in != CI:
        raise ValueError("params['num_inputs'] is %d, the images have %d channel(s)%s" % (n_in, CI, (
            ': a single-channel model does not train on them, pass num_inputs = %d' % CI) if n_in == 1 else ''))
    F, H, W = (int(s) for s in x.shape)
    labels = np.load(params['labels'], mmap_mode='r', allow_pickle=False)
    if labels.ndim != 3:
        raise ValueError("with params['tile'] the labels are (F, H, W) class indices, one byte per pixel; one-hot labels "
                         "of shape %s are not taken" % (labels.shape,))
    if tuple(labels.shape) != (F, H, W):
        raise ValueError('labels %s do not match the images %s' % (labels.shape, x.shape))
    augment = params.get('augment')
    augment = ('rotate',) if augment is None else ((augment,) if isinstance(augment, str) else tuple(augment))
    seed = int(params.get('seed', 0))
    rng = np.random.default_rng(seed)
    tile_sample_plan((H, W), (th, tw), F, 1, np.random.default_rng(0), augment)      # refuses a bad `augment` before any upload
    samples = params.get('samples_per_epoch')
    samples = F * covering_tiles((H, W), (th, tw)) if samples is None else int(samples)
    if samples < 1:
        raise ValueError('samples_per_epoch must be positive, got %d' % samples)
    want_val, validate_every = _validation_keys(params)
    if want_val:                                               # whole raw frames and (F, H, W) labels, as the training pair
        vx, v_planes = open_stack(params['val_images'], 'val_images')
        if len(v_planes) != CI:
            raise ValueError('val_images have %d channel(s), the images %d' % (len(v_planes), CI))
        vlab = _load_labels(params['val_labels'], 'val_labels')
        if tuple(vlab.shape) != tuple(v_planes[0].shape):
            raise ValueError('val_labels %s do not match val_images %s' % (vlab.shape, v_planes[0].shape))
        if th != tw:
            raise ValueError('validation segments whole frames with square tiles (frontend.segment_frames), got tile %r'
                             % (tile,))

    import torch
    from . import utils
    from .frontend import TileSampler
    from .weightmap import device_weightmaps

    cfg_keys = ('name', 'num_outputs', 'num_epochs', 'learning_rate', 'warm_start', 'dropout')
    cfg = {k: params[k] for k in cfg_keys if k in params}
    cfg['shape'], cfg['num_inputs'] = (th, tw), CI             # net.config records the tile: the shape the model segments at
    config = utils.NetConfiguration.from_params(cfg)
    n_out = int(config.num_outputs)
    device = _resolve_device(params, options)
    torch.cuda.set_device(torch.device(device))
    dev = torch.device(device)

    net_p = _net_params(params, device)
    net_p['shape'] = (th, tw)
    net_p['num_inputs'], net_p['num_outputs'] = CI, n_out
    # before any upload: a trainer that does not take this many input channels says so itself
    trainer = _make_trainer(params, net_p, config)

    if CI == 1:
        x_dev = _upload_rows(x, (F, H, W), x.dtype, dev)
    else:                                                      # channel-major planes, resident: (C, F, H, W), plane by plane
        x_dev = torch.empty((CI, F, H, W), dtype=NP_TORCH[np.dtype(x.dtype)], device=dev)
        for c, plane in enumerate(x_planes):
            _upload_rows(plane, (F, H, W), x.dtype, dev, out=x_dev[c])
    y_dev = _upload_rows(labels, (F, H, W), np.uint8, dev)
    if params.get('weights'):
        w_dev = _upload_rows(np.load(params['weights'], mmap_mode='r', allow_pickle=False).reshape((F, H, W)), (F, H, W),
                             np.float32, dev)
    else:
        # once, on the whole frames; the rotation then interpolates the map, as the reference rotates its precomputed TIFFs
        w_dev = device_weightmaps(y_dev, params.get('w0', 10.), params.get('sigma', 5.))
    sampler = TileSampler((H, W), (th, tw), dev, channels=CI)
    normalise = bool(params.get('normalise', True))
    stats = sampler.stats(x_dev) if normalise else None         # ImageNorm of each WHOLE frame, as segment_frames applies it

    batch = max(1, min(int(params.get('batch_size', 16)), samples))
    steps_per_epoch = samples // batch
    epochs, total_steps = _step_budget(params, options, config, steps_per_epoch)
    bufs = [torch.empty((batch, th, tw, CI), dtype=torch.float32, device=dev),
            torch.empty((batch, th, tw, n_out), dtype=torch.uint8, device=dev),
            torch.empty((batch, th, tw, 1), dtype=torch.float32, device=dev)]
    use_graph = bool(options.get('graph', True))
    validator = None
    if want_val:
        from .frontend import segment_frames
        val_fpb = int(params.get('frames_per_batch', 4))
        val_feed = _LabelFeed(vlab, dev, val_fpb, float('inf'))   # resident, like the training labels

        def run_val(net, meter):                               # the frames as SERVER_segment_frames would segment them
            segment_frames(net, vx, tile=th, margin=int(params.get('margin', 32)), frames_per_batch=val_fpb,
                           on_masks=lambda first, m: meter.update(m, val_feed.get(first, m.shape[0])), normalise=normalise)

        validator = _Validator(trainer, net_p, run_val, steps_per_epoch, validate_every, total_steps)

    def begin_epoch(epoch):                                    # ONE plan upload per epoch; a step takes a slice of it
        return [torch.from_numpy(a).to(dev) for a in tile_sample_plan((H, W), (th, tw), F, samples, rng, augment)]

    def fill(state, s, bufs):
        plan, coef = state
        sl = slice(s * batch, (s + 1) * batch)
        sampler.sample(x_dev, y_dev, w_dev, plan[sl], coef[sl], n_out, normalise=normalise, stats=stats, out=bufs)

    run = _run_steps(trainer, bufs, epochs, steps_per_epoch, total_steps, begin_epoch, fill, use_graph, validator, dev)
    return _finish_training(
        params, config, trainer, validator, run, batch,
        {'frames': F, 'frame_shape': [H, W], 'tile': [th, tw], **({'channels': CI} if CI > 1 else {}),
         'augment': list(augment), 'samples_per_epoch': samples, 'seed': seed, 'normalise': normalise},
        use_graph, str(net_p.get('dtype', 'f32')), device,
        'Trained {steps} steps on rotated tiles of whole frames, loss {first_loss} -> {last_loss}, saved {model_dir}')


def SERVER_train(params, options):
    """Train the U-Net on a stack of tiles with the weight-map-weighted softmax cross-entropy.

    params: images (.npy (N,H,W[,C]) float), labels (.npy (N,H,W) class indices or one-hot), weights
    (.npy (N,H,W[,1]); when absent computed with ImageWeightMap(w0, sigma), sequitr/pipeline.py:455-479, on
    the GPU -- sq_weightmap_edt_f32 -- and kept there), dtype ('f32' | 'bf16' activations), plus the
    NetConfiguration keys (name, shape, num_outputs, learning_rate, num_epochs, batch_size, dropout, filters,
    bridge, warm_start ...) and warmup_steps (linear learning-rate warm-up, HISTORY.md section 8).
    Deviation from the reference's defaults: without params['learning_rate'] the step uses train.DEFAULT_LEARNING_RATE
    (0.003) ramped over train.DEFAULT_WARMUP_STEPS (40), not NetConfiguration's 0.01 (sequitr/utils.py:289), which
    diverges on this net under Adam; the values used are written to net.config and train.json.
    options: gpu, max_steps, graph (default True: the step is captured once and replayed as hipGraphs).

    The data path of a step never leaves the device: tiles, one-hot labels and weight maps are uploaded ONCE and stay
    in HBM (2.6 MB per 512x512 tile against 288 GB; a stack above params['resident_gib'], default 64, is staged batch by
    batch through pinned memory instead), an epoch's permutation is one index tensor, a batch is an index_select
    straight into the captured step's static input buffers.  The loop is _run_steps, which the frame path and both
    SERVER_train_volume paths share: the loss of every step lands in a device-side log that is read back once, after the
    last step (no per-step .item(): the host runs ahead of the GPU), and ms_per_step / steady_steps leave the first step
    out -- it carries the first-launch costs and, with `graph`, the capture -- whether or not the step is captured.
    Under torchrun (WORLD_SIZE > 1) the tiles shard across ranks and gradients are all-reduced over RCCL once per step, between
    the two graphs.  Rank 0 saves ``weights.npz`` + ``net.config`` into the next numbered folder of MODELDIR/<name>/
    (sequitr/utils.py:143-223 layout) and ``train.json`` (losses, ms_per_step) into params['output'].

    With params['tile'] = (TH, TW) the job trains on whole frames instead (_train_frame_tiles): images is a raw (F, H, W)
    uint8 / uint16 / float32 stack of any frame size, labels (F, H, W) class indices (one-hot labels are refused), weights
    (F, H, W) or, when absent, the EDT maps of the whole frames.  All three stay in HBM and every step's batch is sampled
    there by one kernel under a random rotation, the reference's tr_augment (sequitr/networks/unet.py:348-401): params
    augment (default ('rotate',); 'flip' adds mirrors, () only crops), samples_per_epoch (default: the number of margin-0
    tiles that cover the stack), seed, normalise (ImageNorm of each whole frame, default True).  The network is built at
    the tile shape and net.config records it, so the model loads into SERVER_segment_frames / SERVER_segment unchanged;
    train.json gains tile, augment, samples_per_epoch, seed and frame_shape.  Single process only: WORLD_SIZE > 1 raises.

    Held-out validation, in both paths: params val_images and val_labels, in the formats of images and labels of that path
    (with `tile`: whole raw frames and (F, H, W) class indices, segmented as SERVER_segment_frames does with the job's
    margin / frames_per_batch; otherwise tiles, scored val_batch at a time), and validate_every, counted in epochs
    (default: only after the last step).  Validation runs between steps, outside the captured graphs, on the inference
    net the segment jobs build for a saved model (UNet2D 'infer': the f32 kernels on the f32 master weights, whatever the
    job's dtype), whose variables are views of the trainer's parameter bucket; the counting is confusion.ConfusionMeter on
    the device.  Nothing the step reads is written, so the losses are bit-identical with and without the keys.  Labels
    >= num_outputs (255 = unlabelled) are ignored.  train.json gains ``validation``: a list of {step, epoch, confusion
    (row = truth, column = prediction), ignored, iou, dice, accuracy, mean_iou, seconds}; ms_per_step leaves the
    validation time out.  Single process only: with WORLD_SIZE > 1 the keys raise.
    """
    _refuse_volume_postprocess(params, 'SERVER_train')
    _refuse_volume_tta(params, options, 'SERVER_train')
    _refuse_blend(params, 'SERVER_train')
    if params.get('tile') is not None:
        return _train_frame_tiles(params, options)
    import torch
    from . import utils
    from .parallel import epoch_schedule
    from .weightmap import device_weightmaps

    want_val, validate_every = _validation_keys(params)
    device = _resolve_device(params, options)
    torch.cuda.set_device(torch.device(device))
    world, rank = int(os.environ.get('WORLD_SIZE', 1)), int(os.environ.get('RANK', 0))
    if world > 1:
        import torch.distributed as dist
        if not dist.is_initialized():
            os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
            backend = os.environ.get('SQ_DIST_BACKEND', 'nccl')    # 'gloo': two ranks on one card (tests)
            if backend == 'nccl':
                dist.init_process_group('nccl', device_id=torch.device(device))
            else:
                dist.init_process_group(backend)

    cfg_keys = ('name', 'shape', 'num_inputs', 'num_outputs', 'num_epochs', 'learning_rate', 'warm_start', 'dropout')
    config = utils.NetConfiguration.from_params({k: params[k] for k in cfg_keys if k in params})
    x = np.load(params['images'], mmap_mode='r', allow_pickle=False)
    if x.ndim == 3:
        x = x[..., np.newaxis]
    onehot = _onehot(np.load(params['labels'], allow_pickle=False), config.num_outputs)
    if params.get('weights'):
        wmap = np.load(params['weights'], allow_pickle=False).reshape(onehot.shape[:3] + (1,)).astype(np.float32)
    else:                                                      # EDT weight maps on the device, left in HBM
        fg = onehot[..., 1:].sum(-1)
        wmap = device_weightmaps(fg, params.get('w0', 10.), params.get('sigma', 5.), device=device)

    net_p = _net_params(params, device)
    net_p.setdefault('shape', tuple(x.shape[1:3]))
    trainer = _make_trainer(params, net_p, config)

    # Every rank must issue the SAME number of optimiser steps (each one is a gradient all-reduce), so the step count
    # comes from rank-independent quantities only and every step is a full batch: one seeded permutation of the whole
    # stack per epoch, cut into world x steps_per_epoch x batch indices; the remainder of the epoch is dropped.
    n_items = int(x.shape[0])
    order_fn, steps_per_epoch = epoch_schedule(n_items, int(params.get('batch_size', 16)), world)
    batch = order_fn.batch
    if order_fn.dropped:
        logger.info('{0} of {1} tiles are left out of every epoch ({2} ranks x {3} steps x batch {4}; a different '
                    'remainder each epoch)'.format(order_fn.dropped, n_items, world, steps_per_epoch, batch))
    epochs, total_steps = _step_budget(params, options, config, steps_per_epoch)

    per_tile = int(np.prod(x.shape[1:])) * 4 + int(np.prod(onehot.shape[1:])) + int(np.prod(onehot.shape[1:3])) * 4
    resident = n_items * per_tile <= float(params.get('resident_gib', 64)) * 2 ** 30
    dev = torch.device(device)
    if resident:                                               # the whole stack lives in HBM for the whole job
        x_dev = torch.from_numpy(np.array(x, dtype=np.float32, order='C')).to(dev)   # a copy: x is a read-only memmap
        y_dev = torch.from_numpy(np.ascontiguousarray(onehot)).to(dev)
        w_dev = wmap if isinstance(wmap, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(wmap)).to(dev)
    bufs = [torch.empty((batch,) + tuple(x.shape[1:]), dtype=torch.float32, device=dev),
            torch.empty((batch,) + tuple(onehot.shape[1:]), dtype=torch.uint8, device=dev),
            torch.empty((batch,) + tuple(onehot.shape[1:3]) + (1,), dtype=torch.float32, device=dev)]

    def begin_epoch(epoch):                                    # the epoch's permutation: on the host, and one index tensor
        order = order_fn(epoch, rank)
        return order, torch.from_numpy(np.ascontiguousarray(order)).to(dev) if resident else None

    def fill(state, s, bufs):
        """fill the step's static input buffers with the tiles of step s (device gather, or pinned staging)"""
        order, order_dev = state
        sl = slice(s * batch, (s + 1) * batch)
        sx, sy, sw = bufs
        if resident:
            idx = order_dev[sl]
            torch.index_select(x_dev, 0, idx, out=sx)
            torch.index_select(y_dev, 0, idx, out=sy)
            torch.index_select(w_dev, 0, idx, out=sw)
        else:
            ih = np.asarray(order[sl])                           # the permutation's own order: the same batch as the resident path
            sx.copy_(torch.from_numpy(np.ascontiguousarray(x[ih], dtype=np.float32)).pin_memory(), non_blocking=True)
            sy.copy_(torch.from_numpy(np.ascontiguousarray(onehot[ih])).pin_memory(), non_blocking=True)
            if isinstance(wmap, torch.Tensor):
                torch.index_select(wmap, 0, torch.from_numpy(ih).to(dev), out=sw)
            else:
                sw.copy_(torch.from_numpy(np.ascontiguousarray(wmap[ih])).pin_memory(), non_blocking=True)

    use_graph = bool(options.get('graph', True))
    validator = None
    if want_val:                                               # tiles and labels in the formats of `images` and `labels`
        vx = np.load(params['val_images'], mmap_mode='r', allow_pickle=False)
        if vx.ndim == 3:
            vx = vx[..., np.newaxis]
        vlab = np.load(params['val_labels'], allow_pickle=False)
        if tuple(vx.shape[1:]) != tuple(x.shape[1:]) or tuple(vlab.shape[:3]) != tuple(vx.shape[:3]):
            raise ValueError('val_images %s / val_labels %s do not match tiles of %s'
                             % (vx.shape, vlab.shape, tuple(x.shape[1:])))
        vx_dev = torch.from_numpy(np.array(vx, dtype=np.float32, order='C')).to(dev)
        vy = _onehot(vlab, config.num_outputs) if vlab.ndim == 4 else np.ascontiguousarray(vlab, dtype=np.uint8)
        vy_dev = torch.from_numpy(vy).to(dev)
        val_batch = int(params.get('val_batch', 32))

        def run_val(net, meter):                               # the tiles as SERVER_segment would segment them
            for i in range(0, vx_dev.shape[0], val_batch):
                meter.update(net.predict(vx_dev[i:i + val_batch]).contiguous(), vy_dev[i:i + val_batch])

        validator = _Validator(trainer, net_p, run_val, steps_per_epoch, validate_every, total_steps)
    run = _run_steps(trainer, bufs, epochs, steps_per_epoch, total_steps, begin_epoch, fill, use_graph, validator, dev)
    # replica check: data-parallel replicas apply the same all-reduced gradient to the same weights, so their
    # parameters must agree bit for bit; two f64 sums of the flat parameter bucket are compared across the ranks
    flat = trainer.pbucket.flat.double()
    chk = torch.stack([flat.sum(), flat.abs().sum()])
    check = {'param_checksum': [float(v) for v in chk.cpu()]}
    if world > 1:
        import torch.distributed as dist
        hi, lo = chk.clone(), chk.clone()
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        check['replicas_identical'] = bool(torch.equal(hi, lo))
        if not check['replicas_identical']:
            logger.error('data-parallel replicas have diverged: parameter checksums span {0} .. {1}'.format(
                [float(v) for v in lo.cpu()], [float(v) for v in hi.cpu()]))
    return _finish_training(params, config, trainer, validator, run, batch, {'tiles': n_items, 'resident': bool(resident)},
                            use_graph, str(net_p.get('dtype', 'f32')), device,
                            'Trained {steps} steps, loss {first_loss:.4f} -> {last_loss:.4f}, saved {model_dir}',
                            after=check, world=world, rank=rank)


def _train_volume_bricks(params, options):
    """SERVER_train_volume with params['brick']: stacks of any size stay raw in HBM, every step's batch of augmented
    bricks is cut there (frontend.sample_plan, VolumeSampler)."""
    import torch
    from . import utils
    from .frontend import NP_TORCH, VolumeSampler, sample_plan, volume_bricks, volume_stats
    from .networks.unet import UNet3DTrain

    wm_kind = params.get('weightmap', 'uniform')
    wm_w0, wm_sigma, wm_spacing = float(params.get('w0', 10.)), float(params.get('sigma', 5.)), float(params.get('spacing', 1.))
    if len(tuple(params['brick'])) != 3:
        raise ValueError("params['brick'] must be (X, Y, Z), got %r" % (params['brick'],))
    bx, by, bz = (int(s) for s in params['brick'])
    x = np.load(params['images'], mmap_mode='r', allow_pickle=False)
    if x.ndim == 5 and x.shape[4] == 1:
        x = x[..., 0]
    if x.ndim != 4 or int(params.get('num_inputs', 1)) != 1:
        raise ValueError("params['brick'] trains on single-channel (N, slices, width, height) stacks only, got shape %s" % (x.shape,))
    if np.dtype(x.dtype) not in NP_TORCH:
        raise TypeError("with params['brick'] the images must be uint8, uint16 or float32, got %s" % x.dtype)
    N, Z, X, Y = (int(s) for s in x.shape)
    augment = params.get('augment')
    augment = (('flip', 'rot90') if bx == by else ('flip',)) if augment is None else \
        ((augment,) if isinstance(augment, str) else tuple(augment))
    seed = int(params.get('seed', 0))
    rng = np.random.default_rng(seed)
    sample_plan((Z, X, Y), (bz, bx, by), N, 1, np.random.default_rng(0), augment)     # refuses a bad `augment` before any upload
    samples = params.get('samples_per_epoch')
    samples = N * volume_bricks((Z, X, Y), (bz, bx, by), 0).per_volume if samples is None else int(samples)
    if samples < 1:
        raise ValueError('samples_per_epoch must be positive, got %d' % samples)

    cfg_keys = ('name', 'num_outputs', 'num_epochs', 'learning_rate', 'warm_start', 'dropout')
    cfg = {k: params[k] for k in cfg_keys if k in params}
    cfg['shape'], cfg['num_inputs'] = (bx, by, bz), 1          # net.config records the brick: SERVER_segment_volume's `brick`
    config = utils.NetConfiguration.from_params(cfg)
    n_out = int(config.num_outputs)
    labels = np.load(params['labels'], mmap_mode='r', allow_pickle=False)
    if labels.ndim == 5:
        labels = labels[..., :n_out]
    if labels.ndim not in (4, 5) or tuple(labels.shape[:4]) != (N, Z, X, Y):
        raise ValueError('labels %s do not match the images %s' % (labels.shape, x.shape))

    device = _resolve_device(params, options)
    torch.cuda.set_device(torch.device(device))
    dev = torch.device(device)

    x_dev = _upload_rows(x, (N, Z, X, Y), x.dtype, dev)
    index_labels = labels.ndim == 4                             # class indices stay at one byte per voxel
    y_dev = _upload_rows(labels, (N, Z, X, Y) if index_labels else (N, Z, X, Y, n_out), np.uint8, dev)
    if params.get('weights'):
        w_dev = _upload_rows(np.load(params['weights'], mmap_mode='r', allow_pickle=False).reshape((N, Z, X, Y)),
                             (N, Z, X, Y, 1), np.float32, dev)
    elif wm_kind == 'edt':
        # once, on the whole volumes: crop and symmetry commute with the map (the spacing is along z, which no op mixes
        # with x or y)
        from .weightmap import device_weightmaps3d
        fg = y_dev if index_labels else y_dev[..., 1:].sum(-1)
        if N * Z * X * Y < (1 << 31):
            w_dev = device_weightmaps3d(fg, wm_w0, wm_sigma, wm_spacing)
        else:
            w_dev = torch.empty((N, Z, X, Y, 1), dtype=torch.float32, device=dev)
            for i in range(N):
                w_dev[i:i + 1] = device_weightmaps3d(fg[i:i + 1], wm_w0, wm_sigma, wm_spacing)
        del fg
    else:
        w_dev = torch.ones((N, Z, X, Y, 1), dtype=torch.float32, device=dev)    # resident, so padding still gets weight 0
    normalise = bool(params.get('normalise', True))
    stats = volume_stats(x_dev) if normalise else None          # ImageNorm of each WHOLE volume, as segment_volumes applies it

    net_p = _net_params(params, device)
    net_p['shape'] = (bx, by, bz)
    net_p['num_inputs'], net_p['num_outputs'] = 1, n_out
    trainer = _make_trainer(params, net_p, config, UNet3DTrain)

    batch = max(1, min(int(params.get('batch_size', 1)), samples))
    steps_per_epoch = samples // batch
    epochs, total_steps = _step_budget(params, options, config, steps_per_epoch)
    sampler = VolumeSampler((Z, X, Y), (bz, bx, by), dev)
    bufs = [torch.empty((batch, bz, bx, by, 1), dtype=torch.float32, device=dev),
            torch.empty((batch, bz, bx, by, n_out), dtype=torch.uint8, device=dev),
            torch.empty((batch, bz, bx, by, 1), dtype=torch.float32, device=dev)]

    def begin_epoch(epoch):                                    # ONE plan upload per epoch; a step takes a slice of it
        return torch.from_numpy(sample_plan((Z, X, Y), (bz, bx, by), N, samples, rng, augment)).to(dev)

    def fill(plan, s, bufs):
        rows = plan[s * batch:(s + 1) * batch]
        sampler.images(x_dev, rows, normalise=normalise, stats=stats, out=bufs[0])
        if index_labels:
            sampler.onehot(y_dev, n_out, rows, out=bufs[1])
        else:
            sampler.copy(y_dev, rows, out=bufs[1])
        sampler.copy(w_dev, rows, out=bufs[2])

    run = _run_steps(trainer, bufs, epochs, steps_per_epoch, total_steps, begin_epoch, fill, False, None, dev)
    edt = wm_kind == 'edt' and not params.get('weights')
    return _finish_training(
        params, config, trainer, None, run, batch,
        {'volumes': N, 'shape': [Z, X, Y], 'brick': [bx, by, bz], 'augment': list(augment), 'samples_per_epoch': samples,
         'seed': seed, 'normalise': normalise}, False, 'f32', device,
        'Trained {steps} steps on bricks of volumes, loss {first_loss} -> {last_loss}, saved {model_dir}',
        after=dict(weightmap='edt', w0=wm_w0, sigma=wm_sigma, spacing=wm_spacing) if edt else None)


def SERVER_train_volume(params, options):
    """Train the volumetric U-Net (UNet3DTrain, f32) on a stack of volumes with the weighted softmax cross-entropy.

    params: images (.npy (N, slices, width, height[, C]) float), labels (.npy (N, slices, width, height) class indices,
    or one-hot with a trailing class axis), weights (.npy, one value per voxel; absent: what `weightmap` says),
    weightmap ('uniform', the default: a weight of 1 everywhere | 'edt': ImageWeightMap(w0, sigma),
    sequitr/pipeline.py:455-479, of the foreground volume -- the 3-D Euclidean transform with the depth axis scaled by
    `spacing`, the slice spacing in in-plane pixels -- computed once on the GPU, sq_weightmap3d_edt_f32, and kept there),
    w0 (10), sigma (5), spacing (1), the NetConfiguration keys (name, shape = (width, height, slices),
    num_outputs, learning_rate, num_epochs, dropout, filters, bridge, batch_norm, warm_start ...), batch_size (default
    1), warmup_steps.  Learning-rate defaults are the trainer's (train.DEFAULT_LEARNING_RATE ramped over
    train.DEFAULT_WARMUP_STEPS), as in SERVER_train.  options: gpu, max_steps.

    Single process, eager steps: the volumes, labels and weights are uploaded once, a batch is an index_select into the
    step's three input buffers.  The loop is _run_steps, SERVER_train's (there: what ms_per_step leaves out and when the
    losses are read back); both paths here run it without capture and without validation.  Writes
    ``weights.npz`` + ``net.config`` into the next numbered folder of MODELDIR/<name>/ and ``train.json`` (losses,
    ms_per_step) into params['output'].  The model loads strictly into UNet3D (SERVER_segment_volume's ``model``).

    With params['brick'] = (X, Y, Z), the network's `shape` convention, the job trains on stacks of any size: the network is
    built at the brick shape, `images` is a raw (N, slices, width, height) uint8 / uint16 / float32 single-channel stack
    that is uploaded as it is and stays raw in HBM, class-index labels stay at one byte per voxel, the weight map (from
    `weights`, 'edt' computed once on the whole volumes, or 'uniform' = ones) is resident, and every step's batch of bricks
    is cut on the GPU at random origins under a random exact symmetry (frontend.sample_plan, VolumeSampler): ImageSample,
    ImageFlip and the quarter turns of ImageRotate, with ImageNorm (params['normalise'], default True) from the statistics
    of each whole volume, as SERVER_segment_volume applies it.  Where a brick leaves a volume shorter than it, the image is
    0 and the weight 0.  params: augment (a subset of ('flip', 'rot90'); default both, 'flip' alone when the brick is not
    square in the plane), samples_per_epoch (default: the number of bricks that tile the stack), seed (the plan's and the
    network's).  Each epoch's plan is drawn on the host and uploaded once.  ``train.json`` gains ``brick``, ``augment``,
    ``samples_per_epoch``, ``seed``; net.config's ``shape`` is the brick, so the model loads into SERVER_segment_volume
    with the same ``brick``.
    """
    _refuse_volume_postprocess(params, 'SERVER_train_volume')
    _refuse_volume_tta(params, options, 'SERVER_train_volume')
    _refuse_blend(params, 'SERVER_train_volume')
    import torch
    from . import utils
    from .networks.unet import UNet3DTrain

    if int(os.environ.get('WORLD_SIZE', 1)) > 1:
        raise RuntimeError('SERVER_train_volume runs in a single process (data-parallel volume training does not exist)')
    wm_kind = params.get('weightmap', 'uniform')
    if wm_kind not in ('uniform', 'edt'):
        raise ValueError("weightmap must be 'uniform' or 'edt', got %r" % (wm_kind,))
    if params.get('brick') is not None:
        return _train_volume_bricks(params, options)
    wm_w0, wm_sigma, wm_spacing = float(params.get('w0', 10.)), float(params.get('sigma', 5.)), float(params.get('spacing', 1.))
    device = _resolve_device(params, options)
    torch.cuda.set_device(torch.device(device))
    dev = torch.device(device)
    x = np.load(params['images'], mmap_mode='r', allow_pickle=False)
    if x.ndim == 4:
        x = x[..., np.newaxis]
    if x.ndim != 5:
        raise ValueError('images must be (N, slices, width, height[, C]), got shape %s' % (x.shape,))
    N, Z, X, Y, C = x.shape
    cfg_keys = ('name', 'shape', 'num_inputs', 'num_outputs', 'num_epochs', 'learning_rate', 'warm_start', 'dropout')
    cfg = {k: params[k] for k in cfg_keys if k in params}
    cfg.setdefault('shape', (X, Y, Z))
    cfg.setdefault('num_inputs', int(C))
    config = utils.NetConfiguration.from_params(cfg)
    labels = np.load(params['labels'], allow_pickle=False)
    onehot = _onehot(labels, config.num_outputs, spatial=3)
    if tuple(onehot.shape[:4]) != (N, Z, X, Y):
        raise ValueError('labels %s do not match the images %s' % (labels.shape, x.shape))
    if params.get('weights'):
        wmap = np.load(params['weights'], allow_pickle=False).reshape((N, Z, X, Y, 1)).astype(np.float32)
    elif wm_kind == 'edt':                                     # volumetric EDT weight maps on the device, left in HBM
        from .weightmap import device_weightmaps3d
        wmap = device_weightmaps3d(onehot[..., 1:].sum(-1), wm_w0, wm_sigma, wm_spacing, device=device)
    else:
        wmap = np.ones((N, Z, X, Y, 1), np.float32)

    net_p = _net_params(params, device)
    net_p['shape'] = tuple(config.shape)
    net_p['num_inputs'], net_p['num_outputs'] = int(config.num_inputs), int(config.num_outputs)
    trainer = _make_trainer(params, net_p, config, UNet3DTrain)

    batch = max(1, min(int(params.get('batch_size', 1)), N))
    steps_per_epoch = N // batch
    epochs, total_steps = _step_budget(params, options, config, steps_per_epoch)
    x_dev = torch.from_numpy(np.array(x, dtype=np.float32, order='C')).to(dev)
    y_dev = torch.from_numpy(np.ascontiguousarray(onehot)).to(dev)
    w_dev = wmap if isinstance(wmap, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(wmap)).to(dev)
    bufs = [torch.empty((batch,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev) for t in (x_dev, y_dev, w_dev)]
    rng = np.random.default_rng(int(params.get('seed', 0)))

    def begin_epoch(epoch):                                    # the epoch's permutation, one index tensor
        return torch.from_numpy(rng.permutation(N)).to(dev)

    def fill(order, s, bufs):
        idx = order[s * batch:(s + 1) * batch]
        for t, out in zip((x_dev, y_dev, w_dev), bufs):
            torch.index_select(t, 0, idx, out=out)

    run = _run_steps(trainer, bufs, epochs, steps_per_epoch, total_steps, begin_epoch, fill, False, None, dev)
    edt = wm_kind == 'edt' and not params.get('weights')
    return _finish_training(params, config, trainer, None, run, batch,
                            {'volumes': int(N), 'shape': [int(Z), int(X), int(Y)]}, False, 'f32', device,
                            'Trained {steps} steps on volumes, loss {first_loss} -> {last_loss}, saved {model_dir}',
                            after=dict(weightmap='edt', w0=wm_w0, sigma=wm_sigma, spacing=wm_spacing) if edt else None)


GAN_KEYS = ('num_outputs', 'batch_size', 'repeat_batch', 'num_levels', 'num_epochs_per_level', 'start_size', 'learning_rate',
            'seed', 'dtype', 'batch_d', 'hbm_budget')


def SERVER_train_gan(params, options):
    """Train the progressive WGAN-GP (networks.gan.GenerativeAdverserialNetwork) on a stack of real images that stays in HBM.

    params: training_data (.npy (N, H, W, C) raw uint8 / uint16 stack, C equal to num_outputs), output (the folder the
    per-level checkpoints ``model_(HxW).npz``, ``export/`` and ``train.json`` go to), crop ((CH, CW), default (512, 512)
    clipped to the image: every step's batch is one GanSampler launch -- per-channel normalisation by each image's own
    moments, a random crop, two random mirrors, the bilinear resize to the level's size; the reference's input pipeline,
    sequitr/networks/gan.py:347-407), and the network's keys: num_outputs, batch_size, repeat_batch, num_levels,
    num_epochs_per_level, start_size, learning_rate, seed, dtype ('f32' | 'bf16' | 'mixed'), batch_d, hbm_budget.
    options: gpu, max_steps (the most steps per fade / stabilisation phase: train(max_steps_per_phase=)), graph (default
    True: the iterations replay as hipGraphs).

    Single process.  After the last level the highest checkpoint is exported with convert_checkpoint_to_model().  Returns
    (and writes to ``train.json``) levels, sizes, steps, d_loss and g_loss of the last discriminator step, graph, dtype,
    crop, images, seconds, export_dir."""
    _refuse_volume_postprocess(params, 'SERVER_train_gan')
    _refuse_volume_tta(params, options, 'SERVER_train_gan')
    _refuse_blend(params, 'SERVER_train_gan')
    import torch
    from .networks import gan

    if int(os.environ.get('WORLD_SIZE', 1)) > 1:
        raise RuntimeError('SERVER_train_gan runs in a single process')
    fn = params.get('training_data')
    if not (isinstance(fn, str) and fn.endswith('.npy')):
        raise ValueError("params['training_data'] must be a .npy stack (N, H, W, C), got %r" % (fn,))
    if not params.get('output'):
        raise ValueError("params['output'] must name the folder for the checkpoints")
    x = np.load(fn, mmap_mode='r', allow_pickle=False)
    if x.ndim != 4:
        raise ValueError('training_data must be (N, H, W, C), got shape %s' % (x.shape,))
    N, H, W, C = (int(v) for v in x.shape)
    n_out = int(params.get('num_outputs', 2))
    if C != n_out:
        raise ValueError('training_data has %d channels, the network (num_outputs) %d' % (C, n_out))
    crop = tuple(int(c) for c in params.get('crop', (512, 512)))
    if len(crop) != 2 or min(crop) < 1:
        raise ValueError("params['crop'] must be a (CH, CW) pair of positive sizes, got %r" % (params.get('crop'),))
    crop = (min(crop[0], H), min(crop[1], W))
    del x

    device = _resolve_device(params, options)
    torch.cuda.set_device(torch.device(device))
    p = {k: params[k] for k in GAN_KEYS if k in params}
    p.update(training_data=fn, crop=crop, device=device, output=params['output'], num_outputs=n_out,
             graph=bool(options.get('graph', True)))
    t_start = time.time()
    net = gan.GenerativeAdverserialNetwork(p, gan.TRAIN)
    net.build()
    net.train(max_steps_per_phase=options.get('max_steps'))
    torch.cuda.synchronize()
    seconds = time.time() - t_start
    d_loss, g_loss = net.last_losses
    export_dir = net.convert_checkpoint_to_model()
    info = {'levels': int(net.num_levels), 'sizes': [list(net.get_size(n)) for n in range(net.num_levels)],
            'steps': int(net.global_step), 'd_loss': d_loss, 'g_loss': g_loss, 'graph': bool(net.use_graph),
            'dtype': str(net.dtype), 'crop': list(crop), 'images': N, 'image_shape': [H, W, C], 'batch_size': int(net.batch_size),
            'seed': int(net.seed), 'seconds': seconds, 'device': device, 'export_dir': export_dir}
    with open(os.path.join(params['output'], 'train.json'), 'w') as f:
        json.dump(info, f, indent=2)
    logger.info('Trained the GAN for {steps} iterations over {levels} levels, losses D {d_loss:.4f} G {g_loss:.4f}, '
                'exported {export_dir}'.format(**info))
    return info
