"""Query network and database network embedded TOGETHER (inference).

The reference calls the two models one after the other (`modelq(data_dict, 'q')`, `model(data_dict, 'db')`:
train.py:308,316; test.py:128,161; datasets_ws_nuscenes.py:1220-1227).  Both are ResNet trunks of one architecture
by default (tools/options.py:85-104), so each layer's convolution exists twice per step with different weights and
very different sizes: a 6-camera panorama is six aerial tiles' worth of pixels.  On MI355X the small launches are the
expensive ones (a 3x3 conv over 64 aerial tiles fills a third of the chip for one wave of workgroups), so
`embed_pair` advances the two trunks in lock-step and issues every layer as ONE grouped launch
(resnet.forward_maps_multi -> agp_conv2d_fwd_grouped); everything behind the trunks is the models' own forward.
Outputs are bit-identical to calling the two models separately (tests/test_gpu_models.py).
ConvNeXt models (mm_imgfe = dbimage_fe = 'convnext_tiny') pair behind Options.convnext_pair: their trunks are 15 small launches each
for '2_2_2', and the lock-step form issues every stem / depthwise + LayerNorm / MLP / downsample step as one grouped launch
(convnext.ConvNeXt.forward_maps_multi -> agp_cnx_*_fwd_grouped; tests/test_gpu_convnext_pair.py).
"""
import torch


from . import convnext, ops, range_guard, resnet

RIDER = True      # False: the database head as a launch of its own behind the query network's tail


def can_pair(modelq, modeldb, qdata, dbdata):
    if modelq.training or modeldb.training or torch.is_grad_enabled():
        return False
    fq, fdbs = modelq.image_fe.fe, [m.fe for m in modeldb.dbimage_fes]
    db_map = dbdata['db_map']
    nmap = db_map.shape[-4]                     # [..., nmap, 3, h, w] and uint8 [..., nmap, h, w, 3] alike
    cnx = [isinstance(f, convnext.ConvNeXt) for f in [fq] + fdbs[:max(nmap, 1)]]
    if any(cnx):                                # ConvNeXt trunks pair among themselves only, and only with Options.convnext_pair
        return all(cnx) and _can_pair_convnext(modelq, modeldb, fq, fdbs, qdata, db_map, nmap)
    if modelq.opt.mfma_precision != modeldb.opt.mfma_precision or db_map.dim() not in (5, 6):
        return False
    if modeldb.opt.share_dbfe is True and nmap > 1:
        return False
    return all((f.fe_type, f.nstages) == (fq.fe_type, fq.nstages) for f in fdbs[:nmap])


def _can_pair_convnext(modelq, modeldb, fq, fdbs, qdata, db_map, nmap):
    """The ConvNeXt rule of can_pair (every trunk is a ConvNeXt; eval under no_grad already holds): Options.convnext_pair on in BOTH
    models, the same three block counts and precision in every trunk, at most convnext.MAX_GROUPS trunks, `db_map` 5-D or 6-D, the
    share_dbfe / nmap rule of the ResNet pair, uint8 inputs only where Options.convnext_u8 enabled them, and NO ConvNeXt range-guard
    tag binding on either model: the grouped launches have no guarded twins, so a guarded pair runs the separate forwards, in which
    each model guards itself."""
    if not (modelq.opt.convnext_pair and modeldb.opt.convnext_pair) or db_map.dim() not in (5, 6):
        return False
    if (modeldb.opt.share_dbfe is True and nmap > 1) or not 1 <= nmap <= len(fdbs) or 1 + nmap > convnext.MAX_GROUPS:
        return False
    trunks = [fq] + fdbs[:nmap]
    if any((f.block_counts(), f.precision) != (fq.block_counts(), fq.precision) or f.takes_training_path() for f in trunks):
        return False
    if range_guard.cnx_tag(modelq.opt, fq.precision, modelq.opt.mfma_precision) is not None \
            or range_guard.cnx_tag(modeldb.opt, fdbs[0].precision) is not None:
        return False
    img = qdata.get('query_image')
    if (torch.is_tensor(img) and img.dtype == torch.uint8 and not fq._u8_enabled) \
            or (db_map.dtype == torch.uint8 and not all(f._u8_enabled for f in fdbs[:nmap])):
        return False                           # (the separate forwards refuse such an input by name)
    return True


def _resized_tiles(modelq, modeldb, qdata, dbdata):
    """Decoded frames (`query_frames` / `db_frames`) -> the resized uint8 tiles under `query_image` / `db_map`, which the pair
    then embeds as it always has: one launch of the camera front end's uint8 mode per key (ops.resize_cameras_u8), bit-identical
    to the fused resize + pack of the separate forwards (tests/test_gpu_camera.py).  The database frames are centre-cropped
    (opt.db_cropsize) in that launch; `query_jitter` / `db_jitter` records jitter the tiles (ops.jitter_cameras_u8)."""
    if 'query_jitter' in qdata and 'query_frames' not in qdata:
        raise ValueError("embed_pair: `query_jitter` (colour jitter records) needs `query_frames`")
    if 'db_jitter' in dbdata and 'db_frames' not in dbdata:
        raise ValueError("embed_pair: `db_jitter` (colour jitter records) needs `db_frames`")
    if 'query_frames' in qdata:
        if 'query_image' in qdata:
            raise ValueError("embed_pair: pass `query_frames` or `query_image`, not both")
        f = qdata['query_frames']
        if not torch.is_tensor(f) or f.dtype != torch.uint8 or f.dim() != 5 or f.shape[-1] != 3:
            raise ValueError("embed_pair: `query_frames` must be uint8 [b, ncam, H0, W0, 3]")
        t = ops.resize_cameras_u8(f, modelq.opt.q_resize)
        if 'query_jitter' in qdata:
            t = ops.jitter_cameras_u8(t, qdata['query_jitter'])
        qdata = {k: v for k, v in qdata.items() if k not in ('query_frames', 'query_jitter')}
        qdata['query_image'] = t
    if 'db_frames' in dbdata:
        if 'db_map' in dbdata:
            raise ValueError("embed_pair: pass `db_frames` or `db_map`, not both")
        f = dbdata['db_frames']
        if not torch.is_tensor(f) or f.dtype != torch.uint8 or f.dim() not in (5, 6) or f.shape[-1] != 3:
            raise ValueError("embed_pair: `db_frames` must be uint8 [b,nmap,H0,W0,3] or [b,ndb,nmap,H0,W0,3]")
        # (the records of `db_jitter` are in the frames' memory order)
        t = ops.resize_cameras_u8(f.reshape(-1, *f.shape[-4:]), modeldb.opt.db_resize, crop=modeldb.opt.db_cropsize)
        if 'db_jitter' in dbdata:
            t = ops.jitter_cameras_u8(t, dbdata['db_jitter'])
        dbdata = {k: v for k, v in dbdata.items() if k not in ('db_frames', 'db_jitter')}
        dbdata['db_map'] = t.view(*f.shape[:-3], *t.shape[-3:])
    return qdata, dbdata


def embed_pair(modelq, modeldb, qdata, dbdata):
    """(modelq(qdata, 'q'), modeldb(dbdata, 'db')) with the image trunks run in lock-step.  Falls back to the two
    separate forwards when the models cannot be paired (training, different trunk architectures).
    Decoded frames (`query_frames`, `db_frames`) are resized to uint8 tiles first (_resized_tiles) and continue as tiles.
    fp16 range guard (Options.fp16_range_guard): the lock-step trunks of BOTH models report through the query model's word when
    its guard is on (else the database model's): a saturated database tile then shows in modelq.fp16_range_ok() /
    poll_fp16_range(), whose message names the database trunks as a possible source.
    ConvNeXt models (Options.convnext_pair on in the ConvNeXt models, else refused): lock-step through ConvNeXt.forward_maps_multi
    when _can_pair_convnext holds -- one grouped launch per stem / depthwise + LayerNorm / MLP / downsample step over the query
    trunk and the map-type trunks, bit-identical to the separate forwards -- and the two separate forwards otherwise (a ResNet on
    the other side, unequal block counts or precisions, more than four trunks, or a ConvNeXt range-guard tag binding on either
    model: each model then guards itself as always, a guard is never skipped).  Everything behind the trunks, each model's
    fp16_range_guard binding included, is the model's own forward.  query_substreams > 1 is refused for a ConvNeXt query model."""
    cnx_db = any(getattr(e, "fe_type", None) == "convnext_tiny" for e in getattr(modeldb, "dbimage_fes", ()))
    cnx_q = getattr(modelq, "_convnext", False)
    if cnx_db and not modeldb.opt.convnext_pair:
        raise NotImplementedError("pair.embed_pair with a ConvNeXt database model (dbimage_fe='convnext_tiny') is not built; call "
                                  "modelq(qdata, 'q') and modeldb(dbdata, 'db') separately")
    if cnx_q and not modelq.opt.convnext_pair:
        raise NotImplementedError("pair.embed_pair with a ConvNeXt query model (mm_imgfe='convnext_tiny') is not built; call "
                                  "modelq(qdata, 'q') and modeldb(dbdata, 'db') separately")
    if cnx_q or cnx_db:
        return _embed_pair_convnext(modelq, modeldb, qdata, dbdata, cnx_q, cnx_db)
    qdata, dbdata = _resized_tiles(modelq, modeldb, qdata, dbdata)
    if not can_pair(modelq, modeldb, qdata, dbdata):
        return modelq(qdata, mode='q'), modeldb(dbdata, mode='db')
    # the fp16 range guard: the grouped trunk launches below run outside either model's forward and hold BOTH models' image trunks
    # -- they report through the query model's word when its guard is on, else the database model's (each model's forward then
    # binds and publishes its own word for the rest of its work); the report names the other model's trunks as a possible source
    for m, other in ((modelq, modeldb), (modeldb, modelq)):
        if range_guard.active(m.opt, m.opt.mfma_precision, False):
            g = range_guard.guard_of(m)
            g.also.add(f"the {type(other).__name__} image trunks run in lock-step with this model's (agplace_amd.pair.embed_pair)")
            with g.bind(range_guard.model_device(m)):
                return _embed_pair_dispatch(modelq, modeldb, qdata, dbdata)
    return _embed_pair_dispatch(modelq, modeldb, qdata, dbdata)


def _embed_pair_convnext(modelq, modeldb, qdata, dbdata, cnx_q, cnx_db):
    """embed_pair with a ConvNeXt model on at least one side (Options.convnext_pair on in every ConvNeXt model)."""
    if cnx_q and modelq.opt.query_substreams > 1:
        raise NotImplementedError("pair.embed_pair with a ConvNeXt query model (mm_imgfe='convnext_tiny') and Options.query_substreams "
                                  f"= {modelq.opt.query_substreams}: row-sliced outputs are not built for this trunk; set "
                                  "query_substreams = 1")
    separate = lambda: (modelq(qdata, mode='q'), modeldb(dbdata, mode='db'))
    # decoded frames become uint8 tiles, which a ConvNeXt model takes only with Options.convnext_u8: without it the model's own
    # forward refuses the frames by name
    if cnx_q and not modelq.image_fe.fe._u8_enabled and ('query_frames' in qdata or 'query_jitter' in qdata):
        return separate()
    if cnx_db and not all(e.fe._u8_enabled for e in modeldb.dbimage_fes) and ('db_frames' in dbdata or 'db_jitter' in dbdata):
        return separate()
    qdata, dbdata = _resized_tiles(modelq, modeldb, qdata, dbdata)
    if not (cnx_q and cnx_db) or not can_pair(modelq, modeldb, qdata, dbdata):
        return modelq(qdata, mode='q'), modeldb(dbdata, mode='db')
    image = modelq.query_image(qdata)
    db_map = dbdata['db_map']
    u8 = db_map.dtype == torch.uint8            # decoded tiles [b,(ndb,)nmap,h,w,3]: normalised by the stem as it reads
    if db_map.dim() == 5:
        db_map = db_map.unsqueeze(1)
    nets, xs = [modelq.image_fe.fe], [image]
    nmap = db_map.shape[2]
    for i in range(nmap):
        nets.append(modeldb.dbimage_fes[i].fe)
        if u8:
            bb, ndb, _, h, w, _ = db_map.shape
            xs.append(db_map[:, :, i].reshape(bb * ndb, 1, h, w, 3))
        else:
            bb, ndb, _, c, h, w = db_map.shape
            xs.append(db_map[:, :, i].reshape(bb * ndb, c, h, w).float())
    maps = convnext.ConvNeXt.forward_maps_multi(nets, xs)
    out_db = modeldb.forward_db(dbdata, trunk_maps={i: (maps[1 + i], None) for i in range(nmap)})
    out_q = modelq.forward_q(qdata, image_maps=maps[0])
    return out_q, out_db


def _embed_pair_dispatch(modelq, modeldb, qdata, dbdata):
    k = modelq.opt.query_substreams
    img = qdata['query_image']
    db_map = dbdata['db_map']
    b = img.shape[0]
    if k > 1 and 'coords' not in qdata and 'points' not in qdata and b % k == 0 and b >= 2 * k and db_map.shape[0] % k == 0:
        return _embed_pair_substreams(modelq, modeldb, qdata, dbdata, k)
    return _embed_pair_one(modelq, modeldb, qdata, dbdata)


def _embed_pair_one(modelq, modeldb, qdata, dbdata, q_rows=None, db_rows=None):
    opt = modelq.opt
    prec = opt.mfma_precision
    image = modelq.query_image(qdata)
    db_map = dbdata['db_map']
    u8 = db_map.dtype == torch.uint8            # decoded tiles [b,(ndb,)nmap,h,w,3]: normalised on the device (DBVanilla2D.forward_db)
    if db_map.dim() == 5:
        db_map = db_map.unsqueeze(1)
    nets, xs, lms, fps = [modelq.image_fe.fe], [image], [[]], [modelq.final_pool_request()]
    nmap = db_map.shape[2]
    for i in range(nmap):
        nets.append(modeldb.dbimage_fes[i].fe)
        if u8:
            bb, ndb, _, h, w, _ = db_map.shape
            xs.append(db_map[:, :, i].reshape(bb * ndb, 1, h, w, 3))
        else:
            bb, ndb, _, c, h, w = db_map.shape
            xs.append(db_map[:, :, i].reshape(bb * ndb, c, h, w))
        lms.append(None)
        fps.append(modeldb.final_pool_request(i))
    maps = resnet.forward_maps_multi(nets, xs, prec=prec, level_means=lms, final_pools=fps)
    # the database network's head (one small vector program) rides in the launch of the query network's first program instead of
    # following the query network's tail on the stream: both are latency chains on a handful of CUs
    head = [] if RIDER else None
    out_db = modeldb.forward_db(dbdata, trunk_maps={i: (maps[1 + i], fps[1 + i]) for i in range(nmap)}, out_rows=db_rows,
                                defer_head=head)
    out_q = modelq.forward_q(qdata, image_maps=(maps[0], lms[0], fps[0]), out_rows=q_rows, rider=head)
    if head:
        head.pop().run()                    # not taken along (per-op query path, or the two programs do not fit one launch)
    return out_q, out_db


def _slice(d, b, lo, hi):
    out = {}
    for name, v in d.items():
        if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == b:
            out[name] = v[lo:hi]
        elif isinstance(v, (list, tuple)) and all(torch.is_tensor(t) and t.shape[0] == b for t in v):
            out[name] = [t[lo:hi] for t in v]
        else:
            out[name] = v
    return out


def _embed_pair_substreams(modelq, modeldb, qdata, dbdata, k):
    """The pairs as k sub-batches on k HIP streams (the caller's + k-1 owned by the query module, as in
    MM._forward_q_substreams): one sub-batch's fusion tail (a latency-bound chain of small launches) runs under the
    other sub-batches' convolutions.  Same arithmetic per sample."""
    dev = qdata['query_image'].device
    cur = torch.cuda.current_stream(dev)
    key = (str(dev), k, cur.cuda_stream)
    pool = modelq.__dict__.setdefault('_substream_pool', {})
    if key not in pool:
        pool[key] = [torch.cuda.Stream(device=dev) for _ in range(k - 1)]
    streams = pool[key]
    bq, bd = qdata['query_image'].shape[0], dbdata['db_map'].shape[0]
    hq, hd = bq // k, bd // k
    outs = [None] * k
    # whole-batch outputs: every sub-batch writes its row slice, nothing is concatenated afterwards
    D = modelq.opt.mm_stg2fuse_dim
    fq = {name: torch.empty((bq, D), dtype=torch.float32, device=dev) for name in modelq.OUT_KEYS}
    dbm = dbdata['db_map']
    ndb = dbm.shape[1] if dbm.dim() == 6 else 1
    fd = torch.empty((bd * ndb, 256), dtype=torch.float32, device=dev)

    def one(i):
        return _embed_pair_one(modelq, modeldb, _slice(qdata, bq, i * hq, (i + 1) * hq), _slice(dbdata, bd, i * hd, (i + 1) * hd),
                               q_rows={name: t[i * hq:(i + 1) * hq] for name, t in fq.items()},
                               db_rows=fd[i * hd * ndb:(i + 1) * hd * ndb])
    for i, st in enumerate(streams):
        st.wait_stream(cur)
        with torch.cuda.stream(st):
            outs[i + 1] = one(i + 1)
    outs[0] = one(0)
    for i, st in enumerate(streams):
        cur.wait_stream(st)
        for o in outs[i + 1]:
            for t in o.values():
                t.record_stream(cur)
    for t in list(fq.values()) + [fd]:
        for st in streams:
            t.record_stream(st)
    from . import ops
    out_q = {name: ops.join_rows([o[0][name] for o in outs]) for name in outs[0][0]}
    out_db = {name: ops.join_rows([o[1][name] for o in outs]) for name in outs[0][1]}
    return out_q, out_db


class CapturedPair:
    """`embed_pair` captured into a hipGraph on a stream of its own (static input tensors: refill them in place between replays).

    replay() enqueues one replay and -- every `poll_every` replays -- looks at the query model's voxel-range mirror in pinned host
    memory (MM.poll_voxel_range: no stream is synchronised) and raises ValueError when an earlier replay embedded a cloud outside
    the device-side coordinate manager's limits; finish() waits for the stream and checks the replays the polls could not have
    seen yet.  Without `coords` in qdata the polls are no-ops.

    Map exponents (agplace_amd/map_exponents.py) only change host-prepared buffers (folded scale / shift, projection planes, the
    pools' eps and 2^e factors), all read at capture time: a graph captured AFTER set_exponents / calibrate replays them;
    changing the exponents afterwards invalidates the capture exactly like a weight reload does -- capture again."""

    def __init__(self, modelq, modeldb, qdata, dbdata, stream=None, warmup=2, poll_every=8):
        dev = (qdata['query_frames'] if 'query_frames' in qdata else qdata['query_image']).device
        self.modelq, self.modeldb, self.qdata, self.dbdata = modelq, modeldb, qdata, dbdata
        self.stream = stream if stream is not None else torch.cuda.Stream(device=dev)
        self.poll_every, self._n = max(1, int(poll_every)), 0
        self.stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(self.stream):
            for _ in range(warmup):             # workspaces and weight planes are built outside the capture
                embed_pair(modelq, modeldb, qdata, dbdata)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=self.stream, capture_error_mode="thread_local"):
            self.out_q, self.out_db = embed_pair(modelq, modeldb, qdata, dbdata)

    def replay(self):
        self._n += 1
        if self._n % self.poll_every == 0:
            self.modelq.poll_voxel_range()
            self.modelq.poll_fp16_range()
            self.modeldb.poll_fp16_range()
        # what the caller's stream has enqueued so far (the refill of the static inputs) comes first
        self.stream.wait_stream(torch.cuda.current_stream(self.stream.device))
        with torch.cuda.stream(self.stream):
            self.graph.replay()
        return self.out_q, self.out_db

    def finish(self):
        self.stream.synchronize()
        if not self.modelq.voxel_coords_in_range():
            self.modelq._raise_voxel_range("a replayed")
        for m in (self.modelq, self.modeldb):
            if not m.fp16_range_ok():
                range_guard.guard_of(m).report("a replayed")
        return self.out_q, self.out_db
