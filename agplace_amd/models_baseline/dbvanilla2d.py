"""DBVanilla2D (database / aerial network), drop-in for reference models_baseline/dbvanilla2d.py:17-114.

`DBVanilla2D(mode='db', dim=args.features_dim)`; `model(data_dict, mode='db') -> {'embedding'}`.
Per map type: ImageFE -> GeM -> MLP(Linear, LayerNorm, ReLU, Linear); stack over map types,
F.normalize, mean over map types; db_map is [b,nmap,3,h,w] (cache/test) or [b,ndb,nmap,3,h,w]
(train), fp32, or the same tiles decoded as uint8 [...,h,w,3]; `db_frames` (uint8 [...,H0,W0,3]) instead of db_map: decoded
frames, centre-cropped (opt.db_cropsize) and resized on the device by Resize(opt.db_resize), with `db_jitter` colour-jittered
(DESIGN.md 1d); uint8 inputs are normalised with opt.image_mean / opt.image_std.  state_dict keys: dbimage_fes.{i}.fe.*, dbimage_pools.{i}.p, dbimage_mlps.{i}.seq.{0,1,3}.*
All arithmetic runs in libagplace_hip.so.  .eval()+no_grad = inference; .train() = end-to-end training
(batch-statistics BatchNorm + conv backward on HIP kernels, train_fns.TrunkFn).
"""
from typing import List

import torch
import torch.nn as nn

from .. import autograd_ops, ops, range_guard, train_fns
from ..convnext import precision_from_options
from ..network.image_fe import ImageFE
from ..network.image_pooling import GeM
from ..network_mm.image_pooling import gem_op
from ..network_mm.ffns import _PreparedLinear
from ..options import get_options
from ..vecprog import VecProgram


class MLP(nn.Module):
    def __init__(self, input_dim, output_dim):
        super().__init__()
        self.seq = nn.Sequential(
            nn.Linear(input_dim, output_dim),
            nn.LayerNorm(output_dim),
            nn.ReLU(),
            nn.Linear(output_dim, output_dim),
        )
        self._p0, self._p3 = _PreparedLinear(self.seq[0]), _PreparedLinear(self.seq[3])

    def forward(self, x):
        out = autograd_ops.linear(x, self.seq[0], self._p0)
        out = autograd_ops.layernorm(out, self.seq[1], relu=True)
        return autograd_ops.linear(out, self.seq[3], self._p3)


class DBVanilla2D(nn.Module):
    def __init__(self, mode: List[str], dim, opt=None):
        super().__init__()
        self.opt = opt = opt or get_options()
        if mode == 'db':
            maptype = opt.maptype.split('_')
            fes = [ImageFE(fe_type=opt.dbimage_fe, layers=opt.dbimage_fe_layers) for _ in maptype]
            self._convnext = opt.dbimage_fe == "convnext_tiny"
            for e in fes:
                if not self._convnext:      # Normalize of the uint8 routes (tiles, frames), which the ResNets alone have
                    e.fe.set_image_norm(opt.image_mean, opt.image_std)
                else:
                    if opt.convnext_train:  # the opt-in training path of the ConvNeXt trunk (agplace_amd/convnext.py)
                        e.fe.enable_training()
                    if opt.convnext_u8:     # its opt-in uint8 routes: tiles and frames, normalised by the stem as it reads
                        e.fe.enable_u8_inputs().set_image_norm(opt.image_mean, opt.image_std)
                    e.fe.set_precision(precision_from_options(opt))     # 3, or the opt-in one-product fp16 inference mode (4)
                    e.model_opt = opt       # (Options.convnext_range_guard: the trunks report through THIS model's guard)
            self.dbimage_fes = nn.ModuleList(fes)
            self.dbimage_pools = nn.ModuleList([GeM() for _ in maptype])
            self.dbimage_mlps = nn.ModuleList([MLP(e.last_dim, dim) for e in fes])

    def freeze_backbone(self):
        """requires_grad=False on the ResNets and GeM exponents (the conv kernels have no backward yet);
        the per-map MLP heads stay trainable through the HIP backward kernels."""
        for m in list(self.dbimage_fes) + list(self.dbimage_pools):
            for p in m.parameters():
                p.requires_grad_(False)
        self._frozen_backbone = True
        return self

    def poll_fp16_range(self):
        """NON-BLOCKING fp16 range check of the guarded inference forwards -- and, with Options.train_range_guard, training
        forwards -- so far (MM.poll_fp16_range)."""
        range_guard.poll(self)

    def fp16_range_ok(self):
        """False if a guarded inference forward since the last report stored a saturated fp16 map value (MM.fp16_range_ok)."""
        return range_guard.ok(self)

    def final_pool_request(self, i):
        """The GeM of map type i's last stage output (dbvanilla2d.py:74) as an ops.PoolReq the trunk's last conv fills."""
        j = 0 if self.opt.share_dbfe is True else i
        return ops.PoolReq(self.dbimage_pools[j].p, eps=self.dbimage_pools[j].eps, want_mean=False, want_gem=True)

    def forward_db(self, data_dict, trunk_maps=None, out_rows=None, defer_head=None):
        """trunk_maps: optional {map index: (stage maps, filled final PoolReq)} of the tiles computed by the caller
        (agplace_amd.pair runs a trunk in lock-step with the query network's); with dbimage_fe='convnext_tiny' the entries are
        (the trunk's three fp32 maps, None) and need Options.convnext_pair (_forward_db_convnext).
        out_rows: optional preallocated fp32 [b * ndb, 256] tensor the fused inference head writes the embedding rows to.
        defer_head: optional list; the fused inference head (one vector program) is then NOT launched but appended to it: the
        caller lets it ride in another program's launch (VecProgram.run(rider=...), agplace_amd.pair) -- the returned embedding
        is written when that launch runs."""
        opt = self.opt
        if getattr(self, "_convnext", False):
            return self._forward_db_convnext(data_dict, trunk_maps)
        # .train() under torch.no_grad() (train.py:315 with --train_modeldb False): batch-statistics BatchNorm with
        # running-stat updates and no tape -- the train-mode kernels run, the autograd Functions record nothing.
        # .eval() with gradients enabled and trainable parameters: the training graph on frozen BatchNorm statistics
        # (train_graph.bn_frozen) -- F.batch_norm(training=False) under autograd.
        train = self.training or (torch.is_grad_enabled() and not getattr(self, "_frozen_backbone", False)
                                  and any(p.requires_grad for p in self.parameters()))
        if not train:
            with range_guard.guarded(self, opt, opt.mfma_precision, False):
                return self._forward_db(data_dict, train, trunk_maps, out_rows, defer_head)
        from .. import train_graph
        # the opt-in fast modes (train_graph.py) for THIS model's forward only, as in MM.forward_q
        # (Options.train_range_guard: the guard word bound around the training FORWARD, published behind it, as in MM.forward_q)
        with train_graph.training_mode(opt.train_precision == 16, opt.train_dgrad_products == 1), \
                range_guard.guarded_train(self, opt):
            return self._forward_db(data_dict, train, trunk_maps, out_rows, defer_head)

    def _forward_db(self, data_dict, train, trunk_maps, out_rows, defer_head):
        opt = self.opt
        frames, jitter, crop, db_map, u8, mode, (b, ndb, nmap, c, h, w), dev = self._db_inputs(data_dict)
        assert c == 3
        prec = 3 if train else opt.mfma_precision
        if (not train and torch.is_grad_enabled() and getattr(self, "_frozen_backbone", False) and prec == 4
                and any(p.requires_grad for p in self.parameters())):
            prec = 2          # heads trained on frozen features: the tight mode, as in MM.forward_q
        # inference: the MLP heads, F.normalize and the mean over map types as ONE program launch (vecprog.hip) when the
        # heads fit it (Linear(<=256, 256): a ResNet18/34 trunk; a ResNet50 head, Linear(1024, dim), runs per op)
        fused = None
        if not train and not torch.is_grad_enabled() and opt.fused_vector_path and nmap <= 4 and all(
                m.seq[0].in_features <= 256 and m.seq[0].in_features % 32 == 0 and m.seq[0].out_features == 256
                and m.seq[3].out_features == 256 for m in self.dbimage_mlps):
            fused = VecProgram(b * ndb, dev)
        if True:
            vecs = []
            for i in range(nmap):
                j = 0 if opt.share_dbfe is True else i
                x = self._db_tile_input(i, frames, jitter, crop, db_map, u8, (b, ndb, nmap, c, h, w))
                if train:
                    # share_dbfe: ONE trunk over every map type (reference :69-72); each application keeps its own
                    # activations and tape (slot i), the parameter gradients of all of them accumulate
                    fe = self.dbimage_fes[j].fe
                    v = train_fns.TrunkFn.apply(train_fns.anchor_of(fe, self.dbimage_pools[j].p), x, fe, self.dbimage_pools[j], train_fns.MapSink(),
                                                prec, False, i if opt.share_dbfe is True else 0)[0]
                else:
                    if trunk_maps is not None and i in trunk_maps:
                        fpool = trunk_maps[i][1]
                    else:
                        fpool = self.final_pool_request(i)
                        self.dbimage_fes[j].forward_maps(x, prec=prec, final_pool=fpool)
                    # (a last map stored with an exponent: the stored map's GeM; the fused head multiplies by 2^e where it loads
                    # the vector, the per-op head with a small launch)
                    v, vscale = (fpool.gem, fpool.scale) if fused is not None else (fpool.true_gem(), None)
                if fused is not None:
                    # MLP + F.normalize of this map type; register 2 + i holds its vector
                    mlp = self.dbimage_mlps[j]
                    fused.linear(0, mlp._p0.get(), v, scale=vscale)
                    fused.layernorm(0, mlp.seq[1], 0, relu=True)
                    fused.linear(2 + i, mlp._p3.get(), 0)
                    if opt.output_l2 is True:
                        fused.l2norm(2 + i, 2 + i)
                    vecs.append(v)
                    continue
                v = self.dbimage_mlps[j](v)
                if opt.output_l2 is True:
                    v = autograd_ops.l2normalize(v)
                vecs.append(v)
            if fused is not None:
                if nmap > 1:
                    wmean = torch.full((1,), 1.0 / nmap, device=dev)
                    fused.wsum(2, [2 + i for i in range(nmap)], [wmean] * nmap)
                if opt.final_l2 is True:
                    fused.l2norm(2, 2)
                out = fused.store(2, out_rows)
                if defer_head is not None:
                    defer_head.append(fused)
                else:
                    fused.run()
                out = out.view(b, ndb, -1)
                if mode == 'cachetest':
                    out = out.view(b, -1)
                return {'embedding': out}
        return {'embedding': self._mean_over_maps(vecs, b, ndb, mode)}

    def _mean_over_maps(self, vecs, b, ndb, mode):
        """The mean over map types of the per-map vectors [b * ndb, dim], in the input's layout, then final_l2."""
        opt, nmap = self.opt, len(vecs)
        if True:
            out = vecs[0] if nmap == 1 else autograd_ops.wsum(
                vecs, [torch.full((1,), 1.0 / nmap, device=vecs[0].device)] * nmap)
            out = out.view(b, ndb, -1)
            if mode == 'cachetest':
                out = out.view(b, -1)
            if opt.final_l2 is True:
                shp = out.shape
                out = autograd_ops.l2normalize(out.reshape(-1, shp[-1])).view(shp)
        return out

    def _db_tile_input(self, i, frames, jitter, crop, db_map, u8, dims):
        """Map type i of a parsed input (_db_inputs) as one trunk input of b * ndb images: ops.RawFrames, uint8 [n,1,h,w,3] tiles
        or a [n,3,h,w] view."""
        b, ndb, nmap, c, h, w = dims
        if frames is not None:
            f = frames[:, :, i]
            return ops.RawFrames(f.reshape(b * ndb, 1, *f.shape[2:]), h, w, crop=crop,      # one "camera" per tile
                                 jitter=None if jitter is None else jitter[:, :, i].reshape(b * ndb, ops.JITTER_RECORD))
        x = db_map[:, :, i].reshape(b * ndb, c, h, w)       # view when possible; strides are honoured
        if u8:
            x = x.permute(0, 2, 3, 1).unsqueeze(1)          # uint8 [n,1,h,w,3]: one "camera" per tile (contiguous again)
        return x

    def _db_inputs(self, data_dict):
        """Validate and parse `db_map` / `db_frames` / `db_jitter`: (frames [b,ndb,nmap,H0,W0,3] or None, jitter [b,ndb,nmap,8] or
        None, crop, db_map as a logical [b,ndb,nmap,3,h,w] view or None, whether db_map is uint8, 'cachetest' | 'train',
        (b, ndb, nmap, c, h, w), device)."""
        opt = self.opt
        crop, db_map = None, None
        frames = data_dict.get('db_frames')
        jitter = data_dict.get('db_jitter')
        if jitter is not None and frames is None:
            raise ValueError("DBVanilla2D.forward_db: `db_jitter` (colour jitter records) needs `db_frames`")
        if frames is not None:
            # decoded uint8 frames [b,nmap,H0,W0,3] or [b,ndb,nmap,H0,W0,3]: resized by torchvision's Resize(opt.db_resize) rule with
            # PIL's arithmetic, normalised and packed in ONE launch in front of the stem (ops.RawFrames); the result
            # is bit-identical to `db_map` = the resized uint8 tiles
            if 'db_map' in data_dict:
                raise ValueError("DBVanilla2D.forward_db: pass `db_frames` or `db_map`, not both")
            if not torch.is_tensor(frames) or frames.dtype != torch.uint8 or frames.dim() not in (5, 6) or frames.shape[-1] != 3:
                raise ValueError("DBVanilla2D.forward_db: `db_frames` must be uint8 [b,nmap,H0,W0,3] or [b,ndb,nmap,H0,W0,3]")
            # opt.db_cropsize: CenterCrop in front of the Resize, a region of interest of the same launch; `db_jitter`: float32
            # [number of frames, 8] colour jitter records on the device, in the frames' memory order (input_pipeline.color_jitter)
            crop = opt.db_cropsize
            if crop is not None:
                ops.center_crop_origin(frames.shape[-3], frames.shape[-2], crop)       # (larger than the frame: NotImplementedError)
                h, w = ops.resized_size(crop, crop, opt.db_resize)
            else:
                h, w = ops.resized_size(frames.shape[-3], frames.shape[-2], opt.db_resize)
            mode = 'cachetest' if frames.dim() == 5 else 'train'
            if frames.dim() == 5:
                frames = frames.unsqueeze(1)
            b, ndb, nmap = frames.shape[:3]
            if jitter is not None:
                if (not torch.is_tensor(jitter) or jitter.dtype != torch.float32 or jitter.dim() < 2
                        or jitter.shape[-1] != ops.JITTER_RECORD or jitter.numel() != b * ndb * nmap * ops.JITTER_RECORD):
                    raise ValueError(f"DBVanilla2D.forward_db: `db_jitter` must be float32 [{b * ndb * nmap}, {ops.JITTER_RECORD}], "
                                     "one record per frame")
                jitter = jitter.reshape(b, ndb, nmap, ops.JITTER_RECORD)
            c, u8, dev = 3, False, frames.device
        else:
            db_map = data_dict['db_map']
            dev = db_map.device
            u8 = db_map.dtype == torch.uint8
            if u8:
                # decoded uint8 tiles [b,nmap,h,w,3] or [b,ndb,nmap,h,w,3] (HWC, as the image decoder leaves them): ToTensor +
                # Normalize happen on the device inside the stem's input packing (ops.pack_cameras_u8, 4x fewer bytes over PCIe)
                if db_map.shape[-1] != 3 or db_map.dim() not in (5, 6):
                    raise NotImplementedError("uint8 db_map must be [b,nmap,h,w,3] or [b,ndb,nmap,h,w,3]")
                db_map = db_map.permute(*range(db_map.dim() - 3), -1, -3, -2)      # logical [...,3,h,w] view, no copy
            if db_map.dim() == 5:      # [b,nmap,3,h,w]  caching / testing
                mode = 'cachetest'
                b, nmap, c, h, w = db_map.shape
                db_map = db_map.unsqueeze(1)
                ndb = 1
            elif db_map.dim() == 6:    # [b,ndb,nmap,3,h,w]  training layout
                mode = 'train'
                b, ndb, nmap, c, h, w = db_map.shape
            else:
                raise NotImplementedError
        return frames, jitter, crop, db_map, u8, mode, (b, ndb, nmap, c, h, w), dev

    def _forward_db_convnext(self, data_dict, trunk_maps):
        """dbimage_fe='convnext_tiny' (agplace_amd/convnext.py) over fp32 `db_map`.  Per map type: the trunk's last map
        (fp32, 384 channels) -> the dense-fp32 GeM -> the per-op MLP(384, dim) -> F.normalize; then the mean over map types.  The
        heads may train on a frozen trunk (freeze_backbone) through the ops' own backward kernels.  Inference only unless
        Options.convnext_train enabled the trunks' training path: then .train() (stochastic depth; under torch.no_grad() nothing is
        saved) and gradients into the trunk run through ConvNeXt.forward_maps_train; with share_dbfe the one trunk is applied per
        map type, each application with its own saved state, and its parameter gradients accumulate.
        uint8 `db_map`, `db_frames` and `db_jitter` are refused by name unless Options.convnext_u8 enabled the trunks' uint8
        inputs; then they are taken as in the ResNet model (one "camera" per tile), in inference and in training."""
        opt = self.opt
        enabled = all(e.fe._train_enabled for e in self.dbimage_fes)
        what = "DBVanilla2D with dbimage_fe='convnext_tiny'" + ("" if enabled else " (inference only; Options.convnext_train opts in)")
        if self.training and not enabled:
            raise NotImplementedError(f"{what}: .train() is not enabled; call .eval()")
        u8_on = all(e.fe._u8_enabled for e in self.dbimage_fes)       # Options.convnext_u8
        if not u8_on and ('db_frames' in data_dict or 'db_jitter' in data_dict):
            raise NotImplementedError(f"{what}: `db_frames` (decoded uint8 frames) is not built; pass fp32 `db_map`")
        # Options.convnext_pair: trunk_maps = {map index: (the trunk's three fp32 maps of that map type's tiles, None)} computed by
        # the caller (pair.embed_pair: ConvNeXt.forward_maps_multi, in lock-step with the query trunk); GeM, heads and the mean over
        # map types are this forward, unchanged.  Without the switch the argument stays refused.
        if trunk_maps is not None and not opt.convnext_pair:
            raise NotImplementedError(f"{what}: lock-step trunks (pair.embed_pair) are not built")
        if not u8_on and data_dict['db_map'].dtype == torch.uint8:
            raise NotImplementedError(f"{what}: uint8 `db_map` is not built; pass fp32 tiles")
        if not enabled and torch.is_grad_enabled() and any(p.requires_grad for e in self.dbimage_fes for p in e.fe.features.parameters()):
            raise NotImplementedError(f"{what}: gradients into the trunk are not enabled; run under torch.no_grad() or "
                                      "freeze_backbone()")
        # (with Options.convnext_u8: uint8 `db_map`, `db_frames` with db_resize / db_cropsize and `db_jitter` under _forward_db's
        # validation; the trunk resizes and jitters to uint8 tiles and its stem normalises them as it reads, ConvNeXt._input)
        frames, jitter, crop, db_map, u8, mode, dims, _ = self._db_inputs(data_dict)
        b, ndb, nmap, c, h, w = dims
        assert c == 3
        # Options.convnext_range_guard: this model's guard word bound around its INFERENCE trunks at precision 4 (the guarded twins
        # of csrc/convnext.hip, the weight planes' clamp flag) and published behind the forward; training forwards are mode 3
        tag = None
        if not any(e.fe.takes_training_path() for e in self.dbimage_fes):
            tag = range_guard.cnx_tag(opt, self.dbimage_fes[0].fe.precision)
        if trunk_maps:
            if self.training or any(e.fe.takes_training_path() for e in self.dbimage_fes):
                raise ValueError(f"{what}: `trunk_maps` is an inference argument (.eval() under torch.no_grad())")
            if tag is not None:
                raise ValueError(f"{what}: `trunk_maps` while Options.convnext_range_guard binds this model's guard around its trunks: "
                                 "maps computed outside the forward would skip the guard; call forward_db without them")
        with range_guard.guarded_cnx(self, tag):
            vecs = []
            for i in range(nmap):
                j = 0 if opt.share_dbfe is True else i
                if trunk_maps and i in trunk_maps:
                    last = trunk_maps[i][0][-1]
                else:
                    x = self._db_tile_input(i, frames, jitter, crop, db_map, u8, dims)
                    if torch.is_tensor(x) and not u8:
                        x = x.float()
                    last, _ = self.dbimage_fes[j](x)
                v = gem_op(last, self.dbimage_pools[j].p, self.dbimage_pools[j].eps)
                v = self.dbimage_mlps[j](v)
                if opt.output_l2 is True:
                    v = autograd_ops.l2normalize(v)
                vecs.append(v)
            out = {'embedding': self._mean_over_maps(vecs, b, ndb, mode)}
        return out

    def forward(self, data_dict, mode: List[str]):
        if mode == 'db':
            return self.forward_db(data_dict)
        raise NotImplementedError
