"""MM (query network), drop-in for reference network_mm/mm.py:31-172.

`MM(drop=None)`; `modelq(data_dict, mode='q') -> dict` with keys imagevec_org, voxvec_org,
shallowvec_org, stg2fusevec, stg2imagevec, stg2voxvec, embedding (mm.py:150-158).  Attribute
names match what train.py:175-190 reads for its optimizer groups.

Scope: the image backbone, GeM, stage-1 Neural-ODE fusion, stage-2 fusion
and the scalar-weight glue run on hand-written gfx950 kernels.  The sparse-voxel branch
(MinkFPN / MinkGeM / ECABasicBlock, agplace_amd/sparse) runs from `coords` [N,4] / `features` [N,1]
exactly like mm.py:86-89, in inference and in .train() mode (agplace_amd/sparse/train.py), or -- without
`coords` -- from raw scans: `points` fp32 [N,3] in metres, `point_offsets` int64 [b+1] and the optional
`pc_rotation` ([3,3] or [b,3,3]), voxelised on the device with Options.quant_size; when
neither is present data_dict carries the voxel branch's dense outputs instead:
    vox_levels  [ [b,64], [b,128], [b,256] ]   globally pooled v1..v3  (fuse_block_toshallow.py:83)
    voxfeatvec  [b,256]                          MinkGeM(voxfeatmap)      (mm.py:89)
    stg2voxvec  [b,256], voxvec_fuse [b,256]     stage-2 voxel outputs    (stage2fuse_blockadd.py:201,207)
The cameras enter as `query_image` -- the normalised fp32 panorama [b,3,h,w] or already resized uint8 tiles [b,ncam,h,w,3] -- or
as `query_frames`: decoded uint8 frames [b,ncam,H0,W0,3], resized on the device by torchvision's Resize(opt.q_resize) rule with
PIL's arithmetic and then handled exactly like the uint8 tiles; `query_jitter` beside them (float32 [b*ncam,8]
records from input_pipeline.color_jitter) runs torchvision's ColorJitter on the resized frames, on the device.  uint8 inputs are
normalised with opt.image_mean / opt.image_std.
Execution modes:
  * .eval() under torch.no_grad(): inference, BatchNorm folded into the conv epilogues.
  * .train() with gradients enabled: end-to-end training.  Batch-statistics BatchNorm and the conv
    backward run on HIP kernels (resnet.ResNet.forward_maps_train / backward_maps, train_graph.py);
    feature maps never become autograd tensors (train_fns.py), the vector path (up-dims, Neural-ODE
    blocks, projections, Basic MLP, stg2fusefc, normalisations) uses autograd_ops.py.
  * .eval() with gradients enabled and trainable parameters: the same training graph on FROZEN BatchNorm
    statistics (train_graph.bn_frozen: running statistics read, not updated, constants of the backward).
  * .eval() + freeze_backbone(): train the fusion path only, on frozen image features.
With mm_imgfe='convnext_tiny' (the 384-wide configuration of _check_convnext_options) the first mode is the default and the other
three are behind Options.convnext_train: the same training graph with train_fns.CnxTrunkFn in TrunkFn's place
(_forward_q_convnext).
"""
import torch
import torch.nn as nn

from .. import autograd_ops, ops, range_guard, sparse, train_fns
from ..convnext import precision_from_options
from ..options import get_options
from .ffns import _PreparedLinear
from .fuse_block_toshallow import FuseBlockToShallow
from ..vecprog import VecProgram, VecProgramUnfit
from .image_fe import ImageFE
from .image_pooling import GeM
from .stage2fuse_blockadd import Stage2FuseBlockAdd


class MM(nn.Module):
    def __init__(self, drop=None, opt=None):
        super().__init__()
        self.opt = opt = opt or get_options()
        self.drop = drop
        self._convnext = opt.mm_imgfe == "convnext_tiny"
        if self._convnext:
            _check_convnext_options(opt)
        self.image_fe = ImageFE(fe_type=opt.mm_imgfe, layers=opt.mm_imgfe_layers)
        if not self._convnext:
            self.image_fe.fe.set_image_norm(opt.image_mean, opt.image_std)       # Normalize of the uint8 routes (tiles, frames)
        else:
            if opt.convnext_train:          # the opt-in training path of the ConvNeXt trunk (agplace_amd/convnext.py)
                self.image_fe.fe.enable_training()
            if opt.convnext_u8:             # its opt-in uint8 routes: tiles and frames, normalised by the stem as it reads
                self.image_fe.fe.enable_u8_inputs().set_image_norm(opt.image_mean, opt.image_std)
            self.image_fe.fe.set_precision(precision_from_options(opt))      # 3, or the opt-in one-product fp16 inference mode (4)
            self.image_fe.model_opt = opt       # (Options.convnext_range_guard: the trunk reports through THIS model's guard)
        self.image_pool = GeM()
        planes = [int(x) for x in opt.mm_voxfe_planes.split('_')]
        layers = [int(x) for x in opt.mm_voxfe_layers.split('_')]
        self.vox_fe = sparse.MinkFPN(in_channels=1, out_channels=planes[-1], planes=planes, layers=layers,
                                     num_top_down=opt.mm_voxfe_ntd, conv0_kernel_size=5, block=sparse.ECABasicBlock)
        self.vox_pool = sparse.MinkGeM()
        self.fuseblocktoshallow = FuseBlockToShallow(
            dims=[opt.mm_stg2fuse_dim for _ in range(len(planes))],
            img_dims=[int(e) for e in opt.mm_imgfe_planes.split('_')],
            vox_dims=[int(e) for e in opt.mm_voxfe_planes.split('_')],
            bev_dims=[int(e) for e in opt.mm_bevfe_planes.split('_')], opt=opt)
        self.stg2fuseblock = Stage2FuseBlockAdd(fusedim=opt.mm_stg2fuse_dim, imgdim=opt.mm_imgfe_dim,
                                                bevdim=opt.mm_bevfe_dim, voxdim=opt.mm_voxfe_dim, opt=opt)
        self.stg2fusefc = nn.Linear(opt.mm_stg2fuse_dim, opt.mm_stg2fuse_dim)
        self._prep_fc = _PreparedLinear(self.stg2fusefc)

        def w(v, learn):
            return nn.Parameter(torch.tensor(v, dtype=torch.float32), requires_grad=learn)
        self.image_weight = w(opt.image_weight, opt.image_learnweight)
        self.vox_weight = w(opt.vox_weight, opt.vox_learnweight)
        self.shallow_weight = w(opt.shallow_weight, opt.shallow_learnweight)
        self.imageorg_weight = w(opt.imagevoxorg_weight, opt.imagevoxorg_learnweight)
        self.voxorg_weight = w(opt.imagevoxorg_weight, opt.imagevoxorg_learnweight)
        self.shalloworg_weight = w(opt.shalloworg_weight, opt.shalloworg_learnweight)
        self.stg2image_weight = w(opt.stg2imagevox_weight, opt.stg2imagevox_learnweight)
        self.stg2vox_weight = w(opt.stg2imagevox_weight, opt.stg2imagevox_learnweight)
        self.stg2fuse_weight = w(opt.stg2fuse_weight, opt.stg2fuse_learnweight)

    def freeze_backbone(self):
        """Fine-tune the fusion path on FROZEN image features (eval-mode BatchNorm, folded convs):
        `image_fe` and the stage-2 `BasicBlock` get requires_grad=False and the model may then be run
        in .eval() with gradients enabled.  Gradient does not flow through feature maps in this mode:
        the stage-2 image block is a constant function of its input (the path fusevec -> projsfuseimg
        -> conv block is cut).  Every vector-path parameter (up-dims, Neural-ODE blocks, projsimgfuse,
        Basic MLP, stg2fusefc) receives its exact gradient w.r.t. the remaining graph.  For end-to-end
        training use .train() instead."""
        for m in [self.image_fe] + list(self.stg2fuseblock.ffnsimg) + list(self.stg2fuseblock.projsfuseimg):
            for p in m.parameters():
                p.requires_grad_(False)
        self.image_pool.p.requires_grad_(False)
        self.stg2fuseblock.poolimage.p.requires_grad_(False)
        self._frozen_backbone = True
        return self


    # ---- the voxel-range flag.  agp_sparse_build zeroes a device word at the start of every build and sets it when it had to clamp
    # a voxel coordinate into the +-32511 range of the 16-bit key fields, met a batch index outside [0, batch size) or a sample of
    # more than 65536 points (from raw `points`, agp_sparse_build_points: when it had to DROP a point -- non-finite, or its voxel outside that
    # range -- or a sample holds more than 65536 voxels; with Options.voxel_capacity, bit 2: more distinct voxels than the capacity,
    # the build is empty): the voxel branch's outputs of that batch are then wrong.  Every inference
    # forward from `coords` or `points` ORs
    # that word into a STICKY device word and copies the sticky word to pinned host memory, both enqueued behind the build on the
    # calling stream -- captured into a hipGraph they are nodes of the graph, so every REPLAY publishes its own flag and the host
    # can look at it without touching the stream (poll_voxel_range).
    def _vox_slot(self, dev):
        key = (str(dev), torch.cuda.current_stream(dev).cuda_stream)
        slots = self.__dict__.setdefault('_vox_flag_slots', {})
        if key not in slots:
            slots[key] = {'sticky': torch.zeros(1, dtype=torch.int32, device=dev),
                          'host': torch.zeros(1, dtype=torch.int32).pin_memory(), 'event': None, 'calls': 0}
        return slots[key]

    def _raise_voxel_range(self, which, word=None):
        if word is None:                   # (a caller that has synchronised, pair.CapturedPair.finish: the sticky words say which bits)
            word = 0
            for sl in self.__dict__.get('_vox_flag_slots', {}).values():
                word |= int(sl['sticky'].item())
        for sl in self.__dict__.get('_vox_flag_slots', {}).values():       # the error is reported once: start again from zero
            sl['sticky'].mul_(0)       # (an elementwise kernel, not zero_(): no eager memset beside replayed graphs, csrc/coords.hip)
            sl['host'].zero_()
            sl['event'] = None
        if word & 4:
            # bit 2 (agp_sparse_build_points_cap): the batch held more distinct voxels than Options.voxel_capacity rows
            also = " (a dropped point or an oversized sample was flagged as well)" if word & 3 else ""
            raise ValueError(f"MM.forward_q: in {which} batch the raw scans held more distinct voxels than the voxel capacity "
                             f"(Options.voxel_capacity = {self.opt.voxel_capacity}): the build came out empty and the voxel "
                             f"branch's outputs of that batch are those of an empty cloud; raise the capacity{also}")
        raise ValueError(f"MM.forward_q: in {which} batch a voxel coordinate lies outside the supported range (|c| <= 32511 after "
                         "flooring; from `coords` the point was clamped into the origin voxel, from raw `points` it was dropped, as "
                         "was a point with a non-finite component), a batch index outside [0, batch size), or one sample holds more "
                         "than 65536 points (`coords`) / voxels (`points`): the voxel branch's outputs of that batch are wrong")

    def poll_voxel_range(self):
        """NON-BLOCKING: raises ValueError if any inference forward from `coords` or raw `points` whose flag has reached the host so far -- eager
        or REPLAYED from a hipGraph -- saw an out-of-range cloud (reads words of pinned host memory; no stream is synchronised,
        so the most recent forwards may not be covered yet: finish a loop with voxel_coords_in_range()).  Call it every few
        replays of a captured forward (agplace_amd.pair.CapturedPair.replay does)."""
        for sl in self.__dict__.get('_vox_flag_slots', {}).values():
            if int(sl['host'][0]) != 0:
                self._raise_voxel_range("an earlier", int(sl['host'][0]))

    def voxel_coords_in_range(self):
        """False if ANY inference forward from `coords` or raw `points` since the last report (eager or replayed) had to clamp a voxel
        coordinate (`coords`) or drop a point (`points`), met a bad batch index or an oversized sample.  Synchronises the device: call it after the loop, not inside it."""
        slots = self.__dict__.get('_vox_flag_slots', {})
        if not slots:
            return True
        torch.cuda.synchronize()
        return all(int(sl['sticky'].item()) == 0 for sl in slots.values())

    # ---- the fp16 range guard (Options.fp16_range_guard, agplace_amd/range_guard.py): the same contract as the voxel-range flag
    def poll_fp16_range(self):
        """NON-BLOCKING: raises ValueError if a guarded inference forward (eager or replayed) whose state has reached the host so
        far stored a saturated fp16 map value -- or, with Options.train_range_guard, a training forward a saturated fp16 plane
        (the message then says so)."""
        range_guard.poll(self)

    def fp16_range_ok(self):
        """False if ANY guarded inference forward since the last report stored a saturated fp16 map value.  Synchronises.
        Under agplace_amd.pair.embed_pair this word also covers the database model's image trunks (run in lock-step with this
        model's)."""
        return range_guard.ok(self)

    def _publish_voxel_flag(self, flag):
        """Behind the build, on the calling stream (which has joined the voxel side stream).  Eager calls also check: the first call
        of a stream its own flag at once, every later call the flag of the call BEFORE it on that stream (an event behind that
        call's copy: the wait is for work the host enqueued a whole forward ago) -- a bad batch is reported one call late, the
        LAST batch of a loop by voxel_coords_in_range()."""
        dev = flag.device
        sl = self._vox_slot(dev)
        capturing = torch.cuda.is_current_stream_capturing()
        if not capturing:
            if sl['event'] is not None:
                sl['event'].synchronize()
                if int(sl['host'][0]) != 0:
                    self._raise_voxel_range("the previous", int(sl['host'][0]))
        sl['sticky'].bitwise_or_(flag)
        sl['host'].copy_(sl['sticky'], non_blocking=True)
        if capturing:
            return
        sl['event'] = torch.cuda.Event()
        sl['event'].record(torch.cuda.current_stream(dev))
        sl['calls'] += 1
        if sl['calls'] == 1:
            sl['event'].synchronize()
            if int(sl['host'][0]) != 0:
                self._raise_voxel_range("this", int(sl['host'][0]))

    def load_reference_state_dict(self, sd):
        """Load a reference checkpoint's `modelq_state_dict` (the voxel branch uses MinkowskiEngine's
        parameter names, so every key has a home)."""
        return self.load_state_dict(sd, strict=True)

    # ==== query
    def query_image(self, data_dict):
        """The image tensor the trunk sees (mm.py:70-75: drop='image' zeroes it); for `query_frames` the frames with the size
        Resize(opt.q_resize) gives them (ops.RawFrames: resized, normalised and packed in one launch in front of the stem)."""
        if 'query_jitter' in data_dict and 'query_frames' not in data_dict:
            raise ValueError("MM.forward_q: `query_jitter` (colour jitter records) needs `query_frames`")
        if 'query_frames' in data_dict:
            if 'query_image' in data_dict:
                raise ValueError("MM.forward_q: pass `query_frames` or `query_image`, not both")
            frames = data_dict['query_frames']
            if not torch.is_tensor(frames) or frames.dtype != torch.uint8 or frames.dim() != 5 or frames.shape[-1] != 3:
                raise ValueError("MM.forward_q: `query_frames` must be uint8 [b, ncam, H0, W0, 3]")
            if self.drop == 'image':
                raise NotImplementedError("drop='image' with uint8 camera frames")
            # `query_jitter`: float32 [b * ncam, 8] colour jitter records on the device (input_pipeline.color_jitter), one per frame
            return ops.RawFrames(frames, *ops.resized_size(frames.shape[2], frames.shape[3], self.opt.q_resize),
                                 jitter=data_dict.get('query_jitter'))
        image = data_dict['query_image']
        if self.drop == 'image':
            if image.dtype == torch.uint8:
                raise NotImplementedError("drop='image' with uint8 camera tiles")
            image = image * 0
        return image

    def final_pool_request(self):
        """The pooling of the last stage output that forward_q consumes: its GeM (image descriptor, mm.py:85) and its mean
        (fusion level 3, fuse_block_toshallow.py:82) -- an ops.PoolReq the trunk's last conv fills in its own launch."""
        return ops.PoolReq(self.image_pool.p, eps=self.image_pool.eps, want_mean=True, want_gem=True)

    OUT_KEYS = ('imagevec_org', 'voxvec_org', 'shallowvec_org', 'stg2fusevec', 'stg2imagevec', 'stg2voxvec', 'embedding')

    def forward_q(self, data_dict, image_maps=None, out_rows=None, rider=None):
        """image_maps: optional (stage maps, level means, final PoolReq) of `query_image(data_dict)` computed by the
        caller -- agplace_amd.pair runs this trunk in lock-step with the database network's (grouped conv launches).  With
        mm_imgfe='convnext_tiny' it is the trunk's list of three fp32 maps and needs Options.convnext_pair (_forward_q_convnext).
        out_rows: optional {output key: preallocated fp32 [b, 256] tensor}: the inference path writes those outputs there
        (a sub-batch's row slice of the whole batch's output: the sub-batches then need no concatenation).
        rider: optional list holding ONE deferred vector program of another network (DBVanilla2D.forward_db(defer_head=...)): the
        fused inference path launches it inside its first program's launch and empties the list; a caller that still finds it
        there (per-op path taken) runs it itself."""
        opt = self.opt
        if self._convnext:
            return self._forward_q_convnext(data_dict, image_maps, out_rows)
        # .train() under torch.no_grad() is a live reference configuration (`with torch.set_grad_enabled(args.train_modelq)`
        # around a model in train mode, train.py:307): batch-statistics BatchNorm with running-stat updates, no tape.
        # The train-mode kernels run; the autograd Functions record nothing when no input requires grad.
        # .eval() with gradients enabled and trainable parameters (fine-tuning on frozen BatchNorm statistics) also takes the
        # training graph: its BatchNorm units read the running statistics and hold them constant in the backward
        # (train_graph.bn_frozen), exactly F.batch_norm(training=False) under autograd.
        train = self.training or (torch.is_grad_enabled() and not getattr(self, "_frozen_backbone", False)
                                  and any(p.requires_grad for p in self.parameters()))
        if not train:
            with range_guard.guarded(self, opt, opt.mfma_precision, False):
                return self._forward_q(data_dict, train, image_maps, out_rows, rider)
        from .. import train_graph
        # the opt-in fast modes (train_graph.py): one-product forward convs, one-product data gradients -- for THIS model's
        # forward only, the process-wide switches restored when it returns
        # (Options.train_range_guard: the model's guard word bound around the training FORWARD, published behind it)
        with train_graph.training_mode(opt.train_precision == 16, opt.train_dgrad_products == 1), \
                range_guard.guarded_train(self, opt):
            return self._forward_q(data_dict, train, image_maps, out_rows, rider)

    def _forward_q_convnext(self, data_dict, image_maps, out_rows):
        """mm_imgfe='convnext_tiny': the trunk's three fp32 maps (96 / 192 / 384 channels) are pooled by
        ops.pool_f32 -- the last one ONCE, for its mean (fusion level 3) and its GeM (the image descriptor) -- the vector path is
        the per-op one (the fused vector programs are 256 columns wide; FCODE(384) is one launch per solve, csrc/fusion_wide.hip),
        and stage 2 packs the last map into the 384-wide BasicBlock.  The image side runs in the mode-3 arithmetic whatever
        Options.mfma_precision says (the ConvNeXt trunk's contract: fp32 range, so neither map exponents nor the fp16 range guard
        have work on it -- at Options.convnext_precision = 4 its fp16 operands saturate, which Options.convnext_range_guard
        reports through this model's guard); the voxel branch runs at Options.mfma_precision as in the ResNet model.  No host synchronisation:
        capturable after one eager warm-up.
        Inference only unless Options.convnext_train opted in.  Then `train` is derived as in forward_q and the training graph of
        the ResNet model runs with train_fns.CnxTrunkFn in TrunkFn's place: the trunk trains through its own node
        (ConvNeXt.forward_maps_train, stochastic depth in .train()), stage 2 reads the last fp32 map through ops.bcast_add_f32
        and hands its map gradient back through ops.pool_f32_bwd.  Options.train_precision / train_dgrad_products act on the
        stage-2 block only: the trunk is mode 3 whatever they say."""
        enabled = self.image_fe.fe._train_enabled
        what = "MM with mm_imgfe='convnext_tiny'" + ("" if enabled else " (inference only)")
        if self.training and not enabled:
            raise NotImplementedError(f"{what}: .train() is not built; call .eval()")
        if not enabled and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError(f"{what}: gradients are not built (a parameter requires one); run under torch.no_grad()")
        # Options.convnext_u8: uint8 `query_image` [b,ncam,h,w,3], `query_frames` with q_resize and `query_jitter`, validated by
        # query_image() as in the ResNet model; the trunk resizes and jitters to uint8 tiles, its stem normalises them as it reads
        u8_on = self.image_fe.fe._u8_enabled
        if not u8_on and ('query_frames' in data_dict or 'query_jitter' in data_dict):
            raise NotImplementedError(f"{what}: `query_frames` (decoded uint8 frames) is not built; pass the fp32 `query_image`")
        if not u8_on and data_dict['query_image'].dtype == torch.uint8:
            raise NotImplementedError(f"{what}: uint8 `query_image` is not built; pass the normalised fp32 panorama")
        # Options.convnext_pair: `image_maps` = the trunk's three fp32 maps of query_image(data_dict), computed by the caller
        # (pair.embed_pair: ConvNeXt.forward_maps_multi, in lock-step with the database trunks); everything behind the trunk is
        # this forward, unchanged.  Row-sliced outputs stay refused, and so does the argument without the switch.
        if out_rows or (image_maps is not None and not self.opt.convnext_pair):
            raise NotImplementedError(f"{what}: lock-step trunks and row-sliced outputs (pair.embed_pair, query sub-streams) are "
                                      "not built")
        train = enabled and (self.training or (torch.is_grad_enabled() and not getattr(self, "_frozen_backbone", False)
                                               and any(p.requires_grad for p in self.parameters())))
        if train and image_maps is not None:
            raise ValueError(f"{what}: `image_maps` is an inference argument (.eval() under torch.no_grad())")
        if not train:
            # Options.convnext_range_guard at trunk precision 4: with fp16_range_guard also binding (mfma_precision 2 / 4) the
            # whole-forward binding below covers the trunk too -- ONE word over the trunk, stage 2 and the voxel branch, published
            # under a tag that names both sources; alone, _forward_q binds around the trunk call only (stage 2 and the voxel branch
            # follow fp16_range_guard as before) and the word is published behind the forward, side streams joined
            tag = range_guard.cnx_tag(self.opt, self.image_fe.fe.precision, self.opt.mfma_precision)
            if image_maps is not None:
                if tag is not None:
                    raise ValueError(f"{what}: `image_maps` while Options.convnext_range_guard binds this model's guard around its "
                                     "trunk: maps computed outside the forward would skip the guard; call forward_q without them")
                with range_guard.guarded(self, self.opt, self.opt.mfma_precision, False):
                    return self._forward_q(data_dict, False, image_maps, None, None)
            if tag is not None:
                if tag != "cnx4":
                    with range_guard.guarded_cnx(self, tag):
                        return self._forward_q(data_dict, False, None, None, None)
                out = self._forward_q(data_dict, False, None, None, None, cnx_guard=True)
                range_guard.publish_tag(self, tag)
                return out
            # (the guard, when Options.fp16_range_guard is on, covers the voxel branch's fp16 maps as in the ResNet model)
            with range_guard.guarded(self, self.opt, self.opt.mfma_precision, False):
                return self._forward_q(data_dict, False, None, None, None)
        if torch.is_grad_enabled() and 'query_image' in data_dict and data_dict['query_image'].requires_grad:
            raise NotImplementedError("ConvNeXt: the gradient of the input image is not built (the stem returns none)")
        from .. import train_graph
        # (Options.train_range_guard: the trunk stores no fp16 and reads no binding; stage 2 and the voxel branch run the ResNet
        # model's training graph, whose fp16 stores report as they do there)
        with train_graph.training_mode(self.opt.train_precision == 16, self.opt.train_dgrad_products == 1), \
                range_guard.guarded_train(self, self.opt):
            return self._forward_q(data_dict, True, None, None, None)

    def _forward_q(self, data_dict, train, image_maps, out_rows, rider, cnx_guard=False):
        """cnx_guard: bind this model's fp16 range guard around the ConvNeXt trunk call ALONE (_forward_q_convnext)."""
        opt = self.opt
        prec = 3 if train else opt.mfma_precision       # training runs on split-bf16 maps (range + precision of gradients)
        if (not train and torch.is_grad_enabled() and getattr(self, "_frozen_backbone", False) and prec == 4
                and any(p.requires_grad for p in self.parameters())):
            # fine-tuning the fusion path on FROZEN features (freeze_backbone): gradients of near-cancelling sums (a mixing weight's
            # gradient is <G, descriptor>) amplify the one-product mode's 2.4e-4 .. 3.8e-4 descriptor error; the frozen trunk runs in
            # the tight two-product mode (3e-5 .. 1.6e-4) whatever the inference default is
            prec = 2
        image = self.query_image(data_dict)
        if self.drop == 'pc':
            if 'coords' in data_dict:
                data_dict = dict(data_dict)
                c = data_dict['coords'].clone()
                c[:, 1:] = c[:, 1:] * 0
                data_dict['coords'] = c
            elif 'points' in data_dict and 'point_offsets' in data_dict:
                # the same cloud from raw scans: every FINITE point at the sensor, one origin voxel per sample (a rotation keeps it there)
                data_dict = dict(data_dict)
                data_dict['points'] = data_dict['points'] * 0
            else:
                raise NotImplementedError("drop='pc' acts on the sparse voxel branch: pass coords / features, or points / point_offsets")
        if not ('image' in opt.output_type and 'vox' in opt.output_type and 'shallow' in opt.output_type):
            raise NotImplementedError   # other output_type values crash in the reference (mm.py:115-118)
        if True:
            output = []
            # ---- voxel branch (mm.py:86-89).  Training: autograd nodes over its pooled vectors, levels from the device-side
            # coordinate manager with one read-back.  Inference: a chain of ~90 small launches (no host synchronisation), so it
            # runs on its own stream AFTER the image branch's long kernels have been enqueued and is joined where its vectors
            # are needed.
            voxmap, vox_train_ctx = None, None
            vox_side = None
            # raw scans (`points` [N,3] + `point_offsets` [b+1], optional `pc_rotation`) instead of `coords`: the lidar front end
            # on the device (agp_sparse_build_points: quantise, deduplicate, rotate) feeds the same branch
            from_points = 'coords' not in data_dict and 'points' in data_dict and 'point_offsets' in data_dict
            if 'coords' in data_dict or from_points:
                data_dict = dict(data_dict)
                if train:
                    if from_points:
                        sp = sparse.SparseTensor.from_points_levels(data_dict['points'], data_dict['point_offsets'], image.shape[0],
                                                                    len(self.vox_fe.convs), opt.quant_size, data_dict.get('pc_rotation'),
                                                                    level_capacity=opt.voxel_capacity)
                    else:
                        sp = sparse.SparseTensor.from_coords_levels(data_dict['features'], data_dict['coords'], image.shape[0], len(self.vox_fe.convs))
                    vsink = train_fns.VoxSink()
                    *vmeans, vgem = train_fns.VoxTrunkFn.apply(train_fns.anchor_of(self.vox_fe, self.vox_pool.p), sp, self.vox_fe, self.vox_pool, vsink)
                    voxmap = vsink.top
                    data_dict['voxfeatvec'], data_dict['vox_levels'] = vgem, list(vmeans)
                    vox_train_ctx = (vsink, vmeans[-1])
                else:
                    dev = image.device
                    # side stream and capacity workspace per CALLING stream: two forwards in flight on two streams (two captured
                    # graphs replayed side by side, bench.py --inflight 2) must share neither
                    vkey = (str(dev), torch.cuda.current_stream(dev).cuda_stream)
                    vpool = self.__dict__.setdefault('_vox_side', {})
                    if vkey not in vpool:
                        vpool[vkey] = (torch.cuda.Stream(device=dev), ops.Workspace())
                    vox_side, vox_ws = vpool[vkey]
                    vox_side.wait_stream(torch.cuda.current_stream(dev))     # inputs are ready; nothing of the image branch yet
            # ---- image branch
            train_ctx = None
            if train:
                # feature maps stay inside the HIP graph; autograd sees the pooled vectors (train_fns.py)
                sink = train_fns.MapSink()
                if self._convnext:
                    # fp32 stream tensors in the sink; the bridge kernels of csrc/pool.hip on either side of stage 2
                    fe = self.image_fe.fe
                    *means, imagefeatvec = train_fns.CnxTrunkFn.apply(train_fns.anchor_of(fe.features, self.image_pool.p), image, fe,
                                                                       self.image_pool, sink)
                else:
                    *means, imagefeatvec = train_fns.TrunkFn.apply(
                        train_fns.anchor_of(self.image_fe.fe, self.image_pool.p), image, self.image_fe.fe, self.image_pool, sink, prec, True)
                levels = [_Pooled(m) for m in means]
                imagefeatmap = sink.maps[-1]
                train_ctx = (sink, means[-1], len(means) - 1)
            else:
                # the level means, l3's GeM (image descriptor) and l3's mean (fusion level 3) come out of the epilogues of
                # the convs that write those maps (ops.PoolReq): no pass re-reads a stage output
                fpool = None
                if self._convnext:
                    # fp32 maps, no conv epilogue to pool in: one pass over each map, the last one for both of its poolings
                    if image_maps is not None:      # (Options.convnext_pair: the caller's lock-step trunk, the same bits)
                        maps = list(image_maps)
                    else:
                        with range_guard.bound(self, cnx_guard):
                            maps = self.image_fe.fe.forward_maps(image)
                    levels = [_Pooled(ops.pool_f32(m, None, want_mean=True, want_gem=False)[0]) for m in maps[:-1]]
                    mean3, imagefeatvec = ops.pool_f32(maps[-1], self.image_pool.p, want_mean=True, want_gem=True, eps=self.image_pool.eps)
                    levels.append(_Pooled(mean3))
                elif image_maps is not None:
                    maps, lvl_means, fpool = image_maps
                else:
                    lvl_means, fpool = [], self.final_pool_request()
                    maps = self.image_fe.forward_maps(image, prec=prec, level_means=lvl_means, final_pool=fpool)
                imagefeatmap = maps[-1]
                if fpool is not None:
                    # (maps stored with an exponent: the pooled vectors are the stored maps', times 2^-e; the fused vector path
                    # restores the factor where its programs load them, the per-op path below with a small launch each)
                    mean3, imagefeatvec = fpool.mean, fpool.gem
                    levels = [_Pooled(m, mp.exp) for m, mp in zip(lvl_means, maps)] + [_Pooled(mean3, fpool.exp)]
            if vox_side is not None:
                cur = torch.cuda.current_stream(image.device)
                with torch.cuda.stream(vox_side):
                    # capacity-mode levels: sort / unique / segment offsets on the device, no host synchronisation, every buffer
                    # from the module's workspace -- the branch is hipGraph-capturable (agplace_amd/sparse/coords.py)
                    if from_points:
                        sp = sparse.SparseTensor.from_points_capacity(data_dict['points'], data_dict['point_offsets'], image.shape[0],
                                                                      opt.quant_size, vox_ws, data_dict.get('pc_rotation'),
                                                                      level_capacity=opt.voxel_capacity)
                    else:
                        sp = sparse.SparseTensor.from_coords_capacity(data_dict['features'], data_dict['coords'], image.shape[0], vox_ws)
                    vox_flag = sp.range_flag
                    voxmap, voxmaplist = self.vox_fe(sp, prec=prec)
                    data_dict['voxfeatvec'] = self.vox_pool(voxmap)
                    data_dict['vox_levels'] = [sparse.modules.global_avg_pool(e) for e in voxmaplist]
                cur.wait_stream(vox_side)
                for t in [voxmap.hi, voxmap.lo, data_dict['voxfeatvec']] + data_dict['vox_levels']:
                    if t is not None:
                        t.record_stream(cur)
                self._publish_voxel_flag(vox_flag)
            # ---- inference: the whole vector path as two launches (vecprog.hip) around the stage-2 conv block
            if not train and not torch.is_grad_enabled() and opt.fused_vector_path and not self._convnext:
                try:
                    return self._vector_path_fused(data_dict, imagefeatmap, levels, imagefeatvec, voxmap, prec, out_rows or {}, rider,
                                                   gem3_exp=fpool.exp)
                except VecProgramUnfit:
                    pass                      # an option set the program cannot express: the per-op path below
            if not train and fpool is not None:
                imagefeatvec = fpool.true_gem()
            if opt.output_l2 is True:
                imagefeatvec = autograd_ops.l2normalize(imagefeatvec)
            imagefeatvec_org = imagefeatvec
            output.append(autograd_ops.wsum([imagefeatvec], [self.image_weight]))
            # ---- voxel branch outputs (computed above) or the dense stand-ins
            voxfeatvec = data_dict['voxfeatvec'].float()
            if opt.output_l2 is True:
                voxfeatvec = autograd_ops.l2normalize(voxfeatvec)
            voxfeatvec_org = voxfeatvec
            output.append(autograd_ops.wsum([voxfeatvec], [self.vox_weight]))
            # ---- stage-1 fusion
            shallowfeatvec = self.fuseblocktoshallow(levels, None, data_dict['vox_levels'], type='vox')
            shallowfeatvecorg = shallowfeatvec
            if opt.output_l2 is True:
                shallowfeatvec = autograd_ops.l2normalize(shallowfeatvec)
            output.append(autograd_ops.wsum([shallowfeatvec], [self.shallow_weight]))
            # ---- stage-2 fusion
            stg2fusevec, stg2imagevec, _, stg2voxvec = self.stg2fuseblock(
                imagefeatmap, None,
                voxmap if voxmap is not None else (data_dict['stg2voxvec'].float(), data_dict['voxvec_fuse'].float()),
                output[-1], type='vox', prec=prec, train_ctx=train_ctx, vox_train_ctx=vox_train_ctx,
                img_prec=3 if self._convnext else None)
            stg2fusevec = autograd_ops.linear(stg2fusevec, self.stg2fusefc, self._prep_fc)
            # ---- final output
            terms, weights = [], []
            for name, vec, wt in (('imageorg', imagefeatvec_org, self.imageorg_weight),
                                  ('voxorg', voxfeatvec_org, self.voxorg_weight),
                                  ('shalloworg', shallowfeatvec, self.shalloworg_weight),
                                  ('stg2image', stg2imagevec, self.stg2image_weight),
                                  ('stg2vox', stg2voxvec, self.stg2vox_weight),
                                  ('stg2fuse', stg2fusevec, self.stg2fuse_weight)):
                if name in opt.final_type:
                    terms.append(vec)
                    weights.append(wt)
            if opt.final_fusetype == 'add':
                x = autograd_ops.wsum(terms, weights)
            elif opt.final_fusetype == 'cat':
                x = torch.cat([autograd_ops.wsum([t], [w]) for t, w in zip(terms, weights)], dim=-1)
            elif opt.final_fusetype == 'catadd':
                x = torch.cat([autograd_ops.wsum([t], [w]) for t, w in zip(terms[:-1], weights[:-1])], dim=-1)
                x = autograd_ops.wsum([x, terms[-1]], [None, weights[-1]])
            else:
                raise NotImplementedError
            if opt.final_l2 is True:
                x = autograd_ops.l2normalize(x)
        return {
            'imagevec_org': imagefeatvec_org,
            'voxvec_org': voxfeatvec_org,
            'shallowvec_org': shallowfeatvecorg,
            'stg2fusevec': stg2fusevec,
            'stg2imagevec': stg2imagevec,
            'stg2voxvec': stg2voxvec,
            'embedding': x,
        }

    def _vector_path_fused(self, data_dict, imagefeatmap, levels, gem3, voxmap, prec, out_rows, rider=None, gem3_exp=0):
        """Everything of forward_q after the backbones (mm.py:91-129) for inference: program 1 = descriptors' F.normalize,
        FuseBlockToShallow, the stage-2 projections of the fusion vector; the stage-2 conv block (and sparse block) on
        their own kernels; program 2 = fusion update, FFNFuse, stg2fusefc, the final weighted sum.  Same arithmetic as
        the per-op path (autograd_ops), 2 launches instead of ~27."""
        opt, s2 = self.opt, self.stg2fuseblock
        if (opt.stg2nlayers != 1 or opt.stg2_type != 'full' or opt.stg2fuse_type is None or opt.final_fusetype != 'add'
                or opt.mm_stg2fuse_dim != 256 or gem3.shape[1] != 256):
            raise VecProgramUnfit("options")
        b, dev = gem3.shape[0], gem3.device
        sparse_vox = voxmap is not None
        vp = VecProgram(b, dev)
        vp.load(0, gem3, ops.pow2_scalar(dev, gem3_exp))
        if opt.output_l2 is True:
            vp.l2norm(0, 0)
        imagevec_org = vp.store(0, out_rows.get('imagevec_org'))
        vp.load(1, data_dict['voxfeatvec'].float())
        if opt.output_l2 is True:
            vp.l2norm(1, 1)
        voxvec_org = vp.store(1, out_rows.get('voxvec_org'))
        r = self.fuseblocktoshallow.emit(vp, levels, data_dict['vox_levels'])
        shallow_org = vp.store(r, out_rows.get('shallowvec_org'))
        shallow_n = shallow_org
        if opt.output_l2 is True:
            vp.l2norm(r, r)
            shallow_n = vp.store(r)
        vp.wsum(1, [r], [self.shallow_weight])
        fusevec = vp.store(1)
        fv_img = fv_vox = fusevec
        # the vector that bcast_add adds into the layer-3 map takes that map's 2^-e: folded into the projection's weights and bias
        # (no projection: one op of this program)
        e3 = imagefeatmap.exp
        if s2._prep_fuseimg[0] is not None:
            vp.linear(2, s2._prep_fuseimg[0].get(exp=-e3), 1)
            fv_img = vp.store(2)
        elif e3:
            vp.wsum(2, [1], [ops.pow2_scalar(dev, -e3)])
            fv_img = vp.store(2)
        if sparse_vox and s2._prep_fusevox[0] is not None:
            vp.linear(3, s2._prep_fusevox[0].get(), 1)
            fv_vox = vp.store(3)
        if rider and vp.fits_beside(rider[0]):
            vp.run(rider=rider.pop())       # the other network's head on workgroups of its own, inside this launch
        else:
            vp.run()
        # ---- stage-2 blocks (stage2fuse_blockadd.py:194-216)
        m = s2._ws.map("add0", imagefeatmap.n, imagefeatmap.h, imagefeatmap.w, imagefeatmap.c, 1, prec, dev)
        ops.bcast_add(imagefeatmap, fv_img, m)
        s2pool = ops.PoolReq(s2.poolimage.p, eps=s2.poolimage.eps, want_mean=True, want_gem=True, gem_out=out_rows.get('stg2imagevec'))
        imap = s2.ffnsimg[0].forward_map(m, prec, pool=s2pool)       # GeM + mean of the block's output ride in its last conv
        # (stored-map poolings: `mean` enters program 2 through a scaled load; the GeM -- an output -- is loaded scaled and stored
        # back over itself by that program, below)
        mean, stg2imagevec, s2scale = s2pool.mean, s2pool.gem, s2pool.scale
        if sparse_vox:
            vm = sparse.modules.seg_affine(voxmap, add=fv_vox)
            vm = s2.ffnsvox[0](vm, prec=prec)
            stg2voxvec = s2.poolvox(vm)
            vf = s2.projsvoxfuse[0][0](vm, prec=prec) if opt.stg2_useproj is True else vm
            voxvec_fuse = sparse.modules.global_avg_pool(vf)
        else:
            stg2voxvec, voxvec_fuse = data_dict['stg2voxvec'].float(), data_dict['voxvec_fuse'].float()
        # ---- program 2
        vt = VecProgram(b, dev)
        if s2._prep_imgfuse[0] is not None:
            vt.linear(0, s2._prep_imgfuse[0].get(), mean, scale=s2scale)
        else:
            vt.load(0, mean, s2scale)
        vt.load(1, fusevec)
        vt.load(2, voxvec_fuse.float())
        vt.wsum(1, [1, 0, 2])
        r = s2.ffnsfuse[0].emit(vt, 1, [0, 2, 3, 4, 5])
        vt.linear(0, self._prep_fc.get(), r)
        stg2fusevec = vt.store(0, out_rows.get('stg2fusevec'))
        regs, weights, nxt = [], [], 1
        for name, vec, wt in (('imageorg', imagevec_org, self.imageorg_weight), ('voxorg', voxvec_org, self.voxorg_weight),
                              ('shalloworg', shallow_n, self.shalloworg_weight), ('stg2image', stg2imagevec, self.stg2image_weight),
                              ('stg2vox', stg2voxvec, self.stg2vox_weight), ('stg2fuse', None, self.stg2fuse_weight)):
            if name not in opt.final_type:
                continue
            if vec is None:
                regs.append(0)
            else:
                if name == 'stg2image' and s2scale is not None:
                    regs.append(vt.load(nxt, vec, s2scale))
                    vt.store(nxt, vec)                      # the true GeM over the stored map's, in place
                    s2scale = None
                else:
                    regs.append(vt.load(nxt, vec.float()))
                nxt += 1
            weights.append(wt)
        if not regs:
            raise VecProgramUnfit("empty final_type")
        if s2scale is not None:                             # stg2imagevec is an output even when the final sum leaves it out
            if nxt >= 6:
                raise VecProgramUnfit("registers")
            vt.load(nxt, stg2imagevec, s2scale)
            vt.store(nxt, stg2imagevec)
        vt.wsum(nxt if nxt < 6 else 0, regs, weights)
        out = nxt if nxt < 6 else 0
        if opt.final_l2 is True:
            vt.l2norm(out, out)
        x = vt.store(out, out_rows.get('embedding'))
        vt.run()
        return {
            'imagevec_org': imagevec_org,
            'voxvec_org': voxvec_org,
            'shallowvec_org': shallow_org,
            'stg2fusevec': stg2fusevec,
            'stg2imagevec': stg2imagevec,
            'stg2voxvec': stg2voxvec,
            'embedding': x,
        }

    def forward(self, data_dict, mode):
        if mode == 'q':
            if self._convnext:
                return self.forward_q(data_dict)        # (no sub-stream split for this trunk)
            k = self.opt.query_substreams
            img = data_dict.get('query_image')
            if (k > 1 and not self.training and not torch.is_grad_enabled() and 'coords' not in data_dict and 'points' not in data_dict
                    and torch.is_tensor(img) and img.shape[0] % k == 0 and img.shape[0] >= 2 * k):
                return self._forward_q_substreams(data_dict, k)
            return self.forward_q(data_dict)
        raise NotImplementedError

    def _forward_q_substreams(self, data_dict, k):
        """Inference only: the batch as k equal sub-batches on k HIP streams (the caller's stream + k-1
        side streams owned by the module).  Same arithmetic per sample; one sub-batch's kernel tails
        overlap the others' kernels (a launch of the 3x3 conv kernel has only a few workgroups per CU at
        these sizes).  Module workspaces are keyed by the launching stream, so the passes do not collide."""
        dev = data_dict['query_image'].device
        cur = torch.cuda.current_stream(dev)
        # side streams per CALLING stream: two forwards in flight on two streams (two captured graphs replayed
        # back to back, bench.py --inflight 2) must not share side streams, whose ids key the workspaces
        key = (str(dev), k, cur.cuda_stream)
        pool = self.__dict__.setdefault('_substream_pool', {})
        if key not in pool:
            pool[key] = [torch.cuda.Stream(device=dev) for _ in range(k - 1)]
        substreams = pool[key]
        b = data_dict['query_image'].shape[0]
        hb = b // k

        def part(i):
            out = {}
            for name, v in data_dict.items():
                if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == b:
                    out[name] = v[i * hb:(i + 1) * hb]
                elif isinstance(v, (list, tuple)) and all(torch.is_tensor(t) and t.shape[0] == b for t in v):
                    out[name] = [t[i * hb:(i + 1) * hb] for t in v]
                else:
                    out[name] = v
            return out
        outs = [None] * k
        # whole-batch outputs; every sub-batch writes its row slice (the fused vector path: no concatenation afterwards)
        full = {name: torch.empty((b, self.opt.mm_stg2fuse_dim), dtype=torch.float32, device=dev) for name in self.OUT_KEYS}

        def rows(i):
            return {name: t[i * hb:(i + 1) * hb] for name, t in full.items()}
        for i, st in enumerate(substreams):
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                outs[i + 1] = self.forward_q(part(i + 1), out_rows=rows(i + 1))
        outs[0] = self.forward_q(part(0), out_rows=rows(0))
        for i, st in enumerate(substreams):
            cur.wait_stream(st)
            for t in outs[i + 1].values():
                t.record_stream(cur)
        for t in full.values():
            for st in substreams:
                t.record_stream(st)
        return {name: ops.join_rows([o[name] for o in outs]) for name in outs[0]}


def _check_convnext_options(opt):
    """mm_imgfe='convnext_tiny' is built for the one configuration in which the reference's own wiring is consistent: the last
    fusion level is nn.Identity() for the image and the voxel vector (fuse_block_toshallow.py:25-30), so the trunk's last plane
    (384), the last voxel plane and the fusion width must agree."""
    def refuse(field, why):
        raise NotImplementedError(f"MM with mm_imgfe='convnext_tiny': {field}={getattr(opt, field)!r} is not built: {why}; the "
                                  "supported configuration is mm_imgfe_layers='a_b_c', mm_imgfe_planes='96_192_384', mm_imgfe_dim=384, "
                                  "mm_stg2fuse_dim=384, mm_voxfe_planes='X_Y_384' (X, Y multiples of 64), mm_voxfe_dim=384")
    if len(opt.mm_imgfe_layers.split('_')) != 3:
        refuse("mm_imgfe_layers", "the ConvNeXt trunk takes exactly three block counts")
    if opt.mm_imgfe_planes != "96_192_384":
        refuse("mm_imgfe_planes", "the trunk's maps have 96, 192 and 384 channels")
    if opt.mm_imgfe_dim != 384:
        refuse("mm_imgfe_dim", "the trunk's last map has 384 channels")
    if opt.mm_stg2fuse_dim != 384:
        refuse("mm_stg2fuse_dim", "the last fusion level is an identity, so the fusion width is the last image plane, 384")
    vox = opt.mm_voxfe_planes.split('_')
    if len(vox) != 3 or not all(v.isdigit() for v in vox) or int(vox[2]) != 384 or any(int(v) % 64 or int(v) <= 0 for v in vox[:2]):
        refuse("mm_voxfe_planes", "the last fusion level is an identity, so the last voxel plane is 384, and the two lower planes "
                                  "are multiples of 64")
    if opt.mm_voxfe_dim != 384:
        refuse("mm_voxfe_dim", "the stage-2 voxel block runs on the last voxel plane, 384")


class _Pooled:
    """An already average-pooled level (saves re-reading l3, which GeM just streamed)."""

    def __init__(self, vec, exp=0):
        self.vec, self.exp = vec, exp          # exp: the pooled map's exponent -- vec is the true mean times 2^-exp

    @property
    def scale(self):
        return ops.pow2_scalar(self.vec.device, self.exp)

    def true(self):
        return ops.scale_pow2(self.vec, self.exp)
