"""Hot-path configuration (the subset of the reference's `opt` the path reads).

The reference evaluates one global argparse namespace at import time in every module
(`opt = parse_arguments()`, e.g. network_mm/ffns.py:10-11).  Here the same fields, with the
same names and defaults (reference tools/options.py:28-58,85-155,221), live in an explicit
dataclass; `from_reference_opt(ns)` adapts a reference namespace.  `set_options()` installs
the process-wide default that modules pick up when no explicit `opt` is passed, which keeps
the reference's zero-argument constructors (`MM()`, `GeM()`, `DiffBlock(dim, ode_dim)`).
"""
from dataclasses import dataclass, field, fields
from typing import List, Optional, Tuple


@dataclass
class Options:
    # data / retrieval
    maptype: str = "satellite"
    features_dim: int = 256
    train_batch_size: int = 16
    infer_batch_size: int = 32
    negs_num_per_query: int = 10
    neg_samples_num: int = 1000
    recall_values: List[int] = field(default_factory=lambda: [1, 5, 10, 20])
    # voxel size in metres of the lidar front end (reference tools/options.py:61); read when MM.forward_q gets raw `points`
    quant_size: float = 2.0
    # shorter edge in pixels that the camera front end resizes decoded frames to (reference tools/options.py:64,66; torchvision
    # Resize(int) on the PIL frame): read when MM.forward_q gets `query_frames` / DBVanilla2D.forward_db gets `db_frames`.  The
    # reference's nuScenes loader hard-codes 192 for the cameras (datasets_ws_nuscenes.py:608): set q_resize=192 there
    q_resize: int = 256
    db_resize: int = 256
    # torchvision CenterCrop(db_cropsize) on the aerial tile in front of Resize(db_resize) (reference tools/options.py,
    # datasets_ws_kitti360.py:257-262): applied to `db_frames` as a region of interest of the resize launch.  None = no crop (the
    # nuScenes loader has it commented out)
    db_cropsize: Optional[int] = None
    # torchvision ColorJitter(j, j, j, hue=min(0.5, j)) strengths of the training loaders (datasets_ws_kitti360.py:236-280): what
    # input_pipeline.color_jitter is called with for the `query_jitter` / `db_jitter` records; 0 = no jitter.  The models apply the
    # records they are handed and never draw any themselves
    q_jitter: float = 0.0
    db_jitter: float = 0.0
    # Normalize(mean, std) of every uint8 camera route (tiles, frames, the walking stem); fp32 `query_image` / `db_map` arrive
    # normalised.  ImageNet's constants (the nuScenes loader); the KITTI-360 loader uses 0.5 / 0.22 (from_reference_opt)
    image_mean: Tuple[float, float, float] = (0.485, 0.456, 0.406)
    image_std: Tuple[float, float, float] = (0.229, 0.224, 0.225)
    # database model
    dbimage_fe: str = "resnet18"
    dbimage_fe_layers: str = "2_2_2"
    share_dbfe: bool = False
    # query model
    mm_imgfe: str = "resnet18"
    mm_imgfe_layers: str = "2_2_2"
    mm_imgfe_planes: str = "64_128_256"
    mm_imgfe_dim: int = 256
    mm_voxfe_layers: str = "1_1_1"
    mm_voxfe_planes: str = "64_128_256"
    mm_voxfe_ntd: int = 0
    mm_voxfe_dim: int = 256
    mm_bevfe_planes: str = "64_128_256"
    mm_bevfe_dim: int = 256
    mm_stg2fuse_dim: int = 256
    output_type: List[str] = field(default_factory=lambda: ["image", "vox", "shallow"])
    output_l2: bool = True
    final_type: List[str] = field(
        default_factory=lambda: ["imageorg", "voxorg", "shalloworg", "stg2image", "stg2vox"])
    final_fusetype: str = "add"
    final_l2: bool = False
    image_weight: float = 1.0
    image_learnweight: bool = False
    vox_weight: float = 1.0
    vox_learnweight: bool = False
    shallow_weight: float = 1.0
    shallow_learnweight: bool = False
    diff_type: str = "fcode@relu"
    diff_direction: str = "backward"
    odeint_method: str = "euler"
    odeint_size: float = 0.1
    tol: float = 1e-3                 # rtol = atol of an adaptive solver (odeint_method = "dopri5" | "bosh3"); fixed grids ignore it
    odeint_max_steps: int = 64        # attempted steps after which an adaptive solve gives up and returns NaN (torchdiffeq: 2^31 - 1)
    imagevoxorg_weight: float = 0.0
    imagevoxorg_learnweight: bool = False
    shalloworg_weight: float = 1.0
    shalloworg_learnweight: bool = False
    stg2imagevox_weight: float = 0.1
    stg2imagevox_learnweight: bool = False
    stg2fuse_weight: float = 0.0
    stg2fuse_learnweight: bool = False
    stg2nlayers: int = 1
    stg2fuse_type: Optional[str] = "basic"
    stg2_type: str = "full"
    stg2_useproj: bool = True
    # MI355X build: MFMA operand precision of the INFERENCE convolutions (include/agplace_hip.h):
    #   4 = F16 (library default since round 5 = what bench.py measures): fp16 activations x fp16 weights, ONE MFMA product;
    #       descriptors 2.4e-4 .. 3.8e-4, feature maps 4.5e-4 .. 8.5e-4 at the bench size (bar 1e-3;
    #       tests/test_gpu_models.py holds every descriptor under 5e-4, also with checkpoint-like statistics); the 64-channel
    #       BasicBlocks of layer 1 run as one fused kernel (csrc/fblock64.hip)
    #   2 = F16W2 (the opt-in "tight" mode; the default of rounds 1-4): fp16 activations x fp16 hi + (e4m3) lo weights, 1.5 MFMA
    #       products; descriptors 3e-5 .. 1.6e-4, maps <= 6e-4 relative to fp32 -- the weights' rounding, a coherent
    #       perturbation, is what the lo product removes; about half the throughput of mode 4
    #   3 = BF16X3: split-bf16 activations and weights, three products, ~1e-5 everywhere, fp32 range
    # Modes 2 and 4 store fp16 maps, which saturate at +-65504: the first inference forward after a weight (re)load counts
    # saturated map elements and warns (resnet.SATURATION_CHECK).  Such a checkpoint stays in modes 2 / 4 with calibrated map
    # exponents (agplace_amd/map_exponents.py: the image path's maps stored times 2^-e, folded into host-prepared constants --
    # same kernels, same speed); mode 3 remains the remedy for what they do not cover (the sparse-voxel branch's maps).  Training
    # (.train()) always runs on split-bf16 maps (3); kNN has its own setting.  The ConvNeXt-tiny trunk (dbimage_fe / mm_imgfe =
    # "convnext_tiny") does not read this field: it follows convnext_precision below.
    mfma_precision: int = 4
    # Opt-in fp16 range guard (agplace_amd/range_guard.py): inference forwards in modes 2 / 4 bind a sticky device word that
    # every kernel storing an inference fp16 map (the table in DESIGN.md section 2) sets when it had to clamp a value to +-65504
    # -- eager forwards then raise ValueError
    # (one call late; the last call by fp16_range_ok()), captured replays publish it to pinned memory for poll_fp16_range().
    # Stored values are the same bits either way.  Mode 3 stores no fp16 maps and never binds; training forwards never bind through
    # this option (their fp16 planes have a switch of their own, train_range_guard below).  Independent of the
    # first-forward warning above (resnet.SATURATION_CHECK).
    fp16_range_guard: bool = False
    # TRAINING (.train(), or .eval() with gradients): 32 (default) = the tight mode -- split-bf16 maps, three MFMA products in
    # every forward and data-gradient conv, one fp16 product in the weight gradients; every parameter gradient within 1e-3 of
    # fp64 autograd (tests/test_gpu_train.py).  16 = the opt-in FAST mode: the forward of the 3x3 stride-1 convs as ONE
    # fp16 x fp16 product (train_graph.FWD_F16; fp32 master weights, fp64-finalised statistics, three-product data gradients);
    # gradient error and cosine against the fp64 oracle: tests/test_gpu_train.py (FASTGRAD lines of
    # test_resnet_trunk_training_gradients[fast] / [dgrad1] and the end-to-end tests' fast cases), timing: bench.py train.fast_mode.
    train_precision: int = 32
    # 3 (default) | 1 = opt-in: the data gradients of the 3x3 convs as ONE bf16 product of the hi planes (train_graph.DGRAD_HI_ONLY),
    # usually together with train_precision = 16; measured error: tests/test_gpu_train.py, timing: bench.py train.fast_mode
    train_dgrad_products: int = 3
    # Opt-in fp16 range guard of the TRAINING forwards (.train(), or .eval() under autograd / frozen BatchNorm), in both
    # train_precision modes: the training graph stores fp16 too -- the fast mode's pre-BatchNorm planes z16 and conv1 -> conv2
    # planes y16, and in both modes the fp16 operand planes of the one-pass weight gradient (the inventory in DESIGN.md section
    # 2) -- all saturating at +-65504.  With the option the model's guard word (agplace_amd/range_guard.py, the contract of
    # fp16_range_guard) is bound around every training forward, not the backward (which stores no fp16 map), and published after
    # it: poll_fp16_range() / fp16_range_ok() then cover training forwards.  The guard reports; it does not rescue.  Stored values
    # are the same bits either way; off (default) = as before, launch for launch.  ConvNeXt trunks store no fp16 in training: the
    # option is accepted with them and binds nothing there.  Not a reference option: from_reference_opt leaves it False.
    train_range_guard: bool = False
    # Opt-in training of the ConvNeXt-tiny trunk (dbimage_fe / mm_imgfe = "convnext_tiny"): DBVanilla2D and MM then call
    # ConvNeXt.enable_training() on its trunks, so .train() (torchvision's stochastic depth, p_k = 0.1 k / 17) and gradients into
    # the trunk run on the kernels of csrc/convnext_bwd.hip (mode-3 products, fixed-order sums: repeatable bit for bit).  False
    # (default): the trunk is inference only and refuses both, as before.  A reference namespace does not carry this field:
    # from_reference_opt(args).copy(convnext_train=True).
    convnext_train: bool = False
    # Opt-in uint8 inputs of the ConvNeXt-tiny trunk: DBVanilla2D and MM then call ConvNeXt.enable_u8_inputs() and
    # set_image_norm(image_mean, image_std) on its trunks, which take uint8 tiles (`db_map`, `query_image`) and decoded frames
    # (`db_frames` / `query_frames`, with db_cropsize, db_jitter / query_jitter) as the ResNet models do: the resize and the jitter
    # write uint8 tiles, the stem normalises them as it reads (csrc/convnext.hip), bit for bit the fp32 route on
    # ops.normalize_cameras_u8's image.  False (default): those inputs are refused by name, as before.  A reference namespace does
    # not carry this field (from_reference_opt leaves it False): from_reference_opt(args).copy(convnext_u8=True).
    convnext_u8: bool = False
    # MFMA operand precision of the ConvNeXt-tiny trunk's INFERENCE path (ConvNeXt.forward_maps; ConvNeXt.set_precision is the
    # op-level form): 3 (default) = bf16 (hi, lo) pairs, three products, as before, launch for launch and bit for bit.  4 = opt-in:
    # the block's LayerNorm output, W1, the GELU output, W2, the downsample's LayerNorm output and its weight are rounded to fp16
    # (nearest even, saturating at +-65504) and every product is ONE fp16 MFMA with fp32 accumulation; the stream, the stem, the
    # depthwise conv, LayerNorm statistics, biases, GELU, layer_scale and the residual add stay fp32 (maps
    # within 1e-3 of fp64).  The training forward and the backward stay in mode 3 whatever this says, the rule mfma_precision has
    # for the ResNets.  4 together with fp16_range_guard is refused (NotImplementedError): the guard's word is not wired into these
    # kernels -- unless convnext_range_guard below is on.  Not a reference option: from_reference_opt leaves it 3.
    convnext_precision: int = 3
    # Opt-in fp16 range guard of the ConvNeXt-tiny trunk's precision 4: the six operands that mode rounds to fp16 saturate at
    # +-65504 and a clamped forward returns finite, wrong maps.  With the switch every INFERENCE forward of a trunk at
    # convnext_precision = 4 binds the model's guard word (agplace_amd/range_guard.py, the contract of fp16_range_guard: eager
    # forwards raise ValueError one call late, fp16_range_ok() closes a loop, captured replays publish for poll_fp16_range()); the
    # guarded twins of the three precision-4 kernels report a block's LayerNorm output, the GELU output and a downsample's LayerNorm
    # output beyond fp16's range, and every forward reports a clamped W1 / W2 / downsample weight plane.  The
    # guard reports; it does not rescue: convnext_precision = 3 is the remedy.  ImageFE on its own binds its own guard;
    # DBVanilla2D and MM bind theirs (MM with fp16_range_guard too: ONE word over the trunk, stage 2 and the voxel branch; with
    # this switch alone the trunk only).  With it, convnext_precision = 4 together with fp16_range_guard is accepted.  Stored values
    # are the same bits either way; off (default) = as before, launch for launch and text for text.  With precision 3, on ResNet
    # trunks and on every training forward (mode 3 whatever is set) it is accepted and binds nothing.  Not a reference option:
    # from_reference_opt leaves it False.
    convnext_range_guard: bool = False
    # Opt-in lock-step ConvNeXt trunks in agplace_amd.pair.embed_pair / pair.CapturedPair: with the switch on in BOTH models' Options
    # (mm_imgfe = dbimage_fe = "convnext_tiny", the same three block counts and convnext_precision, at most 4 trunks, no ConvNeXt
    # range-guard tag binding on either model) the query trunk and the map-type trunks advance together and every step -- stem, a
    # block's depthwise conv + LayerNorm, its MLP, a downsample -- is ONE grouped launch (ConvNeXt.forward_maps_multi ->
    # agp_cnx_*_fwd_grouped); MM.forward_q(image_maps=...) and DBVanilla2D.forward_db(trunk_maps=...) then take the maps.  Outputs are
    # bit for bit those of the two separate forwards, which embed_pair still returns for a pair that does not qualify (a guarded,
    # mixed or unequal pair).  Query sub-streams stay refused for this trunk.  False (default): embed_pair and both arguments refuse
    # a ConvNeXt model as before, text for text.  Not a reference option: from_reference_opt leaves it False.
    convnext_pair: bool = False
    # Opt-in one-launch routes of FCODE(384) (the Neural-ODE blocks of MM on the ConvNeXt-tiny trunk): with a gradient wanted a
    # fixed-grid solve records its trajectory in the one-launch kernel and differentiates through agp_fcode_wide_bwd instead of
    # the any-width sequence of launches, and odeint_method = "dopri5" runs on the adaptive kernels at 384 columns instead of
    # being refused (csrc/fusion_wide.hip, csrc/fusion_adaptive.hip).  False (default): FCODE(384) routes
    # as before, launch for launch.  Other widths ignore it.  A reference namespace does not carry this field
    # (from_reference_opt leaves it False): from_reference_opt(args).copy(fcode_wide=True).
    fcode_wide: bool = False
    # Opt-in further members of torchdiffeq's adaptive Runge-Kutta family: odeint_method = "bosh3" (Bogacki-Shampine 3(2)) then
    # runs on the adaptive kernels (csrc/fusion_adaptive.hip, the Tableau Bosh3) at 256 columns, and at 384
    # columns together with fcode_wide, exactly as "dopri5" does.  False (default): FCODE refuses "bosh3" with
    # NotImplementedError, as before.  "dopri5" does not need it.  A reference namespace does not carry this field
    # (from_reference_opt leaves it False): from_reference_opt(args).copy(odeint_adaptive_family=True).
    odeint_adaptive_family: bool = False
    # Opt-in level capacity of the raw-points route (MM.forward_q from `points` / `point_offsets`, inference and training): an upper
    # bound on the voxels of a whole batch, None or an int in 1 .. 2^30 - 1.  With a value every level of the voxel branch has that
    # many rows instead of one per raw point (SparseTensor.from_points_capacity / from_points_levels, level_capacity);
    # a batch of more distinct voxels is reported as a "voxel capacity" ValueError (bit 2 of the voxel flag) and its voxel branch
    # sees an empty cloud.  The `coords` route ignores it.  Not a reference option: from_reference_opt leaves it None.
    voxel_capacity: Optional[int] = None
    # inference: MM.forward embeds a batch as this many sub-batches on as many HIP streams (1 = off)
    query_substreams: int = 1
    # inference: the vector path (everything after the backbones) as two program launches (agplace_amd/vecprog.py) instead
    # of one launch per Linear / FCODE / LayerNorm / normalize / weighted sum; False selects the per-op path
    fused_vector_path: bool = True
    knn_precision: int = 4      # coarse pass: 4 = fp16 (default, fastest), 3 = split-bf16, 1 = bf16; the result is exact in all
    # losses (tools/options.py:158-159,169,189,48,35)
    otherloss_type: str = "bce"
    otherloss_weight: float = 0.01
    tripletloss_weight: float = 1.0
    margin: float = 0.1
    criterion: str = "triplet"
    negs_num_per_query: int = 10
    train_batch_size: int = 16
    train_positives_dist_threshold: int = 10      # tools/options.py:45
    val_positive_dist_threshold: int = 25         # tools/options.py:44

    def __post_init__(self):
        self.validate()

    def validate(self):
        # the training modes are selected by value (train_precision == 16, train_dgrad_products == 1): anything else would
        # silently give the tight mode
        if self.train_precision not in (16, 32):
            raise ValueError(f"train_precision {self.train_precision!r}: 32 (tight) | 16 (one-product forward convs)")
        if self.train_dgrad_products not in (1, 3):
            raise ValueError(f"train_dgrad_products {self.train_dgrad_products!r}: 3 (tight) | 1 (one-product data gradients)")
        if not (isinstance(self.odeint_max_steps, int) and 1 <= self.odeint_max_steps <= 4096):
            raise ValueError(f"odeint_max_steps {self.odeint_max_steps!r}: an integer in 1 .. 4096")
        for name in ("q_resize", "db_resize"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"{name} {v!r}: a positive integer (the shorter edge after the resize)")
        v = self.db_cropsize
        if v is not None and (isinstance(v, bool) or not isinstance(v, int) or v < 1):
            raise ValueError(f"db_cropsize {v!r}: None or a positive integer (the side of the centre crop)")
        for name in ("q_jitter", "db_jitter"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not (0.0 <= v < float("inf")):
                raise ValueError(f"{name} {v!r}: a finite number >= 0 (the ColorJitter strength)")
        for name in ("image_mean", "image_std"):
            v = getattr(self, name)
            if (not isinstance(v, (tuple, list)) or len(v) != 3
                    or any(isinstance(c, bool) or not isinstance(c, (int, float)) or not (abs(c) < float("inf")) for c in v)):
                raise ValueError(f"{name} {v!r}: three finite numbers")
            setattr(self, name, tuple(float(c) for c in v))
        if any(c <= 0.0 for c in self.image_std):
            raise ValueError(f"image_std {self.image_std!r}: every component must be positive")
        if not isinstance(self.convnext_train, bool):
            raise ValueError(f"convnext_train {self.convnext_train!r}: True | False")
        if not isinstance(self.convnext_u8, bool):
            raise ValueError(f"convnext_u8 {self.convnext_u8!r}: True | False")
        v = self.convnext_precision
        if isinstance(v, bool) or not isinstance(v, int) or v not in (3, 4):
            raise ValueError(f"convnext_precision {v!r}: 3 (three bf16 products) | 4 (one fp16 product, inference only)")
        if not isinstance(self.fcode_wide, bool):
            raise ValueError(f"fcode_wide {self.fcode_wide!r}: True | False")
        if not isinstance(self.odeint_adaptive_family, bool):
            raise ValueError(f"odeint_adaptive_family {self.odeint_adaptive_family!r}: True | False")
        if not isinstance(self.fp16_range_guard, bool):
            raise ValueError(f"fp16_range_guard {self.fp16_range_guard!r}: True | False")
        if not isinstance(self.train_range_guard, bool):
            raise ValueError(f"train_range_guard {self.train_range_guard!r}: True | False")
        if not isinstance(self.convnext_range_guard, bool):
            raise ValueError(f"convnext_range_guard {self.convnext_range_guard!r}: True | False")
        if not isinstance(self.convnext_pair, bool):
            raise ValueError(f"convnext_pair {self.convnext_pair!r}: True | False")
        v = self.voxel_capacity
        if v is not None and (isinstance(v, bool) or not isinstance(v, int) or not 1 <= v < (1 << 30)):
            raise ValueError(f"voxel_capacity {v!r}: None or an integer in 1 .. 2^30 - 1 (rows of every level from raw points)")

    def copy(self, **kw):
        d = {f.name: getattr(self, f.name) for f in fields(self)}
        d.update(kw)
        return Options(**d)


def from_reference_opt(ns) -> Options:
    """Adapt a reference argparse namespace (tools/options.py) to Options."""
    o = Options()
    for f in fields(Options):
        if hasattr(ns, f.name) and f.name not in ("convnext_u8", "convnext_precision", "fcode_wide", "odeint_adaptive_family", "voxel_capacity", "train_range_guard", "convnext_range_guard", "convnext_pair"):      # (not reference options: stay at their defaults)
            v = getattr(ns, f.name)
            if f.name in ("output_type", "final_type") and isinstance(v, str):
                v = v.split("_")
            setattr(o, f.name, v)
    if getattr(ns, "dataset", None) == "kitti360":
        # the KITTI-360 loader's Normalize (datasets_ws_kitti360.py:236-280); every other loader uses ImageNet's constants
        o.image_mean, o.image_std = (0.5,) * 3, (0.22,) * 3
    else:
        # db_cropsize is only live in the KITTI-360 loader (the nuScenes one has the crop commented out)
        o.db_cropsize = Options.__dataclass_fields__["db_cropsize"].default
    o.validate()
    return o


_default = Options()


def get_options() -> Options:
    return _default


def set_options(o: Options) -> Options:
    global _default
    _default = o
    return o
