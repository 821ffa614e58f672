"""ImageFE, drop-in for reference network_mm/image_fe.py (ResNet18/34 branches, :10-46,97-113,153-174; the
convnext_tiny branch, :59-88,118-150).

Constructor `ImageFE(fe_type, layers)` with layers like '2_2_2': only the COUNT of entries matters
for ResNets (reference :15-30).  forward(x[b,3,H,W]) -> (last_map, [l1, l2, l3(, l4)]) as fp32
tensors of logical shape [b,C,h,w] (channels_last memory).  `forward_maps` returns the same
stages as ops.SplitMap without the fp32 export (the fused MM / DBVanilla2D paths use it).

'convnext_tiny' (agplace_amd/convnext.py) is inference only unless `fe.enable_training()` opted in (then .train() and gradients
into the trunk run through ConvNeXt.forward_maps_train); it takes exactly three `layers` entries, which are BLOCK COUNTS
there: features[6:] are dropped and stage i keeps its first layers[i] blocks, last_dim = 384, the list holds the outputs of
features[1], [3], [5].  It runs in the mode-3 arithmetic (prec None or 3) unless Options.convnext_precision = 4 of `opt` (or
`fe.set_precision(4)`) selected the one-product fp16 inference mode (with Options.convnext_range_guard its saturating operands
report through this module's fp16 range guard, or through the model's when a model runs it), and has no ops.SplitMap form:
`forward_maps` with pool requests raises NotImplementedError.  The SqueezeNet branch of the reference is not built.
"""
import torch.nn as nn

from .. import range_guard
from ..options import get_options
from ..convnext import ConvNeXt
from ..resnet import ResNet


class ImageFE(nn.Module):
    _ALLOWED = ("resnet18", "resnet34", "convnext_tiny")
    _LAST_DIM = {"resnet18": {2: 128, 3: 256, 4: 512}, "resnet34": {2: 128, 3: 256, 4: 512},
                 "resnet50": {2: 512, 3: 1024, 4: 2048}}

    def __init__(self, fe_type, layers, opt=None):
        super().__init__()
        self.opt = opt              # None: the process-wide options at call time (get_options())
        self.fe_type = fe_type
        layers = [int(x) for x in layers.split('_')]
        self.layers = layers
        if fe_type not in self._ALLOWED or len(layers) not in (2, 3, 4):
            raise NotImplementedError
        if fe_type == "convnext_tiny":
            if len(layers) == 2:
                raise NotImplementedError      # as the reference (image_fe.py:72-76)
            if len(layers) == 4:
                raise NotImplementedError("ImageFE('convnext_tiny') with four `layers` entries: the reference returns the three maps of "
                                          "features[1], [3], [5] under last_dim = 768, which breaks its own head (the last map has "
                                          "384 channels); use three entries")
            self.last_dim = 384
            # the Options of the MODEL that runs this trunk (DBVanilla2D sets it; None: used on its own): with its
            # convnext_range_guard the trunk's precision-4 operands report through that model's guard, not this module's
            self.model_opt = None
            # Options.convnext_precision of `opt` (None: the process-wide options now); MM / DBVanilla2D set their own afterwards
            self.fe = ConvNeXt(layers).set_precision((opt or get_options()).convnext_precision)
            return
        self.last_dim = self._LAST_DIM[fe_type][len(layers)]
        self.fe = ResNet(fe_type, nstages=len(layers))

    def forward_maps(self, x, prec=None, level_means=None, final_pool=None):
        """prec: MFMA precision mode (include/agplace_hip.h); None = the process-wide Options.mfma_precision, i.e. the
        precision MM / DBVanilla2D run this trunk at."""
        if self.fe_type == "convnext_tiny":
            raise NotImplementedError("ImageFE('convnext_tiny').forward_maps: the ConvNeXt trunk has no ops.SplitMap form (plain fp32 "
                                      "maps, no pool requests); use forward(x) or fe.forward_maps(x)")
        if len(self.layers) not in (3, 4):
            raise NotImplementedError      # reference forward_resnet raises for 2 entries too
        prec = get_options().mfma_precision if prec is None else prec
        return self.fe.forward_maps(x, prec=prec, level_means=level_means, final_pool=final_pool)

    # The op-level drop-in EXPORTS its stage maps (reference image_fe.py:97-113 returns them), so its default is the mode whose
    # MAPS meet the 1e-3 bar on every supported trunk: the one-product mode 4 holds that on ResNet18 (<= 8.5e-4) but not 14 residual
    # blocks deep (ResNet34 layer 3: 1.0e-3; mode 4's contract is on the network OUTPUTS, which MM / DBVanilla2D pool from maps
    # they never export).  prec=None therefore means: the tight two-product mode when the process default is 4.
    def export_precision(self):
        p = get_options().mfma_precision
        return 2 if p == 4 else p

    def forward(self, x, prec=None):
        if self.fe_type == "convnext_tiny":
            if prec not in (None, 3):
                raise ValueError(f"ImageFE('convnext_tiny'): prec must be None or 3 (three bf16 products, fp32 maps), got {prec}")
            if self.fe.precision == 4:
                if prec == 3:
                    raise ValueError("ImageFE('convnext_tiny'): prec=3 on a trunk set to precision 4; call fe.set_precision(3)")
                # (inside a model that turned convnext_range_guard on, the model has accepted the combination and binds its guard)
                in_guarded_model = self.model_opt is not None and self.model_opt.convnext_range_guard
                o = self.opt or get_options()
                if o.fp16_range_guard and not o.convnext_range_guard and not in_guarded_model:
                    raise NotImplementedError("ImageFE('convnext_tiny'): precision 4 together with fp16_range_guard=True is not "
                                              "built (the guard's word is not wired into the fp16 ConvNeXt kernels)")
            # Options.convnext_range_guard of the op-level drop-in: its own guard around its own INFERENCE forward at precision 4 --
            # inside DBVanilla2D / MM it binds nothing, the report goes through the model that runs it (the ResNet path's rule below)
            tag = None
            if self.model_opt is None and not self.fe.takes_training_path():
                tag = range_guard.cnx_tag(self.opt or get_options(), self.fe.precision)
            with range_guard.guarded_cnx(self, tag):
                x_list = self.fe.forward_maps(x)
            return x_list[-1], x_list
        prec = self.export_precision() if prec is None else prec
        # the fp16 range guard of the op-level drop-in (Options.fp16_range_guard): around its own forward only -- inside MM /
        # DBVanilla2D the trunk's maps report through the model that runs it
        with range_guard.guarded(self, self.opt or get_options(), prec, self.training):
            maps = self.forward_maps(x, prec=prec)
            x_list = [m.to_f32() for m in maps]
        return x_list[-1], x_list

    def forward_maps_train(self, x, slot=0):
        """The op-level forward on the TRAINING graph: the trunk's `fe.forward_maps_train(x)` (batch-statistics BatchNorm in
        .train(), what `fe.backward_maps` needs recorded) under THIS module's Options, as MM.forward_q / DBVanilla2D.forward_db run
        their trunks: train_precision / train_dgrad_products select the mode for this forward only (train_graph.training_mode), and
        with train_range_guard the module's fp16 range guard is bound around the forward and published behind it, so that
        poll_fp16_range() / fp16_range_ok() cover it.  Returns the stage outputs (ops.SplitMap; ConvNeXt: fp32 tensors).  The
        ConvNeXt trunk stores no fp16 in training and ignores both: nothing is bound there."""
        opt = self.opt or get_options()
        if self.fe_type == "convnext_tiny":
            return self.fe.forward_maps_train(x)
        from .. import train_graph
        with train_graph.training_mode(opt.train_precision == 16, opt.train_dgrad_products == 1), \
                range_guard.guarded_train(self, opt):
            return self.fe.forward_maps_train(x, slot=slot)

    def poll_fp16_range(self):
        """NON-BLOCKING fp16 range check of the guarded forwards so far (MM.poll_fp16_range)."""
        range_guard.poll(self)

    def fp16_range_ok(self):
        """False if a guarded forward since the last report stored a saturated fp16 map value (MM.fp16_range_ok)."""
        return range_guard.ok(self)
