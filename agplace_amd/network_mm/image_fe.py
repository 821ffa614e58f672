"""ImageFE, drop-in for reference network_mm/image_fe.py (ResNet18/34 branches, :10-46,97-113,153-174).

Constructor `ImageFE(fe_type, layers)` with layers like '2_2_2': only the COUNT of entries matters
for ResNets (reference :15-30).  forward(x[b,3,H,W]) -> (last_map, [l1, l2, l3(, l4)]) as fp32
tensors of logical shape [b,C,h,w] (channels_last memory).  `forward_maps` returns the same
stages as ops.SplitMap without the fp32 export (the fused MM / DBVanilla2D paths use it).
ConvNeXt / SqueezeNet branches of the reference are not built (never selected by its defaults).
"""
import torch.nn as nn

from .. import range_guard
from ..options import get_options
from ..resnet import ResNet


class ImageFE(nn.Module):
    _ALLOWED = ("resnet18", "resnet34")
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
        self.last_dim = self._LAST_DIM[fe_type][len(layers)]
        self.fe = ResNet(fe_type, nstages=len(layers))

    def forward_maps(self, x, prec=None, level_means=None, final_pool=None):
        """prec: MFMA precision mode (include/agplace_hip.h); None = the process-wide Options.mfma_precision, i.e. the
        precision MM / DBVanilla2D run this trunk at."""
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
        prec = self.export_precision() if prec is None else prec
        # the fp16 range guard of the op-level drop-in (Options.fp16_range_guard): around its own forward only -- inside MM /
        # DBVanilla2D the trunk's maps report through the model that runs it
        with range_guard.guarded(self, self.opt or get_options(), prec, self.training):
            maps = self.forward_maps(x, prec=prec)
            x_list = [m.to_f32() for m in maps]
        return x_list[-1], x_list

    def poll_fp16_range(self):
        """NON-BLOCKING fp16 range check of the guarded forwards so far (MM.poll_fp16_range)."""
        range_guard.poll(self)

    def fp16_range_ok(self):
        """False if a guarded forward since the last report stored a saturated fp16 map value (MM.fp16_range_ok)."""
        return range_guard.ok(self)
