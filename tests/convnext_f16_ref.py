"""The fp64 restatement of tests/convnext_ref.py's truncated trunk with a rounding hook at the six places where the trunk's
precision 4 (Options.convnext_precision = 4) rounds to fp16:

    1. the block's LayerNorm output (the MLP's operand)      4. W2
    2. W1                                                    5. the downsample's LayerNorm output
    3. the GELU output (the hidden map)                      6. the downsample's weight

Everything else (stem, depthwise conv, LayerNorm statistics, biases, GELU, layer_scale, residual add, accumulation) is the fp64
arithmetic of the model it is handed.  `rnd=None` rounds nowhere and gives the truth; `rnd=round_f16` emulates precision 4.
"""
import numpy as np
import torch
import torch.nn.functional as F

import convnext_ref as R


def round_f16(t):
    """fp16(t) as fp64: round to nearest even (numpy rounds fp64 -> fp16 directly), saturating at +-65504, NaN kept."""
    a = t.detach().double().clamp(-65504.0, 65504.0).numpy()
    return torch.from_numpy(a.astype(np.float16).astype(np.float64))


def _r(rnd, t):
    return t if rnd is None else rnd(t)


def block_operand(blk, x):
    """Depthwise 7x7 + LayerNorm of the NCHW map x -> the MLP's operand [n,h,w,C], before rounding place 1."""
    return blk.block[2](blk.block[0](x).permute(0, 2, 3, 1))


def block_mlp(blk, xn, resid, rnd=None):
    """resid + layer_scale * MLP(xn) for an operand xn [..., C] (places 1-4 rounded); resid [..., C]."""
    l1, l2 = blk.block[3], blk.block[5]
    hid = R.gelu_exact(F.linear(_r(rnd, xn), _r(rnd, l1.weight), l1.bias))
    y = F.linear(_r(rnd, hid), _r(rnd, l2.weight), l2.bias)
    return resid + blk.layer_scale.reshape(-1) * y


def block(blk, x, rnd=None):
    """One CNBlock on the NCHW map x."""
    return block_mlp(blk, block_operand(blk, x), x.permute(0, 2, 3, 1), rnd).permute(0, 3, 1, 2)


def downsample(layer, x, rnd=None):
    """LayerNorm2d + Conv2d(C, 2C, k=2, s=2) on the NCHW map x (places 5 and 6 rounded)."""
    ln, conv = layer
    return F.conv2d(_r(rnd, ln(x)), _r(rnd, conv.weight), conv.bias, stride=2)


@torch.no_grad()
def forward_maps(model, x, rnd=None):
    """Outputs of features[1], [3], [5] of a truncated trunk (convnext_ref.trunk / seeded_trunk), as convnext_ref.forward_maps."""
    out = []
    for i, layer in enumerate(model.features.children()):
        if i == 0:
            x = layer(x)
        elif i in (1, 3, 5):
            for blk in layer:
                x = block(blk, x, rnd)
            out.append(x)
        else:
            x = downsample(layer, x, rnd)
    return out
