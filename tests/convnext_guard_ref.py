"""What the fp16 range guard of the ConvNeXt trunk's precision 4 (Options.convnext_range_guard) must report, from the fp64
restatement (tests/convnext_f16_ref.py): the largest |value| that reaches each of the six rounding places

    1. the block's LayerNorm output      3. the GELU output      5. the downsample's LayerNorm output
    2. W1                                4. W2                   6. the downsample's weight

per stage, BEFORE the rounding; the guard's flag is `any maximum > 65504`.  Values are propagated as the device propagates them
(rounded to fp16 at the six places, saturating), so a planted saturation reaches the later places the way the kernels see it.

The planting helpers edit a seeded trunk so that exactly ONE place of ONE stage leaves fp16's range and nothing downstream feels
it: the saturated element always meets an exact zero on the other side of its product (a zeroed weight column / row, or a channel
whose LayerNorm gamma and beta are zero), and 65504 x 0 = 0 in the kernels as in the reference.
"""
import copy

import torch
import torch.nn.functional as F

import convnext_f16_ref as H
import convnext_ref as R

LIMIT = 65504.0
SEED = 2
LAYERS = [1, 1, 1]
PLACES = (1, 2, 3, 4, 5, 6)
# (place, stage) of every planted case: the downsample (places 5, 6) follows stages 0 and 1 only
CASES = tuple((place, stage) for place in PLACES for stage in ((0, 1, 2) if place <= 4 else (0, 1)))
BIG = 3.0 * LIMIT           # a planted value: well above 2 x 65504, exactly representable


def _amax(t):
    return float(t.detach().double().abs().max())


@torch.no_grad()
def operand_maxima(model, x):
    """{(stage, place): fp64 max |value| before rounding} of the truncated fp64 trunk `model` on the image x [n,3,H,W]."""
    out = {}
    x = x.double()
    for i, layer in enumerate(model.features.children()):
        if i == 0:
            x = layer(x)
        elif i in (1, 3, 5):
            s = (i - 1) // 2
            acc = {p: 0.0 for p in (1, 2, 3, 4)}
            for blk in layer:
                l1, l2 = blk.block[3], blk.block[5]
                xn = H.block_operand(blk, x)
                hid = R.gelu_exact(F.linear(H.round_f16(xn), H.round_f16(l1.weight), l1.bias))
                for p, v in ((1, xn), (2, l1.weight), (3, hid), (4, l2.weight)):
                    acc[p] = max(acc[p], _amax(v))
                x = H.block(blk, x, H.round_f16)
            for p, v in acc.items():
                out[(s, p)] = v
        else:
            s = (i - 2) // 2
            ln, conv = layer
            out[(s, 5)], out[(s, 6)] = _amax(ln(x)), _amax(conv.weight)
            x = H.downsample(layer, x, H.round_f16)
    return out


def expected_flag(maxima):
    return any(v > LIMIT for v in maxima.values())


def clean_trunk():
    """The seeded '1_1_1' trunk, fp64."""
    return R.seeded_trunk(LAYERS, SEED, torch.float64)


def image(shape, seed=SEED):
    return R.seeded_input(shape, seed)


@torch.no_grad()
def plant(model, place, stage, x, value=BIG):
    """A copy of the fp64 trunk `model` in which place `place` of stage `stage` reaches |value| on the image x and no other place
    feels it.  Channel / unit indices are fixed (3 and 5) so that a case is reproducible."""
    m = copy.deepcopy(model)
    c, j = 3, 5
    if place <= 4:
        blk = m.features[1 + 2 * stage][0]
        ln, l1, l2 = blk.block[2], blk.block[3], blk.block[5]
        if place == 1:          # LayerNorm gamma of channel c; W1 does not read the channel
            before = _amax(_stage_input_operand(m, stage, x)[..., c] - ln.bias[c])
            ln.weight[c] *= value / before
            ln.bias[c] = 0.0
            l1.weight[:, c] = 0.0
        elif place == 2:        # one element of W1; the operand's channel c is exactly zero
            ln.weight[c] = 0.0
            ln.bias[c] = 0.0
            l1.weight[j, c] = value
        elif place == 3:        # Linear1's bias of unit j: GELU(value) = value; W2 does not read the unit
            l1.weight[j, :] = 0.0
            l1.bias[j] = value
            l2.weight[:, j] = 0.0
        else:                   # one element of W2; hidden unit j is exactly GELU(0) = 0
            l1.weight[j, :] = 0.0
            l1.bias[j] = 0.0
            l2.weight[c, j] = value
    else:
        ln, conv = m.features[2 + 2 * stage]
        if place == 5:          # the downsample's LayerNorm gamma of channel c; the conv does not read the channel
            xin = _downsample_input(m, stage, x)
            before = _amax(ln(xin)[:, c] - ln.bias[c])
            ln.weight[c] *= value / before
            ln.bias[c] = 0.0
            conv.weight[:, c] = 0.0
        else:                   # one element of the downsample weight; its input channel c is exactly zero
            ln.weight[c] = 0.0
            ln.bias[c] = 0.0
            conv.weight[j, c, 1, 0] = value
    return m


def plant_boundary(model, stage, value):
    """Hidden unit 5 of stage `stage`'s block: a zero W1 row and b1 = value, so its GELU output is exactly `value` on every pixel
    (65504.0 and 65505.0 are exact in fp32, and GELU(v) = 0.5 v (1 + erf(v / sqrt 2)) = v exactly there); W2 does not read it."""
    return plant(model, 3, stage, None, value)


@torch.no_grad()
def _stage_input(m, stage, x):
    """The fp64 stream that enters stage `stage`'s first block (device propagation: rounded at the six places)."""
    x = x.double()
    for i, layer in enumerate(m.features.children()):
        if i == 1 + 2 * stage:
            return x
        if i == 0:
            x = layer(x)
        elif i in (1, 3, 5):
            for blk in layer:
                x = H.block(blk, x, H.round_f16)
        else:
            x = H.downsample(layer, x, H.round_f16)
    raise ValueError(stage)


def _stage_input_operand(m, stage, x):
    return H.block_operand(m.features[1 + 2 * stage][0], _stage_input(m, stage, x))


@torch.no_grad()
def _downsample_input(m, stage, x):
    cur = _stage_input(m, stage, x)
    for blk in m.features[1 + 2 * stage]:
        cur = H.block(blk, cur, H.round_f16)
    return cur


# ---- the replay test's pair of images: every MFMA operand sits behind a LayerNorm, so an image's SCALE does not reach it, only its
# pattern does.  One hidden unit of stage 0 is made to saturate on one image and not on the other.
@torch.no_grad()
def unit_maxima(model, x, stage=0):
    """Per hidden unit of stage `stage`'s block: max over the pixels of image x of the positive part of Linear1's output (fp64)
    -> [4C].  Scaling the unit's W1 row and bias by a large f makes its GELU output f times this (GELU(v) = v for large v, 0 for
    large -v)."""
    blk = model.features[1 + 2 * stage][0]
    l1 = blk.block[3]
    xn = H.round_f16(_stage_input_operand(model, stage, x))
    pre = F.linear(xn, H.round_f16(l1.weight), l1.bias)
    return pre.reshape(-1, pre.shape[-1]).clamp_min(0.0).max(0).values


@torch.no_grad()
def replay_case(model, good, bad, stage=0):
    """(planted model, unit, ratio): the hidden unit whose maximum over `bad` exceeds its maximum over `good` the most, its W1 row
    and bias scaled so that 65504 lies at the geometric mean of the two maxima; W2 does not read the unit."""
    mg, mb = unit_maxima(model, good, stage), unit_maxima(model, bad, stage)
    ok = (mg > 0.5) & (mb > 0.5)            # (a unit that is positive somewhere on both images)
    ratio = torch.where(ok, mb / mg, torch.zeros_like(mg))
    j = int(ratio.argmax())
    m = copy.deepcopy(model)
    blk = m.features[1 + 2 * stage][0]
    l1, l2 = blk.block[3], blk.block[5]
    f = LIMIT / float((mg[j] * mb[j]).sqrt())
    l1.weight[j, :] *= f
    l1.bias[j] *= f
    l2.weight[:, j] = 0.0
    return m, j, float(ratio[j])
