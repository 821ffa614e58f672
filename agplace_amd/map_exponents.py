"""Calibrated power-of-two map exponents: keep a checkpoint whose activations leave fp16's range in precision modes 2 / 4.

Modes 2 and 4 store every feature map as one fp16 plane (+-65504).  The image path is positively homogeneous between its affine
epilogues, so a map can be STORED as x * 2^-e (e a non-negative integer: exact in fp16 and fp32) and every consumer compensated
in constants the host prepares anyway:

  * a conv reading a map with exponent ei and writing one with eo: folded BatchNorm scale *= 2^(ei - eo), shift *= 2^-eo
    (ops.fold_exp; the residual operand is stored with eo already, see the grouping rule);
  * global pools: the mean of the stored map is the true mean times 2^-e; GeM runs with eps * 2^-e, which makes the same hold for
    it (clamp(x, eps) = 2^e clamp(x 2^-e, eps 2^-e)); the factor 2^e is applied where the vector is read next -- the load of a
    vector program (VecProgram.load(scale=...)), or one small launch on the per-op paths;
  * stage 2: the projected fusion vector that is broadcast-added into the layer-3 map takes 2^-e through the projection's
    prepared weights and bias;
  * whatever exports a map as fp32 (SplitMap.to_f32) multiplies by 2^e.

No kernel, launch count or instruction stream changes; with every exponent 0 every prepared constant is the tensor it was.

Grouping rule.  Maps that meet in a residual add share one exponent: per ResNet stage the incoming identity (the downsample
output; for layer 1 the pooled stem output) and every block output form the group "layer{L}".  Block-internal maps (conv1's
output of a BasicBlock, conv1's and conv2's of a Bottleneck) have their own: "layer{L}.{b}.conv{k}".  In MM the stage-2 image
block adds a vector into the last stage output and its own output onto that sum, so its input and output maps are members of the
last stage's group; its internal map is "stg2.{i}.conv1".  Names carry the model's prefix: "image_fe." in MM,
"dbimage_fes.{i}." in DBVanilla2D, none for ImageFE / ResNet.

Left at exponent 0: the sparse-voxel branch's fp16 maps (its kernels have no folded affine epilogue per map; they stay covered by
the fp16 range guard and by mode 3), the stem's input map (normalised images).  Not offered: negative exponents (scaling small
maps up) and per-channel exponents.  Mode 3 and every training path ignore the exponents.

Exponents are plain attributes, not parameters or buffers: state_dict() keeps the reference's keys.  Calibrate once, ship the
dict (JSON) next to the checkpoint, install it with set_exponents() after loading the weights.  They are part of the
prepared-weights cache keys, so a change re-folds at the next forward; a hipGraph captured before the change keeps replaying the
old constants (agplace_amd.pair.CapturedPair).
"""
import math

import torch

from . import ops
from .resnet import ResNet

F16_MAX = 65504.0


def choose_exponents(absmax, groups=None, headroom_bits=2):
    """absmax: {map name: measured max |x|}; groups: {group name: [member map names]} (maps outside every group stand alone).
    Returns {group name or stand-alone map name: e} with e = max(0, ceil(log2(m * 2^headroom_bits / 65504))), m the largest
    measured maximum of the group -- the smallest e that keeps m * 2^headroom_bits * 2^-e inside fp16.  A group none of whose
    members was measured gets 0.  headroom_bits is policy (how much larger than the calibration batches' peak a later input may
    get), not a measurement.  NaN, infinite or negative maxima raise ValueError: such a calibration run measured nothing."""
    if int(headroom_bits) != headroom_bits or headroom_bits < 0:
        raise ValueError(f"headroom_bits {headroom_bits!r}: a non-negative integer")
    groups = groups or {}
    for name, m in absmax.items():
        m = float(m)
        if math.isnan(m) or math.isinf(m) or m < 0:
            raise ValueError(f"choose_exponents: the measured maximum of {name!r} is {m}; calibrate on finite maps")

    def exp_of(m):
        e = 0
        while math.ldexp(m, int(headroom_bits) - e) > F16_MAX:       # (exact: no logarithm is rounded)
            e += 1
        return e
    out, grouped = {}, set()
    for g, members in groups.items():
        grouped.update(members)
        ms = [float(absmax[n]) for n in members if n in absmax]
        out[g] = exp_of(max(ms)) if ms else 0
    for name, m in absmax.items():
        if name not in grouped:
            out[name] = exp_of(float(m))
    return out


# ------------------------------------------------------------------ the models' maps
def _parts(model):
    """[(prefix, owner module)]: the modules whose forwards report maps to ops.MAP_PROBE, with the prefix of their names."""
    from .models_baseline.dbvanilla2d import DBVanilla2D
    from .network_mm.image_fe import ImageFE
    from .network_mm.mm import MM
    if isinstance(model, ResNet):
        return [("", model)]
    if isinstance(model, ImageFE):
        return [("", model.fe)]
    if isinstance(model, MM):
        return [("image_fe.", model.image_fe.fe)] + [(f"stg2.{i}.", blk) for i, blk in enumerate(model.stg2fuseblock.ffnsimg)]
    if isinstance(model, DBVanilla2D):
        return [(f"dbimage_fes.{i}.", fe.fe) for i, fe in enumerate(model.dbimage_fes)]
    raise TypeError(f"map exponents: ImageFE / ResNet, MM or DBVanilla2D expected, got {type(model).__name__}")


def map_names(model):
    """(groups, standalone): {group name: [member map names]} and [stand-alone (block-internal) map names] of a model -- the
    keys of its exponent dict are the group names and the stand-alone names."""
    groups, alone, last_group = {}, [], None
    for prefix, owner in _parts(model):
        if isinstance(owner, ResNet):
            g, internal = owner.map_exponent_names()
            groups.update({prefix + k: [prefix + n for n in v] for k, v in g.items()})
            alone += [prefix + n for n in internal]
            last_group = prefix + f"layer{owner.nstages}"
        else:       # a stage-2 image block: input and output sit in the residual chain of the trunk's last stage output
            groups[last_group] += [prefix + "in", prefix + "out"]
            alone.append(prefix + "conv1")
    return groups, alone


def get_exponents(model):
    """{name: e} for every group and stand-alone map of the model (zeros included): plain ints, JSON-able."""
    groups, alone = map_names(model)
    out = {}
    for prefix, owner in _parts(model):
        for k, v in owner._map_exp.items():
            out[prefix + k] = int(v)
    return {k: out.get(k, 0) for k in list(groups) + alone}


def set_exponents(model, d):
    """Install {name: e} (names as get_exponents returns them; missing names mean 0).  Takes effect at the next forward."""
    groups, alone = map_names(model)
    known = set(groups) | set(alone)
    for k, v in d.items():
        if k not in known:
            raise ValueError(f"set_exponents: {k!r} is not a map group of this {type(model).__name__}")
        if isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= 64:
            raise ValueError(f"set_exponents: exponent of {k!r} is {v!r}; a non-negative integer (negative exponents are not offered)")
    for prefix, owner in _parts(model):
        # (prefixes end in a dot and "" only occurs alone, so every key has exactly one owner)
        owner._map_exp = {k[len(prefix):]: int(v) for k, v in d.items() if k.startswith(prefix) and int(v)}
    return get_exponents(model)


def clear_exponents(model):
    for _, owner in _parts(model):
        owner._map_exp = {}


def calibrate(model, batches, headroom_bits=2):
    """Measure, choose, install.  Runs the inference batches in precision mode 3 (split-bf16 maps: fp32 range, so the maxima are
    true ones whatever the checkpoint does to fp16), accumulates max |x| of every map of the groups above on the device
    (agp_map_absmax, as each map is produced), reads the table back ONCE, calls choose_exponents and installs the result.
    batches: what the model's forward takes -- data dicts for MM (mode 'q') and DBVanilla2D (mode 'db'), image tensors for
    ImageFE / ResNet.  The model must be in .eval() mode.  Returns the installed dict (get_exponents)."""
    from .network_mm.image_fe import ImageFE
    from .network_mm.mm import MM
    if isinstance(model, MM) and model._convnext:
        raise NotImplementedError("map_exponents.calibrate on MM with mm_imgfe='convnext_tiny': its image side runs in the mode-3 "
                                  "arithmetic (fp32 range), there are no map exponents to calibrate")
    if model.training:
        raise RuntimeError("map_exponents.calibrate: put the model in .eval() mode (exponents act on inference only)")
    if ops.MAP_PROBE is not None:
        raise RuntimeError("map_exponents.calibrate: another calibration is active")
    groups, alone = map_names(model)
    names = [n for members in groups.values() for n in members] + alone
    index = {n: i for i, n in enumerate(names)}
    prefix_of = {id(owner): prefix for prefix, owner in _parts(model)}
    state = {"table": None, "seen": set()}

    def probe(owner, name, m):
        prefix = prefix_of.get(id(owner))
        i = None if prefix is None else index.get(prefix + name)
        if i is None:
            return
        if state["table"] is None:
            state["table"] = torch.empty(len(names), dtype=torch.float32, device=m.hi.device)
            ops.absmax_reset(state["table"])
        state["seen"].add(prefix + name)
        ops.map_absmax(m, state["table"][i:i + 1])

    opt = getattr(model, "opt", None) if not isinstance(model, (ImageFE, ResNet)) else None
    saved = None if opt is None else opt.mfma_precision
    ops.MAP_PROBE = probe
    try:
        if opt is not None:
            opt.mfma_precision = 3
        with torch.no_grad():
            for batch in batches:
                if isinstance(model, (ImageFE, ResNet)):
                    model.forward_maps(batch, prec=3)
                else:
                    model(batch, mode='q' if isinstance(model, MM) else 'db')
    finally:
        ops.MAP_PROBE = None
        if opt is not None:
            opt.mfma_precision = saved
    if state["table"] is None:
        raise ValueError("map_exponents.calibrate: no batch was given, nothing was measured")
    torch.cuda.synchronize()
    vals = state["table"].cpu().tolist()
    absmax = {n: vals[index[n]] for n in names if n in state["seen"]}
    chosen = choose_exponents(absmax, groups, headroom_bits)
    # (a stand-alone map that was never produced -- an unused trunk of a shared database network -- keeps 0)
    return set_exponents(model, chosen)
