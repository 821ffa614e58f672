"""ConvNeXt-tiny image trunk: the parameter container of torchvision.models.convnext_tiny after the reference's
truncation (network_mm/image_fe.py:59-88) and its forward on the kernels of csrc/convnext.hip.

State_dict keys are torchvision's: features.0.{0,1}.*, features.{1,3,5}.{b}.{layer_scale, block.{0,2,3,5}.*},
features.{2,4}.{0,1}.*, classifier.{0,2}.* (registered and unused, frozen like ResNet.fc).  With three `layers` entries
features[6:] are dropped and stage i keeps its first layers[i] blocks, so '2_2_2' and '3_3_9' are different networks.

The trunk stands beside the ResNet machinery: its residual stream is a plain fp32 [n,h,w,C] tensor (the channels_last memory of
logical [n,C,h,w], which is ImageFE.forward's export format, so the returned maps ARE the stream tensors); no ops.SplitMap, halo
format, map exponent, conv dispatch or precision mode 2 / 4.  Arithmetic is the project's mode 3 (three bf16 products, fp32
accumulation); LayerNorm statistics, GELU and the residual add are fp32 and nothing is stored in fp16, so there is no fp16 range
to guard.  Per block: agp_cnx_dwconv_ln_fwd writes the normalised operand, agp_cnx_mlp_fwd runs Linear -> GELU -> Linear with the
4C-wide hidden map in registers only and adds the scaled result to the stream in place.

Training is OPT-IN (`ConvNeXt.enable_training()`, Options.convnext_train): without it .train() and gradients into the trunk are
refused as before and the inference path is untouched.  With it, `forward_maps_train` runs the same kernels out of place (every
block writes a new stream tensor), applies stochastic depth in .train(), and records ONE autograd node (`_TrunkFn`) whose saved
state is the stream tensors plus the per-block stochastic-depth scales; the backward (csrc/convnext_bwd.hip) recomputes the
normalised operand with agp_cnx_dwconv_ln_fwd and never stores the hidden map either.  DBVanilla2D consumes the node's last map
through the dense-fp32 GeM; MM wraps it in train_fns.CnxTrunkFn, which pools the three maps, lends the last stream tensor to the
stage-2 block (ops.bcast_add_f32) and returns one fp32 gradient per map to this node (ops.pool_f32_bwd).

uint8 inputs are OPT-IN too (`ConvNeXt.enable_u8_inputs()`, Options.convnext_u8): the forwards then also take uint8 camera tiles
[n,ncam,h,w,3] or decoded frames (ops.RawFrames: cropped, resized and jittered to such tiles first).  The image they stand for is the
panorama [n,3,h,ncam*w] with v = (u8 / 255 - mean[c]) / std[c] (`set_image_norm`); the stem kernels read the bytes through a second
loader of the same kernel body, so the maps and gradients are, bit for bit, those of the fp32 route on
ops.normalize_cameras_u8(tiles, mean, std), and the training node saves the uint8 tiles instead of an fp32 image.

Precision 4 is OPT-IN as well (`ConvNeXt.set_precision(4)`, Options.convnext_precision) and covers the inference path
(`forward_maps`) only: the three matrix kernels run their PREC = 4 instantiations (agp_cnx_*_f16_fwd), in which the block's LayerNorm
output (one fp16 operand plane instead of two bf16 ones), W1, the GELU output, W2, the downsample's LayerNorm output and its weight
are rounded to fp16 (nearest even, saturating at +-65504, NaN kept) and every product is ONE fp16 MFMA with fp32 accumulation.  The
stream, the stem, the depthwise conv, LayerNorm statistics, biases, GELU, layer_scale and the residual add stay fp32, so the maps
are still fp32 tensors and there is still no fp16 MAP to guard; the fp32 and uint8 stems are the same kernels.  `forward_maps_train`
and the backward stay in mode 3 whatever is set (the ResNets' rule for Options.mfma_precision).  With 3 nothing changes.
The six fp16 OPERANDS do saturate, and a clamped forward returns finite, wrong maps: while the caller has bound an fp16 range guard
(range_guard.Guard.bind -- Options.convnext_range_guard makes ImageFE, DBVanilla2D and MM do it) the three kernels run guarded
twins that report a LayerNorm or GELU output beyond +-65504 into the bound word (real pixels only, NaN kept and not reported, the
same stored bits), and `forward_maps` hands the weight planes' clamp flag (prep_block / prep_down "sat", _half_clamped) to the
bound guard on every forward.  The ops know nothing of Options: no binding, no twin, no flag.

Lock-step trunks (`ConvNeXt.forward_maps_multi`, what pair.embed_pair runs behind Options.convnext_pair): the inference path of up to
MAX_GROUPS trunks of equal block counts and precision, every step ONE grouped launch of the same kernels (`*_fwd_grouped` below,
agp_cnx_*_fwd_grouped): a workgroup finds its trunk from the prefix sums of the per-trunk grids and does what the plain launch gives
that block index there, so each trunk's maps are bit for bit those of `forward_maps`.

Stochastic depth restates torchvision's StochasticDepth(p, "row") (torchvision is not a dependency): block k of the FULL
18-block network has p_k = stochastic_depth_prob * k / 17 (the truncation happens after construction, so a kept block keeps its
k); in .train() each image draws scale = bernoulli(1 - p_k) / (1 - p_k) and out = x + scale[n] * layer_scale * branch(x);
p_k == 0 and .eval() apply no scale.
"""
import ctypes as C

import torch
import torch.nn as nn

from . import _lib, ops, range_guard
from ._lib import check, ptr

DIMS = (96, 192, 384, 768)
DEPTHS = (3, 3, 9, 3)
LN_EPS = 1e-6
STAGE_FIRST_BLOCK = (0, 3, 6)          # index k of a stage's first block in the full network
TRAIN_SWITCH = "opt in with ConvNeXt.enable_training() / Options.convnext_train"


def precision_from_options(opt):
    """Options.convnext_precision for a trunk that `opt` configures; precision 4 together with the fp16 range guard is refused
    unless Options.convnext_range_guard wires the guard's sticky word into the precision-4 kernels: a guard that silently skips the
    trunk would be worse."""
    if opt.convnext_precision == 4 and opt.fp16_range_guard and not getattr(opt, "convnext_range_guard", False):
        raise NotImplementedError("ConvNeXt: convnext_precision=4 together with fp16_range_guard=True is not built (the guard's word "
                                  "is not wired into the fp16 ConvNeXt kernels); use convnext_precision=3 or turn the guard off")
    return opt.convnext_precision


class LayerNorm2d(nn.LayerNorm):
    """Parameter container of torchvision's LayerNorm2d (LayerNorm over the channels of a map)."""


class CNBlock(nn.Module):
    """block.0 depthwise 7x7, block.2 LayerNorm, block.3 Linear(C, 4C), GELU, block.5 Linear(4C, C); layer_scale [C,1,1]."""

    def __init__(self, dim):
        super().__init__()
        self.block = nn.Sequential(nn.Conv2d(dim, dim, kernel_size=7, padding=3, groups=dim, bias=True), nn.Identity(),
                                   nn.LayerNorm(dim, eps=LN_EPS), nn.Linear(dim, 4 * dim), nn.Identity(), nn.Linear(4 * dim, dim),
                                   nn.Identity())
        self.layer_scale = nn.Parameter(torch.ones(dim, 1, 1) * 1e-6)


def _split(w):
    """fp32 -> (hi, lo) bf16 planes: hi = rn(w), lo = rn(w - hi), as csrc/common.hpp split_bf16."""
    hi = w.to(torch.bfloat16)
    return hi.contiguous(), (w - hi.float()).to(torch.bfloat16).contiguous()


def _half(w):
    """fp32 -> ONE fp16 plane (precision 4): round to nearest even, saturating at +-65504, NaN kept."""
    return w.clamp(-65504.0, 65504.0).to(torch.float16).contiguous()


def _half_clamped(*ws):
    """int32 [1] on the tensors' device: 1 if _half clamps an element of any of them (|w| > 65504; NaN is kept, not clamped), else
    0.  Tensor ops only -- no read-back, no synchronisation: the fp16 range guard ORs it into its word (range_guard.note_planes)."""
    flag = (ws[0].abs() > 65504.0).any()
    for w in ws[1:]:
        flag = flag | (w.abs() > 65504.0).any()
    return flag.to(torch.int32).reshape(1)


def _planes(w, prec):
    """The kernel-side planes of a fragment-ordered fp32 tensor: (hi, lo) bf16 for precision 3, (fp16,) for precision 4."""
    if prec == 3:
        return _split(w)
    if prec == 4:
        return (_half(w),)
    raise ValueError(f"ConvNeXt: precision {prec!r}: 3 (three bf16 products) | 4 (one fp16 product)")


def _frag_rows(w):
    """[N, K] -> [N/32, K/16, 64 lanes, 8]: lane (r, h) of row block nb, k-step kk holds w[nb*32 + r][kk*16 + 8h + e] -- the A
    operand of mfma_f32_32x32x16_bf16 as one contiguous 1 KiB read per wave."""
    n, k = w.shape
    return w.reshape(n // 32, 32, k // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous()


def _frag_acc(w2):
    """Linear(4C, C).weight [C, 4C] -> [4C/32, 2, C/32, 64 lanes, 8]: the A operand of the MFMA whose B operand is registers
    8t .. 8t+7 of a 32x32 accumulator over hidden block jb: lane (r, h), element e = 4 ehi + elo holds
    w2[ct*32 + r][jb*32 + elo + 4h + 8 ehi + 16 t] (convnext.hip: acc_row)."""
    c, k = w2.shape
    v = w2.reshape(c // 32, 32, k // 32, 2, 2, 2, 4)        # [ct, r, jb, t, ehi, h, elo]
    return v.permute(2, 3, 0, 5, 1, 4, 6).contiguous()       # [jb, t, ct, h, r, ehi, elo]


def _f32(p):
    return p.detach().float().contiguous()


def prep_stem(conv, ln):
    return dict(w=_f32(conv.weight).reshape(DIMS[0], 48).t().contiguous(), bias=_f32(conv.bias), g=_f32(ln.weight), b=_f32(ln.bias))


def prep_block(blk, prec=3):
    """Kernel-side weights of one CNBlock: the depthwise taps as [49][C], the two Linear layers as fragment-ordered planes
    (prec 3: (hi, lo) bf16; prec 4: one fp16 plane of the same tensors)."""
    dw, ln, l1, l2 = blk.block[0], blk.block[2], blk.block[3], blk.block[5]
    c = dw.weight.shape[0]
    # "sat" (precision 4): whether the W1 / W2 plane holds a clamped element, for the fp16 range guard
    sat = _half_clamped(_f32(l1.weight), _f32(l2.weight)) if prec == 4 else None
    return dict(c=c, sat=sat, dw=_f32(dw.weight).reshape(c, 49).t().contiguous(), dwb=_f32(dw.bias), g=_f32(ln.weight), b=_f32(ln.bias),
                w1=_planes(_frag_rows(_f32(l1.weight)), prec), b1=_f32(l1.bias), w2=_planes(_frag_acc(_f32(l2.weight)), prec),
                b2=_f32(l2.bias), ls=_f32(blk.layer_scale).reshape(c))


def prep_down(ln, conv, prec=3):
    c = conv.weight.shape[1]
    wk = _f32(conv.weight).permute(0, 2, 3, 1).reshape(2 * c, 4 * c)      # k = (ky * 2 + kx) * C + c
    return dict(c=c, sat=_half_clamped(wk) if prec == 4 else None, g=_f32(ln.weight), b=_f32(ln.bias), w=_planes(_frag_rows(wk), prec),
                bias=_f32(conv.bias))


def prep_block_bwd(blk):
    """The backward's extra planes of one CNBlock: (layer_scale * W2)^T and W1^T in fragment order, W2 itself in fp32."""
    l1, l2 = blk.block[3], blk.block[5]
    c = l1.weight.shape[1]
    w2 = _f32(l2.weight)
    return dict(w2t=_split(_frag_rows((_f32(blk.layer_scale).reshape(c, 1) * w2).t().contiguous())),
                w1t=_split(_frag_acc(_f32(l1.weight).t().contiguous())), w2f=w2)


def prep_down_bwd(ln, conv):
    c = conv.weight.shape[1]
    wk = _f32(conv.weight).permute(0, 2, 3, 1).reshape(2 * c, 4 * c)
    return dict(wt=_split(_frag_rows(wk.t().contiguous())))


def bwd_workspace_bytes(n, h, w, c):
    b = _lib.load().agp_cnx_bwd_workspace_bytes(n, h, w, c)
    if b <= 0:
        raise ValueError(f"ConvNeXt: unsupported map [{n},{h},{w},{c}]")
    return b


def workspace_bytes(n, h, w, c):
    b = _lib.load().agp_cnx_workspace_bytes(n, h, w, c)
    if b <= 0:
        raise ValueError(f"ConvNeXt: unsupported map [{n},{h},{w},{c}]")
    return b


def _stream_ok(t, c=None):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.is_contiguous()
            and (c is None or t.shape[3] == c)):
        raise ValueError("ConvNeXt: the stream must be a contiguous fp32 [n,h,w,C] tensor on the GPU")


def stem_fwd(x, p):
    """fp32 [n,3,H,W] (any strides) -> the stream [n,h,w,96]."""
    n, _, H, W = x.shape
    out = torch.empty((n, (H - 4) // 4 + 1, (W - 4) // 4 + 1, DIMS[0]), dtype=torch.float32, device=x.device)
    check(_lib.load().agp_cnx_stem_fwd(ptr(x), *x.stride(), n, H, W, ptr(p["w"]), ptr(p["bias"]), ptr(p["g"]), ptr(p["b"]), LN_EPS,
                                       ptr(out), _lib.stream()), "agp_cnx_stem_fwd")
    return out


def _planes_ok(planes, prec, what):
    """`prec` must be the precision the weights were prepared for (prep_block / prep_down): the kernels cannot tell."""
    if prec not in (3, 4) or len(planes) != (2 if prec == 3 else 1):
        raise ValueError(f"ConvNeXt.{what}: prec={prec!r} does not match the prepared weights ({len(planes)} plane(s)); "
                         "prec is 3 or 4 and the same as in prep_block / prep_down")


def dwconv_ln_fwd(x, p, ws, prec=3):
    """Depthwise 7x7 + LayerNorm of the stream x into the workspace `ws` (uint8, >= workspace_bytes(*x.shape)): two bf16 planes
    (prec 3) or one fp16 plane at its start (prec 4)."""
    _stream_ok(x, p["c"])
    n, h, w, c = x.shape
    if prec == 4:
        check(_lib.load().agp_cnx_dwconv_ln_f16_fwd(ptr(x), n, h, w, c, ptr(p["dw"]), ptr(p["dwb"]), ptr(p["g"]), ptr(p["b"]), LN_EPS,
                                                    ptr(ws), ws.numel(), _lib.stream()), "agp_cnx_dwconv_ln_f16_fwd")
        return
    if prec != 3:
        raise ValueError(f"ConvNeXt.dwconv_ln_fwd: prec {prec!r}: 3 | 4")
    check(_lib.load().agp_cnx_dwconv_ln_fwd(ptr(x), n, h, w, c, ptr(p["dw"]), ptr(p["dwb"]), ptr(p["g"]), ptr(p["b"]), LN_EPS,
                                            ptr(ws), ws.numel(), _lib.stream()), "agp_cnx_dwconv_ln_fwd")


def mlp_fwd(ws, p, resid, out, prec=3):
    """out = resid + layer_scale * MLP(the operand in `ws`); `out` may be `resid`.  prec: that of dwconv_ln_fwd and prep_block."""
    _stream_ok(resid, p["c"])
    _stream_ok(out, p["c"])
    if out.shape != resid.shape:
        raise ValueError("ConvNeXt.mlp_fwd: out and resid differ in shape")
    _planes_ok(p["w1"], prec, "mlp_fwd")
    n, h, w, c = resid.shape
    if prec == 4:
        check(_lib.load().agp_cnx_mlp_f16_fwd(ptr(ws), ws.numel(), n * h * w, c, ptr(p["w1"][0]), ptr(p["b1"]), ptr(p["w2"][0]),
                                              ptr(p["b2"]), ptr(p["ls"]), ptr(resid), ptr(out), _lib.stream()), "agp_cnx_mlp_f16_fwd")
        return out
    check(_lib.load().agp_cnx_mlp_fwd(ptr(ws), ws.numel(), n * h * w, c, ptr(p["w1"][0]), ptr(p["w1"][1]), ptr(p["b1"]),
                                      ptr(p["w2"][0]), ptr(p["w2"][1]), ptr(p["b2"]), ptr(p["ls"]), ptr(resid), ptr(out),
                                      _lib.stream()), "agp_cnx_mlp_fwd")
    return out


def mlp_fwd_rows(ws, p, resid, out, row_scale=None):
    """mlp_fwd with a per-image factor: out = resid + row_scale[image] * layer_scale * MLP(operand); row_scale fp32 [n] or None."""
    _stream_ok(resid, p["c"])
    _stream_ok(out, p["c"])
    if out.shape != resid.shape:
        raise ValueError("ConvNeXt.mlp_fwd_rows: out and resid differ in shape")
    _planes_ok(p["w1"], 3, "mlp_fwd_rows")
    n, h, w, c = resid.shape
    _rows_ok(row_scale, n, resid.device)
    check(_lib.load().agp_cnx_mlp_fwd_rows(ptr(ws), ws.numel(), n * h * w, c, ptr(p["w1"][0]), ptr(p["w1"][1]), ptr(p["b1"]),
                                           ptr(p["w2"][0]), ptr(p["w2"][1]), ptr(p["b2"]), ptr(p["ls"]), ptr(resid), ptr(out),
                                           ptr(row_scale), h * w, _lib.stream()), "agp_cnx_mlp_fwd_rows")
    return out


def _rows_ok(row_scale, n, device):
    if row_scale is not None and not (torch.is_tensor(row_scale) and row_scale.dtype == torch.float32 and row_scale.is_contiguous()
                                      and tuple(row_scale.shape) == (n,) and row_scale.device == device):
        raise ValueError("ConvNeXt: row_scale must be a contiguous fp32 [n] tensor on the stream's device, or None")


def mlp_bwd(ws, p, pb, gy, row_scale, grads, bws):
    """Backward of mlp_fwd_rows for the operand in `ws`: returns gxn [n,h,w,C]; adds into grads = (g_w1 [4C,C], g_b1, g_w2 [C,4C],
    g_b2, g_layer_scale), fp32 buffers in parameter layout.  bws: uint8, >= bwd_workspace_bytes(*gy.shape)."""
    _stream_ok(gy, p["c"])
    n, h, w, c = gy.shape
    _rows_ok(row_scale, n, gy.device)
    gxn = torch.empty_like(gy)
    check(_lib.load().agp_cnx_mlp_bwd(ptr(ws), ws.numel(), n * h * w, c, ptr(gy), ptr(row_scale), h * w, ptr(p["w1"][0]),
                                      ptr(p["w1"][1]), ptr(p["b1"]), ptr(pb["w2t"][0]), ptr(pb["w2t"][1]), ptr(pb["w1t"][0]),
                                      ptr(pb["w1t"][1]), ptr(pb["w2f"]), ptr(p["b2"]), ptr(p["ls"]), ptr(gxn), *[ptr(g) for g in grads],
                                      ptr(bws), bws.numel(), _lib.stream()), "agp_cnx_mlp_bwd")
    return gxn


def dwconv_ln_bwd(x, gxn, gy, p, grads, bws):
    """Backward of dwconv_ln_fwd plus the residual: returns gx = gy + dL/dx through the branch; adds into grads = (g_dw [C,1,7,7],
    g_dwbias, g_ln_w, g_ln_b)."""
    _stream_ok(x, p["c"])
    _stream_ok(gxn, p["c"])
    _stream_ok(gy, p["c"])
    n, h, w, c = x.shape
    gx = torch.empty_like(x)
    check(_lib.load().agp_cnx_dwconv_ln_bwd(ptr(x), ptr(gxn), ptr(gy), n, h, w, c, ptr(p["dw"]), ptr(p["dwb"]), ptr(p["g"]), LN_EPS,
                                            ptr(gx), *[ptr(g) for g in grads], ptr(bws), bws.numel(), _lib.stream()),
          "agp_cnx_dwconv_ln_bwd")
    return gx


def downsample_bwd(x, gout, p, pb, grads, bws):
    """Backward of downsample_fwd: returns gx [n,h,w,C] (exactly 0 on a dropped odd last row / column); adds into grads =
    (g_ln_w, g_ln_b, g_w [2C,C,2,2], g_bias)."""
    _stream_ok(x, p["c"])
    _stream_ok(gout, 2 * p["c"])
    n, h, w, c = x.shape
    gx = torch.empty_like(x)
    g_ln_w, g_ln_b, g_w, g_bias = grads
    check(_lib.load().agp_cnx_downsample_bwd(ptr(x), ptr(gout), n, h, w, c, ptr(p["g"]), ptr(p["b"]), LN_EPS, ptr(pb["wt"][0]),
                                             ptr(pb["wt"][1]), ptr(gx), ptr(g_w), ptr(g_bias), ptr(g_ln_w), ptr(g_ln_b), ptr(bws),
                                             bws.numel(), _lib.stream()), "agp_cnx_downsample_bwd")
    return gx


def stem_bwd(x, gout, p, grads, bws):
    """Backward of stem_fwd (no input gradient): adds into grads = (g_w [96,3,4,4], g_bias, g_ln_w, g_ln_b)."""
    _stream_ok(gout, DIMS[0])
    n, _, H, W = x.shape
    check(_lib.load().agp_cnx_stem_bwd(ptr(x), *x.stride(), n, H, W, ptr(p["w"]), ptr(p["bias"]), ptr(p["g"]), LN_EPS, ptr(gout),
                                       *[ptr(g) for g in grads], ptr(bws), bws.numel(), _lib.stream()), "agp_cnx_stem_bwd")


def _norm3(v):
    return (C.c_float * 3)(*v)


def _tiles_ok(tiles, what):
    if not (torch.is_tensor(tiles) and tiles.is_cuda and tiles.dtype == torch.uint8 and tiles.dim() == 5 and tiles.shape[-1] == 3
            and tiles.is_contiguous() and 0 not in tiles.shape):
        raise ValueError(f"ConvNeXt.{what}: tiles must be a contiguous uint8 [n,ncam,h,w,3] tensor on the GPU")


def stem_u8_fwd(tiles, mean, std, p):
    """stem_fwd on the panorama [n,3,h,ncam*w] of uint8 tiles [n,ncam,h,w,3] (ops.normalize_cameras_u8), which is never written:
    the same bits."""
    _tiles_ok(tiles, "stem_u8_fwd")
    n, ncam, h, w, _ = tiles.shape
    if h < 4 or ncam * w < 4:
        raise ValueError(f"ConvNeXt.stem_u8_fwd: a {h}x{ncam * w} panorama is smaller than the 4x4 stem")
    out = torch.empty((n, (h - 4) // 4 + 1, (ncam * w - 4) // 4 + 1, DIMS[0]), dtype=torch.float32, device=tiles.device)
    check(_lib.load().agp_cnx_stem_u8_fwd(ptr(tiles), n, ncam, h, w, _norm3(mean), _norm3(std), ptr(p["w"]), ptr(p["bias"]), ptr(p["g"]),
                                          ptr(p["b"]), LN_EPS, ptr(out), _lib.stream()), "agp_cnx_stem_u8_fwd")
    return out


def stem_u8_bwd(tiles, mean, std, gout, p, grads, bws):
    """stem_bwd on the panorama of uint8 tiles: the same workspace, partial order and bits."""
    _tiles_ok(tiles, "stem_u8_bwd")
    _stream_ok(gout, DIMS[0])
    n, ncam, h, w, _ = tiles.shape
    check(_lib.load().agp_cnx_stem_u8_bwd(ptr(tiles), n, ncam, h, w, _norm3(mean), _norm3(std), ptr(p["w"]), ptr(p["bias"]), ptr(p["g"]),
                                          LN_EPS, ptr(gout), *[ptr(g) for g in grads], ptr(bws), bws.numel(), _lib.stream()),
          "agp_cnx_stem_u8_bwd")


def downsample_fwd(x, p, prec=3):
    """LayerNorm + 2x2 / stride-2 conv of the stream x -> a new stream [n, h//2, w//2, 2C].  prec: that of prep_down."""
    _stream_ok(x, p["c"])
    _planes_ok(p["w"], prec, "downsample_fwd")
    n, h, w, c = x.shape
    out = torch.empty((n, h // 2, w // 2, 2 * c), dtype=torch.float32, device=x.device)
    if prec == 4:
        check(_lib.load().agp_cnx_downsample_f16_fwd(ptr(x), n, h, w, c, ptr(p["g"]), ptr(p["b"]), LN_EPS, ptr(p["w"][0]),
                                                     ptr(p["bias"]), ptr(out), _lib.stream()), "agp_cnx_downsample_f16_fwd")
        return out
    check(_lib.load().agp_cnx_downsample_fwd(ptr(x), n, h, w, c, ptr(p["g"]), ptr(p["b"]), LN_EPS, ptr(p["w"][0]), ptr(p["w"][1]),
                                             ptr(p["bias"]), ptr(out), _lib.stream()), "agp_cnx_downsample_fwd")
    return out


# ---------------------------------------------------------------------------------------------------------- grouped launches
# One launch per step over 1 .. MAX_GROUPS independent problems (csrc/convnext.hip: the same kernel bodies, a workgroup finds its
# problem from the prefix sums of the per-problem grids): bit for bit what the per-problem ops above write.  The problems of a
# launch share C and the precision.  No guarded twins: under a bound fp16 range guard use the per-problem ops.
MAX_GROUPS = _lib.CNX_MAX_GROUPS


def _group_table(descs, what):
    if not 1 <= len(descs) <= MAX_GROUPS:
        raise ValueError(f"ConvNeXt.{what}: 1 .. {MAX_GROUPS} problems per launch, got {len(descs)}")
    return (_lib.CnxGroup * len(descs))(*descs), len(descs)


def _stem_desc(p, out):
    return dict(wt=ptr(p["w"]), bias=ptr(p["bias"]), ln_w=ptr(p["g"]), ln_b=ptr(p["b"]), out=ptr(out))


def stem_fwd_grouped(xs, ps, norms=None):
    """[stem_fwd(x, p)] (fp32 images) or [stem_u8_fwd(tiles, mean, std, p)] (uint8 tiles, norms = [(mean, std)]) for the problems
    zip(xs, ps) as ONE launch; the xs are all fp32 or all uint8."""
    u8 = xs[0].dtype == torch.uint8
    outs, descs = [], []
    for i, (x, p) in enumerate(zip(xs, ps)):
        if (x.dtype == torch.uint8) != u8:
            raise ValueError("ConvNeXt.stem_fwd_grouped: one launch takes fp32 images or uint8 tiles, not both")
        if u8:
            _tiles_ok(x, "stem_fwd_grouped")
            n, ncam, h, w, _ = x.shape
            if h < 4 or ncam * w < 4:
                raise ValueError(f"ConvNeXt.stem_fwd_grouped: a {h}x{ncam * w} panorama is smaller than the 4x4 stem")
            out = torch.empty((n, (h - 4) // 4 + 1, (ncam * w - 4) // 4 + 1, DIMS[0]), dtype=torch.float32, device=x.device)
            mean, std = norms[i]
            descs.append(_lib.CnxGroup(x=ptr(x), n=n, ncam=ncam, h=h, w=w, mean3=_norm3(mean), std3=_norm3(std), **_stem_desc(p, out)))
        else:
            n, _, H, W = x.shape
            out = torch.empty((n, (H - 4) // 4 + 1, (W - 4) // 4 + 1, DIMS[0]), dtype=torch.float32, device=x.device)
            sn, sc, sh, sw = x.stride()
            descs.append(_lib.CnxGroup(x=ptr(x), sn=sn, sc=sc, sh=sh, sw=sw, n=n, h=H, w=W, **_stem_desc(p, out)))
        outs.append(out)
    name = "agp_cnx_stem_u8_fwd_grouped" if u8 else "agp_cnx_stem_fwd_grouped"
    check(getattr(_lib.load(), name)(*_group_table(descs, "stem_fwd_grouped"), LN_EPS, _lib.stream()), name)
    return outs


def dwconv_ln_fwd_grouped(xs, ps, wss, prec=3):
    """dwconv_ln_fwd(x, p, ws, prec) for the problems zip(xs, ps, wss) as ONE launch (the streams share C)."""
    if prec not in (3, 4):
        raise ValueError(f"ConvNeXt.dwconv_ln_fwd_grouped: prec {prec!r}: 3 | 4")
    c = ps[0]["c"]
    descs = []
    for x, p, ws in zip(xs, ps, wss):
        _stream_ok(x, c)
        n, h, w, _ = x.shape
        descs.append(_lib.CnxGroup(x=ptr(x), n=n, h=h, w=w, wt=ptr(p["dw"]), bias=ptr(p["dwb"]), ln_w=ptr(p["g"]), ln_b=ptr(p["b"]),
                                   workspace=ptr(ws), workspace_bytes=ws.numel()))
    name = "agp_cnx_dwconv_ln_f16_fwd_grouped" if prec == 4 else "agp_cnx_dwconv_ln_fwd_grouped"
    check(getattr(_lib.load(), name)(*_group_table(descs, "dwconv_ln_fwd_grouped"), c, LN_EPS, _lib.stream()), name)


def mlp_fwd_grouped(wss, ps, resids, outs, prec=3):
    """mlp_fwd(ws, p, resid, out, prec) for the problems zip(wss, ps, resids, outs) as ONE launch."""
    c = ps[0]["c"]
    descs = []
    for ws, p, resid, out in zip(wss, ps, resids, outs):
        _stream_ok(resid, c)
        _stream_ok(out, c)
        if out.shape != resid.shape:
            raise ValueError("ConvNeXt.mlp_fwd_grouped: out and resid differ in shape")
        _planes_ok(p["w1"], prec, "mlp_fwd_grouped")
        n, h, w, _ = resid.shape
        descs.append(_lib.CnxGroup(x=ptr(resid), out=ptr(out), n=n, h=h, w=w, workspace=ptr(ws), workspace_bytes=ws.numel(),
                                   w1_hi=ptr(p["w1"][0]), w1_lo=ptr(p["w1"][-1]) if prec == 3 else None, b1=ptr(p["b1"]),
                                   w2_hi=ptr(p["w2"][0]), w2_lo=ptr(p["w2"][-1]) if prec == 3 else None, b2=ptr(p["b2"]),
                                   layer_scale=ptr(p["ls"])))
    name = "agp_cnx_mlp_f16_fwd_grouped" if prec == 4 else "agp_cnx_mlp_fwd_grouped"
    check(getattr(_lib.load(), name)(*_group_table(descs, "mlp_fwd_grouped"), c, _lib.stream()), name)
    return outs


def downsample_fwd_grouped(xs, ps, prec=3):
    """[downsample_fwd(x, p, prec)] for the problems zip(xs, ps) as ONE launch."""
    c = ps[0]["c"]
    outs, descs = [], []
    for x, p in zip(xs, ps):
        _stream_ok(x, c)
        _planes_ok(p["w"], prec, "downsample_fwd_grouped")
        n, h, w, _ = x.shape
        out = torch.empty((n, h // 2, w // 2, 2 * c), dtype=torch.float32, device=x.device)
        descs.append(_lib.CnxGroup(x=ptr(x), out=ptr(out), n=n, h=h, w=w, ln_w=ptr(p["g"]), ln_b=ptr(p["b"]), w1_hi=ptr(p["w"][0]),
                                   w1_lo=ptr(p["w"][-1]) if prec == 3 else None, bias=ptr(p["bias"])))
        outs.append(out)
    name = "agp_cnx_downsample_f16_fwd_grouped" if prec == 4 else "agp_cnx_downsample_fwd_grouped"
    check(getattr(_lib.load(), name)(*_group_table(descs, "downsample_fwd_grouped"), c, LN_EPS, _lib.stream()), name)
    return outs


class _TrunkFn(torch.autograd.Function):
    """The training forward of the whole trunk as one node.  Inputs: the trunk, the input image, the per-block scales, then every
    parameter of `features` (so that autograd accumulates into their .grad: a trunk applied twice adds up).  Outputs: the three
    exported maps; gradients arriving at all three are added into the stream's gradient at their taps."""

    @staticmethod
    def forward(ctx, fe, x, scales, *params):
        maps, saved = fe._run_train(x, scales, keep=True)
        ctx.fe, ctx.x, ctx.scales, ctx.saved = fe, x, scales, saved
        ctx.key = fe._version_key()
        return tuple(m.permute(0, 3, 1, 2) for m in maps)

    @staticmethod
    def backward(ctx, *gmaps):
        fe = ctx.fe
        if fe._version_key() != ctx.key:
            raise RuntimeError("ConvNeXt: a parameter changed between the training forward and its backward")
        grads = fe._run_backward(ctx.x, ctx.scales, ctx.saved, gmaps)
        return (None, None, None) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[3:]))


class ConvNeXt(nn.Module):
    """`layers`: the three block counts of the reference's 'a_b_c'."""

    stochastic_depth_prob = 0.1        # torchvision's convnext_tiny; a module attribute, not a parameter

    def __init__(self, layers):
        super().__init__()
        layers = [int(v) for v in layers]
        if len(layers) != 3 or min(layers) < 0:
            raise NotImplementedError("ConvNeXt: three non-negative `layers` entries (the reference's truncation to features[:6])")
        self.layers = layers
        feats = [nn.Sequential(nn.Conv2d(3, DIMS[0], kernel_size=4, stride=4, bias=True), LayerNorm2d(DIMS[0], eps=LN_EPS))]
        for i in range(3):
            feats.append(nn.Sequential(*[CNBlock(DIMS[i]) for _ in range(min(layers[i], DEPTHS[i]))]))
            if i < 2:
                feats.append(nn.Sequential(LayerNorm2d(DIMS[i], eps=LN_EPS), nn.Conv2d(DIMS[i], DIMS[i + 1], kernel_size=2, stride=2, bias=True)))
        self.features = nn.Sequential(*feats)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.classifier = nn.Sequential(LayerNorm2d(DIMS[3], eps=LN_EPS), nn.Flatten(1), nn.Linear(DIMS[3], 1000))
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                nn.init.trunc_normal_(m.weight, std=0.02)
                nn.init.zeros_(m.bias)
        # registered and unused, as in the reference (never part of a forward: frozen like ResNet.fc)
        self.classifier.requires_grad_(False)
        self._prep, self._prep_key = {}, None          # {precision: kernel-side weights} of the parameter versions in _prep_key
        self._prep_bwd, self._prep_bwd_key = None, None
        self.precision = 3
        self._train_enabled = False
        self._u8_enabled = False
        # ToTensor + Normalize of uint8 inputs (tiles, frames); the owning model sets them from its Options (set_image_norm)
        self.image_mean, self.image_std = ops.IMAGENET_MEAN, ops.IMAGENET_STD
        self.last_row_scales = None
        self._ws = ops.Workspace()

    # ------------------------------------------------------------------ training switch
    def enable_training(self, flag=True):
        """Opt in to (or out of) the training path: .train() and gradients into the trunk.  Off by default; while off both are
        refused and nothing changes for inference."""
        self._train_enabled = bool(flag)
        return self

    # ------------------------------------------------------------------ precision of the inference path
    def set_precision(self, p):
        """MFMA operand precision of `forward_maps` (Options.convnext_precision): 3 (default) = bf16 (hi, lo) pairs and three
        products; 4 = the operands rounded to fp16 and ONE product (module docstring).  `forward_maps_train` and the backward stay
        in 3 whatever is set here.  A captured graph holds the kernels and weight planes of the precision it was captured with:
        after a change run one eager forward (it prepares the planes), then capture again, as after a weight reload."""
        if isinstance(p, bool) or p not in (3, 4):
            raise ValueError(f"ConvNeXt.set_precision({p!r}): 3 (three bf16 products) | 4 (one fp16 product, inference only)")
        self.precision = int(p)
        return self

    # ------------------------------------------------------------------ uint8 inputs
    def enable_u8_inputs(self, flag=True):
        """Opt in to (or out of) uint8 inputs (Options.convnext_u8): `forward_maps` / `forward_maps_train` then also take uint8
        camera tiles [n,ncam,h,w,3] or decoded frames (ops.RawFrames), which the stem reads with ToTensor + Normalize
        (set_image_norm) on the fly.  Off by default; while off only the fp32 image is accepted, as before."""
        self._u8_enabled = bool(flag)
        return self

    def set_image_norm(self, mean, std):
        """Normalize(mean, std) of this trunk's uint8 inputs (Options.image_mean / image_std)."""
        self.image_mean, self.image_std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        return self

    def _input(self, x, what):
        """The stem's input: an fp32 [n,3,H,W] image as it is; with uint8 inputs enabled, uint8 tiles [n,ncam,h,w,3] made
        contiguous, and an ops.RawFrames cropped and resized (ops.resize_cameras_u8) and jittered (ops.jitter_cameras_u8) to such
        tiles.  Anything else: ValueError."""
        if self._u8_enabled:
            if isinstance(x, ops.RawFrames):
                tiles = ops.resize_cameras_u8(x.frames, (x.h, x.w), crop=x.crop)
                return tiles if x.jitter is None else ops.jitter_cameras_u8(tiles, x.jitter)
            if torch.is_tensor(x) and x.dtype == torch.uint8:
                if not (x.is_cuda and x.dim() == 5 and x.shape[-1] == 3 and 0 not in x.shape):
                    raise ValueError(f"ConvNeXt.{what}: uint8 input must be [n,ncam,h,w,3] camera tiles on the GPU")
                return x.contiguous()
        if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 3):
            raise ValueError(f"ConvNeXt.{what}: x must be an fp32 [n,3,H,W] tensor on the GPU")
        return x

    @staticmethod
    def _geometry(x):
        """(n, H, W) of a stem input: the fp32 image's, or the panorama's (h, ncam * w) of uint8 tiles."""
        if x.dtype == torch.uint8:
            n, ncam, h, w, _ = x.shape
            return n, h, ncam * w
        return x.shape[0], x.shape[2], x.shape[3]

    def _stem(self, x, p):
        return stem_u8_fwd(x, self.image_mean, self.image_std, p) if x.dtype == torch.uint8 else stem_fwd(x, p)

    def sd_probs(self):
        """Per stage, the stochastic-depth probability p_k of each kept block: stochastic_depth_prob * k / 17 with k the block's
        index in the full 18-block network (torchvision sets them before the reference truncates)."""
        total = sum(DEPTHS) - 1.0
        return [[self.stochastic_depth_prob * (STAGE_FIRST_BLOCK[s] + b) / total for b in range(len(self.features[1 + 2 * s]))]
                for s in range(3)]

    # ------------------------------------------------------------------ weights
    def _version_key(self):
        return tuple((p.data_ptr(), p._version) for p in self.parameters())

    def _prepared(self, prec=3):
        """Kernel-side weights for precision `prec`, cached per (parameter version, precision): rebuilt when a parameter changes
        (ResNet._version_key's rule).  The training forward and the backward always ask for 3."""
        key = self._version_key()
        if key != self._prep_key:
            self._prep, self._prep_key = {}, key
        if prec not in self._prep:
            with torch.no_grad():
                prep = {"stem": prep_stem(*self.features[0])}
                for s in range(3):
                    prep[("blocks", s)] = [prep_block(blk, prec) for blk in self.features[1 + 2 * s]]
                    if s < 2:
                        prep[("down", s)] = prep_down(*self.features[2 + 2 * s], prec)
                if prec == 4:       # one clamp flag over every fp16 weight plane of this parameter version (prep_block, prep_down)
                    flags = [p["sat"] for k, v in prep.items() if k != "stem" for p in (v if isinstance(v, list) else [v])]
                    prep["sat"] = torch.stack(flags).amax(0) if flags else None
            self._prep[prec] = prep
        return self._prep[prec]

    def _prepared_bwd(self):
        key = self._version_key()
        if key != self._prep_bwd_key:
            with torch.no_grad():
                prep = {}
                for s in range(3):
                    prep[("blocks", s)] = [prep_block_bwd(blk) for blk in self.features[1 + 2 * s]]
                    if s < 2:
                        prep[("down", s)] = prep_down_bwd(*self.features[2 + 2 * s])
            self._prep_bwd, self._prep_bwd_key = prep, key
        return self._prep_bwd

    # ------------------------------------------------------------------ forward
    @staticmethod
    def map_sizes(h, w):
        """[(h, w)] of the three exported maps; ValueError if the input is too small for three stages."""
        if h < 4 or w < 4:
            raise ValueError(f"ConvNeXt: a {h}x{w} input is smaller than the 4x4 stem")
        sizes = [((h - 4) // 4 + 1, (w - 4) // 4 + 1)]
        for _ in range(2):
            sizes.append((sizes[-1][0] // 2, sizes[-1][1] // 2))
        if min(sizes[-1]) < 1:
            raise ValueError(f"ConvNeXt: a {h}x{w} input is too small for three stages (map sizes {sizes})")
        return sizes

    def block_counts(self):
        """The blocks each of the three stages keeps (`layers` capped at convnext_tiny's depths)."""
        return [len(self.features[1 + 2 * s]) for s in range(3)]

    def takes_training_path(self):
        """Whether `forward_maps` would hand this call to `forward_maps_train` (mode 3, no fp16: nothing for the range guard)."""
        wants_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.features.parameters())
        return self._train_enabled and (self.training or wants_grad)

    def forward_maps(self, x):
        """fp32 [n,3,H,W] on the GPU (any strides) -> the outputs of features[1], [3], [5] as fp32 tensors of logical shape
        [n,C,h,w] in channels_last memory.  The inference path: allocates the three maps, launches on the current stream and never
        synchronises (capturable after one eager call has prepared the weights).  With the training switch on, .train() or
        trainable trunk parameters under enabled gradients go through `forward_maps_train` instead.  With uint8 inputs enabled
        (enable_u8_inputs) x may also be uint8 tiles [n,ncam,h,w,3] or an ops.RawFrames: H, W are then the panorama's (h, ncam*w);
        frames need their resize tables on the device before a capture (one eager call, or ops.prepare_resize).
        At precision 4, while the caller has bound an fp16 range guard (range_guard.Guard.bind; Options.convnext_range_guard does
        it in ImageFE / DBVanilla2D / MM), the three matrix kernels run their guarded twins and the weight planes' clamp flag is
        handed to that guard; the maps are the same bits."""
        wants_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.features.parameters())
        if self._train_enabled and (self.training or wants_grad):
            return self.forward_maps_train(x)
        if self.training:
            raise NotImplementedError(f"ConvNeXt: .train() is not enabled (inference only; {TRAIN_SWITCH}); call .eval()")
        if torch.is_grad_enabled() and (getattr(x, "requires_grad", False) or wants_grad):
            raise NotImplementedError("ConvNeXt: gradients into the trunk are not enabled (inference only): run under "
                                      "torch.no_grad() or freeze the trunk (requires_grad_(False) / freeze_backbone()), or "
                                      + TRAIN_SWITCH)
        x = self._input(x, "forward_maps")
        n, H, W = self._geometry(x)
        sizes = self.map_sizes(H, W)
        prec = self.precision
        prep = self._prepared(prec)
        ws = self._ws.tensor("cnx_ws", (max(workspace_bytes(n, h, w, DIMS[s]) for s, (h, w) in enumerate(sizes)),), torch.uint8,
                             x.device)
        if prec == 4:
            # under a bound fp16 range guard (range_guard.Guard.bind; the kernels below then run their guarded twins): the clamp
            # flag of the fp16 weight planes, on EVERY forward that uses them; without a binding nothing happens
            range_guard.note_planes(prep["sat"])
        maps, cur = [], None
        for s in range(3):
            cur = self._stem(x, prep["stem"]) if s == 0 else downsample_fwd(cur, prep[("down", s - 1)], prec)
            for p in prep[("blocks", s)]:
                dwconv_ln_fwd(cur, p, ws, prec)
                mlp_fwd(ws, p, cur, cur, prec)
            maps.append(cur.permute(0, 3, 1, 2))
        return maps

    @staticmethod
    def forward_maps_multi(nets, xs):
        """[net.forward_maps(x) for net, x in zip(nets, xs)] -- the inference path only -- with the 1 .. MAX_GROUPS trunks advancing in
        lock-step: the stem, every block's depthwise conv + LayerNorm and MLP, and every downsample are ONE grouped launch over all
        trunks (stem_fwd_grouped ...; trunks given fp32 images and trunks given uint8 tiles / frames take one stem launch per kind).
        The trunks have the same block counts and precision; sizes, weights (each trunk's own prepared planes) and operand workspaces
        (each trunk's own, keyed by the launch stream) are their own, and each x follows its trunk's enable_u8_inputs rule.  The maps
        are bit for bit those of forward_maps.  Launches on the current stream, never synchronises, capturable after one eager call.
        While the caller has bound an fp16 range guard at precision 4 the grouped launches, which have no guarded twins, are not
        used: every trunk then runs its own forward_maps, guarded as there."""
        nets, xs = list(nets), list(xs)
        if not 1 <= len(nets) <= MAX_GROUPS or len(xs) != len(nets):
            raise ValueError(f"ConvNeXt.forward_maps_multi: 1 .. {MAX_GROUPS} trunks and one input each, got {len(nets)} and {len(xs)}")
        counts = [net.block_counts() for net in nets]
        if any(c != counts[0] for c in counts) or any(net.precision != nets[0].precision for net in nets):
            raise ValueError("ConvNeXt.forward_maps_multi: the trunks must have the same block counts and precision, got "
                             f"{[(c, net.precision) for c, net in zip(counts, nets)]}")
        for net in nets:
            if net.training or net.takes_training_path():
                raise NotImplementedError("ConvNeXt.forward_maps_multi: the inference path only (.eval() under torch.no_grad(), or a "
                                          "frozen trunk); training forwards run per trunk (forward_maps)")
            if torch.is_grad_enabled() and any(p.requires_grad for p in net.features.parameters()):
                raise NotImplementedError("ConvNeXt.forward_maps_multi: gradients into the trunk are not enabled (inference only): run "
                                          "under torch.no_grad() or freeze the trunks")
        prec = nets[0].precision
        if prec == 4 and range_guard.bound_word() is not None:
            return [net.forward_maps(x) for net, x in zip(nets, xs)]
        xs = [net._input(x, "forward_maps_multi") for net, x in zip(nets, xs)]
        if torch.is_grad_enabled() and any(getattr(x, "requires_grad", False) for x in xs):
            raise NotImplementedError("ConvNeXt.forward_maps_multi: the gradient of an input image is not built")
        preps = [net._prepared(prec) for net in nets]
        wss, seen = [], {}
        for net, x in zip(nets, xs):
            n, H, W = net._geometry(x)
            sizes = net.map_sizes(H, W)
            k = seen[id(net)] = seen.get(id(net), -1) + 1         # (one trunk given twice: an operand workspace per use)
            wss.append(net._ws.tensor("cnx_ws" if k == 0 else f"cnx_ws_multi{k}",
                                      (max(workspace_bytes(n, h, w, DIMS[s]) for s, (h, w) in enumerate(sizes)),), torch.uint8, x.device))
        maps, curs = [[] for _ in nets], [None] * len(nets)
        for s in range(3):
            if s == 0:
                for u8 in (False, True):
                    idx = [i for i, x in enumerate(xs) if (x.dtype == torch.uint8) == u8]
                    if idx:
                        outs = stem_fwd_grouped([xs[i] for i in idx], [preps[i]["stem"] for i in idx],
                                                [(nets[i].image_mean, nets[i].image_std) for i in idx])
                        for i, o in zip(idx, outs):
                            curs[i] = o
            else:
                curs = downsample_fwd_grouped(curs, [p[("down", s - 1)] for p in preps], prec)
            for b in range(counts[0][s]):
                ps = [p[("blocks", s)][b] for p in preps]
                dwconv_ln_fwd_grouped(curs, ps, wss, prec)
                mlp_fwd_grouped(wss, ps, curs, curs, prec)
            for m, cur in zip(maps, curs):
                m.append(cur.permute(0, 3, 1, 2))
        return maps

    # ------------------------------------------------------------------ training
    def forward_maps_train(self, x, row_scales=None):
        """The training forward (needs enable_training()): the three maps of `forward_maps`, out of place, as one autograd node.

        row_scales: None = in .train() draw, per block with p_k > 0 and per image, scale = bernoulli(1 - p_k) / (1 - p_k) on the
        device from torch's current CUDA generator; in .eval() no scale.  Or a list with one entry per block (stage by stage):
        an fp32 [n] tensor used in place of the draw, or None for no scale.  Under torch.no_grad(), or with no trainable trunk
        parameter, nothing is saved.  An input that requires a gradient is refused: the stem returns no image gradient.
        x: as in `forward_maps`; from uint8 tiles or frames the node saves the uint8 tiles, not an fp32 image."""
        if not self._train_enabled:
            raise NotImplementedError(f"ConvNeXt: training (.train(), gradients) is not enabled; {TRAIN_SWITCH}")
        x = self._input(x, "forward_maps_train")
        if torch.is_grad_enabled() and x.requires_grad:
            raise NotImplementedError("ConvNeXt: the gradient of the input image is not built (the stem returns none)")
        n = x.shape[0]
        nblocks = sum(len(self.features[1 + 2 * s]) for s in range(3))
        if row_scales is None:
            row_scales = [None] * nblocks
            if self.training:
                probs = [p for stage in self.sd_probs() for p in stage]
                row_scales = [None if p == 0.0 else torch.bernoulli(torch.full((n,), 1.0 - p, dtype=torch.float32, device=x.device))
                              * (1.0 / (1.0 - p)) for p in probs]
        elif len(row_scales) != nblocks:
            raise ValueError(f"ConvNeXt.forward_maps_train: row_scales needs {nblocks} entries (one per block), got {len(row_scales)}")
        scales = tuple(None if r is None else r.detach().contiguous() for r in row_scales)
        self.last_row_scales = scales          # what this forward applied (drawn or given), for inspection
        params = [p for p in self.features.parameters()]
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            return list(_TrunkFn.apply(self, x.detach(), scales, *params))
        with torch.no_grad():
            maps, _ = self._run_train(x, scales, keep=False)
        return [m.permute(0, 3, 1, 2) for m in maps]

    def _ws_bytes(self, n, sizes, fn):
        return max(fn(n, h, w, DIMS[s]) for s, (h, w) in enumerate(sizes))

    def _run_train(self, x, scales, keep):
        """keep: every block writes a new stream tensor and the block inputs are returned (the saved state); else in place."""
        n, H, W = self._geometry(x)
        sizes = self.map_sizes(H, W)
        prep = self._prepared()
        ws = self._ws.tensor("cnx_ws", (self._ws_bytes(n, sizes, workspace_bytes),), torch.uint8, x.device)
        maps, saved, cur, k = [], [], None, 0
        for s in range(3):
            cur = self._stem(x, prep["stem"]) if s == 0 else downsample_fwd(cur, prep[("down", s - 1)])
            inputs = []
            for p in prep[("blocks", s)]:
                dwconv_ln_fwd(cur, p, ws)
                out = torch.empty_like(cur) if keep else cur
                mlp_fwd_rows(ws, p, cur, out, scales[k])
                inputs.append(cur)
                cur, k = out, k + 1
            saved.append(inputs)
            maps.append(cur)
        return maps, (saved, maps) if keep else None

    def _run_backward(self, x, scales, saved, gmaps):
        """Gradients of every parameter of `features`, in parameters() order, as fp32 tensors in parameter layout."""
        inputs, maps = saved
        n, H, W = self._geometry(x)
        sizes = self.map_sizes(H, W)
        prep, pb = self._prepared(), self._prepared_bwd()
        dev = x.device
        ws = self._ws.tensor("cnx_ws", (self._ws_bytes(n, sizes, workspace_bytes),), torch.uint8, dev)
        bws = self._ws.tensor("cnx_bws", (self._ws_bytes(n, sizes, bwd_workspace_bytes),), torch.uint8, dev)
        params = list(self.features.parameters())
        grads = {id(p): torch.zeros(p.shape, dtype=torch.float32, device=dev) for p in params}
        G = lambda *ps: [grads[id(p)] for p in ps]
        nb = [len(b) for b in inputs]
        g = None
        for s in (2, 1, 0):
            gm = gmaps[s]
            if gm is not None:
                gm = gm.permute(0, 2, 3, 1).float().contiguous()
                g = gm if g is None else g + gm
            elif g is None:
                g = torch.zeros_like(maps[s])
            k0 = sum(nb[:s])
            for b in reversed(range(nb[s])):
                blk, p, xin = self.features[1 + 2 * s][b], prep[("blocks", s)][b], inputs[s][b]
                dw, ln, l1, l2 = blk.block[0], blk.block[2], blk.block[3], blk.block[5]
                dwconv_ln_fwd(xin, p, ws)                  # the operand, recomputed
                gxn = mlp_bwd(ws, p, pb[("blocks", s)][b], g, scales[k0 + b],
                              G(l1.weight, l1.bias, l2.weight, l2.bias, blk.layer_scale), bws)
                g = dwconv_ln_bwd(xin, gxn, g, p, G(dw.weight, dw.bias, ln.weight, ln.bias), bws)
            if s > 0:
                ln, conv = self.features[2 * s]
                g = downsample_bwd(maps[s - 1], g, prep[("down", s - 1)], pb[("down", s - 1)], G(ln.weight, ln.bias, conv.weight, conv.bias),
                                   bws)
            else:
                conv, ln = self.features[0]
                if x.dtype == torch.uint8:      # the saved uint8 tiles, normalised on the fly as in the forward
                    stem_u8_bwd(x, self.image_mean, self.image_std, g, prep["stem"], G(conv.weight, conv.bias, ln.weight, ln.bias), bws)
                else:
                    stem_bwd(x, g, prep["stem"], G(conv.weight, conv.bias, ln.weight, ln.bias), bws)
        return [grads[id(p)] for p in params]
