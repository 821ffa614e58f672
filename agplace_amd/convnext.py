"""ConvNeXt-tiny image trunk, inference only: the parameter container of torchvision.models.convnext_tiny after the reference's
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
"""
import torch
import torch.nn as nn

from . import _lib, ops
from ._lib import check, ptr

DIMS = (96, 192, 384, 768)
DEPTHS = (3, 3, 9, 3)
LN_EPS = 1e-6


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


def prep_block(blk):
    """Kernel-side weights of one CNBlock: the depthwise taps as [49][C], the two Linear layers as fragment-ordered planes."""
    dw, ln, l1, l2 = blk.block[0], blk.block[2], blk.block[3], blk.block[5]
    c = dw.weight.shape[0]
    return dict(c=c, dw=_f32(dw.weight).reshape(c, 49).t().contiguous(), dwb=_f32(dw.bias), g=_f32(ln.weight), b=_f32(ln.bias),
                w1=_split(_frag_rows(_f32(l1.weight))), b1=_f32(l1.bias), w2=_split(_frag_acc(_f32(l2.weight))), b2=_f32(l2.bias),
                ls=_f32(blk.layer_scale).reshape(c))


def prep_down(ln, conv):
    c = conv.weight.shape[1]
    wk = _f32(conv.weight).permute(0, 2, 3, 1).reshape(2 * c, 4 * c)      # k = (ky * 2 + kx) * C + c
    return dict(c=c, g=_f32(ln.weight), b=_f32(ln.bias), w=_split(_frag_rows(wk)), bias=_f32(conv.bias))


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


def dwconv_ln_fwd(x, p, ws):
    """Depthwise 7x7 + LayerNorm of the stream x into the workspace `ws` (uint8, >= workspace_bytes(*x.shape))."""
    _stream_ok(x, p["c"])
    n, h, w, c = x.shape
    check(_lib.load().agp_cnx_dwconv_ln_fwd(ptr(x), n, h, w, c, ptr(p["dw"]), ptr(p["dwb"]), ptr(p["g"]), ptr(p["b"]), LN_EPS,
                                            ptr(ws), ws.numel(), _lib.stream()), "agp_cnx_dwconv_ln_fwd")


def mlp_fwd(ws, p, resid, out):
    """out = resid + layer_scale * MLP(the operand in `ws`); `out` may be `resid`."""
    _stream_ok(resid, p["c"])
    _stream_ok(out, p["c"])
    if out.shape != resid.shape:
        raise ValueError("ConvNeXt.mlp_fwd: out and resid differ in shape")
    n, h, w, c = resid.shape
    check(_lib.load().agp_cnx_mlp_fwd(ptr(ws), ws.numel(), n * h * w, c, ptr(p["w1"][0]), ptr(p["w1"][1]), ptr(p["b1"]),
                                      ptr(p["w2"][0]), ptr(p["w2"][1]), ptr(p["b2"]), ptr(p["ls"]), ptr(resid), ptr(out),
                                      _lib.stream()), "agp_cnx_mlp_fwd")
    return out


def downsample_fwd(x, p):
    """LayerNorm + 2x2 / stride-2 conv of the stream x -> a new stream [n, h//2, w//2, 2C]."""
    _stream_ok(x, p["c"])
    n, h, w, c = x.shape
    out = torch.empty((n, h // 2, w // 2, 2 * c), dtype=torch.float32, device=x.device)
    check(_lib.load().agp_cnx_downsample_fwd(ptr(x), n, h, w, c, ptr(p["g"]), ptr(p["b"]), LN_EPS, ptr(p["w"][0]), ptr(p["w"][1]),
                                             ptr(p["bias"]), ptr(out), _lib.stream()), "agp_cnx_downsample_fwd")
    return out


class ConvNeXt(nn.Module):
    """`layers`: the three block counts of the reference's 'a_b_c'."""

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
        self._prep, self._prep_key = None, None
        self._ws = ops.Workspace()

    # ------------------------------------------------------------------ weights
    def _version_key(self):
        return tuple((p.data_ptr(), p._version) for p in self.parameters())

    def _prepared(self):
        """Kernel-side weights, rebuilt when a parameter changes (ResNet._version_key's rule)."""
        key = self._version_key()
        if key != self._prep_key:
            with torch.no_grad():
                prep = {"stem": prep_stem(*self.features[0])}
                for s in range(3):
                    prep[("blocks", s)] = [prep_block(blk) for blk in self.features[1 + 2 * s]]
                    if s < 2:
                        prep[("down", s)] = prep_down(*self.features[2 + 2 * s])
            self._prep, self._prep_key = prep, key
        return self._prep

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

    def forward_maps(self, x):
        """fp32 [n,3,H,W] on the GPU (any strides) -> the outputs of features[1], [3], [5] as fp32 tensors of logical shape
        [n,C,h,w] in channels_last memory.  Inference only; allocates the three maps, launches on the current stream and never
        synchronises (capturable after one eager call has prepared the weights)."""
        if self.training:
            raise NotImplementedError("ConvNeXt: .train() is not built (inference only); call .eval()")
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.features.parameters())):
            raise NotImplementedError("ConvNeXt: gradients into the trunk are not built (inference only): run under "
                                      "torch.no_grad() or freeze the trunk (requires_grad_(False) / freeze_backbone())")
        if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 3):
            raise ValueError("ConvNeXt.forward_maps: x must be an fp32 [n,3,H,W] tensor on the GPU")
        n, _, H, W = x.shape
        sizes = self.map_sizes(H, W)
        prep = self._prepared()
        ws = self._ws.tensor("cnx_ws", (max(workspace_bytes(n, h, w, DIMS[s]) for s, (h, w) in enumerate(sizes)),), torch.uint8,
                             x.device)
        maps, cur = [], None
        for s in range(3):
            cur = stem_fwd(x, prep["stem"]) if s == 0 else downsample_fwd(cur, prep[("down", s - 1)])
            for p in prep[("blocks", s)]:
                dwconv_ln_fwd(cur, p, ws)
                mlp_fwd(ws, p, cur, cur)
            maps.append(cur.permute(0, 3, 1, 2))
        return maps
