"""ConvNeXt-tiny training on the GPU (csrc/convnext_bwd.hip, agplace_amd/convnext.py: forward_maps_train) against fp64 autograd
through the CPU restatement (tests/convnext_ref.py, tests/convnext_train_ref.py): the backward kernels alone, the trunk through
ImageFE, DBVanilla2D on top of it.  Every test prints its error next to the fp32 CPU autograd's own error (e32) on the same data.

Bounds.  Ceilings: 1e-4 (rel_l2) for the data gradients of a kernel (gxn, gx), the project's mode-3 map bar; 1e-3 for every
parameter gradient, at kernel and at network level, the tight-mode bar of tests/test_gpu_train.py (a parameter gradient is a sum
over pixels with cancellation, the same reason that bar is ten times the map bar).  The asserted bounds are 4 x the worst value
first measured on an MI355X (the margin tests/test_gpu_convnext.py uses for box-to-box accumulation order), never above the ceiling:
MEASURED below.  First measured on an MI355X (worst case of each group, with the fp32 CPU autograd's error on the same data):
  MLP backward gxn            7.82e-06 (e32 4.59e-07; C=96, P=1)        w1 / b1 / w2 / b2 / layer_scale  7.12e-06 (e32 2.01e-07)
  LayerNorm + depthwise gx    1.07e-07 (e32 1.08e-07; plain fp32)       dw / bias / gamma / beta         1.64e-07 (e32 1.56e-07)
  the same over 260 tiles (8 256 pixels)                                dw / bias / gamma / beta         2.94e-07 (e32 5.38e-07)
  downsample gx               4.55e-06 (e32 2.58e-07)                   LN / conv parameters             5.14e-06 (e32 3.76e-07)
  stem parameters             2.41e-07 (e32 1.85e-07; plain fp32)
  trunk '2_1_2', all 48 parameter tensors: eval 1.26e-05, train with injected scales 1.30e-05 (e32 6.58e-07)
  DBVanilla2D '1_1_1', trunk + GeM p + heads: 2.28e-05 (GeM p; e32 1.1e-06)
"""
import copy
import functools
import math

import pytest
import torch

import convnext_ref as R
import convnext_train_ref as T
from gpu_util import rel_l2

pytestmark = pytest.mark.gpu

SEED = 2
STAGE = {96: 1, 192: 3, 384: 5}
DATA_CEILING, PARAM_CEILING = 1e-4, 1e-3
# worst rel_l2 measured on an MI355X per group of checks
MEASURED = {"mlp_gxn": 7.82e-6, "mlp_param": 7.12e-6, "dwln_gx": 1.07e-7, "dwln_param": 1.64e-7, "down_gx": 4.55e-6,
            "dwln_many_param": 2.94e-7, "down_param": 5.14e-6, "stem_param": 2.41e-7, "net_param": 1.30e-5, "db_param": 2.28e-5}


def bound(key):
    ceiling = DATA_CEILING if key.endswith(("gxn", "gx")) else PARAM_CEILING
    return min(4 * MEASURED[key], ceiling)


@functools.lru_cache(maxsize=None)
def full_model():
    m32 = R.randomize_convnext(R.ConvNeXtTiny(), SEED).eval()
    return m32, copy.deepcopy(m32).double()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def operand(ws, P, C):
    """hi + lo of the normalised operand agp_cnx_dwconv_ln_fwd left in the workspace, as fp64 [P, C] (exact)."""
    ppad = (P + 31) // 32 * 32
    planes = ws[:2 * ppad * C * 2].view(torch.bfloat16).view(2, ppad, C)[:, :P]
    return (planes[0].double() + planes[1].double()).cpu()


def report(what, got, want, e32, key):
    err, floor = rel_l2(got, want), rel_l2(e32, want)
    print(f"{what}: rel_l2 {err:.3g} (fp32 CPU autograd {floor:.3g}) bound {bound(key):.3g}")
    assert err <= bound(key), (what, err, bound(key))
    return err


def zeros_like_params(dev, *shapes):
    return [torch.zeros(s, dtype=torch.float32, device=dev) for s in shapes]


# ------------------------------------------------------------------------------------------------------ MLP backward
class MlpCase:
    """One block's MLP backward on the device, its operand read back, and the fp64 / fp32 truths from that operand."""

    def __init__(self, dev, C, n, h, w, rows):
        from agplace_amd import convnext as cnx
        self.cnx, self.C, self.n, self.hw = cnx, C, n, h * w
        _, m64 = full_model()
        self.blk = blk = m64.features[STAGE[C]][0]
        P = n * h * w
        x = R.seeded_input((n, C, h, w), SEED + C + P, torch.float64) * 0.7
        gy = R.seeded_input((P, C), SEED + 3 * C + P, torch.float64)
        self.scale = None
        if rows == "kept":
            self.scale = torch.full((n,), 1.0 / 0.9, dtype=torch.float32)
        elif rows == "dropped":
            self.scale = torch.full((n,), 1.0 / 0.9, dtype=torch.float32)
            self.scale[n - 1] = 0.0
        pix = None if self.scale is None else self.scale.double().repeat_interleave(h * w)
        dblk = copy.deepcopy(blk).float().to(dev)
        self.p, self.pb = cnx.prep_block(dblk), cnx.prep_block_bwd(dblk)
        self.xs = nhwc(x).float().to(dev)
        self.ws = torch.empty(cnx.workspace_bytes(n, h, w, C), dtype=torch.uint8, device=dev)
        self.bws = torch.empty(cnx.bwd_workspace_bytes(n, h, w, C), dtype=torch.uint8, device=dev)
        cnx.dwconv_ln_fwd(self.xs, self.p, self.ws)
        xn = operand(self.ws, P, C)
        self.gy = gy.float().reshape(n, h, w, C).to(dev)
        self.sd = None if self.scale is None else self.scale.to(dev)
        self.want = T.mlp_truth(blk, xn, gy, pix, torch.float64)
        self.e32 = T.mlp_truth(blk, xn, gy, pix, torch.float32)
        pre = blk.block[3](xn)
        assert 0.2 <= float((pre < 0).double().mean()) <= 0.8

    def grads(self, dev):
        C = self.C
        return zeros_like_params(dev, (4 * C, C), (4 * C,), (C, 4 * C), (C,), (C, 1, 1))

    def run(self, grads):
        return self.cnx.mlp_bwd(self.ws, self.p, self.pb, self.gy, self.sd, grads, self.bws)


@pytest.mark.parametrize("rows", ["none", "kept", "dropped"])
@pytest.mark.parametrize("nhw", [(1, 1, 1), (3, 7, 3), (2, 5, 13)])
@pytest.mark.parametrize("C", [96, 192, 384])
def test_mlp_backward(dev, C, nhw, rows):
    """P = 1, 63 and 130; at (2, 5, 13) the tile of pixels 64..95 straddles both images, so a per-tile factor would show."""
    case = MlpCase(dev, C, *nhw, rows)
    g = case.grads(dev)
    gxn = case.run(g).reshape(-1, C)
    what = f"MLP bwd C={C} {nhw} rows={rows}"
    report(f"{what} gxn", gxn, case.want["gxn"], case.e32["gxn"], "mlp_gxn")
    for name, got in zip(("w1", "b1", "w2", "b2", "ls"), g):
        report(f"{what} {name}", got.reshape(case.want[name].shape), case.want[name], case.e32[name], "mlp_param")
    if rows == "dropped":
        tail = gxn[(case.n - 1) * case.hw:]
        assert bool((tail == 0).all()), "the dropped image's gxn must be exactly 0"
        if case.n == 1:
            assert all(bool((t == 0).all()) for t in g), "a dropped image contributed to a parameter gradient"


def test_mlp_backward_pixel_slices_accumulate_and_repeat(dev):
    """Three pixel slices of the weight-gradient sweep with a ragged last one (and a ragged last tile); a second call doubles
    every parameter gradient to one fp32 rounding step; two runs from zeroed buffers are bit-equal."""
    from agplace_amd import _lib
    L = int(_lib.load().agp_cnx_bwd_slice_pixels())
    n, h, w = 2, (2 * L + 300) // 4, 2
    P = n * h * w
    assert L == 1024 and math.ceil(P / L) == 3 and P % L and P % 32
    case = MlpCase(dev, 96, n, h, w, "dropped")
    g1, g2 = case.grads(dev), case.grads(dev)
    gx1 = case.run(g1)
    gx2 = case.run(g2)
    assert torch.equal(gx1, gx2) and all(torch.equal(a, b) for a, b in zip(g1, g2)), "two runs from zeroed buffers differ"
    report("MLP bwd slices gxn", gx1.reshape(P, 96), case.want["gxn"], case.e32["gxn"], "mlp_gxn")
    for name, got in zip(("w1", "b1", "w2", "b2", "ls"), g1):
        report(f"MLP bwd slices {name}", got.reshape(case.want[name].shape), case.want[name], case.e32[name], "mlp_param")
    case.run(g2)
    for name, a, b in zip(("w1", "b1", "w2", "b2", "ls"), g1, g2):
        assert bool(((b - 2 * a).abs() <= 2.0 ** -23 * b.abs()).all()), f"{name}: the second call did not add its gradient"


# ------------------------------------------------------------------------------- LayerNorm + depthwise 7x7 backward
@pytest.mark.parametrize("hw", [(4, 6), (9, 5)])
@pytest.mark.parametrize("C", [96, 192, 384])
def test_layernorm_depthwise_backward(dev, C, hw):
    """Every 7x7 window crosses a border and the second image is other data, 3x + 1: a bleed into the neighbouring image shows."""
    from agplace_amd import convnext as cnx
    _, m64 = full_model()
    blk = m64.features[STAGE[C]][1]
    x = R.seeded_input((2, C, *hw), SEED + C, torch.float64)
    x[1] = 3.0 * x[1] + 1.0
    gxn = R.seeded_input((2, *hw, C), SEED + C + 1, torch.float64)
    gy = R.seeded_input((2, C, *hw), SEED + C + 2, torch.float64)
    want, e32 = T.dwln_truth(blk, x, gxn, gy, torch.float64), T.dwln_truth(blk, x, gxn, gy, torch.float32)
    p = cnx.prep_block(copy.deepcopy(blk).float().to(dev))
    bws = torch.empty(cnx.bwd_workspace_bytes(2, *hw, C), dtype=torch.uint8, device=dev)
    g = zeros_like_params(dev, (C, 1, 7, 7), (C,), (C,), (C,))
    gx = cnx.dwconv_ln_bwd(nhwc(x).float().to(dev), gxn.float().to(dev), nhwc(gy).float().to(dev), p, g, bws)
    what = f"LN+dw bwd C={C} {hw}"
    report(f"{what} gx", gx.permute(0, 3, 1, 2), want["gx"], e32["gx"], "dwln_gx")
    for name, got in zip(("dw", "dwb", "g", "b"), g):
        report(f"{what} {name}", got, want[name], e32[name], "dwln_param")


def test_layernorm_depthwise_backward_many_tiles(dev):
    """65 x 4 = 260 tiles of 4 x 8 pixels (ragged last row and column of tiles): the workgroups' partial sums go through two
    levels of 16-wide group sums before the final one, and the depthwise weight gradient through 33 workgroups of 8 tiles."""
    from agplace_amd import convnext as cnx
    C, hw = 96, (258, 30)
    _, m64 = full_model()
    blk = m64.features[STAGE[C]][2]
    x = R.seeded_input((1, C, *hw), SEED + 40, torch.float64)
    gxn = R.seeded_input((1, *hw, C), SEED + 41, torch.float64)
    gy = R.seeded_input((1, C, *hw), SEED + 42, torch.float64)
    want, e32 = T.dwln_truth(blk, x, gxn, gy, torch.float64), T.dwln_truth(blk, x, gxn, gy, torch.float32)
    p = cnx.prep_block(copy.deepcopy(blk).float().to(dev))
    bws = torch.empty(cnx.bwd_workspace_bytes(1, *hw, C), dtype=torch.uint8, device=dev)
    g = zeros_like_params(dev, (C, 1, 7, 7), (C,), (C,), (C,))
    gx = cnx.dwconv_ln_bwd(nhwc(x).float().to(dev), gxn.float().to(dev), nhwc(gy).float().to(dev), p, g, bws)
    report("LN+dw bwd 260 tiles gx", gx.permute(0, 3, 1, 2), want["gx"], e32["gx"], "dwln_gx")
    for name, got in zip(("dw", "dwb", "g", "b"), g):
        report(f"LN+dw bwd 260 tiles {name}", got, want[name], e32[name], "dwln_many_param")


# ------------------------------------------------------------------------------------------------ downsample backward
@pytest.mark.parametrize("nhw", [(2, 7, 9), (1, 5, 4), (3, 2, 3)])
@pytest.mark.parametrize("C", [96, 192, 384])
def test_downsample_backward(dev, C, nhw):
    from agplace_amd import convnext as cnx
    _, m64 = full_model()
    ds = m64.features[STAGE[C] + 1]
    n, h, w = nhw
    x = R.seeded_input((n, C, h, w), SEED + 7 * C + h, torch.float64) * 2.0 + 0.5
    gout = R.seeded_input((n, 2 * C, h // 2, w // 2), SEED + 7 * C + h + 1, torch.float64)
    (gx64, want), (gx32, e32) = T.module_truth(ds, x, gout, torch.float64), T.module_truth(ds, x, gout, torch.float32)
    dds = copy.deepcopy(ds).float().to(dev)
    bws = torch.empty(cnx.bwd_workspace_bytes(n, h, w, C), dtype=torch.uint8, device=dev)
    g = zeros_like_params(dev, (C,), (C,), (2 * C, C, 2, 2), (2 * C,))
    gx = cnx.downsample_bwd(nhwc(x).float().to(dev), nhwc(gout).float().to(dev), cnx.prep_down(*dds), cnx.prep_down_bwd(*dds), g, bws)
    what = f"downsample bwd C={C} {nhw}"
    report(f"{what} gx", gx.permute(0, 3, 1, 2), gx64, gx32, "down_gx")
    for name, got in zip(("0.weight", "0.bias", "1.weight", "1.bias"), g):
        report(f"{what} {name}", got, want[name], e32[name], "down_param")
    dropped = gx[:, 2 * (h // 2):], gx[:, :, 2 * (w // 2):]
    assert h % 2 or w % 2
    assert all(bool((d == 0.0).all()) for d in dropped), "a dropped row / column must get a gradient of exactly 0.0"
    assert all(bool((d == 0).all()) for d in (gx64[:, :, 2 * (h // 2):], gx64[:, :, :, 2 * (w // 2):]))


# ------------------------------------------------------------------------------------------------------ stem backward
def test_stem_backward_strided_input(dev):
    from agplace_amd import convnext as cnx
    _, m64 = full_model()
    stem = m64.features[0]
    base = R.seeded_input((2, 3, 37, 90), SEED)
    x = base[:, :, 1:35, 3:83:2]                       # [2,3,34,40], neither contiguous nor unit-stride
    gout = R.seeded_input((2, 96, 8, 10), SEED + 1, torch.float64)
    (_, want), (_, e32) = T.module_truth(stem, x, gout, torch.float64, False), T.module_truth(stem, x, gout, torch.float32, False)
    xd = base.to(dev)[:, :, 1:35, 3:83:2]
    assert not xd.is_contiguous()
    bws = torch.empty(cnx.bwd_workspace_bytes(2, 8, 10, 96), dtype=torch.uint8, device=dev)
    g = zeros_like_params(dev, (96, 3, 4, 4), (96,), (96,), (96,))
    cnx.stem_bwd(xd, nhwc(gout).float().to(dev), cnx.prep_stem(*copy.deepcopy(stem).float().to(dev)), g, bws)
    for name, got in zip(("0.weight", "0.bias", "1.weight", "1.bias"), g):
        report(f"stem bwd {name}", got, want[name], e32[name], "stem_param")


def test_bwd_workspace_has_no_hidden_map_term(dev):
    """Per-slice partial planes and one stream-sized map: 8 C^2 floats per 1024 pixels, never P x 4C."""
    from agplace_amd import _lib
    L = _lib.load()
    for C in (96, 192, 384):
        for n, h, w in ((1, 1, 1), (2, 17, 25), (64, 64, 64)):
            P = n * h * w
            slices = math.ceil(P / 1024)
            assert 0 < L.agp_cnx_bwd_workspace_bytes(n, h, w, C) <= 4 * (slices * (8 * C * C + 7 * C) + 2.7 * P * C + 3 * 49 * C) + 65536


# -------------------------------------------------------------------------------------------------------------- trunk
LAYERS = "2_1_2"
SHAPE = (2, 3, 32, 48)                   # maps 8x12, 4x6, 2x3


@functools.lru_cache(maxsize=None)
def trunk32():
    return R.seeded_trunk([int(v) for v in LAYERS.split("_")], SEED, torch.float32)


def device_fe(dev, train):
    from agplace_amd.network.image_fe import ImageFE
    fe = ImageFE("convnext_tiny", LAYERS)
    fe.fe.load_state_dict(trunk32().state_dict(), strict=True)
    fe.fe.enable_training()
    return fe.to(dev).train(train)


@functools.lru_cache(maxsize=None)
def map_weights():
    sizes = [(96, 8, 12), (192, 4, 6), (384, 2, 3)]
    return [R.seeded_input((SHAPE[0], *s), SEED + 20 + i, torch.float64) for i, s in enumerate(sizes)]


@functools.lru_cache(maxsize=None)
def trunk_truth(which, dtype):
    """Per-parameter gradients of the weighted sum of ALL THREE maps through the restatement; computed once per case."""
    m = copy.deepcopy(trunk32()).to(dtype).eval()
    x = R.seeded_input(SHAPE, SEED).to(dtype)
    R.check_weights_are_felt(copy.deepcopy(trunk32()).double(), R.seeded_input(SHAPE, SEED))
    maps = T.forward_maps_scaled(m, x, injected_scales(dtype) if which == "train" else None)
    loss = sum((a * b.to(dtype)).sum() for a, b in zip(maps, map_weights()))
    names, ps = zip(*m.features.named_parameters())
    return dict(zip(names, torch.autograd.grad(loss, ps))), [v.detach() for v in maps]


def injected_scales(dtype=torch.float32):
    """One entry per block of '2_1_2': the first block unscaled, the others kept at 1 / (1 - p_k); image 0 dropped in block 3."""
    probs = [p for stage in T.sd_probs([2, 1, 2]) for p in stage]
    scales = [None] + [torch.full((SHAPE[0],), 1.0 / (1.0 - p), dtype=dtype) for p in probs[1:]]
    scales[3][0] = 0.0
    return scales


def device_loss(maps, dev):
    return sum((m * w.float().to(dev)).sum() for m, w in zip(maps, map_weights()))


def check_trunk_grads(fe, maps, which, key):
    (want, maps64), (e32, _) = trunk_truth(which, torch.float64), trunk_truth(which, torch.float32)
    for i, (m, r) in enumerate(zip(maps, maps64)):              # the training forward itself: the mode-3 map bar
        err = rel_l2(m, r)
        print(f"trunk {which} map {i}: rel_l2 {err:.3g}")
        assert m.dtype == torch.float32 and tuple(m.shape) == tuple(r.shape) and err < 1e-4, (which, i, err)
    worst = 0.0
    for name, p in fe.fe.features.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, name
        worst = max(worst, report(f"trunk {which} {name}", p.grad, want[name], e32[name], key))
    print(f"trunk {which}: worst parameter gradient rel_l2 {worst:.3g}")


def test_trunk_gradients_eval(dev):
    fe = device_fe(dev, False)
    last, maps = fe(R.seeded_input(SHAPE, SEED).to(dev))
    assert last is maps[-1] and [tuple(m.shape[1:]) for m in maps] == [(96, 8, 12), (192, 4, 6), (384, 2, 3)]
    device_loss(maps, dev).backward()
    check_trunk_grads(fe, maps, "eval", "net_param")


def test_trunk_gradients_train_with_injected_row_scales(dev):
    fe = device_fe(dev, True)
    maps = fe.fe.forward_maps_train(R.seeded_input(SHAPE, SEED).to(dev),
                                    row_scales=[None if s is None else s.to(dev) for s in injected_scales()])
    device_loss(maps, dev).backward()
    check_trunk_grads(fe, maps, "train", "net_param")


def test_trunk_drawn_scales_and_seeded_repeat(dev):
    fe = device_fe(dev, True)
    fe.fe.stochastic_depth_prob = 1.0                 # p_k = k / 17: both outcomes occur among 8 images x 4 scaled blocks
    x = R.seeded_input((8, 3, 32, 32), SEED).to(dev)
    runs = []
    for _ in range(2):
        torch.manual_seed(11)
        with torch.no_grad():
            maps = fe(x)[1]
        runs.append(([m.clone() for m in maps], fe.fe.last_row_scales))
    probs = [p for stage in fe.fe.sd_probs() for p in stage]
    assert probs == pytest.approx([0.0, 1 / 17, 3 / 17, 6 / 17, 7 / 17])
    scales = runs[0][1]
    assert scales[0] is None and len(scales) == 5
    seen = set()
    for p, s in zip(probs[1:], scales[1:]):
        keep = torch.tensor(1.0 / (1.0 - p), dtype=torch.float32)
        assert tuple(s.shape) == (8,) and bool(((s == 0) | (s.cpu() == keep).to(dev)).all()), (p, s)
        seen |= {float(v) == 0.0 for v in s.cpu()}
    assert seen == {True, False}
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b), "two forwards under the same torch.manual_seed differ"
    for a, b in zip(runs[0][1][1:], runs[1][1][1:]):
        assert torch.equal(a, b)


def test_whole_step_is_repeatable(dev):
    fe = device_fe(dev, True)
    x = R.seeded_input(SHAPE, SEED).to(dev)
    scales = [None if s is None else s.to(dev) for s in injected_scales()]
    runs = []
    for _ in range(2):
        fe.zero_grad(set_to_none=True)
        device_loss(fe.fe.forward_maps_train(x, row_scales=scales), dev).backward()
        runs.append({k: p.grad.clone() for k, p in fe.fe.features.named_parameters()})
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), f"{k}: two forward + backward passes from the same state differ"


def test_input_gradient_is_refused(dev):
    fe = device_fe(dev, False)
    with pytest.raises(NotImplementedError, match="input image"):
        fe(torch.zeros(1, 3, 32, 32, device=dev, requires_grad=True))


# -------------------------------------------------------------------------------------------------------------- model
def db_model(dev, share):
    from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
    from agplace_amd.options import Options
    opt = Options(dbimage_fe="convnext_tiny", dbimage_fe_layers="1_1_1", convnext_train=True, maptype="a_b", share_dbfe=share)
    torch.manual_seed(3)
    model = DBVanilla2D("db", 256, opt=opt)
    m32s = []
    for i, e in enumerate(model.dbimage_fes):
        m32 = R.seeded_trunk([1, 1, 1], SEED + i, torch.float32)
        e.fe.load_state_dict(m32.state_dict(), strict=True)
        m32s.append(m32)
    return model.to(dev), opt, m32s


def db_truth(model, opt, m32s, tiles, wgt, dtype):
    """Gradients of sum(wgt * embedding) through the restatement's trunks and the oracle's head arithmetic."""
    import torch.nn.functional as F
    from oracle import nets
    ms = [copy.deepcopy(m).to(dtype) for m in m32s]
    state = {k: v.detach().to(dtype).cpu().clone().requires_grad_(True) for k, v in model.state_dict().items()
             if not k.startswith("dbimage_fes.")}
    b, ndb, nmap, c, h, w = tiles.shape
    vecs = []
    for i in range(nmap):
        j = 0 if opt.share_dbfe is True else i
        last = R.forward_maps(ms[j], tiles[:, :, i].reshape(-1, c, h, w).to(dtype))[-1]
        vecs.append(nets.db_mlp(nets.gem_flat(last, state[f"dbimage_pools.{j}.p"]), state, f"dbimage_mlps.{j}."))
    out = torch.stack(vecs, dim=1)
    if opt.output_l2:
        out = F.normalize(out, p=2, dim=-1)
    out = out.mean(dim=1).view(b, ndb, -1)
    if opt.final_l2:
        out = F.normalize(out, p=2, dim=-1)
    (out * wgt.to(dtype)).sum().backward()
    grads = {k: v.grad for k, v in state.items()}
    for i, m in enumerate(ms):
        grads.update({f"dbimage_fes.{i}.fe.features.{k}": p.grad for k, p in m.features.named_parameters()})
    return grads


@pytest.mark.parametrize("share", [True, False])
def test_dbvanilla2d_gradients(dev, share):
    """.eval() with gradients enabled: trunk, GeM p and head gradients of a loss on the embedding; with share_dbfe one trunk
    serves both map types and its gradients accumulate."""
    model, opt, m32s = db_model(dev, share)
    model.eval()
    tiles = R.seeded_input((2, 2, 2, 3, 32, 32), SEED + 11)
    wgt = R.seeded_input((2, 2, 256), SEED + 12, torch.float64)
    want, e32 = (db_truth(model, opt, m32s, tiles, wgt, d) for d in (torch.float64, torch.float32))
    out = model({"db_map": tiles.to(dev)}, mode="db")["embedding"]
    (out * wgt.float().to(dev)).sum().backward()
    used = (0,) if share else (0, 1)
    checked = 0
    for name, p in model.named_parameters():
        idx = int(name.split(".")[1])
        if "classifier" in name:
            continue
        if idx not in used:
            assert p.grad is None and want[name] is None, name
            continue
        assert p.grad is not None, name
        report(f"DBVanilla2D share={share} {name}", p.grad, want[name], e32[name], "db_param")
        checked += 1
    assert checked == len(used) * (len(list(m32s[0].features.parameters())) + 1 + 6)


def test_dbvanilla2d_train_under_no_grad_saves_nothing(dev):
    """The reference with --train_modeldb False: .train() under torch.no_grad() draws scales and records no tape; a training
    forward + backward right after it is not blocked."""
    model, _, _ = db_model(dev, False)
    model.train()
    tiles = R.seeded_input((2, 2, 2, 3, 32, 32), SEED + 11).to(dev)
    with torch.no_grad():
        out = model({"db_map": tiles}, mode="db")["embedding"]
    assert tuple(out.shape) == (2, 2, 256) and out.grad_fn is None and not out.requires_grad and bool(torch.isfinite(out).all())
    out = model({"db_map": tiles}, mode="db")["embedding"]
    assert out.grad_fn is not None
    (out * R.seeded_input((2, 2, 256), SEED + 12).to(dev)).sum().backward()
    g = model.dbimage_fes[1].fe.features[0][0].weight.grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
