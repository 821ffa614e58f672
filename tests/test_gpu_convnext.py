"""ConvNeXt-tiny trunk on the GPU (csrc/convnext.hip, agplace_amd/convnext.py) against the fp64 CPU restatement
(tests/convnext_ref.py): the four kernels alone, the trunk through ImageFE, DBVanilla2D on top of it.

Bounds.  Stem (plain fp32 arithmetic): max(8 x e32, 1e-6), e32 = the fp32 CPU restatement's own error on the same data.
Depthwise + LayerNorm operand and downsample: rel_l2 < 2e-5, the project's mode-3 kernel bound.  Exported maps and the
embedding: 1e-4 in rel_l2 and rel_max, the project's mode-3 bar.  Fused MLP (two chained three-product GEMMs with a GELU
between them): first measured on an MI355X at rel_l2 <= 3.98e-6 and rel_max <= 5.53e-6 over C in {96, 192, 384} x P in {1, 63, 130}
(DESIGN.md section 2); the bounds below are 4x those, which covers box-to-box accumulation-order differences.
"""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

import convnext_ref as R
from gpu_util import rel_l2, rel_max

pytestmark = pytest.mark.gpu

SEED = 2
MLP_L2_BOUND, MLP_MAX_BOUND = 4 * 3.98e-6, 4 * 5.53e-6
STAGE = {96: 1, 192: 3, 384: 5}          # features index of the stage with C channels


@functools.lru_cache(maxsize=None)
def full_model():
    """The whole seeded network in fp32 (the weights the device gets) and the same weights in fp64 (the truth)."""
    m32 = R.randomize_convnext(R.ConvNeXtTiny(), SEED).eval()
    return m32, copy.deepcopy(m32).double()


@functools.lru_cache(maxsize=None)
def trunks(layers):
    m32 = R.seeded_trunk([int(v) for v in layers.split("_")], SEED, torch.float32)
    return m32, copy.deepcopy(m32).double()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def operand(ws, P, C):
    """hi + lo of the normalised operand agp_cnx_dwconv_ln_fwd left in the workspace, as fp64 [P, C] (exact)."""
    ppad = (P + 31) // 32 * 32
    planes = ws[:2 * ppad * C * 2].view(torch.bfloat16).view(2, ppad, C)[:, :P]
    return (planes[0].double() + planes[1].double()).cpu()


# ------------------------------------------------------------------------------------------------------------ kernels
def test_stem_strided_input(dev):
    from agplace_amd import convnext as cnx
    m32, m64 = full_model()
    base = R.seeded_input((2, 3, 37, 90), SEED)
    x = base[:, :, 1:35, 3:83:2]                       # [2,3,34,40], neither contiguous nor unit-stride
    assert not x.is_contiguous()
    with torch.no_grad():
        want = m64.features[0](x.double())
        e32_l2, e32_max = rel_l2(m32.features[0](x), want), rel_max(m32.features[0](x), want)
        xd = base.to(dev)[:, :, 1:35, 3:83:2]
        got = cnx.stem_fwd(xd, cnx.prep_stem(*copy.deepcopy(m32.features[0]).to(dev)))
    assert tuple(got.shape) == (2, 8, 10, 96)
    l2, mx = rel_l2(got.permute(0, 3, 1, 2), want), rel_max(got.permute(0, 3, 1, 2), want)
    print(f"stem: rel_l2 {l2:.3g} (fp32 CPU {e32_l2:.3g}) rel_max {mx:.3g} (fp32 CPU {e32_max:.3g})")
    assert l2 <= max(8 * e32_l2, 1e-6) and mx <= max(8 * e32_max, 1e-6)


@pytest.mark.parametrize("hw", [(4, 6), (9, 5)])
@pytest.mark.parametrize("C", [96, 192, 384])
def test_dwconv_layernorm_operand(dev, C, hw):
    """Every 7x7 window of these maps crosses a border, and the two images differ, so a window that bleeds into the neighbouring
    image (or reads a wrapped row) shows."""
    from agplace_amd import convnext as cnx
    _, m64 = full_model()
    blk = m64.features[STAGE[C]][1]
    x = R.seeded_input((2, C, *hw), SEED + C, torch.float64)
    x[1] = 3.0 * x[1] + 1.0
    with torch.no_grad():
        want = blk.block[2](blk.block[0](x).permute(0, 2, 3, 1)).reshape(-1, C)
        xs = nhwc(x).float().to(dev)
        ws = torch.empty(cnx.workspace_bytes(*xs.shape), dtype=torch.uint8, device=dev)
        cnx.dwconv_ln_fwd(xs, cnx.prep_block(copy.deepcopy(blk).float().to(dev)), ws)
    got = operand(ws, want.shape[0], C)
    err = rel_l2(got, want)
    print(f"dwconv+ln C={C} {hw}: rel_l2 {err:.3g} rel_max {rel_max(got, want):.3g}")
    assert err < 2e-5


@pytest.mark.parametrize("nhw", [(2, 7, 9), (1, 5, 4), (3, 2, 3)])
@pytest.mark.parametrize("C", [96, 192, 384])
def test_downsample_odd_sizes(dev, C, nhw):
    from agplace_amd import convnext as cnx
    _, m64 = full_model()
    ds = m64.features[STAGE[C] + 1]
    n, h, w = nhw
    x = R.seeded_input((n, C, h, w), SEED + 7 * C + h, torch.float64) * 2.0 + 0.5
    with torch.no_grad():
        want = ds(x)
        got = cnx.downsample_fwd(nhwc(x).float().to(dev), cnx.prep_down(*copy.deepcopy(ds).float().to(dev)))
    assert tuple(got.shape) == (n, h // 2, w // 2, 2 * C)
    err = rel_l2(got.permute(0, 3, 1, 2), want)
    print(f"downsample C={C} {nhw}: rel_l2 {err:.3g} rel_max {rel_max(got.permute(0, 3, 1, 2), want):.3g}")
    assert err < 2e-5


@pytest.mark.parametrize("P", [1, 63, 130])
@pytest.mark.parametrize("C", [96, 192, 384])
def test_fused_mlp(dev, C, P):
    """The MLP alone: its fp64 truth starts from the very operand (hi + lo) the kernel reads, so the depthwise kernel's error
    is not in the figure.  Out of place and in place, each twice."""
    from agplace_amd import convnext as cnx
    _, m64 = full_model()
    blk = m64.features[STAGE[C]][0]
    x = R.seeded_input((1, C, P, 1), SEED + C + P, torch.float64) * 0.7
    with torch.no_grad():
        xs = nhwc(x).float().to(dev)                                # the stream [1, P, 1, C]
        p = cnx.prep_block(copy.deepcopy(blk).float().to(dev))
        ws = torch.empty(cnx.workspace_bytes(*xs.shape), dtype=torch.uint8, device=dev)
        cnx.dwconv_ln_fwd(xs, p, ws)
        xn = operand(ws, P, C)
        pre = blk.block[3](xn)
        neg = float((pre < 0).double().mean())
        branch = blk.layer_scale.reshape(C) * blk.block[5](R.gelu_exact(pre))
        resid = xs.double().cpu().reshape(P, C)
        want = resid + branch
        assert 0.2 <= neg <= 0.8 and rel_l2(want, resid) >= 0.3, (neg, rel_l2(want, resid))
        outs = [cnx.mlp_fwd(ws, p, xs, torch.full_like(xs, float("nan"))) for _ in range(2)]
        for _ in range(2):
            inplace = xs.clone()
            outs.append(cnx.mlp_fwd(ws, p, inplace, inplace))
    for o in outs[1:]:
        assert torch.equal(o, outs[0]), "runs of the fused MLP differ (out of place, out of place, in place, in place)"
    got = outs[0].reshape(P, C)
    l2, mx = rel_l2(got, want), rel_max(got, want)
    print(f"fused MLP C={C} P={P}: rel_l2 {l2:.3g} rel_max {mx:.3g}")
    assert l2 < MLP_L2_BOUND <= 1e-4 and mx < MLP_MAX_BOUND <= 1e-4


def test_workspace_has_no_hidden_map_term(dev):
    from agplace_amd import _lib
    L = _lib.load()
    for C in (96, 192, 384):
        for n, h, w in ((1, 1, 1), (2, 17, 25), (64, 64, 64)):
            assert 0 < L.agp_cnx_workspace_bytes(n, h, w, C) <= 1.25 * n * h * w * C * 4 + 65536


# -------------------------------------------------------------------------------------------------------------- trunk
def device_fe(layers, m32, dev):
    from agplace_amd.network.image_fe import ImageFE
    fe = ImageFE("convnext_tiny", layers)
    fe.fe.load_state_dict(m32.state_dict(), strict=True)
    return fe.to(dev).eval()


def check_maps(maps, want, what):
    for i, (m, r) in enumerate(zip(maps, want)):
        assert m.dtype == torch.float32 and tuple(m.shape) == tuple(r.shape), (what, i, m.shape, r.shape)
        assert m.is_contiguous(memory_format=torch.channels_last) or m.shape[2] * m.shape[3] == 1, (what, i, "not channels_last")
        l2, mx = rel_l2(m, r), rel_max(m, r)
        print(f"{what} map {i}: rel_l2 {l2:.3g} rel_max {mx:.3g}")
        assert l2 < 1e-4 and mx < 1e-4, (what, i, l2, mx)


@pytest.mark.parametrize("layers,shape", [("2_2_2", (2, 3, 70, 100)), ("1_1_1", (2, 3, 70, 100)), ("3_3_9", (1, 3, 32, 32))])
def test_trunk_maps(dev, layers, shape):
    m32, m64 = trunks(layers)
    x = R.seeded_input(shape, SEED)
    R.check_weights_are_felt(m64, x)
    with torch.no_grad():
        want = R.forward_maps(m64, x.double())
        fe = device_fe(layers, m32, dev)
        last, maps = fe(x.to(dev))
    assert last is maps[-1] and len(maps) == 3 and fe.last_dim == 384 == last.shape[1]
    check_maps(maps, want, layers)


def test_trunk_follows_the_reference_control_flow(dev, golden):
    """The fixture's maps came out of the reference's own ImageFE('convnext_tiny', '2_1_2') (tests/golden/make_convnext_flow.py)."""
    g = golden("convnext_flow")
    layers = str(g["layers"])
    m32 = R.seeded_trunk([int(v) for v in layers.split("_")], int(g["seed"]), torch.float32)
    with torch.no_grad():
        _, maps = device_fe(layers, m32, dev)(torch.from_numpy(g["x"]).to(dev))
    check_maps(maps, [torch.from_numpy(g[f"map{i}"]) for i in range(3)], "fixture")


def test_too_small_input_and_gradients_are_refused(dev):
    m32, _ = trunks("1_1_1")
    fe = device_fe("1_1_1", m32, dev)
    with torch.no_grad(), pytest.raises(ValueError, match="too small"):
        fe(torch.zeros(1, 3, 15, 64, device=dev))
    with pytest.raises(NotImplementedError, match="gradients"):
        fe(torch.zeros(1, 3, 32, 32, device=dev))
    with torch.no_grad(), pytest.raises(NotImplementedError, match="train"):
        fe.train()(torch.zeros(1, 3, 32, 32, device=dev))


def test_captured_forward_replays_bit_equal(dev):
    m32, _ = trunks("1_1_1")
    fe = device_fe("1_1_1", m32, dev)
    x = R.seeded_input((2, 3, 40, 36), SEED).to(dev)
    with torch.no_grad():
        eager = [m.clone() for m in fe(x)[1]]              # the warm-up: prepares the weights
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            _, maps = fe(x)
        for m in maps:
            m.zero_()
        graph.replay()
        torch.cuda.synchronize()
    for a, b in zip(maps, eager):
        assert torch.equal(a, b)


# -------------------------------------------------------------------------------------------------------------- model
def db_reference(db_map, state, opt, m64s):
    """The restatement's last map, then the oracle's head arithmetic (oracle/nets.py: dbvanilla2d_forward_db), in fp64."""
    from oracle import nets
    if db_map.dim() == 5:
        db_map = db_map.unsqueeze(1)
    b, ndb, nmap, c, h, w = db_map.shape
    vecs = []
    for i in range(nmap):
        j = 0 if opt.share_dbfe is True else i
        m = R.forward_maps(m64s[j], db_map[:, :, i].reshape(-1, c, h, w).double())[-1]
        vecs.append(nets.db_mlp(nets.gem_flat(m, state[f"dbimage_pools.{j}.p"]), state, f"dbimage_mlps.{j}."))
    out = torch.stack(vecs, dim=1)
    if opt.output_l2:
        out = F.normalize(out, p=2, dim=-1)
    out = out.mean(dim=1).view(b, ndb, -1)
    if opt.final_l2:
        out = F.normalize(out, p=2, dim=-1)
    return out


def db_model(dev, maptype="a", share=False):
    from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
    from agplace_amd.options import Options
    opt = Options(dbimage_fe="convnext_tiny", dbimage_fe_layers="2_1_2", maptype=maptype, share_dbfe=share)
    torch.manual_seed(3)
    model = DBVanilla2D("db", 256, opt=opt)
    m64s = []
    for i, e in enumerate(model.dbimage_fes):
        m32 = R.seeded_trunk([2, 1, 2], SEED + i, torch.float32)
        e.fe.load_state_dict(m32.state_dict(), strict=True)
        m64s.append(copy.deepcopy(m32).double())
    return model.to(dev).eval(), opt, m64s


@pytest.mark.parametrize("shape,maptype,share", [((2, 1, 3, 64, 64), "a", False), ((1, 2, 1, 3, 64, 64), "a", False),
                                                 ((2, 2, 3, 64, 64), "a_b", False), ((2, 2, 3, 64, 64), "a_b", True)])
def test_dbvanilla2d_embedding(dev, shape, maptype, share):
    model, opt, m64s = db_model(dev, maptype, share)
    tiles = R.seeded_input(shape, SEED + 11)
    with torch.no_grad():
        got = model({"db_map": tiles.to(dev)}, mode="db")["embedding"]
        want = db_reference(tiles, {k: v.detach().double().cpu() for k, v in model.state_dict().items()}, opt, m64s)
    want = want.view(got.shape)
    l2, mx = rel_l2(got, want), rel_max(got, want)
    print(f"DBVanilla2D {shape} {maptype} share={share}: rel_l2 {l2:.3g} rel_max {mx:.3g}")
    assert l2 < 1e-4 and mx < 1e-4


def test_dbvanilla2d_refusals_and_frozen_trunk_heads(dev):
    from agplace_amd import pair
    model, _, _ = db_model(dev)
    tiles = R.seeded_input((2, 1, 3, 64, 64), SEED + 11).to(dev)
    with pytest.raises(NotImplementedError, match="gradients"):
        model({"db_map": tiles}, mode="db")
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="uint8"):
            model({"db_map": torch.zeros(2, 1, 64, 64, 3, dtype=torch.uint8, device=dev)}, mode="db")
        with pytest.raises(NotImplementedError, match="db_frames"):
            model({"db_frames": torch.zeros(2, 1, 80, 80, 3, dtype=torch.uint8, device=dev)}, mode="db")
        with pytest.raises(NotImplementedError, match="embed_pair"):
            pair.embed_pair(None, model, {}, {"db_map": tiles})
        with pytest.raises(NotImplementedError, match="train"):
            model.train()({"db_map": tiles}, mode="db")
        want = model.eval()({"db_map": tiles}, mode="db")["embedding"]
    # trainable heads on a frozen trunk: the existing mechanism (freeze_backbone + the ops' own backward kernels)
    model.freeze_backbone()
    out = model({"db_map": tiles}, mode="db")["embedding"]
    assert torch.equal(out.detach(), want)
    out.square().sum().backward()
    g = model.dbimage_mlps[0].seq[0].weight.grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    assert all(p.grad is None for p in model.dbimage_fes.parameters())
