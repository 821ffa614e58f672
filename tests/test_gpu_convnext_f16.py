"""Precision 4 of the ConvNeXt-tiny trunk on the GPU (Options.convnext_precision = 4, ConvNeXt.set_precision(4);
csrc/convnext.hip PREC = 4, agp_cnx_*_f16_fwd) against the fp64 restatement (tests/convnext_ref.py) and its fp16 emulation
(tests/convnext_f16_ref.py: fp64 arithmetic, rounded to fp16 in the six places the kernels round).

Bound of the MLP, downsample and trunk tests: E = rel_l2(emulation, truth) on the same data, computed in the test; the device's
rel_l2 against the truth must be <= 1.5 E, and <= 1e-3 for the trunk's maps.  The device rounds values that differ from the
emulation's in the last fp32 bits, so single roundings fall differently while the error's size does not; a dropped k-step, a bf16
operand or a truncating conversion lands at 2x to 8x.  The operand plane is held to 1.5 x the error of fp16(truth).  Each test
prints device against truth, E, and device against emulation (reported, not gated).

Measured on an MI355X (rel_l2: device against truth / E / device against emulation):
  operand plane, C = 96 / 192 / 384     2.00e-4 .. 2.10e-4 / the same (fp16 of the truth) / 1.6e-7 .. 1.1e-5
  fused MLP, C x P = 1 / 63 / 130       1.92e-4 .. 2.61e-4 / equal to three digits / 5.4e-8 .. 9.8e-6
  downsample, odd sizes, C = 96 / 192   2.76e-4 .. 2.95e-4 / equal to three digits / 1.3e-7 .. 9.0e-6
  2_2_2 maps at [2,3,64,96]             2.53e-4, 4.46e-4, 5.66e-4 / 2.53e-4, 4.47e-4, 5.66e-4 / 6.8e-5, 2.6e-4, 4.2e-4
  2_2_2 maps at strided [2,3,38,52]     2.48e-4, 4.42e-4, 5.50e-4 / equal to three digits / 5.9e-5, 2.5e-4, 3.9e-4
  DBVanilla2D embedding, 4 against 3    1.95e-4;  MM outputs the image reaches, 4 against 3: 1.25e-4 .. 2.42e-4
"""
import copy
import functools

import pytest
import torch

import convnext_f16_ref as H
import convnext_ref as R
import mm_convnext_ref as ref
from gpu_util import rel_l2, to_dev
from oracle import nets

pytestmark = pytest.mark.gpu

SEED = 2
FACTOR = 1.5
STAGE = {96: 1, 192: 3, 384: 5}          # features index of the stage with C channels
KEYS = ("imagevec_org", "voxvec_org", "shallowvec_org", "stg2fusevec", "stg2imagevec", "stg2voxvec", "embedding")


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


def plane(ws, P, C):
    """The fp16 operand plane agp_cnx_dwconv_ln_f16_fwd left at the start of the workspace, as fp64 [P, C] (exact)."""
    ppad = (P + 31) // 32 * 32
    return ws[:ppad * C * 2].view(torch.float16).view(ppad, C)[:P].double().cpu()


def report(what, got, truth, emu):
    """Prints the three figures; returns (device against truth, E)."""
    err, e, de = rel_l2(got, truth), rel_l2(emu, truth), rel_l2(got, emu)
    print(f"f16 {what}: device-truth {err:.3g}  E {e:.3g}  device-emulation {de:.3g}")
    return err, e


# ------------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("hw", [(4, 6), (9, 5)])
@pytest.mark.parametrize("C", [96, 192, 384])
def test_operand_plane(dev, C, hw):
    """Every 7x7 window crosses a border and the two images differ (tests/test_gpu_convnext.py); the plane is one fp16 plane."""
    from agplace_amd import convnext as cnx
    _, m64 = full_model()
    blk = m64.features[STAGE[C]][1]
    x = R.seeded_input((2, C, *hw), SEED + C, torch.float64)
    x[1] = 3.0 * x[1] + 1.0
    with torch.no_grad():
        want = H.block_operand(blk, x).reshape(-1, C)
        xs = nhwc(x).float().to(dev)
        ws = torch.zeros(cnx.workspace_bytes(*xs.shape), dtype=torch.uint8, device=dev)
        cnx.dwconv_ln_fwd(xs, cnx.prep_block(copy.deepcopy(blk).float().to(dev), prec=4), ws, prec=4)
    P = want.shape[0]
    got = plane(ws, P, C)
    err, floor = rel_l2(got, want), rel_l2(H.round_f16(want), want)
    print(f"f16 operand C={C} {hw}: device-truth {err:.3g}  fp16(truth)-truth {floor:.3g}  device-fp16(truth) {rel_l2(got, H.round_f16(want)):.3g}")
    assert err <= FACTOR * floor
    assert not bool(ws[(P + 31) // 32 * 32 * C * 2:].any()), "the fp16 mode wrote past its one plane"


@pytest.mark.parametrize("P", [1, 63, 130])
@pytest.mark.parametrize("C", [96, 192, 384])
def test_fused_mlp(dev, C, P):
    """The MLP alone: truth and emulation start from the very fp16 operand the kernel reads.  Out of place and in place, each
    twice, all four bit-equal."""
    from agplace_amd import convnext as cnx
    _, m64 = full_model()
    blk = m64.features[STAGE[C]][0]
    x = R.seeded_input((1, C, P, 1), SEED + C + P, torch.float64) * 0.7
    with torch.no_grad():
        xs = nhwc(x).float().to(dev)                                # the stream [1, P, 1, C]
        p = cnx.prep_block(copy.deepcopy(blk).float().to(dev), prec=4)
        ws = torch.empty(cnx.workspace_bytes(*xs.shape), dtype=torch.uint8, device=dev)
        cnx.dwconv_ln_fwd(xs, p, ws, prec=4)
        xn = plane(ws, P, C)
        resid = xs.double().cpu().reshape(P, C)
        want, emu = H.block_mlp(blk, xn, resid), H.block_mlp(blk, xn, resid, H.round_f16)
        neg = float((blk.block[3](xn) < 0).double().mean())
        assert 0.2 <= neg <= 0.8 and rel_l2(want, resid) >= 0.3, (neg, rel_l2(want, resid))
        outs = [cnx.mlp_fwd(ws, p, xs, torch.full_like(xs, float("nan")), prec=4) for _ in range(2)]
        for _ in range(2):
            inplace = xs.clone()
            outs.append(cnx.mlp_fwd(ws, p, inplace, inplace, prec=4))
    for o in outs[1:]:
        assert torch.equal(o, outs[0]), "runs of the fused fp16 MLP differ (out of place, out of place, in place, in place)"
    err, e = report(f"MLP C={C} P={P}", outs[0].reshape(P, C), want, emu)
    assert err <= FACTOR * e


@pytest.mark.parametrize("nhw", [(2, 7, 9), (1, 5, 4), (3, 2, 3)])
@pytest.mark.parametrize("C", [96, 192])
def test_downsample_odd_sizes(dev, C, nhw):
    from agplace_amd import convnext as cnx
    _, m64 = full_model()
    ds = m64.features[STAGE[C] + 1]
    n, h, w = nhw
    x = R.seeded_input((n, C, h, w), SEED + 7 * C + h, torch.float64) * 2.0 + 0.5
    with torch.no_grad():
        want, emu = H.downsample(ds, x), H.downsample(ds, x, H.round_f16)
        got = cnx.downsample_fwd(nhwc(x).float().to(dev), cnx.prep_down(*copy.deepcopy(ds).float().to(dev), prec=4), prec=4)
    assert tuple(got.shape) == (n, h // 2, w // 2, 2 * C)
    err, e = report(f"downsample C={C} {nhw}", got.permute(0, 3, 1, 2), want, emu)
    assert err <= FACTOR * e


def test_saturation_and_nan(dev):
    """A LayerNorm weight of 1e5 puts the operand beyond 65504: the plane saturates and the block's output stays finite.  A NaN
    in the stream stays a NaN in the plane (the clamp alone would make it -65504)."""
    from agplace_amd import convnext as cnx
    _, m64 = full_model()
    C, hw = 96, (9, 12)
    blk = copy.deepcopy(m64.features[STAGE[C]][0]).float()
    with torch.no_grad():
        blk.block[2].weight.fill_(1e5)
        xs = nhwc(R.seeded_input((1, C, *hw), SEED)).to(dev)
        p = cnx.prep_block(blk.to(dev), prec=4)
        ws = torch.empty(cnx.workspace_bytes(*xs.shape), dtype=torch.uint8, device=dev)
        cnx.dwconv_ln_fwd(xs, p, ws, prec=4)
        pl = plane(ws, hw[0] * hw[1], C)
        out = cnx.mlp_fwd(ws, p, xs, torch.empty_like(xs), prec=4)
        assert float(pl.abs().max()) == 65504.0 and float((pl.abs() == 65504.0).double().mean()) > 0.1
        assert bool(torch.isfinite(out).all())
        xs[0, 0, 0, 5] = float("nan")                   # pixel (0, 0), channel 5: reaches the 4 x 4 pixels whose window holds it
        cnx.dwconv_ln_fwd(xs, p, ws, prec=4)
        bad = torch.isnan(plane(ws, hw[0] * hw[1], C)).view(*hw, C)
    assert bool(bad[:4, :4].all()) and int(bad.sum()) == 16 * C


# -------------------------------------------------------------------------------------------------------------- trunk
def device_fe(layers, m32, dev, prec=3):
    from agplace_amd.network.image_fe import ImageFE
    from agplace_amd.options import Options
    fe = ImageFE("convnext_tiny", layers, opt=Options(convnext_precision=prec))
    fe.fe.load_state_dict(m32.state_dict(), strict=True)
    return fe.to(dev).eval()


@functools.lru_cache(maxsize=None)
def trunk_input(which):
    if which == "plain":
        return R.seeded_input((2, 3, 64, 96), SEED)
    base = R.seeded_input((2, 3, 41, 110), SEED)
    return base[:, :, 2:40, 3:107:2]                    # [2,3,38,52]: odd map sizes (9x13, 4x6, 2x3), neither contiguous nor unit-stride


@functools.lru_cache(maxsize=None)
def trunk_truth(which):
    """(truth, emulation) of the 2_2_2 trunk's three maps: computed once."""
    _, m64 = trunks("2_2_2")
    x = trunk_input(which).double()
    R.check_weights_are_felt(m64, x)
    return H.forward_maps(m64, x), H.forward_maps(m64, x, H.round_f16)


@pytest.mark.parametrize("which", ["plain", "strided"])
def test_trunk_maps(dev, which):
    m32, _ = trunks("2_2_2")
    want, emu = trunk_truth(which)
    fe = device_fe("2_2_2", m32, dev, prec=4)
    assert fe.fe.precision == 4
    x = trunk_input(which)
    xd = x.to(dev) if which == "plain" else R.seeded_input((2, 3, 41, 110), SEED).to(dev)[:, :, 2:40, 3:107:2]
    assert xd.is_contiguous() == (which == "plain")
    with torch.no_grad():
        last, maps = fe(xd)
    assert last is maps[-1] and len(maps) == 3
    figures = []
    for i, (m, r, e) in enumerate(zip(maps, want, emu)):
        assert m.dtype == torch.float32 and tuple(m.shape) == tuple(r.shape)
        figures.append(report(f"trunk 2_2_2 {which} map {i}", m, r, e))
    for err, e in figures:
        assert err <= FACTOR * e and err <= 1e-3, figures


def test_switch(dev):
    """3 after 4 is the default model bit for bit; 4 differs; the training forward ignores the switch."""
    m32, _ = trunks("1_1_1")
    x = R.seeded_input((2, 3, 40, 36), SEED).to(dev)
    with torch.no_grad():
        default = [m.clone() for m in device_fe("1_1_1", m32, dev)(x)[1]]
        fe = device_fe("1_1_1", m32, dev)
        four = [m.clone() for m in fe.fe.set_precision(4).forward_maps(x)]
        back = fe.fe.set_precision(3).forward_maps(x)
        again = [m.clone() for m in fe.fe.set_precision(4).forward_maps(x)]       # both sets of planes stay cached
    for d, f, b, a in zip(default, four, back, again):
        assert torch.equal(b, d) and not torch.equal(f, d) and torch.equal(a, f)
        assert rel_l2(f, d) < 1e-3
    scales = [None, torch.tensor([0.0, 1.0 / 0.9], device=dev), torch.tensor([1.0 / 0.8, 1.0 / 0.8], device=dev)]
    runs = []
    for prec in (3, 4):
        t = device_fe("1_1_1", m32, dev, prec=prec)
        t.fe.enable_training()
        t.train()
        assert t.fe.precision == prec
        runs.append([m.detach().clone() for m in t.fe.forward_maps_train(x, row_scales=scales)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_captured_forward_replays_bit_equal(dev):
    m32, _ = trunks("1_1_1")
    fe = device_fe("1_1_1", m32, dev, prec=4)
    x = R.seeded_input((2, 3, 40, 36), SEED).to(dev)
    with torch.no_grad():
        eager = [m.clone() for m in fe(x)[1]]              # the warm-up: prepares the fp16 planes
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            _, maps = fe(x)
        for m in maps:
            m.zero_()
        graph.replay()
        torch.cuda.synchronize()
    for a, b in zip(maps, eager):
        assert torch.equal(a, b)


# -------------------------------------------------------------------------------------------------------------- models
def u8(shape, seed):
    t = torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    t.view(-1)[0], t.view(-1)[-1] = 0, 255
    return t


def _db(dev, prec):
    from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
    from agplace_amd.options import Options
    opt = Options(dbimage_fe="convnext_tiny", dbimage_fe_layers="1_1_1", features_dim=384, convnext_u8=True, convnext_precision=prec)
    torch.manual_seed(3)
    model = DBVanilla2D("db", 384, opt=opt)
    model.dbimage_fes[0].fe.load_state_dict(R.seeded_trunk([1, 1, 1], SEED, torch.float32).state_dict(), strict=True)
    return model.to(dev).eval(), opt


def test_dbvanilla2d(dev):
    from agplace_amd import ops, pair
    tiles = u8((2, 1, 64, 64, 3), 8).to(dev)
    (m3, opt), (m4, _) = _db(dev, 3), _db(dev, 4)
    with torch.no_grad():
        image = ops.normalize_cameras_u8(tiles, opt.image_mean, opt.image_std).unsqueeze(1)       # [2,1,3,64,64]
        e3 = m3({"db_map": image}, mode="db")["embedding"]
        e4 = m4({"db_map": image}, mode="db")["embedding"]
        e4_u8 = m4({"db_map": tiles}, mode="db")["embedding"]
        with pytest.raises(NotImplementedError, match="embed_pair"):
            pair.embed_pair(None, m4, {}, {"db_map": image})
    err = rel_l2(e4, e3)
    print(f"f16 DBVanilla2D embedding: precision 4 against 3 rel_l2 {err:.3g}")
    assert e4.shape == (2, 384) and err <= 1e-3 and not torch.equal(e4, e3)
    assert torch.equal(e4_u8, e4)


@functools.lru_cache(maxsize=None)
def _mm_state():
    return ref.seeded_params(ref.options("1_1_1"), seed=5, dtype=torch.float32)[0]


def _mm(dev, prec):
    from agplace_amd.network_mm.mm import MM
    m = MM(opt=ref.options("1_1_1", convnext_u8=True, convnext_precision=prec))
    m.load_state_dict(_mm_state(), strict=True)
    return m.to(dev).eval()


def test_mm(dev):
    from agplace_amd import map_exponents, ops
    m3, m4 = _mm(dev, 3), _mm(dev, 4)
    data = {k: v for k, v in to_dev(nets.synth_query(2, 32, 96, ref.options(), seed=9), dev).items() if k != "query_image"}
    tiles = u8((2, 2, 32, 48, 3), 10).to(dev)
    with torch.no_grad():
        image = ops.normalize_cameras_u8(tiles, m3.opt.image_mean, m3.opt.image_std)
        o3 = m3(dict(data, query_image=image), mode="q")
        o4 = m4(dict(data, query_image=image), mode="q")
        o4_u8 = m4(dict(data, query_image=tiles), mode="q")
        blank = m3(dict(data, query_image=image * 0), mode="q")      # which outputs the image reaches at all
        with pytest.raises(NotImplementedError, match="calibrate"):
            map_exponents.calibrate(m4, [])
    felt = [k for k in KEYS if not torch.equal(blank[k], o3[k])]
    assert "imagevec_org" in felt and "embedding" in felt
    for k in KEYS:
        err = rel_l2(o4[k], o3[k])
        print(f"f16 MM {k}: precision 4 against 3 rel_l2 {err:.3g}" + ("" if k in felt else " (the image does not reach it)"))
    for k in KEYS:
        assert rel_l2(o4[k], o3[k]) <= 1e-3, k
        assert torch.equal(o4[k], o3[k]) == (k not in felt), k
        assert torch.equal(o4_u8[k], o4[k]), k


def test_range_guard_with_precision_4_is_refused(dev):
    from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
    from agplace_amd.network.image_fe import ImageFE
    from agplace_amd.network_mm.mm import MM
    from agplace_amd.options import Options
    with pytest.raises(NotImplementedError, match="fp16_range_guard"):
        MM(opt=ref.options("1_1_1", convnext_precision=4, fp16_range_guard=True))
    with pytest.raises(NotImplementedError, match="fp16_range_guard"):
        DBVanilla2D("db", 256, opt=Options(dbimage_fe="convnext_tiny", dbimage_fe_layers="1_1_1", convnext_precision=4, fp16_range_guard=True))
    fe = ImageFE("convnext_tiny", "1_1_1", opt=Options(convnext_precision=4, fp16_range_guard=True)).to(dev).eval()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="fp16_range_guard"):
        fe(torch.zeros(1, 3, 32, 32, device=dev))
    # the guard with precision 3 keeps working as before: nothing to bind, nothing refused
    ok = ImageFE("convnext_tiny", "1_1_1", opt=Options(fp16_range_guard=True)).to(dev).eval()
    with torch.no_grad():
        assert len(ok(torch.zeros(1, 3, 32, 32, device=dev))[1]) == 3
