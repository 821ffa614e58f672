"""-m gpu tests of MM's opt-in training on the ConvNeXt-tiny trunk (Options.convnext_train): the two bridge kernels of
csrc/pool.hip (agp_bcast_add_f32_fwd, agp_pool_f32_bwd) and the model end to end against the fp64 reference of
tests/mm_convnext_train_ref.py.

Kernel bounds.  agp_bcast_add_f32_fwd is held bit for bit.  agp_pool_f32_bwd: rel_l2 of `out` against fp64 autograd (plus the
base's exact hi + lo) and the relative error of gp[0] = dL/dp, each case printing its figure; the asserted bounds are 4 x the
worst value measured on an MI355X (the margin tests/test_gpu_convnext_bwd.py uses for box-to-box order), never above the project's
data-gradient ceiling 1e-4, and 1e-3 for gp.  At one pixel per plane ([1,1,1,96]) GeM is max(x, eps) whatever p is, so dL/dp is
analytically zero: there the error of gp[0] is taken relative to the sum the kernel subtracts, sum |ggem y ln(y) / p|.
MEASURED (MI355X, worst over the shapes and term sets below):
  out  rel_l2          2.34e-07  ([1,1,1,96], ggem alone; with a base 3.3e-08, gmean alone 3.9e-08)
  gp   relative error  4.25e-08  ([2,4,6,384]; [1,1,1,96]: 2.3e-08 of the subtracted sum)
so the asserted bounds are 9.4e-07 and 1.7e-07.  The sums have a fixed order, so the figures repeat from run to run.

End to end: the project's tight rule (tests/test_gpu_train.py: _compare_grads) on every parameter gradient, outputs within
OUT_BARS; min_checked is counted from the reference's own non-zero gradients, so a silently missing gradient fails.
"""
import functools

import pytest
import torch

import mm_convnext_ref as ref
import mm_convnext_train_ref as tref
from oracle import nets
from gpu_util import cpu_state, randomize_bn, rel_l2, to_dev
from test_gpu_mm_convnext import _cloud
from test_gpu_train import OUT_BARS, _compare_grads, _fast_path_census, _unit_mask

pytestmark = pytest.mark.gpu

B, H, W = 2, 64, 96
LAYERS = "1_1_1"
KEYS = ("imagevec_org", "voxvec_org", "shallowvec_org", "stg2fusevec", "stg2imagevec", "stg2voxvec", "embedding")
LOSS_KEYS = ("embedding", "stg2imagevec", "imagevec_org", "stg2fusevec")
DATA_CEILING, GP_CEILING = 1e-4, 1e-3
# worst figures measured on an MI355X over test_pool_f32_bwd_matches_fp64_autograd's cases
MEASURED_OUT, MEASURED_GP = 2.34e-7, 4.25e-8


def _bound(measured, ceiling):
    return min(4 * measured, ceiling)


# ----------------------------------------------------------------------------------------------- kernel: bcast_add_f32
def _poisoned_map(dev, n, h, w, c, pad=1, guard=4096):
    """A split-bf16 map carved out of the middle of two buffers filled with the poison value -3: (SplitMap, hi buffer, lo buffer,
    guard)."""
    from agplace_amd import ops
    numel = n * (h + 2 * pad) * (w + 2 * pad) * c
    bufs = [torch.full((guard + numel + guard,), -3.0, dtype=torch.bfloat16, device=dev) for _ in range(2)]
    hi, lo = (b[guard:guard + numel].view(n, h + 2 * pad, w + 2 * pad, c) for b in bufs)
    return ops.SplitMap(hi, lo, n, h, w, c, pad), bufs[0], bufs[1], guard


@pytest.mark.parametrize("n,h,w,c", [(1, 1, 1, 64), (2, 4, 6, 384), (3, 5, 7, 192)])
def test_bcast_add_f32_is_bit_equal_and_leaves_the_halo_alone(dev, n, h, w, c):
    from agplace_amd import ops
    g = torch.Generator().manual_seed(n * 1000 + c)
    x = torch.randn(n, h, w, c, generator=g).to(dev)
    v = torch.randn(n, c, generator=g).to(dev)
    m, bhi, blo, guard = _poisoned_map(dev, n, h, w, c)
    ops.bcast_add_f32(x, v, m)
    s = x + v[:, None, None, :]
    hi = s.bfloat16()
    lo = (s - hi.float()).bfloat16()
    for name, plane, want, buf in (("hi", m.hi, hi, bhi), ("lo", m.lo, lo, blo)):
        assert torch.equal(plane[:, 1:-1, 1:-1].view(torch.int16), want.view(torch.int16)), name
        rest = plane.clone()
        rest[:, 1:-1, 1:-1] = -3.0
        assert bool((rest == -3.0).all()), f"{name}: halo written"
        assert bool((buf[:guard] == -3.0).all()) and bool((buf[-guard:] == -3.0).all()), f"{name}: memory around the map written"


def test_bcast_add_f32_refuses_96_channels_and_writes_nothing(dev):
    from agplace_amd import _lib
    n, h, w, c = 2, 3, 5, 96
    x, v = torch.randn(n, h, w, c, device=dev), torch.randn(n, c, device=dev)
    m, bhi, blo, _ = _poisoned_map(dev, n, h, w, c)
    L = _lib.load()
    rc = L.agp_bcast_add_f32_fwd(x.data_ptr(), v.data_ptr(), n, h, w, c, m.hi.data_ptr(), m.lo.data_ptr(), 1, _lib.stream())
    torch.cuda.synchronize()
    assert rc == _lib.E_UNSUPPORTED
    assert bool((bhi == -3.0).all()) and bool((blo == -3.0).all())
    assert L.agp_bcast_add_f32_fwd(None, v.data_ptr(), n, h, w, 64, m.hi.data_ptr(), m.lo.data_ptr(), 1, _lib.stream()) == 1
    assert L.agp_bcast_add_f32_fwd(x.data_ptr(), v.data_ptr(), n, 0, w, 64, m.hi.data_ptr(), m.lo.data_ptr(), 1, _lib.stream()) == 1


# ------------------------------------------------------------------------------------------------ kernel: pool_f32_bwd
POOL_SHAPES = [(1, 1, 1, 96), (2, 4, 6, 384), (3, 5, 7, 192), (1, 33, 47, 96)]
POOL_TERMS = [("gmean",), ("ggem",), ("gmean", "ggem"), ("gmean", "ggem", "base")]
P_GEM = 2.7


@functools.lru_cache(maxsize=None)
def _pool_case(n, h, w, c):
    """CPU inputs of one shape and the fp64 truths of each term, computed once and never modified."""
    g = torch.Generator().manual_seed(h * 100 + c)
    x = (0.7 * torch.randn(n, h, w, c, generator=g) + 0.3)
    gmean, ggem = torch.randn(n, c, generator=g), torch.randn(n, c, generator=g)
    base = torch.randn(n, h, w, c, generator=g)
    bhi = base.bfloat16()
    blo = (base - bhi.float()).bfloat16()
    x64 = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    p64 = torch.tensor([P_GEM], dtype=torch.float64, requires_grad=True)
    gx_mean, = torch.autograd.grad((x64.mean((2, 3)) * gmean.double()).sum(), x64)
    y64 = nets.gem(x64, p64).flatten(1)
    gx_gem, gp_gem = torch.autograd.grad((y64 * ggem.double()).sum(), [x64, p64])
    yd = y64.detach()
    sub = float((ggem.double() * yd * yd.log() / P_GEM).abs().sum())
    return dict(x=x, gmean=gmean, ggem=ggem, bhi=bhi, blo=blo, base64=bhi.double() + blo.double(),
                gx_mean=gx_mean.permute(0, 2, 3, 1), gx_gem=gx_gem.permute(0, 2, 3, 1), gp=float(gp_gem), sub=sub)


def _run_pool_bwd(dev, case, terms, gp=None):
    from agplace_amd import ops
    x = case["x"].to(dev)
    n, h, w, c = x.shape
    p = torch.tensor([P_GEM], device=dev)
    kw = {}
    if "gmean" in terms:
        kw["gmean"] = case["gmean"].to(dev)
    if "ggem" in terms:
        _, y = ops.pool_f32(x.permute(0, 3, 1, 2), p, want_mean=False, want_gem=True)
        kw.update(ggem=case["ggem"].to(dev), gem_y=y, p=p, gp=gp)
    if "base" in terms:
        m = ops.SplitMap.alloc(n, h, w, c, 1, 3, dev)
        m.hi[:, 1:-1, 1:-1] = case["bhi"].to(dev)
        m.lo[:, 1:-1, 1:-1] = case["blo"].to(dev)
        kw["base"] = m
    return ops.pool_f32_bwd(x, **kw)


@pytest.mark.parametrize("terms", POOL_TERMS, ids=["+".join(t) for t in POOL_TERMS])
@pytest.mark.parametrize("n,h,w,c", POOL_SHAPES)
def test_pool_f32_bwd_matches_fp64_autograd(dev, n, h, w, c, terms):
    from agplace_amd import ops
    case = _pool_case(n, h, w, c)
    gp = ops.new_gp(dev) if "ggem" in terms else None
    out = _run_pool_bwd(dev, case, terms, gp)
    want = sum(case[k] for k, t in (("gx_mean", "gmean"), ("gx_gem", "ggem"), ("base64", "base")) if t in terms)
    assert out.shape == (n, h, w, c) and out.dtype == torch.float32 and out.is_contiguous()
    err = rel_l2(out, want)
    print(f"pool_f32_bwd [{n},{h},{w},{c}] {'+'.join(terms)}: out rel_l2 {err:.3e} (bound {_bound(MEASURED_OUT, DATA_CEILING):.3e})")
    gerr = None
    if gp is not None:
        got = float(gp[0])
        gerr = abs(got - case["gp"]) / (case["sub"] if h * w == 1 else abs(case["gp"]))
        print(f"pool_f32_bwd [{n},{h},{w},{c}] {'+'.join(terms)}: gp {got:.6e} want {case['gp']:.6e} relative error {gerr:.3e} "
              f"(bound {_bound(MEASURED_GP, GP_CEILING):.3e})")
    assert err <= _bound(MEASURED_OUT, DATA_CEILING), err
    if gerr is not None:
        assert gerr <= _bound(MEASURED_GP, GP_CEILING), gerr


def test_pool_f32_bwd_repeats_bit_for_bit_and_leaves_gp_ready(dev):
    """Two calls give the same bits (out and dL/dp), the second into the SAME gp buffer: its ticket was left at zero, so
    gp[0] is exactly twice one call's value."""
    from agplace_amd import _lib, ops
    case = _pool_case(1, 33, 47, 96)
    terms = ("gmean", "ggem", "base")
    gp1, gp2 = ops.new_gp(dev), ops.new_gp(dev)
    a = _run_pool_bwd(dev, case, terms, gp1)
    b = _run_pool_bwd(dev, case, terms, gp2)
    assert torch.equal(a, b) and torch.equal(gp1[:1], gp2[:1]) and float(gp1[0]) != 0
    assert int(gp1[_lib.GP_FLOATS - 1:].view(torch.int32)) == 0          # the arrival ticket
    c = _run_pool_bwd(dev, case, terms, gp1)
    assert torch.equal(a, c) and float(gp1[0]) == 2 * float(gp2[0])


@pytest.mark.parametrize("n,h,w,c", POOL_SHAPES)
def test_pool_f32_bwd_with_base_alone_is_exact(dev, n, h, w, c):
    case = _pool_case(n, h, w, c)
    out = _run_pool_bwd(dev, case, ("base",))
    assert torch.equal(out.cpu().double(), case["base64"])


def test_pool_f32_bwd_refuses_an_empty_request(dev):
    from agplace_amd import _lib
    x, out = torch.randn(1, 2, 2, 96, device=dev), torch.empty(1, 2, 2, 96, device=dev)
    L = _lib.load()
    assert L.agp_pool_f32_bwd(x.data_ptr(), None, None, None, None, 1e-6, None, None, 0, 1, 2, 2, 96, out.data_ptr(), None,
                              _lib.stream()) == 1


# ----------------------------------------------------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def _state():
    """The seeded fp32 state (trunk weights under which every block is felt), BatchNorm randomised; shared, never modified."""
    from agplace_amd.network_mm.mm import MM
    p32, _ = ref.seeded_params(ref.options(LAYERS), seed=5, dtype=torch.float32)
    m = MM(opt=ref.options(LAYERS))
    m.load_state_dict(p32, strict=True)
    return {k: v.clone() for k, v in randomize_bn(m).state_dict().items()}


@functools.lru_cache(maxsize=None)
def _data():
    return nets.synth_query(B, H, W, ref.options(), seed=9)


@functools.lru_cache(maxsize=None)
def _cloud_data():
    d = {"query_image": _data()["query_image"]}
    d["coords"], d["features"] = _cloud(21)
    return d


@functools.lru_cache(maxsize=None)
def _cotangents():
    g = torch.Generator().manual_seed(2)
    return {k: torch.randn(B, 384, generator=g) for k in LOSS_KEYS + ("stg2voxvec", "voxvec_org")}


def _model(dev, training, **kw):
    from agplace_amd.network_mm.mm import MM
    m = MM(opt=ref.options(LAYERS, convnext_train=True, **kw))
    m.load_state_dict(_state(), strict=True)
    return m.to(dev).train(training)


def _loss(out, keys, double=False):
    G = _cotangents()
    return sum((out[k] * (G[k].double() if double else G[k].to(out[k].device))).sum() for k in keys)


def _reference(model, learn_mixing=False):
    """(params, trunk, scales): the model's state in fp64 as gradient leaves (mixing weights only on request), the adopted fp64
    trunk, and the stochastic-depth scales the last forward applied."""
    params = {k: (v.double() if v.is_floating_point() else v) for k, v in cpu_state(model).items()}
    for k, v in params.items():
        if v.is_floating_point() and "running_" not in k and (learn_mixing or not k.endswith("_weight")):
            v.requires_grad_(True)
    trunk = tref.adopt_trunk(params, LAYERS.split("_"))
    drawn = model.image_fe.fe.last_row_scales
    scales = None if drawn is None else [None if s is None else s.double().cpu() for s in drawn]
    return params, trunk, scales


def _fmask(sp):
    return ((sp.hi[:sp.n].float() + sp.lo[:sp.n].float()) > 0).float().cpu()


def _pattern(model, sparse_vox):
    u1, u2 = model.stg2fuseblock.ffnsimg[0]._units
    pat = {"stg2fuseblock.ffnsimg.0.relu1": _unit_mask(u1), "stg2fuseblock.ffnsimg.0.relu2": _unit_mask(u2)}
    if sparse_vox:
        tr = model.vox_fe._train_obj
        pat["vox_fe.relu0"] = _fmask(tr.u0.saved[3])
        for i in range(3):
            pat[f"vox_fe.relus.{i}"] = _fmask(tr.down[i].saved[3])
            pat[f"vox_fe.blocks.{i}.0.relu1"] = _fmask(tr.blocks[i][0].u1.saved[3])
            pat[f"vox_fe.blocks.{i}.0.relu2"] = _fmask(tr.blocks[i][0].saved[5])
        bt = model.stg2fuseblock.ffnsvox[0]._train_obj
        pat["stg2fuseblock.ffnsvox.0.relu1"] = _fmask(bt.u1.saved[3])
        pat["stg2fuseblock.ffnsvox.0.relu2"] = _fmask(bt.saved[5])
    return pat


MUST = ("image_fe.fe.features.0.0.weight", "image_fe.fe.features.5.0.block.3.weight", "image_pool.p", "stg2fuseblock.poolimage.p",
        "stg2fuseblock.ffnsimg.0.conv1.weight", "stg2fuseblock.projsfuseimg.0.0.weight",
        "fuseblocktoshallow.blocks.0.blocks.0.func.func.fc.weight", "stg2fusefc.weight")
SKIP = ("image_fe.fe.classifier.",)


def _end_to_end(dev, training, sparse_vox, mode="tight", frozen_trunk=False, **kw):
    model = _model(dev, training, **kw)
    if frozen_trunk:
        model.image_fe.requires_grad_(False)
    data = _cloud_data() if sparse_vox else _data()
    keys = LOSS_KEYS + (("stg2voxvec", "voxvec_org") if sparse_vox else ())
    bn = model.stg2fuseblock.ffnsimg[0].bn1
    before = bn.running_mean.clone()
    out = model(to_dev(data, dev), mode="q")
    _loss(out, keys).backward()
    assert torch.equal(before, bn.running_mean) != training             # running statistics move in .train() only
    params, trunk, scales = _reference(model)
    assert training == any(s is not None for s in scales)
    pattern = _pattern(model, sparse_vox)
    d64 = ref.cast(data, torch.float64)
    gen = torch.Generator().manual_seed(3)
    noise = 1 + 1e-5 * torch.randn(d64["query_image"].shape, generator=gen, dtype=torch.float64)
    fnoise = 1 + 1e-5 * torch.randn(d64["features"].shape, generator=gen, dtype=torch.float64) if sparse_vox else None

    def run_oracle(pert):
        d = dict(d64)
        if pert:
            d["query_image"] = d64["query_image"] * noise
            if sparse_vox:
                d["features"] = d64["features"] * fnoise
        return _loss(tref.forward_q(d, params, model.opt, trunk, scales, training, pattern), keys, double=True)

    with torch.no_grad():
        free = tref.forward_q(d64, params, model.opt, trunk, scales, training, None)
    for k in KEYS:
        print(f"mm_convnext_train [{mode} train={training} sparse={sparse_vox}] {k}: rel_l2 {rel_l2(out[k], free[k]):.3e}")
    for k in keys:
        assert rel_l2(out[k], free[k]) < OUT_BARS[mode], (k, rel_l2(out[k], free[k]))
    # every tensor the reference gives a non-zero gradient must be compared: count them from the reference itself
    for v in params.values():
        v.grad = None
    run_oracle(False).backward()
    live = [n for n, p in model.named_parameters() if p.requires_grad and not n.startswith(SKIP) and params[n].grad is not None
            and float(params[n].grad.abs().max()) != 0 and not (training and n.endswith(("conv1.bias", "conv2.bias")))]
    must = MUST + (("vox_fe.blocks.2.0.conv2.kernel",) if sparse_vox else ())
    if frozen_trunk:
        must = tuple(m for m in must if not m.startswith("image_fe."))
        assert all(p.grad is None for p in model.image_fe.parameters())
    assert not [m for m in must if m not in live], [m for m in must if m not in live]
    print(f"mm_convnext_train [{mode} train={training} sparse={sparse_vox}]: {len(live)} parameter tensors with a gradient")
    _compare_grads(model, params, run_oracle, noise, min_checked=len(live), skip=SKIP, must=must, batch_stats=training, mode=mode)
    return model


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_training_gradients_with_dense_stand_ins(dev, training):
    _end_to_end(dev, training, sparse_vox=False)


def test_training_gradients_from_coords(dev):
    _end_to_end(dev, True, sparse_vox=True)


def test_frozen_trunk_under_trainable_exponents(dev):
    """image_fe frozen by hand (not freeze_backbone): the training graph still runs, the trunk gets no gradient, and the GeM
    exponent's comes from ops.pool_f32_bwd alone."""
    _end_to_end(dev, False, sparse_vox=False, frozen_trunk=True)


def test_fast_modes_act_on_the_stage_2_block(dev):
    model = _end_to_end(dev, True, sparse_vox=False, mode="dgrad1", train_precision=16, train_dgrad_products=1)
    _fast_path_census("dgrad1", blocks=[("stg2fuseblock.ffnsimg.0", model.stg2fuseblock.ffnsimg[0])])


def test_two_steps_from_one_state_are_bit_equal(dev):
    data = to_dev(_data(), dev)
    grads = []
    for _ in range(2):
        model = _model(dev, True)
        torch.cuda.manual_seed(77)
        _loss(model(data, mode="q"), LOSS_KEYS).backward()
        grads.append({n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
    assert set(grads[0]) == set(grads[1]) and len(grads[0]) > 60
    assert any(n.startswith("image_fe.fe.features.") for n in grads[0]) and "image_pool.p" in grads[0]
    diff = [n for n in grads[0] if not torch.equal(grads[0][n], grads[1][n])]
    assert not diff, diff[:8]


def test_train_mode_under_no_grad_saves_nothing(dev):
    model = _model(dev, True)
    with torch.no_grad():
        out = model(to_dev(_data(), dev), mode="q")
    assert all(out[k].grad_fn is None and not out[k].requires_grad for k in KEYS)
    params, trunk, scales = _reference(model)
    assert any(s is not None for s in scales)
    with torch.no_grad():
        want = tref.forward_q(ref.cast(_data(), torch.float64), params, model.opt, trunk, scales, True, None)
    for k in KEYS:
        assert rel_l2(out[k], want[k]) < OUT_BARS["tight"], (k, rel_l2(out[k], want[k]))


def test_frozen_backbone_trains_the_fusion_path_on_constant_maps(dev, monkeypatch):
    """freeze_backbone().eval() with gradients: the existing non-train per-op path, the trunk's maps constants; mixing weights,
    stg2fusefc and an FCODE weight against fp64 autograd at the 2e-4 of the any-width route (tests/test_gpu_fcode_wide.py)."""
    import oracle.nets as onets
    learn = dict(shallow_learnweight=True, shalloworg_learnweight=True, stg2imagevox_learnweight=True, imagevoxorg_learnweight=True)
    model = _model(dev, False, **learn).freeze_backbone().eval()
    out = model(to_dev(_data(), dev), mode="q")
    assert model.image_fe.fe.last_row_scales is None                       # the training forward did not run
    _loss(out, LOSS_KEYS).backward()
    params, trunk, _ = _reference(model, learn_mixing=True)
    # the oracle cuts the path the product cuts: the stage-2 conv block sees a detached input (tests/test_gpu_models.py)
    orig = onets.basic_block_conv
    monkeypatch.setattr(onets, "basic_block_conv", lambda x, p_, pre, training=False, pattern=None: orig(x.detach(), p_, pre, training, pattern))
    _loss(tref.forward_q(ref.cast(_data(), torch.float64), params, model.opt, trunk), LOSS_KEYS, double=True).backward()
    got = dict(model.named_parameters())
    watch = ["shallow_weight", "shalloworg_weight", "stg2image_weight", "imageorg_weight", "stg2fusefc.weight", "stg2fusefc.bias",
             "fuseblocktoshallow.blocks.1.blocks.0.func.func.fc.weight"]
    for k in watch:
        assert got[k].grad is not None and params[k].grad is not None and float(params[k].grad.abs().max()) > 0, k
        err = rel_l2(got[k].grad, params[k].grad.reshape(got[k].grad.shape))
        print(f"mm_convnext_train frozen {k}: rel_l2 {err:.3e}")
        assert err < 2e-4, (k, err)
    assert all(p.grad is None for n, p in got.items() if n.startswith(("image_fe.", "stg2fuseblock.ffnsimg.")))


def test_switch_leaves_inference_untouched(dev):
    from agplace_amd.network_mm.mm import MM
    data = to_dev(_data(), dev)
    on = _model(dev, False)
    off = MM(opt=ref.options(LAYERS))
    off.load_state_dict(_state(), strict=True)
    off = off.to(dev).eval()
    with torch.no_grad():
        a, b = on(data, mode="q"), off(data, mode="q")
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
