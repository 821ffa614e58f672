"""The fp16 range guard of the ConvNeXt trunk's precision 4 (Options.convnext_range_guard) on the GPU: the guarded twins of the three
PREC = 4 kernels (csrc/convnext.hip), the weight planes' clamp flag, and the report through ImageFE, DBVanilla2D and MM.

What must be reported comes from the fp64 reference (tests/convnext_guard_ref.py); tests/test_convnext_guard_host.py asserts that
every case used here keeps its saturating place above 2 x 65504 and every other place below 65504 / 4 (the exact-boundary pair and
the replay pair have their own conditions there), so the device's rounding cannot move a decision.  Saturation is a clamp, not a
fault: every forward here returns finite maps.
"""
import copy
import functools

import pytest
import torch

import convnext_guard_ref as G
import convnext_ref as R
import mm_convnext_ref as ref

pytestmark = pytest.mark.gpu

STAGE = {96: 1, 192: 3, 384: 5}          # features index of the stage with C channels
STREAMS = ((1, 5, 7), (2, 8, 8))         # 35 pixels: partial 4x8 tiles, a 3-row MLP tail tile, odd downsample sizes; two images
CNX_TEXT = "ConvNeXt trunk's precision-4 products.*convnext_precision = 3"


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


@functools.lru_cache(maxsize=None)
def full_model():
    return R.randomize_convnext(R.ConvNeXtTiny(), G.SEED).float().eval()


@functools.lru_cache(maxsize=None)
def clean():
    return G.clean_trunk()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


class Bound:
    """A fresh Guard whose word is bound around fn(): .run(fn) -> (fn's result, the word after the work)."""

    def __init__(self, dev):
        from agplace_amd import range_guard
        self.g, self.dev = range_guard.Guard("test"), dev

    def run(self, fn):
        from agplace_amd import range_guard
        torch.cuda.synchronize()
        with self.g.bind(self.dev) as w:
            assert range_guard.bound_word() is w
            w.mul_(0)
            out = fn()
        assert range_guard.bound_word() is None
        torch.cuda.synchronize()
        return out, int(w.item())


def fp16_plane(ws, rows, C):
    return ws[:rows * C * 2].view(torch.float16).view(rows, C)


# ------------------------------------------------------------------------------------------------------------ op level
@pytest.mark.parametrize("nhw", STREAMS)
@pytest.mark.parametrize("C", [96, 192, 384])
def test_dwconv_ln_twin(dev, C, nhw):
    from agplace_amd import convnext as cnx
    n, h, w = nhw
    blk = copy.deepcopy(full_model().features[STAGE[C]][0])
    x = nhwc(R.seeded_input((n, C, h, w), G.SEED + C)).to(dev)
    rows = (n * h * w + 31) // 32 * 32

    def run(block, xs, bound):
        p = cnx.prep_block(copy.deepcopy(block).to(dev), prec=4)
        ws = torch.zeros(cnx.workspace_bytes(n, h, w, C), dtype=torch.uint8, device=dev)
        fn = lambda: cnx.dwconv_ln_fwd(xs, p, ws, prec=4)
        word = Bound(dev).run(fn)[1] if bound else fn()
        return fp16_plane(ws, rows, C).clone(), word

    plain, _ = run(blk, x, False)
    got, word = run(blk, x, True)
    assert word == 0 and torch.equal(got, plain) and float(plain.float().abs().max()) < G.LIMIT / 4
    blk.block[2].weight.data[3] = 1e6                       # one LayerNorm gamma: channel 3 of every pixel leaves fp16's range
    plain, _ = run(blk, x, False)
    got, word = run(blk, x, True)
    assert word == 1 and torch.equal(got, plain) and float(plain.float().abs().max()) == G.LIMIT
    if w % 8:
        # only the OUT-OF-IMAGE positions of the partial tile would saturate: the one tap reads 3 pixels to the left and the image
        # is zero except in column w - 3, so every real pixel's conv is 0 in all channels (LayerNorm output = beta) while the
        # position at column w (computed, never stored) sees a different value per channel
        dw = blk.block[0]
        dw.weight.data.zero_()
        dw.bias.data.zero_()
        dw.weight.data[:, 0, 3, 0] = torch.linspace(-1.0, 1.0, C)
        blk.block[2].weight.data.fill_(1e6)
        xs = torch.zeros_like(x)
        xs[:, :, w - 3, :] = 1.0
        got, word = run(blk, xs, True)
        assert word == 0
        assert torch.equal(got[:n * h * w].float(), blk.block[2].bias.data.half().float().to(dev).expand(n * h * w, C))
        xs[:, :, w - 4, :] = 1.0                            # now the real column w - 1 sees it too
        assert run(blk, xs, True)[1] == 1


@pytest.mark.parametrize("nhw", STREAMS)
@pytest.mark.parametrize("C", [96, 192, 384])
def test_mlp_twin(dev, C, nhw):
    """The fp16 operand plane is written by the test.  Rows P .. P + 31 of the workspace (tile padding of the 3-row tail tile when
    P = 35, beyond every tile when P = 128) hold values that would saturate the hidden map: the kernel must not report them."""
    from agplace_amd import convnext as cnx
    n, h, w = nhw
    P = n * h * w
    rows = (P + 31) // 32 * 32 + 32
    p = cnx.prep_block(copy.deepcopy(full_model().features[STAGE[C]][0]).to(dev), prec=4)
    resid = nhwc(R.seeded_input((n, C, h, w), G.SEED + C + 1)).to(dev)
    base = R.seeded_input((rows, C), G.SEED + C + 2).half()

    def run(plane, bound):
        ws = torch.zeros(rows * C * 2, dtype=torch.uint8, device=dev)
        fp16_plane(ws, rows, C).copy_(plane)
        fn = lambda: cnx.mlp_fwd(ws, p, resid, torch.empty_like(resid), prec=4)
        return Bound(dev).run(fn) if bound else (fn(), None)

    hot = torch.full((C,), 60000.0).half()                  # Linear1 of such a row: some hidden unit far beyond 65504
    padded = base.clone()
    padded[P:P + 32] = hot
    plain, _ = run(padded, False)
    out, word = run(padded, True)
    assert word == 0 and torch.equal(out, plain) and bool(torch.isfinite(out).all())
    assert torch.equal(run(base, True)[0], plain)           # (the rows past P are not read at all)
    last = padded.clone()
    last[P - 1] = hot                                       # the last real row: the tail tile's row (P - 1) % 32
    plain, _ = run(last, False)
    out, word = run(last, True)
    assert word == 1 and torch.equal(out, plain) and bool(torch.isfinite(out).all())
    first = base.clone()
    first[0] = hot
    assert run(first, True)[1] == 1
    # the tail tile's padding rows hold a ZERO operand, so their hidden values are GELU(b1): a unit with b1 = 1e5 whose W1 row
    # brings every real row back to exactly 0 (two weights of -50000 against operand channels that are exactly 1) is beyond
    # fp16's range in the padding rows only, and lanes p0 + r >= P must not report it
    blk = copy.deepcopy(full_model().features[STAGE[C]][0])
    blk.block[3].weight.data[5].zero_()
    blk.block[3].weight.data[5, :2] = -50000.0
    blk.block[3].bias.data[5] = 1e5
    p = cnx.prep_block(blk.to(dev), prec=4)
    ones = base.clone()
    ones[:, :2] = 1.0
    out, word = run(ones, True)
    assert word == 0 and bool(torch.isfinite(out).all())
    blk.block[3].bias.data[5] = 2e5                         # (with b1 = 2e5 every real row sits at 1e5: reported)
    p = cnx.prep_block(blk, prec=4)
    assert run(ones, True)[1] == 1


@pytest.mark.parametrize("nhw", STREAMS)
@pytest.mark.parametrize("C", [96, 192])
def test_downsample_twin(dev, C, nhw):
    from agplace_amd import convnext as cnx
    n, h, w = nhw
    ds = copy.deepcopy(full_model().features[STAGE[C] + 1])
    x = nhwc(R.seeded_input((n, C, h, w), G.SEED + C + 3)).to(dev)

    def run(layer, bound):
        p = cnx.prep_down(*copy.deepcopy(layer).to(dev), prec=4)
        fn = lambda: cnx.downsample_fwd(x, p, prec=4)
        return Bound(dev).run(fn) if bound else (fn(), None)

    plain, _ = run(ds, False)
    out, word = run(ds, True)
    assert word == 0 and torch.equal(out, plain) and tuple(out.shape) == (n, h // 2, w // 2, 2 * C)
    ds[0].weight.data[C - 1] = -1e6
    plain, _ = run(ds, False)
    out, word = run(ds, True)
    assert word == 1 and torch.equal(out, plain) and bool(torch.isfinite(out).all())


# ---------------------------------------------------------------------------------------------------------- model level
def f32_state(m64):
    """The fp64 reference trunk's weights as the fp32 state_dict the device gets (the reference model stays fp64)."""
    return {k: v.detach().float() for k, v in m64.state_dict().items()}


def device_fe(m64, dev, prec=4, **kw):
    from agplace_amd.network.image_fe import ImageFE
    from agplace_amd.options import Options
    fe = ImageFE("convnext_tiny", "1_1_1", opt=Options(convnext_precision=prec, **kw))
    fe.fe.load_state_dict(f32_state(m64), strict=True)
    return fe.to(dev).eval()


def first_call_reports(model, call):
    """A fresh model's first guarded call checks its own batch at once: True if it raised the ConvNeXt report."""
    try:
        call()
    except ValueError as e:
        assert "this batch" in str(e) and "precision-4 products" in str(e) and "convnext_precision = 3" in str(e), str(e)
        assert model.fp16_range_ok()                        # reported once: the word is clean again
        return True
    assert model.fp16_range_ok()
    return False


@pytest.mark.parametrize("value,flag", [(65504.0, False), (65505.0, True)])
def test_exact_boundary_at_the_gelu_site(dev, value, flag):
    x = G.image((2, 3, 32, 32)).to(dev)
    fe = device_fe(G.plant_boundary(clean(), 0, value), dev, convnext_range_guard=True)
    assert first_call_reports(fe, lambda: fe(x)) == flag


@pytest.mark.parametrize("shape", [(2, 3, 32, 32), (1, 3, 36, 44)])
def test_clean_model_does_not_report(dev, shape):
    x = G.image(shape).to(dev)
    fe = device_fe(clean(), dev, convnext_range_guard=True)
    assert not G.expected_flag(G.operand_maxima(clean(), x.cpu()))
    assert not first_call_reports(fe, lambda: fe(x))
    fe(x)
    fe.poll_fp16_range()
    assert fe.fp16_range_ok()


@pytest.mark.parametrize("place,stage", G.CASES)
def test_every_place_and_stage_reports(dev, place, stage):
    for shape in ((2, 3, 32, 32), (1, 3, 36, 44)):
        x = G.image(shape)
        m = G.plant(clean(), place, stage, x)
        assert G.expected_flag(G.operand_maxima(m, x))
        fe = device_fe(m, dev, convnext_range_guard=True)
        xd = x.to(dev)
        assert first_call_reports(fe, lambda: fe(xd)), (place, stage, shape)


@functools.lru_cache(maxsize=None)
def replay_pair(shape):
    """(planted fp64 trunk, good image, bad image): one hidden unit of stage 0 saturates on the bad image only."""
    good, bad = G.image(shape, 11), G.image(shape, 12)
    m, _, ratio = G.replay_case(clean(), good, bad)
    assert ratio >= 1.3
    assert not G.expected_flag(G.operand_maxima(m, good)) and G.expected_flag(G.operand_maxima(m, bad))
    return m, good, bad


def run_sequence(call, model, good, bad, match=CNX_TEXT):
    """The eager contract: a good first batch passes, a bad batch is found by the next call (or by fp16_range_ok()), the word is
    clean after the report and the run goes on."""
    call(good)
    assert model.fp16_range_ok()
    call(bad)                                               # reported one call late ...
    assert not model.fp16_range_ok()                        # ... or by the synchronising check
    with pytest.raises(ValueError, match="the previous batch.*" + match):
        call(good)
    assert model.fp16_range_ok()
    call(good)
    model.poll_fp16_range()
    assert model.fp16_range_ok()


def test_imagefe_eager_contract(dev):
    m, good, bad = replay_pair((1, 3, 32, 32))
    fe = device_fe(m, dev, convnext_range_guard=True)
    run_sequence(lambda t: fe(t), fe, good.to(dev), bad.to(dev))
    # a bad FIRST batch is reported as "this" batch
    fresh = device_fe(m, dev, convnext_range_guard=True)
    xb = bad.to(dev)
    assert first_call_reports(fresh, lambda: fresh(xb))
    # without the switch nothing is bound and nothing is made
    off = device_fe(m, dev)
    off(xb)
    assert "_fp16_guard" not in off.__dict__ and off.fp16_range_ok()


def _db(m64, dev, **kw):
    from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
    from agplace_amd.options import Options
    opt = Options(dbimage_fe="convnext_tiny", dbimage_fe_layers="1_1_1", features_dim=384, convnext_precision=4, **kw)
    torch.manual_seed(3)
    model = DBVanilla2D("db", 384, opt=opt)
    for e in model.dbimage_fes:
        e.fe.load_state_dict(f32_state(m64), strict=True)
    return model.to(dev).eval()


def test_dbvanilla2d_reports_through_the_model(dev):
    m, good, bad = replay_pair((1, 3, 32, 32))
    model = _db(m, dev, convnext_range_guard=True)
    run_sequence(lambda t: model({"db_map": t}, mode="db"), model, good.unsqueeze(1).to(dev), bad.unsqueeze(1).to(dev))
    assert all("_fp16_guard" not in e.__dict__ for e in model.dbimage_fes)       # the trunks bind nothing of their own
    off = _db(m, dev)
    off({"db_map": bad.unsqueeze(1).to(dev)}, mode="db")
    assert "_fp16_guard" not in off.__dict__


@functools.lru_cache(maxsize=None)
def _mm_state():
    return ref.seeded_params(ref.options("1_1_1"), seed=5, dtype=torch.float32)[0]


def _mm(m64, dev, **kw):
    from agplace_amd.network_mm.mm import MM
    model = MM(opt=ref.options("1_1_1", convnext_precision=4, **kw))
    model.load_state_dict(_mm_state(), strict=True)
    model.image_fe.fe.load_state_dict(f32_state(m64), strict=True)
    return model.to(dev).eval()


def _mm_data(dev):
    """One sample's voxel cloud from coords (the image comes from the test)."""
    from oracle import sparse as osparse
    coords, features = osparse.synth_cloud(1, 120, extent=20, seed=3)
    return {"coords": coords.to(dev), "features": features.to(dev)}


def test_mm_with_only_the_new_switch_covers_the_trunk_alone(dev):
    m, good, bad = replay_pair((1, 3, 32, 96))
    model = _mm(m, dev, convnext_range_guard=True)
    data = _mm_data(dev)
    run_sequence(lambda t: model(dict(data, query_image=t), mode="q"), model, good.to(dev), bad.to(dev))
    # the voxel branch saturates (tests/test_gpu_range_guard.py: features x 1e6) and is NOT covered: it follows fp16_range_guard
    hot = dict(data, features=data["features"] * 1e6, query_image=good.to(dev))
    model(hot, mode="q")
    model(hot, mode="q")
    model.poll_fp16_range()
    assert model.fp16_range_ok()
    with pytest.raises(ValueError) as e:
        model(dict(data, query_image=bad.to(dev)), mode="q")
        model(dict(data, query_image=good.to(dev)), mode="q")
    assert "mfma_precision" not in str(e.value) and "precision-4 products" in str(e.value)
    assert model.image_fe.fp16_range_ok() and "_fp16_guard" not in model.image_fe.__dict__


def test_mm_with_both_switches_has_one_word_over_trunk_and_maps(dev):
    m, good, bad = replay_pair((1, 3, 32, 96))
    model = _mm(m, dev, convnext_range_guard=True, fp16_range_guard=True)
    data = _mm_data(dev)
    both = CNX_TEXT + ".*mfma_precision = 3"
    run_sequence(lambda t: model(dict(data, query_image=t), mode="q"), model, good.to(dev), bad.to(dev), match=both)
    # the voxel branch alone: the same word, the same report naming both sources
    call = lambda f: model(dict(data, features=f, query_image=good.to(dev)), mode="q")
    call(data["features"])
    assert model.fp16_range_ok()
    call(data["features"] * 1e6)
    assert not model.fp16_range_ok()
    with pytest.raises(ValueError, match="precision mode 4.*stage 2, the voxel branch"):
        call(data["features"])
    assert model.fp16_range_ok()


def test_clamped_weight_plane_is_reported_by_every_forward(dev):
    x = G.image((2, 3, 32, 32))
    m = G.plant(clean(), 4, 1, x)                           # one element of stage 1's W2
    fe = device_fe(m, dev, convnext_range_guard=True)
    xd = x.to(dev)
    assert first_call_reports(fe, lambda: fe(xd))           # forward 1: reported at once, the word starts again from zero
    fe(xd)                                                  # forward 2: the same cached planes report again
    assert not fe.fp16_range_ok()
    with pytest.raises(ValueError, match="the previous batch.*fp16 weight plane"):
        fe(xd)
    # a reload of in-range weights ends it: new planes, new flag
    fe.fe.load_state_dict(f32_state(clean()), strict=True)
    fe(xd)
    fe(xd)
    assert fe.fp16_range_ok()


# ------------------------------------------------------------------------------------------------------------ same bits
@pytest.mark.parametrize("case", ["clean", "activation", "weight"])
def test_guarded_and_unguarded_forwards_are_the_same_bits(dev, case):
    x = G.image((1, 3, 36, 44))
    m = {"clean": clean, "activation": lambda: G.plant(clean(), 1, 2, x), "weight": lambda: G.plant(clean(), 6, 0, x)}[case]()
    xd = x.to(dev)
    trunk = device_fe(m, dev).fe
    plain = [t.clone() for t in trunk.forward_maps(xd)]
    b = Bound(dev)
    maps, word = b.run(lambda: [t.clone() for t in trunk.forward_maps(xd)])
    assert all(torch.equal(a, p) and bool(torch.isfinite(a).all()) for a, p in zip(maps, plain))
    # the kernels' word: activations only; the weight planes' flag waits in the guard until it publishes
    assert word == int(case == "activation")
    assert len(b.g._pending) == 1
    b.g.publish(dev, "cnx4") if case == "clean" else pytest.raises(ValueError, b.g.publish, dev, "cnx4")


def test_precision_3_ignores_the_switch(dev):
    x = G.image((2, 3, 32, 32))
    m = G.plant(clean(), 3, 0, x)                           # would saturate at precision 4; bf16 pairs have fp32's range
    xd = x.to(dev)
    on, off = device_fe(m, dev, prec=3, convnext_range_guard=True), device_fe(m, dev, prec=3)
    for a, p in zip(on(xd)[1], off(xd)[1]):
        assert torch.equal(a, p)
    assert "_fp16_guard" not in on.__dict__ and on.fp16_range_ok()
    b = Bound(dev)
    maps, word = b.run(lambda: on.fe.forward_maps(xd))
    assert word == 0 and not b.g._pending
    for a, p in zip(maps, off(xd)[1]):
        assert torch.equal(a, p)


# --------------------------------------------------------------------------------------------------------------- replay
def test_captured_forward_reports_on_every_replay(dev):
    m, good, bad = replay_pair((1, 3, 32, 32))
    fe = device_fe(m, dev, convnext_range_guard=True)
    x = good.clone().to(dev)
    eager = [t.clone() for t in fe(x)[1]]                   # the one eager guarded forward: word, mirrors, planes
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, maps = fe(x)
    graph.replay()
    torch.cuda.synchronize()
    fe.poll_fp16_range()
    assert fe.fp16_range_ok() and all(torch.equal(a, e) for a, e in zip(maps, eager))
    x.copy_(bad.to(dev))
    graph.replay()
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="an earlier batch.*" + CNX_TEXT):
        fe.poll_fp16_range()
    x.copy_(good.to(dev))
    graph.replay()
    torch.cuda.synchronize()
    fe.poll_fp16_range()
    assert fe.fp16_range_ok() and all(torch.equal(a, e) for a, e in zip(maps, eager))


def test_first_guarded_forward_inside_a_capture_is_refused(dev):
    fresh = device_fe(clean(), dev, convnext_range_guard=True)
    x = G.image((1, 3, 32, 32)).to(dev)
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="EAGER forward"):
        with torch.cuda.graph(graph):
            fresh(x)
    torch.cuda.synchronize()
