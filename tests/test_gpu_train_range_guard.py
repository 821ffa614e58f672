"""The training range guard (Options.train_range_guard): the two training map kernels that convert to fp16 (agp_map_affine,
agp_affine_maxpool3x3s2_fwd) report a clamped value into the bound word and store the same bits either way; the trunk, MM and
DBVanilla2D report a saturated training forward through poll_fp16_range() in both train_precision modes, eager and replayed; the
inference guard is what it was."""
import pytest
import torch

pytestmark = pytest.mark.gpu

F16_MAX = 65504.0
BEYOND = float(torch.nextafter(torch.tensor(F16_MAX), torch.tensor(float("inf"))))       # 65504.00390625: the next fp32
INF, NAN = float("inf"), float("nan")
# name -> (value one known element takes, reported without a ReLU, reported with the ReLU folded in)
SPECIALS = {"none": (None, False, False), "max": (F16_MAX, False, False), "beyond": (BEYOND, True, True),
            "neg": (-7.0e4, True, False), "inf": (INF, True, True), "nan": (NAN, False, False)}
LAYOUTS = ("pair+h16", "f16", "pair")        # split pair plus the operand plane | ONE fp16 plane | split pair only (never tracked)


def _bound(dev, fn, preset=0):
    """fn() with a word holding `preset` bound on this thread -> (fn's result, the word after the work)."""
    from agplace_amd import _lib
    lib = _lib.load()
    word = torch.full((1,), preset, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    prev = lib.agp_range_flag_set(word.data_ptr())
    try:
        out = fn()
    finally:
        lib.agp_range_flag_set(prev)
    torch.cuda.synchronize()
    return out, int(word.item())


def _bits(t):
    return None if t is None else t.view(torch.int16).clone()


def _same_bits(a, b):
    return all((p is None and q is None) or torch.equal(p, q) for p, q in zip(a, b))


def _special_input(dev, c, h, w, py, px, name, a_prec):
    """A map of ones with a 2 at (py, px) of channel c - 3 and per-channel (scale, shift) that put exactly SPECIALS[name] on that
    element (+-inf / NaN: on the whole channel) and small values everywhere else.  Returns (map, scale, shift, channel)."""
    from agplace_amd import ops
    ch = c - 3
    x = torch.ones(1, c, h, w)
    x[0, ch, py, px] = 2.0
    scale = 0.25 * (1.0 + (torch.arange(c) % 5).float())
    shift = 0.125 * (torch.arange(c) % 3).float()
    v = SPECIALS[name][0]
    if v is not None:
        scale[ch], shift[ch] = (v if v != v or abs(v) == INF else v / 2.0), 0.0
        if abs(v) < INF:
            assert float(torch.tensor(2.0) * scale[ch]) == v             # fp32, exact: the element IS the special value
    return ops.pack_f32(x.to(dev), c, 1, a_prec), scale.to(dev), shift.to(dev), ch


def _out_map(dev, n, h, w, c, layout):
    from agplace_amd import ops
    o = ops.SplitMap.alloc(n, h, w, c, 1, 4 if layout == "f16" else 3, dev)
    for t in (o.hi, o.lo):
        if t is not None:
            t[:, 1:-1, 1:-1].zero_()
    return o.with_h16() if layout == "pair+h16" else o


# c = 24: three channel groups do not divide the grid stride -- affine_kernel's generic path; 64 / 128: its two-items-per-trip path
@pytest.mark.parametrize("c", [64, 128, 24])
def test_map_affine_reports_exactly_the_clamped_fp16_stores(dev, c):
    from agplace_amd import train_graph
    h, w, py, px = 5, 7, 2, 3
    for layout in LAYOUTS:
        for relu in (0, 1):
            for name, (val, rep_plain, rep_relu) in SPECIALS.items():
                # (the fast mode's y16 is written from a z that is ONE fp16 plane; the pairs from a pair)
                a, scale, shift, ch = _special_input(dev, c, h, w, py, px, name, 4 if layout == "f16" else 3)
                res = None
                if layout == "pair+h16" and relu:                        # a block's conv2: a (zero) residual pair rides along
                    from agplace_amd import ops
                    res = ops.pack_f32(torch.zeros(1, c, h, w, device=dev), c, 1, 3)

                def run():
                    o = _out_map(dev, 1, h, w, c, layout)
                    train_graph.map_affine(a, scale, shift, o, residual=res, relu=bool(relu))
                    return o
                plain = run()
                torch.cuda.synchronize()
                expect = int(layout != "pair" and (rep_relu if relu else rep_plain))
                for preset in ((0, 2) if name == "beyond" else (0,)):
                    o, word = _bound(dev, run, preset)
                    assert word == (preset | expect), (c, layout, relu, name, preset, word)      # only ever ORed into
                    assert _same_bits([_bits(t) for t in (o.hi, o.lo, o.h16)], [_bits(t) for t in (plain.hi, plain.lo, plain.h16)]), \
                        (c, layout, relu, name)
                f16 = {"pair+h16": plain.h16, "f16": plain.hi, "pair": None}[layout]
                if f16 is not None and name not in ("none", "nan"):      # the stored value: clamped, the ReLU first
                    got = float(f16[0, 1 + py, 1 + px, ch])
                    want = 0.0 if (relu and val < 0) else max(-F16_MAX, min(F16_MAX, val))
                    assert got == want, (c, layout, relu, name, got)


def test_affine_maxpool_reports_exactly_the_clamped_fp16_stores(dev):
    """z [1, 9, 11, 64] (odd sizes: the special element sits in the last row and column, inside the edge window only)."""
    from agplace_amd import train_graph
    c, h, w = 64, 9, 11
    ho, wo = 5, 6
    for layout in LAYOUTS:
        for name, (val, _, rep_relu) in SPECIALS.items():
            z, scale, shift, ch = _special_input(dev, c, h, w, h - 1, w - 1, name, 3)

            def run():
                o = _out_map(dev, 1, ho, wo, c, layout)
                am = torch.zeros(1, ho, wo, c, dtype=torch.uint8, device=dev)
                train_graph.affine_maxpool(z, scale, shift, o, am)
                return o, am
            plain, am0 = run()
            torch.cuda.synchronize()
            expect = int(layout != "pair" and rep_relu)                   # (the ReLU is part of the kernel)
            for preset in ((0, 2) if name == "beyond" else (0,)):
                (o, am), word = _bound(dev, run, preset)
                assert word == (preset | expect), (layout, name, preset, word)
                assert _same_bits([_bits(t) for t in (o.hi, o.lo, o.h16)], [_bits(t) for t in (plain.hi, plain.lo, plain.h16)]), (layout, name)
                assert torch.equal(am, am0), (layout, name)
            f16 = {"pair+h16": plain.h16, "f16": plain.hi, "pair": None}[layout]
            if f16 is not None and name not in ("none", "nan"):
                got = float(f16[0, ho, wo, ch])                           # the last window (halo 1): it alone sees the element
                want = 0.0 if val < 0 else min(F16_MAX, val)              # (a negative channel pools to the ReLU's zero)
                assert got == want, (layout, name, got, want)


# ----------------------------------------------------------------------------------------------------------- trunk level
MODES = {"fast": dict(train_precision=16), "tight": dict()}


def _trunk(dev, mode, seed=11, **extra):
    from agplace_amd.network_mm.image_fe import ImageFE
    from agplace_amd.options import Options
    torch.manual_seed(seed)
    return ImageFE("resnet18", "2_2_2", opt=Options(train_range_guard=True, **MODES[mode], **extra)).to(dev).train()


def _trunk_step(fe, x, gmeans, zero=True):
    """One training step of the op-level trunk: forward on the training graph, loss = <mean(map), G>, backward.  Returns the
    loss as a device tensor (no synchronisation: the step is capturable)."""
    from agplace_amd import ops, train_graph
    if zero:
        for p in fe.parameters():
            p.grad = None
    maps = fe.forward_maps_train(x)
    loss, grads = 0, []
    for m, g in zip(maps, gmeans):
        loss = loss + (ops.pool_map(m, None, want_mean=True, want_gem=False)[0] * g).sum()
        gm = ops.SplitMap.alloc(m.n, m.h, m.w, m.c, 1, 3, m.hi.device)
        train_graph.pool_bwd(m, gm, gmean=g)
        grads.append(gm)
    fe.fe.backward_maps(grads)
    return loss


def _gmeans(dev, n=2):
    g = torch.Generator().manual_seed(1)
    return [torch.randn(n, c, generator=g).to(dev) for c in (64, 128, 256)]


def _clean(model):
    torch.cuda.synchronize()
    model.poll_fp16_range()
    return model.fp16_range_ok()


@pytest.mark.parametrize("mode", list(MODES))
def test_trunk_training_forward_reports(dev, mode):
    """(a) a hot conv1 weight: the fast mode's z16 saturates while BatchNorm renormalises y; (b) a hot BatchNorm gamma: conv1's
    output saturates -- the fast mode's y16 plane, the tight mode's fp16 operand plane of conv2's weight gradient."""
    import torch.nn.functional as F
    fe = _trunk(dev, mode)
    x, G = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(12)).to(dev), _gmeans(dev)
    assert torch.isfinite(_trunk_step(fe, x, G)).item()
    assert _clean(fe)
    grads = [p.grad for p in fe.parameters() if p.grad is not None]
    assert len(grads) > 40 and all(torch.isfinite(g).all() for g in grads)
    blk = fe.fe.layer1[0]
    unit = lambda: fe.fe._units["t.l0.0.c0"]                              # conv1 + bn1 of that block
    cases = [("b", blk.bn1.weight)] + ([("a", blk.conv1.weight)] if mode == "fast" else [])
    for case, prm in cases:
        keep = prm.detach().clone()
        with torch.no_grad():
            prm.mul_(1.0e6)
        loss = _trunk_step(fe, x, G)
        torch.cuda.synchronize()
        assert torch.isfinite(loss).item(), case
        xin, z, y, mean, rstd = unit().saved[:5]
        if case == "a":
            # fp32 on the host: the conv's true output leaves fp16's range; what the step stored is the clamped plane
            z32 = F.conv2d(xin.to_f32().cpu().contiguous(), prm.detach().cpu(), padding=1)
            assert float(z32.abs().max()) > F16_MAX
            assert z.lo is None and float(z.hi[:, 1:-1, 1:-1].float().abs().max()) == F16_MAX
        else:
            cv = lambda t: t.detach().float().cpu().view(1, -1, 1, 1)
            y32 = torch.relu((z.to_f32().cpu() - cv(mean)) * cv(rstd) * cv(blk.bn1.weight) + cv(blk.bn1.bias))
            assert float(y32.max()) > F16_MAX
            plane = y.hi if mode == "fast" else y.h16                     # y16 | the operand plane beside the bf16 pair
            assert (y.lo is None) == (mode == "fast") and plane is not None
            assert float(plane[:, 1:-1, 1:-1].float().max()) == F16_MAX
        with pytest.raises(ValueError, match=r"^ImageFE: .*a training forward \(Options.train_precision = " + ("16" if mode == "fast" else "32")):
            fe.poll_fp16_range()
        with torch.no_grad():
            prm.copy_(keep)
        assert torch.isfinite(_trunk_step(fe, x, G)).item()              # reported once (the report resets): a clean step polls clean
        assert _clean(fe), case


# ------------------------------------------------------------------------------------------------------------------ models
def _mm_case(dev, opt):
    from agplace_amd.network_mm.mm import MM
    from gpu_util import to_dev
    from oracle import nets
    torch.manual_seed(21)
    m = MM(opt=opt).to(dev).train()
    data = to_dev(nets.synth_query(2, 64, 96, opt, seed=1), dev)           # dense stand-ins for the voxel branch

    def step():
        out = m(data, mode="q")
        loss = out["embedding"].sum() + out["stg2imagevec"].sum()
        loss.backward()
        return loss
    return m, step, m.stg2fuseblock.ffnsimg[0].bn1.weight


def _db_case(dev, opt):
    from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
    torch.manual_seed(22)
    m = DBVanilla2D("db", opt.features_dim, opt=opt).to(dev).train()
    tiles = {"db_map": torch.randn(1, 2, 1, 3, 64, 64, generator=torch.Generator().manual_seed(23)).to(dev)}

    def step():
        loss = m(tiles, mode="db")["embedding"].sum()
        loss.backward()
        return loss
    return m, step, m.dbimage_fes[0].fe.layer1[0].bn1.weight


@pytest.mark.parametrize("which", ["MM", "DBVanilla2D"])
def test_models_report_a_saturated_training_forward(dev, which):
    from agplace_amd.options import Options
    case = _mm_case if which == "MM" else _db_case
    model, step, gamma = case(dev, Options(train_precision=16, train_range_guard=True))
    assert torch.isfinite(step()).item()
    assert _clean(model)
    keep = gamma.detach().clone()
    with torch.no_grad():
        gamma.mul_(1.0e6)                                                # a hot stage-2 (MM) / trunk (DBVanilla2D) BatchNorm gamma
    loss = step()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).item()
    with pytest.raises(ValueError, match="^" + which + r": .*a training forward"):
        model.poll_fp16_range()
    with torch.no_grad():
        gamma.copy_(keep)
    assert torch.isfinite(step()).item()
    assert _clean(model)
    # the same model without the option never raises, hot or not, and owns no guard
    off, step_off, gamma_off = case(dev, Options(train_precision=16))
    step_off()
    with torch.no_grad():
        gamma_off.mul_(1.0e6)
    for _ in range(2):
        assert torch.isfinite(step_off()).item()
        torch.cuda.synchronize()
        off.poll_fp16_range()
        assert off.fp16_range_ok()
    assert "_fp16_guard" not in off.__dict__


# ----------------------------------------------------------------------------------------------------------------- capture
def test_captured_training_step_replays_publish_their_own_state(dev):
    fe = _trunk(dev, "fast")
    x = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(12)).to(dev)
    xs, G = x.clone(), _gmeans(dev)
    _trunk_step(fe, xs, G)                                               # the word and the mirrors are made by an EAGER step
    assert _clean(fe)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss = _trunk_step(fe, xs, G, zero=False)
    g.replay()
    assert _clean(fe) and torch.isfinite(loss).item()
    xs.copy_(x * 1.0e6)                                                  # hot: the stem input's fp16 operand plane saturates
    g.replay()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).item()
    with pytest.raises(ValueError, match="^ImageFE: .*a training forward"):
        fe.poll_fp16_range()
    xs.copy_(x)
    g.replay()
    assert _clean(fe)
    # a FIRST guarded training forward inside a capture: the existing RuntimeError
    fresh = _trunk(dev, "fast", seed=13)
    g2 = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="EAGER forward"):
        with torch.cuda.graph(g2):
            fresh.forward_maps_train(xs)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- the inference guard
def test_inference_guard_is_untouched_by_training_forwards(dev):
    """Two expectations of tests/test_gpu_range_guard.py on a model that also trains with the training guard: the eager reporting
    sequence of an inference forward (one call late / fp16_range_ok(), reported once, clean afterwards) and the bound-only-when-
    active rule (mode 3 never reports), before and after guarded training forwards on the same model's one Guard."""
    fe = _trunk(dev, "fast", fp16_range_guard=True)
    x, G = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(12)).to(dev), _gmeans(dev)

    def inference_sequence():
        fe.eval()
        with torch.no_grad():
            fe(x, prec=4)
            assert fe.fp16_range_ok()
            fe(x * 3.0e4, prec=4)                                        # reported one call late (eager), ...
            assert not fe.fp16_range_ok()                                # ... or by the synchronising check
            with pytest.raises(ValueError, match="fp16's range.*mfma_precision = 3"):
                fe(x, prec=4)
            assert fe.fp16_range_ok()                                    # reported once: the word starts again from zero
            fe(x * 3.0e4, prec=3)                                        # mode 3 stores no fp16 map and never binds
            fe(x, prec=4)
            fe.poll_fp16_range()
            assert fe.fp16_range_ok()
        fe.train()
    inference_sequence()
    for _ in range(2):
        assert torch.isfinite(_trunk_step(fe, x, G)).item()
    assert _clean(fe)
    inference_sequence()
    assert torch.isfinite(_trunk_step(fe, x, G)).item()
    assert _clean(fe)
