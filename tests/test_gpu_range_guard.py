"""The fp16 range guard (Options.fp16_range_guard, include/agplace_hip.h agp_range_flag_set): every kernel family that stores an
fp16 map reports a clamped value into the bound word, never changes a stored value, and the models report it."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


def _guarded(dev, fn):
    """fn() with a fresh word bound on this thread -> (fn's result, the word after the work)."""
    from agplace_amd import _lib
    lib = _lib.load()
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    prev = lib.agp_range_flag_set(word.data_ptr())
    try:
        out = fn()
    finally:
        lib.agp_range_flag_set(prev)
    torch.cuda.synchronize()
    return out, int(word.item())


def _hi(m):
    return m.hi.clone()


# ----------------------------------------------------------------------------------------------------- kernel families
def test_generic_conv_threshold_and_relu_semantics(dev):
    """1x1 conv (the generic kernel, igemm.hip): outputs of about 6.0e4 leave the word at 0, about 7.0e4 set it; a large NEGATIVE
    value counts without ReLU and does not with the ReLU (it is stored as 0, not clamped)."""
    from agplace_amd import ops
    n, h, w, cin, cout = 2, 8, 8, 64, 128
    x = torch.ones(n, cin, h, w, device=dev)
    xm = ops.pack_f32(x, cin, 1, 4)

    def run(c, relu):
        cw = ops.ConvWeights(torch.full((cout, cin, 1, 1), c / cin, device=dev), None, None, 1, 0)
        out = ops.SplitMap.alloc(n, h, w, cout, 1, 4, dev)
        return _guarded(dev, lambda: (ops.conv2d(xm, cw, out, relu=relu, prec=4), _hi(out))[1])

    (o1, f1), (o2, f2) = run(6.0e4, False), run(7.0e4, False)
    assert f1 == 0 and f2 == 1
    assert abs(float(o1[:, 1:-1, 1:-1].float().max()) - 6.0e4) < 64
    assert float(o2[:, 1:-1, 1:-1].float().max()) == 65504.0
    assert run(-7.0e4, False)[1] == 1
    assert run(-7.0e4, True)[1] == 0
    assert run(7.0e4, True)[1] == 1


def _conv_case(dev, cin, cout, k, stride, prec, big, relu=True, seed=0):
    from agplace_amd import ops
    g = torch.Generator().manual_seed(seed)
    n, h, w = 2, 14, 18
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    scale = (0.5 + torch.rand(cout, generator=g)) * (2.0e5 if big else 1.0)
    shift = 0.3 * torch.randn(cout, generator=g)
    pad = k // 2
    ho, wo = ops.conv_out_size(h, k, stride, pad), ops.conv_out_size(w, k, stride, pad)
    xm = ops.pack_f32(x.to(dev), cin, 1, prec)
    cw = ops.ConvWeights(wt.to(dev), scale.to(dev), shift.to(dev), stride, pad)
    return xm, cw, (n, ho, wo, cout)


# (cin, cout, k, stride, prec): kxr2 (64 channels), kxrw (128), kxr (mode 2's 3x3), the generic kernel in modes 4 and 2
CONV_FAMILIES = {"kxr2": (64, 64, 3, 1, 4), "kxrw": (64, 128, 3, 1, 4), "kxr_f16w2": (64, 128, 3, 1, 2),
                 "generic_1x1": (64, 256, 1, 1, 4), "generic_s2": (64, 128, 3, 2, 4), "generic_f16w2": (128, 128, 1, 1, 2)}


@pytest.mark.parametrize("family", list(CONV_FAMILIES))
def test_conv_families_flag_and_bits(dev, family):
    from agplace_amd import ops
    cin, cout, k, stride, prec = CONV_FAMILIES[family]
    for big in (False, True):
        for relu in (True, False):
            xm, cw, shp = _conv_case(dev, cin, cout, k, stride, prec, big, relu)
            o_plain = ops.SplitMap.alloc(*shp, 1, prec, dev)
            ops.conv2d(xm, cw, o_plain, relu=relu, prec=prec)
            o = ops.SplitMap.alloc(*shp, 1, prec, dev)
            hi, flag = _guarded(dev, lambda: (ops.conv2d(xm, cw, o, relu=relu, prec=prec), _hi(o))[1])
            assert flag == int(big), (family, big, relu)
            assert torch.equal(hi, o_plain.hi)


def test_grouped_3x3_and_stage_entry(dev):
    """The grouped launches: 3x3 stride-1 convs of several trunks (igemm_kxr2 / kxrw) and the stage entry (igemm_s2: 3x3/s2 +
    1x1/s2 downsample in one launch) -- the flag from either output, the same bits either way."""
    from agplace_amd import ops
    for cout in (64, 128):
        for big in (False, True):
            jobs, plain = [], []
            for i in range(2):
                xm, cw, shp = _conv_case(dev, 64, cout, 3, 1, 4, big and i == 1, seed=10 + i)
                jobs.append((xm, cw, ops.SplitMap.alloc(*shp, 1, 4, dev), None, True))
                o = ops.SplitMap.alloc(*shp, 1, 4, dev)
                ops.conv2d(xm, cw, o, relu=True, prec=4)
                plain.append(o)
            outs, flag = _guarded(dev, lambda: ops.conv2d_grouped(jobs, 4))
            assert flag == int(big)
            for a, b in zip(outs, plain):
                assert torch.equal(a.hi, b.hi)
    # stage entry: saturation only in the DOWNSAMPLE (its scale), the 3x3 output in range
    g = torch.Generator().manual_seed(5)
    n, h, w, cin, cout = 2, 16, 20, 64, 128
    x = torch.randn(n, cin, h, w, generator=g)
    xm = ops.pack_f32(x.to(dev), cin, 1, 4)
    for which in ("none", "conv", "down"):
        w3 = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
        w1 = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
        s3 = (0.5 + torch.rand(cout, generator=g)) * (2e5 if which == "conv" else 1.0)
        s1 = (0.5 + torch.rand(cout, generator=g)) * (2e5 if which == "down" else 1.0)
        c3 = ops.ConvWeights(w3.to(dev), s3.to(dev), torch.zeros(cout, device=dev), 2, 1)
        c1 = ops.ConvWeights(w1.to(dev), s1.to(dev), torch.zeros(cout, device=dev), 2, 0)
        ho, wo = ops.conv_out_size(h, 3, 2, 1), ops.conv_out_size(w, 3, 2, 1)

        def jobs():
            return [(xm, c3, ops.SplitMap.alloc(n, ho, wo, cout, 1, 4, dev), None, True),
                    (xm, c1, ops.SplitMap.alloc(n, ho, wo, cout, 1, 4, dev), None, False)]
        plain = ops.conv2d_grouped(jobs(), 4)
        outs, flag = _guarded(dev, lambda: ops.conv2d_grouped(jobs(), 4))
        assert flag == int(which != "none"), which
        for a, b in zip(outs, plain):
            assert torch.equal(a.hi, b.hi)


@pytest.mark.parametrize("prec", [4, 2])
def test_stem_families(dev, prec):
    """The fused stem + max-pool (stem_walk.hip in mode 4, igemm_d16.hip's pooled kernel in mode 2), the unpooled packed stem conv
    (igemm_d16.hip), and the stem reading an fp32 image itself (its conversion of the image to fp16 is guarded too)."""
    from agplace_amd import ops
    g = torch.Generator().manual_seed(21)
    n, h, w = 2, 64, 96
    x = torch.randn(n, 3, h, w, generator=g)
    wt = torch.randn(64, 3, 7, 7, generator=g) / 147 ** 0.5
    h1, w1 = ops.conv_out_size(h, 7, 2, 3), ops.conv_out_size(w, 7, 2, 3)
    h2, w2 = ops.conv_out_size(h1, 3, 2, 1), ops.conv_out_size(w1, 3, 2, 1)
    xm = ops.pack_f32(x.to(dev), 4, 3, prec)
    for big in (False, True):
        scale = (0.5 + torch.rand(64, generator=g)) * (2e5 if big else 1.0)
        cw = ops.ConvWeights(wt.to(dev), scale.to(dev), (0.3 * torch.randn(64, generator=g)).to(dev), 2, 3, stem=True)
        ref = ops.stem_pool(xm, cw, ops.SplitMap.alloc(n, h2, w2, 64, 1, prec, dev), prec=prec)
        out = ops.SplitMap.alloc(n, h2, w2, 64, 1, prec, dev)
        hi, flag = _guarded(dev, lambda: (ops.stem_pool(xm, cw, out, prec=prec), _hi(out))[1])
        assert flag == int(big) and torch.equal(hi, ref.hi)
        ref = ops.SplitMap.alloc(n, h1, w1, 64, 1, prec, dev)
        ops.conv2d(xm, cw, ref, relu=True, prec=prec)
        out = ops.SplitMap.alloc(n, h1, w1, 64, 1, prec, dev)
        hi, flag = _guarded(dev, lambda: (ops.conv2d(xm, cw, out, relu=True, prec=prec), _hi(out))[1])
        assert flag == int(big) and torch.equal(hi, ref.hi)
    if prec == 4:
        cw = ops.ConvWeights(wt.to(dev), (0.5 + torch.rand(64, generator=g)).to(dev), torch.zeros(64, device=dev), 2, 3, stem=True)
        for amp in (1.0, 1e5):      # an image beyond fp16's range saturates in the stem's own conversion of it
            xi = (x * amp).to(dev)
            assert ops.stem_walk_reads(xi)
            ref = ops.stem_pool_raw(xi, cw, ops.SplitMap.alloc(n, h2, w2, 64, 1, 4, dev), mean=(0., 0., 0.), std=(1., 1., 1.))
            out = ops.SplitMap.alloc(n, h2, w2, 64, 1, 4, dev)
            hi, flag = _guarded(dev, lambda: (ops.stem_pool_raw(xi, cw, out, mean=(0., 0., 0.), std=(1., 1., 1.)), _hi(out))[1])
            assert flag == int(amp > 1) and torch.equal(hi, ref.hi)


@pytest.mark.parametrize("exact", [True, False])
def test_fused_basicblock_intermediate_saturation(dev, exact):
    """fblock64.hip, both forms: the block's INTERMEDIATE map (converted to fp16 in LDS, never stored) saturates while the
    block's output stays in range -- the flag is set; ordinary scales leave it at 0; the same output bits either way."""
    from agplace_amd import ops
    g = torch.Generator().manual_seed(3)
    n, h, w = 2, 28, 36
    x = torch.relu(torch.randn(n, 64, h, w, generator=g))
    xm = ops.pack_f32(x.to(dev), 64, 1, 4)
    ws = [torch.randn(64, 64, 3, 3, generator=g) / (64 * 9) ** 0.5 for _ in range(2)]
    for case in ("ordinary", "intermediate"):
        s1 = (0.5 + torch.rand(64, generator=g)) * (2e5 if case == "intermediate" else 1.0)
        s2 = (0.5 + torch.rand(64, generator=g)) * (1e-6 if case == "intermediate" else 1.0)
        cws = [ops.ConvWeights(ws[0].to(dev), s1.to(dev), torch.zeros(64, device=dev), 1, 1),
               ops.ConvWeights(ws[1].to(dev), s2.to(dev), torch.zeros(64, device=dev), 1, 1)]
        assert ops.bblock64_ok(xm, cws[0], cws[1], 4)
        ref = ops.bblock64_grouped([(xm, cws[0], cws[1], ops.SplitMap.alloc(n, h, w, 64, 1, 4, dev))], exact=exact)[0]
        out = ops.SplitMap.alloc(n, h, w, 64, 1, 4, dev)
        res, flag = _guarded(dev, lambda: ops.bblock64_grouped([(xm, cws[0], cws[1], out)], exact=exact)[0])
        assert torch.equal(res.hi, ref.hi)
        assert float(res.hi.float().abs().max()) < 1e3        # the block's OUTPUT is in range
        assert flag == int(case == "intermediate"), case


# ----------------------------------------------------------------------------------------------------- models
def _flag_probe(monkeypatch):
    """Records agp_range_flag_get() inside every trunk forward (resnet.ResNet.forward_maps and the lock-step trunks)."""
    from agplace_amd import _lib, resnet
    seen = []
    orig = resnet.ResNet.forward_maps

    def probe(self, *a, **k):
        seen.append(_lib.load().agp_range_flag_get())
        return orig(self, *a, **k)
    monkeypatch.setattr(resnet.ResNet, "forward_maps", probe)
    return seen


def _run_model_sequence(call, model, good, bad):
    """The reporting contract: a normal batch passes, a saturating batch is found by the next call (or fp16_range_ok()), the
    run goes on clean afterwards."""
    call(good)
    assert model.fp16_range_ok()
    call(bad)                                         # reported one call late (eager), ...
    assert not model.fp16_range_ok()                  # ... or by the synchronising check
    with pytest.raises(ValueError, match="fp16's range.*mfma_precision = 3"):
        call(good)
    assert model.fp16_range_ok()                      # reported once: the word starts again from zero
    call(good)
    model.poll_fp16_range()
    assert model.fp16_range_ok()


@pytest.mark.parametrize("prec", [4, 2])
def test_imagefe_reports(dev, prec, monkeypatch):
    from agplace_amd.network_mm.image_fe import ImageFE
    from agplace_amd.options import Options
    seen = _flag_probe(monkeypatch)
    torch.manual_seed(2)
    fe = ImageFE("resnet18", "2_2_2", opt=Options(fp16_range_guard=True)).to(dev).eval()
    x = torch.randn(2, 3, 64, 96, device=dev)
    _run_model_sequence(lambda t: fe(t, prec=prec), fe, x, x * 3.0e4)
    assert seen and all(s is not None for s in seen)
    # the same model in mode 3, and a model with the guard off, never bind
    seen.clear()
    fe(x * 3.0e4, prec=3)
    ImageFE("resnet18", "2_2_2").to(dev).eval()(x, prec=prec)
    assert seen and all(s is None for s in seen)


def test_dbvanilla2d_resnet50_reports(dev, monkeypatch):
    from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
    from agplace_amd.options import Options
    seen = _flag_probe(monkeypatch)
    opt = Options(dbimage_fe="resnet50", dbimage_fe_layers="3_4_6", fp16_range_guard=True)
    torch.manual_seed(4)
    mdb = DBVanilla2D("db", opt.features_dim, opt=opt).to(dev).eval()
    tiles = torch.randn(2, 1, 1, 3, 64, 64, device=dev)              # 6-D: [b, ndb, nmap, 3, h, w]
    _run_model_sequence(lambda t: mdb({"db_map": t}, mode="db"), mdb, tiles, tiles * 3.0e4)
    assert seen and all(s is not None for s in seen)
    seen.clear()
    m3 = DBVanilla2D("db", opt.features_dim, opt=opt.copy(mfma_precision=3)).to(dev).eval()
    m3({"db_map": tiles * 3.0e4}, mode="db")
    assert seen and all(s is None for s in seen) and m3.fp16_range_ok()


def _query(dev, opt, seed=1):
    from oracle import nets
    from oracle import sparse as osparse
    data = nets.synth_query(2, 64, 192, opt, seed=seed)
    d = {k: v for k, v in data.items() if k not in ("vox_levels", "voxfeatvec", "stg2voxvec", "voxvec_fuse")}
    d["coords"], d["features"] = osparse.synth_cloud(2, 120, extent=20, seed=3)
    return {k: v.to(dev) for k, v in d.items()}


def test_mm_forward_q_from_coords_reports(dev, monkeypatch):
    from agplace_amd.network_mm.mm import MM
    from agplace_amd.options import Options
    seen = _flag_probe(monkeypatch)
    opt = Options(fp16_range_guard=True)
    torch.manual_seed(0)
    model = MM(opt=opt).to(dev).eval()
    d = _query(dev, opt)

    def call(img):
        model({**d, "query_image": img}, mode="q")
    _run_model_sequence(call, model, d["query_image"], d["query_image"] * 3.0e4)
    assert seen and all(s is not None for s in seen)
    assert model.voxel_coords_in_range()
    seen.clear()
    off = MM(opt=Options()).to(dev).eval()
    off(d, mode="q")
    assert seen and all(s is None for s in seen)


def test_captured_pair_replays_report(dev):
    from agplace_amd import pair
    from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
    from agplace_amd.network_mm.mm import MM
    from agplace_amd.options import Options
    opt = Options(fp16_range_guard=True)
    torch.manual_seed(0)
    mq = MM(opt=opt).to(dev).eval()
    mdb = DBVanilla2D("db", opt.features_dim, opt=opt).to(dev).eval()
    from oracle import nets
    from gpu_util import to_dev
    full = to_dev(nets.synth_query(2, 64, 192, opt, seed=1), dev)
    tiles = {"db_map": torch.randn(2, 1, 3, 64, 64, device=dev)}
    good = full["query_image"].clone()
    cp = pair.CapturedPair(mq, mdb, full, tiles, poll_every=1)
    for _ in range(3):
        cp.replay()
    cp.finish()
    ref = {k: v.clone() for k, v in cp.out_q.items()}
    full["query_image"].copy_(good * 3.0e4)                # one saturating replay ...
    cp.replay()
    full["query_image"].copy_(good)                        # ... then normal inputs again
    with pytest.raises(ValueError, match="fp16's range"):
        for _ in range(4):
            cp.replay()
            torch.cuda.synchronize()                       # (lets the mirror land; a live loop sees it a replay or two later)
    cp.replay()
    cp.finish()                                            # reported once, the run goes on
    for k in ref:
        assert torch.equal(ref[k], cp.out_q[k]), k
    full["query_image"].copy_(good * 3.0e4)
    cp.replay()
    with pytest.raises(ValueError, match="fp16's range"):
        cp.finish()                                        # the last replay of a loop: finish() finds it


def test_capture_needs_one_eager_forward_first(dev):
    """The word and the mirrors are made outside any capture: torch.cuda.graph on its own capture stream works after one eager
    forward and raises a clear RuntimeError without it."""
    from agplace_amd.network_mm.image_fe import ImageFE
    from agplace_amd.options import Options
    torch.manual_seed(2)
    x = torch.randn(1, 3, 64, 96, device=dev)
    fe = ImageFE("resnet18", "2_2_2", opt=Options(fp16_range_guard=True)).to(dev).eval()
    fe(x, prec=4)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y, _ = fe(x, prec=4)
    g.replay()
    torch.cuda.synchronize()
    assert fe.fp16_range_ok()
    x.mul_(3.0e4)
    g.replay()
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="fp16's range"):
        fe.poll_fp16_range()
    fresh = ImageFE("resnet18", "2_2_2", opt=Options(fp16_range_guard=True)).to(dev).eval()
    g2 = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="EAGER forward"):
        with torch.cuda.graph(g2):
            fresh(x, prec=4)
    torch.cuda.synchronize()


def test_photograph_like_inputs_are_clean(dev):
    """No false positives: the full-size photograph-like query of test_gpu_models.py (checkpoint-like statistics) reports clean."""
    import test_gpu_models as tm
    from agplace_amd.network_mm.mm import MM
    from agplace_amd.options import Options
    from oracle import nets
    from gpu_util import to_dev
    opt = Options(mfma_precision=4, fp16_range_guard=True)
    torch.manual_seed(77)
    model = MM(opt=opt).to(dev)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.momentum = 1.0
    model.train()
    dc = to_dev(nets.synth_query(4, 224, 1344, opt, seed=5), dev)
    dc["query_image"] = tm._image_like_tiles(4, 6, 224, 224, seed=6).to(dev)
    model(dc, mode="q")
    model.eval()
    d2 = to_dev(nets.synth_query(2, 224, 1344, opt, seed=7), dev)
    d2["query_image"] = tm._image_like_tiles(2, 6, 224, 224, seed=8).to(dev)
    model(d2, mode="q")
    model(d2, mode="q")
    assert model.fp16_range_ok()


# ----------------------------------------------------------------------------------------------------- voxel branch and map writers
def _cloud(dev, nb=2, npts=3000, seed=3):
    g = torch.Generator().manual_seed(seed)
    rows = [torch.cat([torch.full((npts, 1), float(b)), torch.randint(-30, 30, (npts, 3), generator=g).float()], 1) for b in range(nb)]
    coords = torch.cat(rows, 0)
    return coords, torch.randn((coords.shape[0], 1), generator=g)


def test_sparse_gather_gemm_and_seg_affine(dev):
    """The voxel branch's gather-GEMM (agp_sparse_conv_fwd: the generic kernel's gather configurations) and agp_seg_affine_fwd
    (the residual output of every voxel block): large weights / scales set the flag, ordinary ones do not, same bits either way."""
    from agplace_amd.sparse import SparseTensor
    from agplace_amd.sparse.modules import MinkowskiConvolution, seg_affine
    coords, _ = _cloud(dev)
    sp = SparseTensor.from_coords(torch.ones((coords.shape[0], 1), device=dev), coords.to(dev), nbatch=2)
    g = torch.Generator().manual_seed(4)
    x = sp.with_feats(torch.randn((sp.n + 1, 64), generator=g).half().to(dev))
    x.hi[sp.n].zero_()
    for cout in (64, 128):
        for big in (False, True):
            torch.manual_seed(cout)
            conv = MinkowskiConvolution(64, cout, kernel_size=3).to(dev)
            if big:
                conv.kernel.data.mul_(1e6)
            for relu in (False, True):
                plain = conv(x, None, relu=relu, prec=4).hi[:sp.n].clone()
                hi, flag = _guarded(dev, lambda: conv(x, None, relu=relu, prec=4).hi[:sp.n].clone())
                assert flag == int(big), (cout, big, relu)
                assert torch.equal(hi, plain)
    res = sp.with_feats(torch.randn((sp.n + 1, 64), generator=g).half().to(dev))
    for big in (False, True):
        scale = (0.5 + torch.rand(2, 64, generator=g)).to(dev) * (2e5 if big else 1.0)
        for r in (None, res):
            plain = seg_affine(x, scale=scale, residual=r, relu=True).hi[:sp.n].clone()
            hi, flag = _guarded(dev, lambda: seg_affine(x, scale=scale, residual=r, relu=True).hi[:sp.n].clone())
            assert flag == int(big) and torch.equal(hi, plain)
    # a residual SUM of two in-range maps that leaves the range: 4.0e4 + 4.0e4
    y = sp.with_feats(torch.full((sp.n + 1, 64), 4.0e4, device=dev).half())
    assert _guarded(dev, lambda: seg_affine(y, residual=y, relu=True))[1] == 1
    assert _guarded(dev, lambda: seg_affine(y, residual=None, relu=True))[1] == 0


@pytest.mark.parametrize("mode", ["capacity", "exact"])
def test_sparse_first_conv(dev, mode):
    """The first voxel conv (1 input channel): agp_sparse_conv0_fwd in capacity mode (the inference path from coords; its fp16
    form converts the voxel features into an fp16 tile, guarded too) and agp_sparse_conv_cin1_fwd in exact mode."""
    from agplace_amd import ops
    from agplace_amd.sparse import SparseTensor
    from agplace_amd.sparse.modules import MinkowskiConvolution
    coords, feats = _cloud(dev, seed=5)
    torch.manual_seed(6)
    conv = MinkowskiConvolution(1, 32, kernel_size=5).to(dev)
    for amp in (1.0, 1e8):
        f = (feats * amp).to(dev)

        def run():
            sp = (SparseTensor.from_coords_capacity(f, coords.to(dev), 2, ops.Workspace()) if mode == "capacity"
                  else SparseTensor.from_coords(f, coords.to(dev), nbatch=2))
            n = int(sp.n_dev.item()) if sp.n_dev is not None else sp.n
            return conv(sp, None, relu=True, prec=4).hi[:n].clone()
        plain = run()
        hi, flag = _guarded(dev, run)
        assert flag == int(amp > 1), (mode, amp)
        assert torch.equal(hi, plain)


@pytest.mark.parametrize("cout", [32, 64])
def test_sparse_first_conv_search_form(dev, cout):
    """agp_sparse_conv0_fwd's other route (conv0_search_kernel: every precision but AGP_PREC_F16; mode 2 stores fp16): 40 voxels
    too far apart to be neighbours and unit weights, so a voxel's output is its own feature.  One feature of 70000 sets the word,
    60000 leaves it at 0, and the stored bits are the same with and without the binding."""
    from agplace_amd import ops
    from agplace_amd.sparse import SparseTensor
    from agplace_amd.sparse.modules import MinkowskiConvolution
    ij = torch.arange(20)
    coords = torch.cat([torch.stack([torch.full((20,), float(b)), 8.0 * (ij % 5), 8.0 * (ij // 5), torch.zeros(20)], 1) for b in range(2)], 0)
    conv = MinkowskiConvolution(1, cout, kernel_size=5).to(dev)
    conv.kernel.data.fill_(1.0)
    for planted in (60000.0, 70000.0):
        f = torch.ones(40, 1)
        f[17] = planted

        def run():
            sp = SparseTensor.from_coords_capacity(f.to(dev), coords.to(dev), 2, ops.Workspace())
            return conv(sp, None, relu=True, prec=2).hi[:int(sp.n_dev.item())].clone()
        plain = run()
        hi, flag = _guarded(dev, run)
        assert flag == int(planted > 65504.0), (cout, planted)
        assert torch.equal(hi, plain)
        assert float(hi.float().max()) == min(planted, 65504.0) and float(hi.float().min()) == 1.0


def test_bcast_add_and_input_packs(dev):
    """agp_bcast_add_fwd (the image branch's stage-2 fusion map) and the fp32 input packs (agp_pack_f32_to_nhwc: the 4-channel
    stem form and the generic form; agp_pack_f32_to_nhwc4_h16 of the fast training stem)."""
    from agplace_amd import ops
    g = torch.Generator().manual_seed(8)
    n, h, w, c = 2, 10, 12, 64
    xm = ops.pack_f32(torch.randn(n, c, h, w, generator=g).to(dev), c, 1, 4)
    for big in (False, True):
        vec = (torch.randn(n, c, generator=g) * (1e5 if big else 1.0)).to(dev)
        plain = ops.bcast_add(xm, vec, ops.SplitMap.alloc(n, h, w, c, 1, 4, dev)).hi.clone()
        out, flag = _guarded(dev, lambda: ops.bcast_add(xm, vec, ops.SplitMap.alloc(n, h, w, c, 1, 4, dev)))
        assert flag == int(big) and torch.equal(out.hi, plain)
    for amp in (1.0, 1e5):
        for cin, cpad, hw in ((3, 4, (16, 32)), (64, 64, (9, 11)), (3, 4, (15, 17))):     # NCHW4 fast path, generic, unaligned
            x = (torch.randn(2, cin, *hw, generator=g) * amp).to(dev)
            plain = ops.pack_f32(x, cpad, 1, 4).hi.clone()
            out, flag = _guarded(dev, lambda: ops.pack_f32(x, cpad, 1, 4))
            assert flag == int(amp > 1), (cin, amp)
            assert torch.equal(out.hi, plain)
        x = (torch.randn(2, 3, 16, 32, generator=g) * amp).to(dev)
        from agplace_amd import _lib

        def pack_h16():
            hi = torch.zeros(2, 18, 34, 4, dtype=torch.int16, device=dev)
            h16 = torch.zeros_like(hi)
            sn, sc, sh, sw = x.stride()
            _lib.check(_lib.load().agp_pack_f32_to_nhwc4_h16(x.data_ptr(), sn, sc, sh, sw, 2, 3, 16, 32, 1, hi.data_ptr(), None,
                                                             h16.data_ptr(), _lib.stream()), "agp_pack_f32_to_nhwc4_h16")
            return h16
        plain = pack_h16()
        h16, flag = _guarded(dev, pack_h16)
        assert flag == int(amp > 1) and torch.equal(h16, plain)


def test_mm_voxel_branch_alone_reports(dev):
    """MM.forward_q from coords where ONLY the voxel features leave fp16's range (the image is ordinary): reported."""
    from agplace_amd.network_mm.mm import MM
    from agplace_amd.options import Options
    opt = Options(fp16_range_guard=True)
    torch.manual_seed(0)
    model = MM(opt=opt).to(dev).eval()
    d = _query(dev, opt)

    def call(f):
        model({**d, "features": f}, mode="q")
    _run_model_sequence(call, model, d["features"], d["features"] * 1e6)
    assert model.voxel_coords_in_range()


def test_paired_trunks_report_through_the_query_model(dev):
    """pair.embed_pair: the lock-step trunks hold BOTH models' images; with only the query model guarded, a saturated database tile
    is reported by the query model, and the message names the database trunks as a possible source."""
    from agplace_amd import pair
    from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
    from agplace_amd.network_mm.mm import MM
    from agplace_amd.options import Options
    from gpu_util import to_dev
    from oracle import nets
    torch.manual_seed(0)
    mq = MM(opt=Options(fp16_range_guard=True)).to(dev).eval()
    mdb = DBVanilla2D("db", 256, opt=Options()).to(dev).eval()
    q = to_dev(nets.synth_query(2, 64, 192, mq.opt, seed=1), dev)
    tiles = torch.randn(2, 1, 3, 64, 64, device=dev)
    assert pair.can_pair(mq, mdb, q, {"db_map": tiles})
    pair.embed_pair(mq, mdb, q, {"db_map": tiles})
    assert mq.fp16_range_ok()
    pair.embed_pair(mq, mdb, q, {"db_map": tiles * 3.0e4})
    assert not mq.fp16_range_ok()
    with pytest.raises(ValueError, match="DBVanilla2D image trunks"):
        pair.embed_pair(mq, mdb, q, {"db_map": tiles})
    pair.embed_pair(mq, mdb, q, {"db_map": tiles})
    assert mq.fp16_range_ok() and mdb.fp16_range_ok()
