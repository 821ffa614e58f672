"""-m gpu: the stage entry without a stored downsample map -- igemm_kxrw's residual COMPUTED from a second operand stream (the 1x1 /
stride-2 downsample inside the block's second conv, ops.conv2d_grouped2), igemm_s2 without its downsample part
(ops.conv2d_s2_nods) and the trunks' route through both (resnet.FUSE_DOWNSAMPLE).

Reference: fp64 from the UNROUNDED fp32 operands, relu(s2 * conv3x3(h) + t2 + s_d * conv1x1/s2(x) + t_d).  Bar: conv_sched_util
BARS[4] = 6e-4 on the whole map and on the worst 64 x 128 raster block (the project's bar of precision mode 4; the storage
roundings of the fused form measure 3.5e-4 to 3.6e-4 against fp64 in a CPU emulation of these shapes).  Trunk level, switch on
against switch off: 1e-3, the model tests' bar, on every stage map (the two forms differ by the fp16 rounding of the downsample map
and of one more sum, some 4e-4 per entry block)."""
import pytest
import torch
import torch.nn.functional as F

from conv_sched_util import (BARS, WIDE_CASES, assert_only_the_interior_was_written, guarded_map, images, regime, weights,
                             worst_block)
from gpu_util import randomize_bn, rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


def _signs(v, seed):
    """A few channels negative, a few zero (a BatchNorm gamma may be either)."""
    v = v.clone()
    idx = torch.randperm(v.numel(), generator=torch.Generator().manual_seed(seed))
    v[idx[:5]] *= -1
    v[idx[5:8]] = 0
    return v


def _block(cin2, cmid, cout, hin, win, n, seed, first=0):
    """The operands of a block's second conv with its downsample, on the CPU: x (stage input, cin2 x hin x win), h (conv2's input,
    cmid x hout x wout), both convs' weights and folded BatchNorm constants."""
    ho, wo = (hin - 1) // 2 + 1, (win - 1) // 2 + 1
    w2, s2, t2 = weights(cmid, cout, seed)
    wd, sd, td = weights(cin2, cout, seed + 1, k=1)
    return dict(x=images(cin2, hin, win, n, seed + 2, first), h=images(cmid, ho, wo, n, seed + 3, first), w2=w2, s2=_signs(s2, seed),
                t2=t2, wd=wd, sd=_signs(sd, seed + 1), td=td, ho=ho, wo=wo, cout=cout)


def _ref64(q, lo=0, hi=None):
    x, h = q["x"][lo:hi].double(), q["h"][lo:hi].double()
    y = F.conv2d(h, q["w2"].double(), None, 1, 1) * q["s2"].double().view(1, -1, 1, 1) + q["t2"].double().view(1, -1, 1, 1)
    d = F.conv2d(x, q["wd"].double(), None, 2, 0) * q["sd"].double().view(1, -1, 1, 1) + q["td"].double().view(1, -1, 1, 1)
    return torch.relu(y + d)


def _device_block(q, dev):
    """(conv2 with the summed shift, the folded downsample stream, the packed maps) of a block on the device."""
    from agplace_amd import ops
    cw = ops.ConvWeights(q["w2"].to(dev), q["s2"].to(dev), (q["t2"] + q["td"]).to(dev), 1, 1)
    sw = ops.Stream2Weights(q["wd"].to(dev), q["sd"].to(dev), q["td"].to(dev))
    assert sw.fusable
    xm = ops.pack_f32(q["x"].to(dev), q["x"].shape[1], 1, 4)
    hm = ops.pack_f32(q["h"].to(dev), q["h"].shape[1], 1, 4)
    return cw, sw, xm, hm


def _fused_job(q, dev, lo=0, hi=None, out=None):
    from agplace_amd import ops
    cw, sw, xm, hm = q["dev"] if "dev" in q else _device_block(q, dev)
    hi = xm.n if hi is None else hi
    if out is None:
        out = ops.SplitMap.alloc(hi - lo, q["ho"], q["wo"], q["cout"], 1, 4, dev)
    return (ops.slice_map(hm, lo, hi), cw, out, None, True, (ops.slice_map(xm, lo, hi), sw))


def _parity(what, got, ref):
    assert bool(torch.isfinite(got).all()), what
    whole = rel_l2(got, ref)
    worst, where = worst_block(got, ref, bm=256, cols=128)
    print("%s: whole map %.3g worst block %.3g (bar %.3g) at %s" % (what, whole, worst, BARS[4], where))
    assert whole < BARS[4] and worst < BARS[4], (what, whole, worst, where)


# (cin2, conv2's cin, cout, hin, win): one chunk, two, four; 96 -> 128 has 9 macro-steps: the other X-buffer parity
SMALL = {"64_128_13x27": (64, 128, 128, 13, 27), "128_256_9x11": (128, 256, 256, 9, 11), "32_128_8x10": (32, 128, 128, 8, 10),
         "odd_steps_96_128_cin2_32": (32, 96, 128, 8, 10)}


@pytest.mark.parametrize("case", list(SMALL))
def test_fused_conv2_all_half(dev, case):
    from agplace_amd import ops
    cin2, cmid, cout, hin, win = SMALL[case]
    n = 3
    q = _block(cin2, cmid, cout, hin, win, n, seed=7)
    out, bufs = guarded_map(n, q["ho"], q["wo"], cout, 4, dev)
    job = _fused_job(q, dev, out=out)
    p = ops.conv_tile_plan([job[:5]], 4)
    rows = n * q["ho"] * (q["wo"] + 2)
    assert p["kernel"] == "kxrw" and regime(p) == "all-half" and rows % 128 != 0, (p, rows)      # a partial last tile
    ops.conv2d_grouped2([job])
    torch.cuda.synchronize()
    assert_only_the_interior_was_written(out, bufs)
    _parity(case, out.to_f32().cpu(), _ref64(q))


_BIG = {}


def _big(dev):
    """32 images of the bench's stage-2 entry (64 x 56 x 340 -> 128 x 28 x 170), their all-half chunked outputs and the fp64
    reference of the first 3 images; computed once."""
    from agplace_amd import ops
    if not _BIG:
        (cmid, cout, ho, wo, nmax), _ = WIDE_CASES["mixed_stage2"]
        q = _block(64, cmid, cout, 2 * ho, 2 * wo, nmax, seed=21)
        assert (q["ho"], q["wo"]) == (ho, wo)
        q["dev"] = _device_block(q, dev)
        chunks = ops.SplitMap.alloc(nmax, ho, wo, cout, 1, 4, dev)
        k = WIDE_CASES["all_half_control"][0][4]
        for a in range(0, nmax, k):
            b = min(nmax, a + k)
            job = _fused_job(q, dev, a, b, out=ops.slice_map(chunks, a, b))
            assert regime(ops.conv_tile_plan([job[:5]], 4)) == "all-half"
            ops.conv2d_grouped2([job])
        _BIG.update(q=q, chunks=chunks, ref3=_ref64(q, 0, 3))
    return _BIG


@pytest.mark.parametrize("case", ["full_only", "mixed_stage2"])
def test_fused_conv2_full_and_mixed_schedules(dev, case):
    from agplace_amd import ops
    big = _big(dev)
    (_, _, _, _, n), want = WIDE_CASES[case]
    job = _fused_job(big["q"], dev, 0, n)
    assert regime(ops.conv_tile_plan([job[:5]], 4)) == want
    ops.conv2d_grouped2([job])
    torch.cuda.synchronize()
    assert torch.equal(job[2].hi, big["chunks"].hi[:n]), case
    _parity(case + " images 0..2", ops.slice_map(job[2], 0, 3).to_f32().cpu(), big["ref3"])


def _plane_job(q, dev):
    """The block's conv2 with a stored residual plane (random), and a plain one, on the same conv."""
    from agplace_amd import ops
    cw, _, _, hm = q["dev"]
    res = ops.pack_f32(images(q["cout"], q["ho"], q["wo"], hm.n, 99).to(dev), q["cout"], 1, 4)
    return (hm, cw, ops.SplitMap.alloc(hm.n, q["ho"], q["wo"], q["cout"], 1, 4, dev), res, True, None)


def test_grouped_launches_equal_single_ones(dev):
    from agplace_amd import ops
    qa, qb, qc = _block(64, 128, 128, 13, 27, 3, seed=31), _block(64, 128, 128, 20, 9, 2, seed=33), _block(64, 128, 128, 9, 9, 4, seed=35)
    for q in (qa, qb, qc):
        q["dev"] = _device_block(q, dev)

    def plain(q):
        j = _plane_job(q, dev)
        return j[:3] + (None,) + j[4:]
    for name, mk in (("two streams", lambda: [_fused_job(qa, dev), _fused_job(qb, dev)]),
                     ("stream + plane residual + plain", lambda: [_fused_job(qa, dev), _plane_job(qb, dev), plain(qc)])):
        group, single = mk(), mk()
        ops.conv2d_grouped2(group)
        for j in single:
            ops.conv2d_grouped2([j])
        torch.cuda.synchronize()
        for i, (g, s) in enumerate(zip(group, single)):
            assert torch.equal(g[2].hi, s[2].hi), (name, i)
    # the problems WITHOUT a stream are what the existing grouped entry computes
    a, b = _plane_job(qb, dev), _plane_job(qb, dev)
    ops.conv2d_grouped2([a])
    ops.conv2d(b[0], b[1], b[2], residual=b[3], relu=True, prec=4)
    assert torch.equal(a[2].hi, b[2].hi)


@pytest.mark.parametrize("trunks", [1, 2])
@pytest.mark.parametrize("shape", [(64, 64, 57, 85), (128, 256, 29, 85)], ids=["tn2_64_64_57x85", "tn4_128_256_29x85"])
def test_s2_without_downsample_is_bit_identical(dev, shape, trunks):
    from agplace_amd import ops
    cin, cout, h, w = shape
    ho, wo = ops.conv_out_size(h, 3, 2, 1), ops.conv_out_size(w, 3, 2, 1)
    old_c, old_d, new = [], [], []
    for t in range(trunks):
        n = 2 - t
        w3, s3, t3 = weights(cin, cout, 40 + t)
        w1, s1, t1 = weights(cin, cout, 50 + t, k=1)
        xm = ops.pack_f32(images(cin, h, w, n, 60 + t).to(dev), cin, 1, 4)
        c3 = ops.ConvWeights(w3.to(dev), s3.to(dev), t3.to(dev), 2, 1)
        c1 = ops.ConvWeights(w1.to(dev), s1.to(dev), t1.to(dev), 2, 0)
        old_c.append((xm, c3, ops.SplitMap.alloc(n, ho, wo, cout, 1, 4, dev), None, True))
        old_d.append((xm, c1, ops.SplitMap.alloc(n, ho, wo, cout, 1, 4, dev), None, False))
        new.append((xm, c3, guarded_map(n, ho, wo, cout, 4, dev), True))
    assert ops.conv_tile_plan(old_c + old_d, 4)["kernel"] == "s2"
    ops.conv2d_grouped(old_c + old_d, 4)
    ops.conv2d_s2_nods([(x, c, o[0], r) for x, c, o, r in new])
    torch.cuda.synchronize()
    for o, (_, _, (m, bufs), _) in zip(old_c, new):
        assert_only_the_interior_was_written(m, bufs)
        assert torch.equal(o[2].hi, m.hi)


def _guarded(dev, fn):
    from agplace_amd import _lib
    lib = _lib.load()
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    prev = lib.agp_range_flag_set(word.data_ptr())
    try:
        fn()
    finally:
        lib.agp_range_flag_set(prev)
    torch.cuda.synchronize()
    return int(word.item())


@pytest.mark.parametrize("big", [False, True], ids=["in_range", "leaves_range"])
def test_range_guard_twin(dev, big):
    """The guarded instantiations store the same bits; the word is set when a BLOCK OUTPUT leaves +-65504 (here through the
    downsample term alone: its folded weights stay far inside fp16) and stays 0 otherwise."""
    q = _block(64, 128, 128, 13, 27, 3, seed=41)
    if big:
        q["sd"] = q["sd"] * 3.0e4
    plain, guarded = _fused_job(q, dev), _fused_job(q, dev)
    from agplace_amd import ops
    ops.conv2d_grouped2([plain])
    flag = _guarded(dev, lambda: ops.conv2d_grouped2([guarded]))
    assert torch.equal(plain[2].hi, guarded[2].hi)
    assert flag == int(big)
    assert (float(plain[2].hi.float().max()) == 65504.0) == big


# ------------------------------------------------------------------------------------------------------------------ trunks
def _trunks(dev):
    from agplace_amd.network_mm.image_fe import ImageFE
    torch.manual_seed(0)
    fa = randomize_bn(ImageFE("resnet18", "2_2_2")).to(dev).eval()
    fb = randomize_bn(ImageFE("resnet18", "2_2_2"), seed=3).to(dev).eval()
    xa = torch.randn(11, 3, 64, 96, generator=torch.Generator().manual_seed(1)).to(dev)
    xb = torch.randn(5, 3, 32, 32, generator=torch.Generator().manual_seed(2)).to(dev)
    return fa, fb, xa, xb


def _maps(nets, xs):
    from agplace_amd import resnet
    return [[m.hi.clone() for m in maps] for maps in resnet.forward_maps_multi(nets, xs, prec=4)]


def test_trunks_switch_pairing_and_capture(dev, monkeypatch):
    from agplace_amd import resnet
    fa, fb, xa, xb = _trunks(dev)
    assert resnet.FUSE_DOWNSAMPLE
    on = _maps([fa.fe, fb.fe], [xa, xb])
    assert not any(str(k[0]).startswith("ds") for k in fa.fe._ws.bufs), "the fused route asks for no downsample map"
    monkeypatch.setattr(resnet, "FUSE_DOWNSAMPLE", False)
    off = _maps([fa.fe, fb.fe], [xa, xb])
    monkeypatch.setattr(resnet, "FUSE_DOWNSAMPLE", True)
    for r in range(2):
        for li, (a, b) in enumerate(zip(on[r], off[r])):
            e = rel_l2(a.float(), b.float())
            print("trunk %d stage %d: switch on against off %.3g (bar 1e-3)" % (r, li, e))
            assert e < 1e-3, (r, li, e)
        assert not torch.equal(on[r][1], off[r][1])          # (the route was taken)
    # one trunk alone equals the lock-step pair
    for r, (net, x) in enumerate(((fa.fe, xa), (fb.fe, xb))):
        alone = _maps([net], [x])[0]
        for a, b in zip(alone, on[r]):
            assert torch.equal(a, b), r
    # a captured graph replays to the eager bits
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        live = resnet.forward_maps_multi([fa.fe, fb.fe], [xa, xb], prec=4)
    for maps in live:
        for m in maps:
            m.hi.zero_()
    g.replay()
    torch.cuda.synchronize()
    for r in range(2):
        for a, m in zip(on[r], live[r]):
            assert torch.equal(a, m.hi), r


def test_unfusable_block_keeps_the_stored_downsample(dev, monkeypatch):
    """A downsample gamma that takes the folded weights past 65504 marks the block not fusable: the old route, the switch-off
    bits; the other entry block of the trunk stays fused."""
    from agplace_amd import resnet
    fa, _, xa, _ = _trunks(dev)
    bn = fa.fe.layer2[0].downsample[1]
    bn.weight.data.mul_(3.0e6)
    fuse = fa.fe._prepared_fuse(scaled=True)
    assert fuse[(1, 0)] is None and fuse[(2, 0)] is not None
    on = _maps([fa.fe], [xa[:2]])[0]
    monkeypatch.setattr(resnet, "FUSE_DOWNSAMPLE", False)
    off = _maps([fa.fe], [xa[:2]])[0]
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
