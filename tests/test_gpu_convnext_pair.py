"""-m gpu tests of Options.convnext_pair: the grouped ConvNeXt launches (agp_cnx_*_fwd_grouped), ConvNeXt.forward_maps_multi, and
pair.embed_pair / pair.CapturedPair on ConvNeXt models.

Lock-step changes the SHAPE of the launches and never the arithmetic: a workgroup of a grouped launch does exactly what the plain
launch gives the same block index inside the same problem.  So every comparison here is torch.equal against the plain entry points
or the two separate model forwards; there is no tolerance.

Shapes: the smallest at which grouping can go wrong.  The images [2,3,36,100], [3,3,40,44] and [1,3,32,32] give stem maps of 9x25,
10x11 and 8x8: P = 450 and 330 are no multiples of the 32-pixel tile, so those problems end in a partial tile and the next problem
starts mid-grid; the 4x8 depthwise tiles are cut on both axes; the three problems have 15 + 11 + 2 MLP tiles and 42 + 18 + 2
depthwise tiles.  The same three geometries are used at C = 96, 192 and 384, in both precisions, with 1, 2 and 3 problems.
"""
import functools

import pytest
import torch
import torch.nn as nn

import convnext_guard_ref as G
import convnext_ref as R
import mm_convnext_ref as ref
from gpu_util import to_dev
from oracle import nets

pytestmark = pytest.mark.gpu

IMAGES = ((2, 3, 36, 100), (3, 3, 40, 44), (1, 3, 32, 32))
STREAMS = ((2, 9, 25), (3, 10, 11), (1, 8, 8))          # the stem maps of IMAGES
NGROUPS = (1, 2, 3)
KEYS = ("imagevec_org", "voxvec_org", "shallowvec_org", "stg2fusevec", "stg2imagevec", "stg2voxvec", "embedding")


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _u8(shape, seed):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _randomize(mod, seed):
    g = torch.Generator().manual_seed(seed)
    for p in mod.parameters():
        p.data = torch.randn(p.shape, generator=g) * (0.2 if p.dim() > 1 else 0.5)
    return mod


def _ws(cx, nhw, C, dev):
    return torch.full((cx.workspace_bytes(*nhw, C),), 0x5a, dtype=torch.uint8, device=dev)


# ------------------------------------------------------------------------------------------------------------ op level
def test_stem_grouped_equals_plain_fp32(dev):
    from agplace_amd import convnext as cx
    ps = [cx.prep_stem(*[m.to(dev) for m in _randomize(nn.Sequential(nn.Conv2d(3, 96, 4, 4), cx.LayerNorm2d(96)), 20 + i)])
          for i in range(3)]
    xs = [_rand(s, 30 + i).to(dev) for i, s in enumerate(IMAGES)]
    xs[1] = xs[1].permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)          # strides are honoured per problem
    want = [cx.stem_fwd(x, p) for x, p in zip(xs, ps)]
    assert [tuple(w.shape[:3]) for w in want] == list(STREAMS)
    for ng in NGROUPS:
        got = cx.stem_fwd_grouped(xs[:ng], ps[:ng])
        for i in range(ng):
            assert torch.equal(got[i], want[i]), (ng, i)
    rev = cx.stem_fwd_grouped(xs[::-1], ps[::-1])                                # the small problem first: other prefix sums
    for i in range(3):
        assert torch.equal(rev[2 - i], want[i]), i


def test_stem_grouped_equals_plain_uint8(dev):
    """The uint8 loader with ncam = 2: panoramas 36x100, 40x44 and 32x32 from two cameras each, a Normalize per problem."""
    from agplace_amd import convnext as cx
    ps = [cx.prep_stem(*[m.to(dev) for m in _randomize(nn.Sequential(nn.Conv2d(3, 96, 4, 4), cx.LayerNorm2d(96)), 40 + i)])
          for i in range(3)]
    tiles = [_u8((n, 2, h, w // 2, 3), 50 + i).to(dev) for i, (n, _, h, w) in enumerate(IMAGES)]
    norms = [((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)), ((0.5, 0.5, 0.5), (0.22, 0.22, 0.22)), ((0.1, 0.2, 0.3), (0.3, 0.2, 0.1))]
    want = [cx.stem_u8_fwd(t, *nm, p) for t, nm, p in zip(tiles, norms, ps)]
    assert [tuple(w.shape[:3]) for w in want] == list(STREAMS)
    for ng in NGROUPS:
        got = cx.stem_fwd_grouped(tiles[:ng], ps[:ng], norms[:ng])
        for i in range(ng):
            assert torch.equal(got[i], want[i]), (ng, i)
    with pytest.raises(ValueError, match="not both"):
        cx.stem_fwd_grouped([tiles[0], _rand(IMAGES[1], 1).to(dev)], ps[:2], norms[:2])


@pytest.mark.parametrize("prec", [3, 4])
@pytest.mark.parametrize("C", [96, 192, 384])
def test_block_kernels_grouped_equal_plain(dev, C, prec):
    """agp_cnx_dwconv_ln(_f16)_fwd_grouped and agp_cnx_mlp(_f16)_fwd_grouped: the operand workspaces (every byte: a launch writes
    nothing past its own rows) and the outputs, out of place and in place."""
    from agplace_amd import convnext as cx
    ps = [cx.prep_block(_randomize(cx.CNBlock(C), 60 + i).to(dev), prec) for i in range(3)]
    xs = [_rand((*nhw, C), 70 + i).to(dev) for i, nhw in enumerate(STREAMS)]
    want_ws, want_out = [], []
    for x, p, nhw in zip(xs, ps, STREAMS):
        ws = _ws(cx, nhw, C, dev)
        cx.dwconv_ln_fwd(x, p, ws, prec)
        want_ws.append(ws)
        want_out.append(cx.mlp_fwd(ws, p, x, torch.empty_like(x), prec))
    for ng in NGROUPS:
        wss = [_ws(cx, nhw, C, dev) for nhw in STREAMS[:ng]]
        cx.dwconv_ln_fwd_grouped(xs[:ng], ps[:ng], wss, prec)
        for i in range(ng):
            assert torch.equal(wss[i], want_ws[i]), ("operand", ng, i)
        outs = cx.mlp_fwd_grouped(wss, ps[:ng], xs[:ng], [torch.empty_like(x) for x in xs[:ng]], prec)
        for i in range(ng):
            assert torch.equal(outs[i], want_out[i]), ("mlp", ng, i)
        inplace = [x.clone() for x in xs[:ng]]
        cx.mlp_fwd_grouped(wss, ps[:ng], inplace, inplace, prec)
        for i in range(ng):
            assert torch.equal(inplace[i], want_out[i]), ("mlp in place", ng, i)
    assert not torch.equal(want_out[0], xs[0])


@pytest.mark.parametrize("prec", [3, 4])
@pytest.mark.parametrize("C", [96, 192, 384])
def test_downsample_grouped_equals_plain(dev, C, prec):
    """Odd sizes: 9x25 -> 4x12, 10x11 -> 5x5, 8x8 -> 4x4 (96, 75 and 16 output pixels: two partial last tiles)."""
    from agplace_amd import convnext as cx
    mods = [_randomize(nn.Sequential(cx.LayerNorm2d(C), nn.Conv2d(C, 2 * C, 2, 2)), 80 + i).to(dev) for i in range(3)]
    ps = [cx.prep_down(*m, prec) for m in mods]
    xs = [_rand((*nhw, C), 90 + i).to(dev) for i, nhw in enumerate(STREAMS)]
    want = [cx.downsample_fwd(x, p, prec) for x, p in zip(xs, ps)]
    for ng in NGROUPS:
        got = cx.downsample_fwd_grouped(xs[:ng], ps[:ng], prec)
        for i in range(ng):
            assert got[i].shape == want[i].shape and torch.equal(got[i], want[i]), (ng, i)


def test_grouped_entries_validate(dev):
    from agplace_amd import convnext as cx
    p = cx.prep_block(_randomize(cx.CNBlock(96), 1).to(dev), 3)
    x = _rand((1, 8, 8, 96), 2).to(dev)
    with pytest.raises(ValueError, match="1 .. 4 problems"):
        cx.dwconv_ln_fwd_grouped([x] * 5, [p] * 5, [_ws(cx, (1, 8, 8), 96, dev)] * 5)
    with pytest.raises(RuntimeError, match="AGP_E_BADARG"):
        cx.dwconv_ln_fwd_grouped([x], [p], [torch.zeros(64, dtype=torch.uint8, device=dev)])          # a workspace too small
    with pytest.raises(ValueError, match="does not match the prepared weights"):
        cx.mlp_fwd_grouped([_ws(cx, (1, 8, 8), 96, dev)], [p], [x], [x], prec=4)


# ------------------------------------------------------------------------------------------------------ forward_maps_multi
def _trunk(dev, layers, seed, prec=3, u8=False):
    from agplace_amd.convnext import ConvNeXt
    net = ConvNeXt([int(v) for v in layers.split("_")])
    net.load_state_dict(R.seeded_trunk([int(v) for v in layers.split("_")], seed, torch.float32).state_dict(), strict=True)
    net.set_precision(prec)
    if u8:
        net.enable_u8_inputs().set_image_norm((0.5,) * 3, (0.22,) * 3)
    return net.to(dev).eval()


@pytest.mark.parametrize("prec", [3, 4])
@pytest.mark.parametrize("layers", ["2_2_2", "1_2_1"])
def test_forward_maps_multi_equals_forward_maps(dev, layers, prec):
    from agplace_amd.convnext import ConvNeXt
    nets3 = [_trunk(dev, layers, 100 + i, prec) for i in range(3)]
    xs = [_rand(s, 110 + i).to(dev) for i, s in enumerate(IMAGES)]
    want = [net.forward_maps(x) for net, x in zip(nets3, xs)]
    for ng in (2, 3):                                       # [query, tiles] and [query, tiles, tiles2]
        got = ConvNeXt.forward_maps_multi(nets3[:ng], xs[:ng])
        for i in range(ng):
            assert len(got[i]) == 3
            for s in range(3):
                assert got[i][s].shape == want[i][s].shape and got[i][s].stride() == want[i][s].stride()
                assert torch.equal(got[i][s], want[i][s]), (ng, i, s)
    # the plain forward after the lock-step one: the same bits again (the trunks' workspaces and planes are their own)
    again = nets3[1].forward_maps(xs[1])
    assert all(torch.equal(a, w) for a, w in zip(again, want[1]))


def test_forward_maps_multi_mixed_inputs_and_refusals(dev):
    """A uint8-tile trunk beside an fp32 one (one stem launch per loader), one trunk given twice, and what is refused."""
    from agplace_amd.convnext import ConvNeXt
    a, b = _trunk(dev, "1_2_1", 120), _trunk(dev, "1_2_1", 121, u8=True)
    x, tiles = _rand(IMAGES[0], 122).to(dev), _u8((3, 2, 40, 22, 3), 123).to(dev)
    want_a, want_b = a.forward_maps(x), b.forward_maps(tiles)
    got = ConvNeXt.forward_maps_multi([a, b, a], [x, tiles, x])
    for g, w in zip(got, (want_a, want_b, want_a)):
        assert all(torch.equal(gm, wm) for gm, wm in zip(g, w))
    with pytest.raises(ValueError, match="same block counts and precision"):
        ConvNeXt.forward_maps_multi([a, _trunk(dev, "2_2_2", 124)], [x, x])
    with pytest.raises(ValueError, match="same block counts and precision"):
        ConvNeXt.forward_maps_multi([a, _trunk(dev, "1_2_1", 125, prec=4)], [x, x])
    with pytest.raises(ValueError, match="1 .. 4 trunks"):
        ConvNeXt.forward_maps_multi([a] * 5, [x] * 5)
    with pytest.raises(ValueError, match="fp32"):
        ConvNeXt.forward_maps_multi([a, a], [x, tiles])     # uint8 into a trunk without enable_u8_inputs


# -------------------------------------------------------------------------------------------------------------- models
@functools.lru_cache(maxsize=None)
def _mm_state(layers):
    return ref.seeded_params(ref.options(layers), seed=5, dtype=torch.float32)[0]


def _mm(dev, layers="2_2_2", **kw):
    from agplace_amd.network_mm.mm import MM
    m = MM(opt=ref.options(layers, **kw))
    m.load_state_dict(_mm_state(layers), strict=True)
    return m.to(dev).eval()


def _db(dev, layers="2_2_2", maptype="a", fe="convnext_tiny", **kw):
    from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
    from agplace_amd.options import Options
    opt = Options(dbimage_fe=fe, dbimage_fe_layers=layers, features_dim=384, maptype=maptype, **kw)
    torch.manual_seed(3)
    model = DBVanilla2D("db", 384, opt=opt)
    if fe == "convnext_tiny":
        for i, e in enumerate(model.dbimage_fes):
            e.fe.load_state_dict(R.seeded_trunk([int(v) for v in layers.split("_")], 200 + i, torch.float32).state_dict(), strict=True)
    return model.to(dev).eval()


def _query(dev, cloud=False):
    """A 32 x 96 query with the dense voxel stand-ins, or with a cloud in `coords` / `features`."""
    d = to_dev(nets.synth_query(2, 32, 96, ref.options(), seed=9), dev)
    if cloud:
        from oracle import sparse as osparse
        d = {"query_image": d["query_image"]}
        coords, features = osparse.synth_cloud(2, 120, extent=20, seed=3)
        d["coords"], d["features"] = coords.to(dev), features.to(dev)
    return d


class _Spy:
    """Counts the calls of ConvNeXt.forward_maps_multi: the lock-step path was taken (or was not)."""

    def __init__(self, monkeypatch):
        from agplace_amd import convnext
        self.calls, real = 0, convnext.ConvNeXt.forward_maps_multi

        def counted(nets_, xs):
            self.calls += 1
            return real(nets_, xs)
        monkeypatch.setattr(convnext.ConvNeXt, "forward_maps_multi", staticmethod(counted))


def _same(pair_out, want_q, want_db):
    out_q, out_db = pair_out
    assert set(out_q) == set(want_q) == set(KEYS) and set(out_db) == set(want_db) == {"embedding"}
    for k in KEYS:
        assert out_q[k].shape == want_q[k].shape and torch.equal(out_q[k], want_q[k]), k
    assert out_db["embedding"].shape == want_db["embedding"].shape and torch.equal(out_db["embedding"], want_db["embedding"])
    assert float(out_db["embedding"].abs().max()) > 0 and float(out_q["embedding"].abs().max()) > 0


@pytest.mark.parametrize("layers,prec,maptype,six_d,cloud", [
    ("2_2_2", 3, "a", False, False),
    ("1_2_1", 4, "a_b", True, True),
    ("1_2_1", 3, "a_b", False, True),
    ("2_2_2", 4, "a", True, False),
])
def test_embed_pair_equals_the_separate_forwards(dev, monkeypatch, layers, prec, maptype, six_d, cloud):
    from agplace_amd import pair
    nmap = len(maptype.split("_"))
    mq = _mm(dev, layers, convnext_pair=True, convnext_precision=prec)
    mdb = _db(dev, layers, maptype, convnext_pair=True, convnext_precision=prec)
    qd = _query(dev, cloud)
    tiles = _rand((3, 2, nmap, 3, 40, 44) if six_d else (3, nmap, 3, 40, 44), 300).to(dev)
    dd = {"db_map": tiles}
    want_q, want_db = mq(qd, mode="q"), mdb(dd, mode="db")
    spy = _Spy(monkeypatch)
    _same(pair.embed_pair(mq, mdb, qd, dd), want_q, want_db)
    assert spy.calls == 1
    assert want_db["embedding"].shape == ((3, 2, 384) if six_d else (3, 384))


def test_embed_pair_uint8_tiles_frames_and_jitter(dev, monkeypatch):
    from agplace_amd import input_pipeline as ip, ops, pair
    kw = dict(convnext_pair=True, convnext_u8=True)
    mq = _mm(dev, "1_2_1", q_resize=32, **kw)
    mdb = _db(dev, "1_2_1", db_resize=40, **kw)
    data = {k: v for k, v in _query(dev).items() if k != "query_image"}
    qframes, dframes = _u8((2, 2, 40, 60, 3), 10).to(dev), _u8((3, 1, 50, 55, 3), 11).to(dev)
    qrec = ip.color_jitter(4, 0.4, 0.3, 0.2, 0.1, generator=torch.Generator().manual_seed(6)).to(dev)
    drec = ip.color_jitter(3, 0.4, 0.3, 0.2, 0.1, generator=torch.Generator().manual_seed(7)).to(dev)
    qtiles, dtiles = ops.resize_cameras_u8(qframes, 32), ops.resize_cameras_u8(dframes, 40)
    assert qtiles.shape == (2, 2, 32, 48, 3) and dtiles.shape == (3, 1, 40, 44, 3)
    spy = _Spy(monkeypatch)
    routes = [(dict(data, query_image=qtiles), {"db_map": dtiles}),
              (dict(data, query_frames=qframes), {"db_frames": dframes}),
              (dict(data, query_frames=qframes, query_jitter=qrec), {"db_frames": dframes, "db_jitter": drec})]
    outs = []
    for n, (qd, dd) in enumerate(routes):
        want_q, want_db = mq(qd, mode="q"), mdb(dd, mode="db")
        got = pair.embed_pair(mq, mdb, qd, dd)
        _same(got, want_q, want_db)
        assert spy.calls == n + 1
        outs.append(got[1]["embedding"])
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])        # frames = their tiles; the jitter is felt
    # without convnext_u8 the separate forwards refuse the frames by name, and so does the pair
    with pytest.raises(NotImplementedError, match="query_frames"):
        pair.embed_pair(_mm(dev, "1_2_1", convnext_pair=True), mdb, routes[1][0], routes[1][1])


def test_fall_backs_equal_the_separate_forwards(dev, monkeypatch):
    """A ResNet database model, unequal precisions, unequal block counts, five trunks: no lock-step, no error, the same outputs."""
    from agplace_amd import pair
    qd, on = _query(dev), dict(convnext_pair=True)
    mq = _mm(dev, "1_2_1", **on)
    want_q = mq(qd, mode="q")
    spy = _Spy(monkeypatch)
    cases = [(_db(dev, "2_2_2", fe="resnet18", **on), (3, 1, 3, 64, 64)),
             (_db(dev, "1_2_1", convnext_precision=4, **on), (3, 1, 3, 40, 44)),
             (_db(dev, "2_2_2", **on), (3, 1, 3, 40, 44)),
             (_db(dev, "1_2_1", maptype="a_b_c_d", **on), (1, 4, 3, 32, 32))]
    for mdb, shape in cases:
        dd = {"db_map": _rand(shape, 310).to(dev)}
        _same(pair.embed_pair(mq, mdb, qd, dd), want_q, mdb(dd, mode="db"))
    assert spy.calls == 0


def test_a_bound_guard_is_never_skipped(dev, monkeypatch):
    """Options.convnext_range_guard at precision 4 on the database model: the pair runs the separate forwards, equal bits, and a
    saturating tile (the input of tests/test_gpu_convnext_guard.py: one hidden unit of stage 0 saturates on the bad image only)
    is reported by the model that owns the trunk, one call late, as in its own forward."""
    import test_gpu_convnext_guard as TG
    from agplace_amd import pair
    m, good, bad = TG.replay_pair((1, 3, 32, 32))
    mdb = TG._db(m, dev, convnext_range_guard=True, convnext_pair=True)
    mq = TG._mm(TG.clean(), dev, convnext_pair=True)
    qd = dict(TG._mm_data(dev), query_image=G.image((1, 3, 32, 96)).to(dev))
    spy = _Spy(monkeypatch)
    good_d, bad_d = {"db_map": good.unsqueeze(1).to(dev)}, {"db_map": bad.unsqueeze(1).to(dev)}
    want_q, want_db = mq(qd, mode="q"), mdb(good_d, mode="db")
    _same(pair.embed_pair(mq, mdb, qd, good_d), want_q, want_db)
    TG.run_sequence(lambda t: pair.embed_pair(mq, mdb, qd, {"db_map": t}), mdb, good_d["db_map"], bad_d["db_map"])
    assert spy.calls == 0 and mq.fp16_range_ok()
    # the same pair without the guard runs in lock-step (precision 4 on both models)
    _same(pair.embed_pair(mq, TG._db(m, dev, convnext_pair=True), qd, good_d), want_q, want_db)
    assert spy.calls == 1


# -------------------------------------------------------------------------------------------------------- CapturedPair
def _fills(dev, n):
    return [(_rand((2, 3, 32, 96), 400 + i).to(dev), _rand((3, 2, 3, 40, 44), 420 + i).to(dev)) for i in range(n)]


def _static(dev, cloud):
    qd = {k: (v.clone() if torch.is_tensor(v) else [t.clone() for t in v]) for k, v in _query(dev, cloud).items()}
    return qd, {"db_map": torch.zeros(3, 2, 3, 40, 44, device=dev)}


def _eager(mq, mdb, qd, dd, img, tiles):
    q, d = mq(dict(qd, query_image=img), mode="q"), mdb({"db_map": tiles}, mode="db")
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in q.items()}, d["embedding"].clone()


@pytest.mark.parametrize("prec,cloud", [(3, True), (4, False)])
def test_captured_pair_replays_equal_eager(dev, prec, cloud):
    from agplace_amd import pair
    mq = _mm(dev, "1_2_1", convnext_pair=True, convnext_precision=prec)
    mdb = _db(dev, "1_2_1", "a_b", convnext_pair=True, convnext_precision=prec)
    qd, dd = _static(dev, cloud)
    fills = _fills(dev, 3)
    want = [_eager(mq, mdb, qd, dd, *f) for f in fills]
    cp = pair.CapturedPair(mq, mdb, qd, dd, poll_every=1)
    for (img, tiles), (wq, wd) in zip(fills, want):
        qd["query_image"].copy_(img)
        dd["db_map"].copy_(tiles)
        cp.replay()
        out_q, out_db = cp.finish()
        for k in KEYS:
            assert torch.equal(out_q[k], wq[k]), k
        assert torch.equal(out_db["embedding"], wd)
    assert not torch.equal(want[0][1], want[1][1])


def test_two_captured_pairs_alternate_on_two_streams(dev):
    from agplace_amd import pair
    mq = _mm(dev, "1_2_1", convnext_pair=True)
    mdb = _db(dev, "1_2_1", "a_b", convnext_pair=True)
    statics = [_static(dev, False) for _ in range(2)]
    fills = _fills(dev, 6)
    want = [_eager(mq, mdb, *statics[i % 2], *f) for i, f in enumerate(fills)]
    cps = [pair.CapturedPair(mq, mdb, qd, dd, stream=torch.cuda.Stream(device=dev)) for qd, dd in statics]
    got = []
    for i, (img, tiles) in enumerate(fills):                # three replays each, alternately; both stay in flight
        qd, dd = statics[i % 2]
        if i >= 2:                                          # this capture's previous replay: collect it before the refill
            out_q, out_db = cps[i % 2].finish()
            got.append(({k: v.clone() for k, v in out_q.items()}, out_db["embedding"].clone()))
        qd["query_image"].copy_(img)
        dd["db_map"].copy_(tiles)
        cps[i % 2].replay()
    for cp in cps:
        out_q, out_db = cp.finish()
        got.append(({k: v.clone() for k, v in out_q.items()}, out_db["embedding"].clone()))
    assert len(got) == 6
    for i, ((gq, gd), (wq, wd)) in enumerate(zip(got, want)):
        for k in KEYS:
            assert torch.equal(gq[k], wq[k]), (i, k)
        assert torch.equal(gd, wd), i
