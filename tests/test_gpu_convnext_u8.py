"""-m gpu tests of the ConvNeXt-tiny trunk's uint8 inputs (Options.convnext_u8): agp_normalize_u8_cams, the uint8 stems
(agp_cnx_stem_u8_fwd / _bwd), the trunk, DBVanilla2D and MM.

The anchor is ops.normalize_cameras_u8: the fp32 panorama [n,3,h,ncam*w] uint8 tiles [n,ncam,h,w,3] stand for.  It is held to
torch ON THE CPU at 1e-6 absolute (about four ulps at the largest magnitude 1 / 0.22: each side is two divisions and one
subtraction); everything behind it is held BIT FOR BIT to the fp32 route on that image -- the uint8 stems are the fp32 stems'
kernel bodies on another loader -- and the trunk's maps to the fp64 restatement (tests/convnext_ref.py) on the fp64-normalised
image at the bars of tests/test_gpu_convnext.py (rel_l2, rel_max < 1e-4).
"""
import copy
import functools

import pytest
import torch

import convnext_ref as R
import mm_convnext_ref as ref
from gpu_util import rel_l2, rel_max, to_dev
from oracle import nets

pytestmark = pytest.mark.gpu

SEED = 2
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
KITTI = ((0.5, 0.5, 0.5), (0.22, 0.22, 0.22))
KEYS = ("imagevec_org", "voxvec_org", "shallowvec_org", "stg2fusevec", "stg2imagevec", "stg2voxvec", "embedding")


def u8(shape, seed):
    """Random bytes with both ends of the range present."""
    t = torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    t.view(-1)[0], t.view(-1)[-1] = 0, 255
    return t


def panorama(tiles, mean, std, dtype=torch.float32):
    """torch on the CPU: ToTensor + Normalize of every tile, width-concatenated."""
    n, ncam, h, w, _ = tiles.shape
    m, s = (torch.tensor(v, dtype=dtype).view(1, 3, 1, 1) for v in (mean, std))
    return (tiles.permute(0, 4, 2, 1, 3).reshape(n, 3, h, ncam * w).to(dtype) / 255 - m) / s


@functools.lru_cache(maxsize=None)
def stem32():
    return R.randomize_convnext(R.ConvNeXtTiny(), SEED).eval().features[0]


def stem_prep(dev):
    from agplace_amd import convnext as cnx
    return cnx.prep_stem(*copy.deepcopy(stem32()).to(dev))


# ------------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("mean,std", [IMAGENET, KITTI], ids=["imagenet", "kitti360"])
def test_normalize_matches_torch_on_the_cpu(dev, mean, std):
    from agplace_amd import ops
    tiles = u8((2, 3, 10, 14, 3), 1)
    want = panorama(tiles, mean, std)
    got = ops.normalize_cameras_u8(tiles.to(dev), mean, std)
    assert got.shape == (2, 3, 10, 42) and got.dtype == torch.float32 and got.is_contiguous()
    diff = float((got.cpu() - want).abs().max())
    print(f"normalize_cameras_u8 mean {mean[0]} std {std[0]}: max abs diff {diff:.3g}, bit-equal {torch.equal(got.cpu(), want)}")
    assert diff <= 1e-6
    # the tiles are distinguishable: camera 1's first column is panorama column 14
    assert torch.equal(got[:, :, :, 14], ops.normalize_cameras_u8(tiles[:, 1:2].contiguous().to(dev), mean, std)[:, :, :, 0])


def test_normalize_and_stem_argument_checks(dev):
    from agplace_amd import _lib, ops
    import ctypes as C
    L = _lib.load()
    m, s = (C.c_float * 3)(*IMAGENET[0]), (C.c_float * 3)(*IMAGENET[1])
    t = torch.zeros(1, 1, 8, 8, 3, dtype=torch.uint8, device=dev)
    o = torch.zeros(1, 3, 8, 8, device=dev)
    p = stem_prep(dev)
    so = torch.zeros(1, 2, 2, 96, device=dev)
    for args in ((None, 1, 1, 8, 8), (t.data_ptr(), 0, 1, 8, 8), (t.data_ptr(), 1, 0, 8, 8), (t.data_ptr(), 1, 1, 3, 8),
                 (t.data_ptr(), 1, 3, 8, 1), (t.data_ptr(), 1, 1, 8, -1)):
        assert L.agp_normalize_u8_cams(*args, m, s, o.data_ptr(), _lib.stream()) == 1, args
        assert L.agp_cnx_stem_u8_fwd(*args, m, s, p["w"].data_ptr(), p["bias"].data_ptr(), p["g"].data_ptr(), p["b"].data_ptr(), 1e-6,
                                     so.data_ptr(), _lib.stream()) == 1, args
    assert L.agp_normalize_u8_cams(t.data_ptr(), 1, 1, 8, 8, m, s, None, _lib.stream()) == 1
    with pytest.raises(ValueError, match="uint8"):
        ops.normalize_cameras_u8(o)
    with pytest.raises(ValueError, match="4x4"):
        ops.normalize_cameras_u8(torch.zeros(1, 1, 3, 8, 3, dtype=torch.uint8, device=dev))


STEM_SHAPES = [(2, 3, 10, 14, 3),      # w % 4 = 2: patches straddle cameras; 42 % 4 = 2 columns and 2 rows dropped; P = 40
               (1, 1, 4, 4, 3),        # one patch
               (3, 2, 8, 12, 3),       # aligned
               (1, 5, 7, 5, 3)]        # w = 5: every patch straddles, one spans a whole camera


@pytest.mark.parametrize("shape", STEM_SHAPES, ids=["x".join(map(str, s)) for s in STEM_SHAPES])
@pytest.mark.parametrize("mean,std", [IMAGENET, KITTI], ids=["imagenet", "kitti360"])
def test_stem_forward_is_the_fp32_stem_on_the_panorama(dev, shape, mean, std):
    from agplace_amd import convnext as cnx, ops
    tiles = u8(shape, 3).to(dev)
    p = stem_prep(dev)
    want = cnx.stem_fwd(ops.normalize_cameras_u8(tiles, mean, std), p)
    got = cnx.stem_u8_fwd(tiles, mean, std, p)
    n, ncam, h, w, _ = shape
    assert got.shape == (n, (h - 4) // 4 + 1, (ncam * w - 4) // 4 + 1, 96)
    assert torch.equal(got, want)
    assert float(got.abs().max()) > 0 and bool(torch.isfinite(got).all())


def test_stem_forward_reads_nothing_outside_its_tiles(dev):
    """The tiles are a slice of a larger buffer: whatever stands in the bytes around them, the output is the same."""
    from agplace_amd import convnext as cnx
    shape = (2, 3, 10, 14, 3)
    tiles = u8(shape, 3).to(dev)
    numel, guard = tiles.numel(), 4099                      # (an odd offset: the slice is not even 2-byte aligned)
    p = stem_prep(dev)
    want = cnx.stem_u8_fwd(tiles, *IMAGENET, p)
    outs = []
    for sentinel in (0, 255, 93):
        buf = torch.full((guard + numel + guard,), sentinel, dtype=torch.uint8, device=dev)
        view = buf[guard:guard + numel].view(shape)
        view.copy_(tiles)
        outs.append(cnx.stem_u8_fwd(view, *IMAGENET, p))
    for o in outs:
        assert torch.equal(o, want)


def _stem_bwd(dev, tiles, gout, mean, std, route):
    from agplace_amd import convnext as cnx, ops
    p = stem_prep(dev)
    n, ho, wo, _ = gout.shape
    grads = [torch.zeros(s, device=dev) for s in ((96, 3, 4, 4), (96,), (96,), (96,))]
    bws = torch.empty(cnx.bwd_workspace_bytes(n, ho, wo, 96), dtype=torch.uint8, device=dev)
    if route == "u8":
        cnx.stem_u8_bwd(tiles, mean, std, gout, p, grads, bws)
    else:
        cnx.stem_bwd(ops.normalize_cameras_u8(tiles, mean, std), gout, p, grads, bws)
    return grads


@pytest.mark.parametrize("shape", [(3, 3, 16, 36, 3),        # P = 324: 11 tiles, two workgroup partials of 8 tiles
                                   (2, 3, 10, 14, 3)], ids=["3x3x16x36", "2x3x10x14"])
def test_stem_backward_is_the_fp32_stem_backward_on_the_panorama(dev, shape):
    tiles = u8(shape, 4).to(dev)
    n, ncam, h, w, _ = shape
    ho, wo = (h - 4) // 4 + 1, (ncam * w - 4) // 4 + 1
    gout = torch.randn(n, ho, wo, 96, generator=torch.Generator().manual_seed(5)).to(dev)
    want = _stem_bwd(dev, tiles, gout, *KITTI, "f32")
    got = _stem_bwd(dev, tiles, gout, *KITTI, "u8")
    again = _stem_bwd(dev, tiles, gout, *KITTI, "u8")
    for name, g, r, a in zip(("g_w", "g_bias", "g_ln_w", "g_ln_b"), got, want, again):
        assert float(r.abs().max()) > 0, name
        assert torch.equal(g, r), name
        assert torch.equal(g, a), f"{name}: two runs differ"


# -------------------------------------------------------------------------------------------------------------- trunk
TRUNK_TILES = (2, 3, 40, 14, 3)           # panorama 40 x 42: maps 10x10, 5x5, 2x2; patches straddle cameras


def _trunk(dev, train=False):
    from agplace_amd.convnext import ConvNeXt
    fe = ConvNeXt((1, 1, 1))
    fe.load_state_dict(R.seeded_trunk([1, 1, 1], SEED, torch.float32).state_dict(), strict=True)
    fe.enable_u8_inputs().set_image_norm(*KITTI)
    if train:
        fe.enable_training()
    else:
        fe.requires_grad_(False)
    return fe.to(dev).eval()


def test_trunk_maps_from_tiles_equal_the_fp32_route_and_meet_fp64(dev):
    from agplace_amd import ops
    tiles = u8(TRUNK_TILES, 6)
    fe = _trunk(dev)
    with torch.no_grad():
        got = fe.forward_maps(tiles.to(dev))
        same = fe.forward_maps(ops.normalize_cameras_u8(tiles.to(dev), *KITTI))
        m64 = R.seeded_trunk([1, 1, 1], SEED, torch.float64)
        x64 = panorama(tiles, *KITTI, dtype=torch.float64)
        R.check_weights_are_felt(m64, x64)
        want = R.forward_maps(m64, x64)
    assert [tuple(m.shape) for m in got] == [(2, 96, 10, 10), (2, 192, 5, 5), (2, 384, 2, 2)]
    for i, (a, b, r) in enumerate(zip(got, same, want)):
        assert torch.equal(a, b), i
        l2, mx = rel_l2(a, r), rel_max(a, r)
        print(f"convnext_u8 trunk map {i}: rel_l2 {l2:.3g} rel_max {mx:.3g}")
        assert l2 < 1e-4 and mx < 1e-4, (i, l2, mx)


def test_trunk_training_from_tiles_equals_the_fp32_route(dev):
    """forward_maps_train with given row_scales: maps and every parameter gradient, bit for bit; the node saved the uint8 tiles."""
    from agplace_amd import ops
    tiles = u8(TRUNK_TILES, 6).to(dev)
    fe = _trunk(dev, train=True)
    scales = [None, torch.tensor([0.0, 1.0 / 0.9], device=dev), torch.tensor([1.0 / 0.8, 1.0 / 0.8], device=dev)]
    cot = [torch.randn(s, generator=torch.Generator().manual_seed(7 + i)).to(dev)
           for i, s in enumerate(((2, 96, 10, 10), (2, 192, 5, 5), (2, 384, 2, 2)))]
    runs = []
    for x in (tiles, ops.normalize_cameras_u8(tiles, *KITTI)):
        fe.zero_grad(set_to_none=True)
        maps = fe.forward_maps_train(x, row_scales=scales)
        saved = maps[0].grad_fn.x
        assert saved.dtype == x.dtype and saved.data_ptr() == x.data_ptr()
        sum((m * c).sum() for m, c in zip(maps, cot)).backward()
        runs.append(([m.detach().clone() for m in maps], {n: p.grad.clone() for n, p in fe.features.named_parameters()}))
    (maps_a, grads_a), (maps_b, grads_b) = runs
    for a, b in zip(maps_a, maps_b):
        assert torch.equal(a, b)
    assert len(grads_a) == len(list(fe.features.parameters())) and "0.0.weight" in grads_a
    for n in grads_a:
        assert float(grads_b[n].abs().max()) > 0, n
        assert torch.equal(grads_a[n], grads_b[n]), n


def test_trunk_refuses_uint8_without_the_switch_and_bad_tiles_with_it(dev):
    from agplace_amd import ops
    from agplace_amd.convnext import ConvNeXt
    off = ConvNeXt((1, 1, 1)).requires_grad_(False).to(dev).eval()
    tiles = u8(TRUNK_TILES, 6).to(dev)
    with torch.no_grad():
        with pytest.raises(ValueError, match="fp32"):
            off.forward_maps(tiles)
        with pytest.raises(ValueError, match="fp32"):
            off.forward_maps(ops.RawFrames(tiles, 32, 32))
        on = _trunk(dev)
        with pytest.raises(ValueError, match="uint8"):
            on.forward_maps(tiles[..., :2])
        with pytest.raises(ValueError, match="uint8"):
            on.forward_maps(tiles[0])
        with pytest.raises(ValueError, match="too small"):
            on.forward_maps(tiles[:, :1, :, :4].contiguous())            # panorama 40 x 4: one patch wide


# -------------------------------------------------------------------------------------------------------------- model
def _db(dev, train=False, maptype="a", share=False, **kw):
    from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
    from agplace_amd.options import Options
    opt = Options(dbimage_fe="convnext_tiny", dbimage_fe_layers="1_1_1", features_dim=384, convnext_u8=True, db_resize=64,
                  maptype=maptype, share_dbfe=share, convnext_train=train, image_mean=KITTI[0], image_std=KITTI[1], **kw)
    torch.manual_seed(3)
    model = DBVanilla2D("db", 384, opt=opt)
    for i, e in enumerate(model.dbimage_fes):
        e.fe.load_state_dict(R.seeded_trunk([1, 1, 1], SEED + i, torch.float32).state_dict(), strict=True)
    return model.to(dev).train(train)


@pytest.mark.parametrize("crop", [None, 72])
def test_dbvanilla2d_frames_tiles_and_fp32_agree(dev, crop):
    from agplace_amd import ops
    model = _db(dev, db_cropsize=crop)
    frames = u8((2, 1, 80, 80, 3), 8).to(dev)
    with torch.no_grad():
        tiles = ops.resize_cameras_u8(frames, 64, crop=crop)
        assert tiles.shape == (2, 1, 64, 64, 3)
        image = ops.normalize_cameras_u8(tiles, *KITTI)                               # [2,3,64,64]: one camera per tile
        e_frames = model({"db_frames": frames}, mode="db")["embedding"]
        e_tiles = model({"db_map": tiles}, mode="db")["embedding"]
        e_f32 = model({"db_map": image.unsqueeze(1)}, mode="db")["embedding"]
        e_6d = model({"db_frames": frames.view(1, 2, 1, 80, 80, 3)}, mode="db")["embedding"]
        e_tiles_6d = model({"db_map": tiles.view(1, 2, 1, 64, 64, 3)}, mode="db")["embedding"]
    assert e_frames.shape == (2, 384) and e_6d.shape == (1, 2, 384) and float(e_frames.abs().max()) > 0
    assert torch.equal(e_frames, e_tiles) and torch.equal(e_tiles, e_f32)
    assert torch.equal(e_6d.view(2, 384), e_frames) and torch.equal(e_tiles_6d, e_6d)
    if crop is not None:                                                               # the crop is felt
        with torch.no_grad():
            assert not torch.equal(_db(dev)({"db_frames": frames}, mode="db")["embedding"], e_frames)


def test_dbvanilla2d_jitter_equals_jittered_tiles(dev):
    from agplace_amd import input_pipeline as ip, ops
    model = _db(dev)
    frames = u8((2, 1, 80, 80, 3), 8).to(dev)
    rec = ip.color_jitter(2, 0.4, 0.3, 0.2, 0.1, generator=torch.Generator().manual_seed(5)).to(dev)
    with torch.no_grad():
        tiles = ops.resize_cameras_u8(frames, 64)
        jittered = ops.jitter_cameras_u8(tiles, rec)
        assert not torch.equal(jittered, tiles)
        got = model({"db_frames": frames, "db_jitter": rec}, mode="db")["embedding"]
        want = model({"db_map": jittered}, mode="db")["embedding"]
        plain = model({"db_map": tiles}, mode="db")["embedding"]
    assert torch.equal(got, want) and not torch.equal(got, plain)


def test_dbvanilla2d_training_gradients_from_frames_equal_those_from_tiles(dev):
    """.train() with convnext_train, two map types on ONE shared trunk, the stochastic-depth draw seeded."""
    from agplace_amd import ops
    model = _db(dev, train=True, maptype="a_b", share=True)
    frames = u8((2, 2, 80, 80, 3), 9).to(dev)
    tiles = torch.stack([ops.resize_cameras_u8(frames[:, i:i + 1].contiguous(), 64)[:, 0] for i in range(2)], dim=1)
    cot = torch.randn(2, 384, generator=torch.Generator().manual_seed(1)).to(dev)
    runs = []
    for data in ({"db_frames": frames}, {"db_map": tiles}):
        model.zero_grad(set_to_none=True)
        torch.cuda.manual_seed(77)
        out = model(data, mode="db")["embedding"]
        (out * cot).sum().backward()
        runs.append((out.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}))
    (out_a, ga), (out_b, gb) = runs
    assert torch.equal(out_a, out_b)
    assert set(ga) == set(gb) and "dbimage_fes.0.fe.features.0.0.weight" in ga
    assert float(ga["dbimage_fes.0.fe.features.0.0.weight"].abs().max()) > 0
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n


# ----------------------------------------------------------------------------------------------------------------- MM
B, NCAM, H0, W0, QRES = 2, 2, 40, 60, 32          # frames [2,2,40,60,3] at q_resize = 32: tiles 32 x 48, panorama 32 x 96


@functools.lru_cache(maxsize=None)
def _mm_state():
    return ref.seeded_params(ref.options("1_1_1"), seed=5, dtype=torch.float32)[0]


def _mm(dev, train=False, drop=None):
    from agplace_amd.network_mm.mm import MM
    opt = ref.options("1_1_1", convnext_u8=True, q_resize=QRES, convnext_train=train)
    m = MM(drop=drop, opt=opt)
    m.load_state_dict(_mm_state(), strict=True)
    return m.to(dev).train(train)


def _mm_routes(dev):
    """The dense stand-ins of a 32 x 96 query and the three forms of its image: frames, uint8 tiles, the fp32 panorama."""
    from agplace_amd import ops
    data = {k: v for k, v in to_dev(nets.synth_query(B, 32, 96, ref.options(), seed=9), dev).items() if k != "query_image"}
    frames = u8((B, NCAM, H0, W0, 3), 10).to(dev)
    tiles = ops.resize_cameras_u8(frames, QRES)
    assert tiles.shape == (B, NCAM, 32, 48, 3)
    return data, frames, tiles, ops.normalize_cameras_u8(tiles, *IMAGENET)


def test_mm_three_routes_give_the_same_outputs(dev):
    from agplace_amd import input_pipeline as ip, ops
    m = _mm(dev)
    data, frames, tiles, image = _mm_routes(dev)
    rec = ip.color_jitter(B * NCAM, 0.4, 0.3, 0.2, 0.1, generator=torch.Generator().manual_seed(6)).to(dev)
    with torch.no_grad():
        a = m(dict(data, query_frames=frames), mode="q")
        b = m(dict(data, query_image=tiles), mode="q")
        c = m(dict(data, query_image=image), mode="q")
        ja = m(dict(data, query_frames=frames, query_jitter=rec), mode="q")
        jb = m(dict(data, query_image=ops.jitter_cameras_u8(tiles, rec)), mode="q")
        with pytest.raises(NotImplementedError, match="drop='image'"):
            _mm(dev, drop="image")(dict(data, query_image=tiles), mode="q")
    for k in KEYS:
        assert a[k].shape == (B, 384) and float(a[k].abs().max()) > 0, k
        assert torch.equal(a[k], b[k]) and torch.equal(b[k], c[k]), k
        assert torch.equal(ja[k], jb[k]), k
    assert not torch.equal(ja["imagevec_org"], a["imagevec_org"])


def test_mm_training_step_from_frames_equals_the_one_from_tiles(dev):
    m = _mm(dev, train=True)
    data, frames, tiles, _ = _mm_routes(dev)
    cot = torch.randn(B, 384, generator=torch.Generator().manual_seed(2)).to(dev)
    runs = []
    for d in (dict(data, query_frames=frames), dict(data, query_image=tiles)):
        m.zero_grad(set_to_none=True)
        torch.cuda.manual_seed(77)
        out = m(d, mode="q")
        sum((out[k] * cot).sum() for k in ("embedding", "stg2imagevec", "imagevec_org", "stg2fusevec")).backward()
        runs.append(({k: out[k].detach().clone() for k in KEYS}, {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}))
    (oa, ga), (ob, gb) = runs
    for k in KEYS:
        assert torch.equal(oa[k], ob[k]), k
    assert set(ga) == set(gb) and len(ga) > 60 and float(ga["image_fe.fe.features.0.0.weight"].abs().max()) > 0
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n


def test_mm_captured_replay_from_frames_equals_eager(dev):
    """The graph rule of the ResNet model: the resize tables are uploaded before the capture (ops.prepare_resize); the warm-up
    that prepares the weights runs on uint8 tiles and never touches them."""
    from agplace_amd import ops
    m = _mm(dev)
    data, frames, tiles, _ = _mm_routes(dev)
    d = dict(data, query_frames=frames)
    with torch.no_grad():
        m(dict(data, query_image=tiles), mode="q")
        ops.prepare_resize(H0, W0, 32, 48, dev)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = m(d, mode="q")
        inputs = {t.data_ptr() for v in d.values() for t in (v if isinstance(v, list) else [v])}
        for v in out.values():
            if v.data_ptr() not in inputs:
                v.zero_()
        graph.replay()
        torch.cuda.synchronize()
        eager = m(d, mode="q")
    for k in KEYS:
        assert torch.equal(out[k], eager[k]), k
