"""-m gpu tests of the camera front end's centre crop and colour jitter (csrc/camera.hip's region of interest, csrc/jitter.hip,
DESIGN.md 1d).  The bar is ZERO differing bytes: the uint8 modes against the numpy restatements tests/camera_ref.py and
tests/colour_ref.py (which tests/test_camera_ref.py and tests/test_colour_ref.py hold to Pillow itself), the packed modes
against the uint8 modes + pack_cameras_u8, and the models fed frames (+ crop, + jitter records) against the same models fed
the reference's uint8 tiles."""
import itertools

import numpy as np
import pytest
import torch

import camera_ref
import colour_ref
from gpu_util import randomize_bn, to_dev
from oracle import nets
from oracle import sparse as osparse

pytestmark = pytest.mark.gpu

KITTI_NORM = ((0.5, 0.5, 0.5), (0.22, 0.22, 0.22))


def _frames(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


@pytest.fixture(autouse=True)
def _no_grad(request):
    if "training" in request.node.name:
        yield
    else:
        with torch.no_grad():
            yield


def _planes(m):
    return [p.view(torch.int16) for p in (m.hi, m.lo) if p is not None]


def _same_planes(a, b):
    pa, pb = _planes(a), _planes(b)
    assert len(pa) == len(pb)
    for x, y in zip(pa, pb):
        assert torch.equal(x, y)


def _nbad(got, want):
    """(differing bytes, the first few of them) of a device tensor against a numpy array"""
    g = got.cpu().numpy()
    assert g.shape == want.shape and g.dtype == want.dtype
    bad = np.argwhere(g != want)
    return len(bad), [(tuple(i), int(g[tuple(i)]), int(want[tuple(i)])) for i in bad[:4]]


# ------------------------------------------------------------------------------------------------ centre crop
_CROP = {}


def _crop_case():
    """frames [2, 2, 45, 72, 3], CenterCrop(37): rows from 4 (an even difference), columns from 18 (17.5 rounds to even), so the
    window's rows start 54 bytes into rows of 216 bytes: no 16-byte alignment anywhere"""
    if not _CROP:
        src = _frames((2, 2, 45, 72, 3), 41)
        win = colour_ref.center_crop(src, 37)
        assert win.shape == (2, 2, 37, 37, 3) and np.array_equal(win, src[:, :, 4:41, 18:55])
        _CROP.update(src=src, win=win)
        for hw in ((24, 24), (24, 30)):
            out = camera_ref.resize_frames(win, *hw)
            out.setflags(write=False)
            _CROP[hw] = out
    return _CROP


@pytest.mark.parametrize("size", [24, (24, 30)], ids=["int24", "24x30"])
def test_crop_u8_mode_equals_reference_on_the_window(dev, size):
    from agplace_amd import ops
    c = _crop_case()
    hw = (24, 24) if size == 24 else size
    assert ops.center_crop_origin(45, 72, 37) == colour_ref.center_crop_origin(45, 72, 37) == (4, 18)
    got = ops.resize_cameras_u8(torch.from_numpy(c["src"]).to(dev), size, crop=37)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 2) + hw + (3,)
    n, first = _nbad(got, c[hw])
    assert n == 0, (n, first)
    # the same bytes as the uncropped op on the numpy-cropped window
    assert torch.equal(got, ops.resize_cameras_u8(torch.from_numpy(c["win"]).to(dev), hw))


@pytest.mark.parametrize("prec", [3, 2, 4])
def test_crop_packed_mode_equals_resize_then_pack_of_the_window(dev, prec):
    from agplace_amd import ops
    c = _crop_case()
    fr, win = torch.from_numpy(c["src"]).to(dev), torch.from_numpy(c["win"]).to(dev)
    for hw in ((24, 24), (24, 30)):
        want = ops.pack_cameras_u8(ops.resize_cameras_u8(win, hw), prec)
        got = ops.pack_cameras_resized_u8(fr, hw, prec, crop=37)
        assert (got.n, got.h, got.w, got.c, got.pad) == (2, hw[0], 2 * hw[1], 4, 3) and (got.lo is None) == (prec != 3)
        _same_planes(got, want)
    want = ops.pack_cameras_u8(ops.resize_cameras_u8(win, (24, 30)), prec, *KITTI_NORM)
    _same_planes(ops.pack_cameras_resized_u8(fr, (24, 30), prec, *KITTI_NORM, crop=37), want)


def test_crop_origin_rounds_halves_to_even(dev):
    from agplace_amd import ops
    for h0, w0, c in [(70, 72, 37), (38, 41, 37), (40, 39, 37), (9, 12, 4), (37, 37, 37), (16384, 16383, 1)]:
        assert ops.center_crop_origin(h0, w0, c) == colour_ref.center_crop_origin(h0, w0, c), (h0, w0, c)
    assert ops.center_crop_origin(70, 72, 37) == (16, 18)
    # both kinds of half on the device: 70 -> 16.5 -> 16, 72 -> 17.5 -> 18
    src = _frames((1, 1, 70, 72, 3), 42)
    got = ops.resize_cameras_u8(torch.from_numpy(src).to(dev), (37, 37), crop=37)
    n, first = _nbad(got, colour_ref.center_crop(src, 37))
    assert n == 0, (n, first)


def test_crop_equal_to_the_frame_is_the_uncropped_call(dev):
    from agplace_amd import ops
    fr = torch.from_numpy(_frames((1, 2, 37, 37, 3), 43)).to(dev)
    assert torch.equal(ops.resize_cameras_u8(fr, (24, 30), crop=37), ops.resize_cameras_u8(fr, (24, 30)))
    assert torch.equal(ops.resize_cameras_u8(fr, 24, crop=37), ops.resize_cameras_u8(fr, 24))
    for prec in (3, 4):
        _same_planes(ops.pack_cameras_resized_u8(fr, (24, 30), prec, crop=37), ops.pack_cameras_resized_u8(fr, (24, 30), prec))


def test_crop_window_at_the_end_of_the_allocation(dev):
    """n = ncam = 1, crop = the frame's height, a narrower width, and the frame's last byte the last byte of its buffer (at
    several alignments): the window's last row ends 18 bytes before the buffer does, its first row starts 18 bytes in."""
    from agplace_amd import ops
    src = _frames((1, 1, 37, 49, 3), 44)
    assert colour_ref.center_crop_origin(37, 49, 37) == (0, 6)
    want = camera_ref.resize_frames(colour_ref.center_crop(src, 37), 24, 24)
    for total in (src.size, src.size + 5, 8192):
        buf = torch.zeros(total, dtype=torch.uint8, device=dev)
        fr = buf[total - src.size:].view(src.shape)
        fr.copy_(torch.from_numpy(src))
        n, first = _nbad(ops.resize_cameras_u8(fr, 24, crop=37), want)
        assert n == 0, (total, n, first)


# ------------------------------------------------------------------------------------------------ colour jitter
def _records():
    """36 records: all 24 orders of the four ops (contrast first, in the middle and last among them), then 12 with ops left
    out.  Factors below 1, above 1 and large enough to clip both ways; hue shifts 0, 1, 128, 243; one record with no op at all."""
    rng = np.random.default_rng(7)
    shifts = [0, 1, 128, 243]
    recs = []
    for i, order in enumerate(itertools.permutations([1, 2, 3, 4])):
        kind = i % 3
        f = [rng.uniform(0.2, 0.95, 3), rng.uniform(1.05, 1.9, 3), rng.uniform(2.5, 4.0, 3)][kind]
        recs.append(list(order) + [float(v) for v in f] + [shifts[i % 4]])
    recs += [
        [0, 0, 0, 0, 1.0, 1.0, 1.0, 0],            # nothing: the frame comes back unchanged
        [0, 0, 0, 0, 0.3, 0.3, 0.3, 99],           # nothing either: factors without their ops are not applied
        [1, 0, 3, 4, 1.3, 1.0, 0.6, 243],          # contrast absent
        [4, 3, 0, 1, 0.7, 1.0, 3.5, 128],
        [2, 0, 0, 0, 1.0, 3.0, 1.0, 0],            # contrast alone, clipping both ways
        [0, 0, 0, 2, 1.0, 0.0, 1.0, 0],            # contrast last and alone at factor 0: the flat grey frame
        [0, 4, 0, 0, 1.0, 1.0, 1.0, 0],            # hue shift 0 (the HSV round trip alone)
        [0, 4, 0, 0, 1.0, 1.0, 1.0, 1],
        [3, 0, 2, 0, 1.0, 0.5, 0.0, 0],            # saturation 0 = grey, then contrast
        [1, 2, 0, 0, 0.0, 1.5, 1.0, 0],            # brightness 0 = black, contrast of a black frame
        [0, 1, 0, 0, 4.0, 1.0, 1.0, 0],
        [0, 0, 3, 0, 1.0, 1.0, 4.0, 0],
    ]
    r = np.array(recs, dtype=np.float32)
    assert len({tuple(x[:4]) for x in r[:24]}) == 24 and len(r) == 36
    return r


_JIT = {}


def _jitter_case(name):
    """(tiles, records, colour_ref's jittered tiles), computed once and shared read-only.  small0 .. small2: [4, 3, 19, 23, 3]
    with records 0-11, 12-23, 24-35; big0 / big1: [2, 1, 96, 341, 3] = 32 736 pixels, four workgroups per frame in the reduction."""
    if name not in _JIT:
        recs = _records()
        if name.startswith("small"):
            k = int(name[5:])
            tiles, r = _frames((4, 3, 19, 23, 3), 50 + k), recs[12 * k:12 * k + 12]
        else:
            k = int(name[3:])
            # contrast last behind a hue turn and a clipping saturation / contrast first; then contrast in the middle / absent
            r = recs[[[5, 8], [12, 26]][k]]
            tiles = _frames((2, 1, 96, 341, 3), 60 + k)
        want = colour_ref.jitter_frames(tiles, r)
        for a in (tiles, r, want):
            a.setflags(write=False)
        _JIT[name] = (tiles, r, want)
    return _JIT[name]


@pytest.mark.parametrize("name", ["small0", "small1", "small2", "big0", "big1"])
def test_jitter_u8_mode_equals_colour_ref(dev, name):
    from agplace_amd import ops
    tiles, recs, want = _jitter_case(name)
    t = torch.from_numpy(tiles.copy()).to(dev)
    got = ops.jitter_cameras_u8(t, torch.from_numpy(recs.copy()).to(dev))
    assert got.dtype == torch.uint8 and got.shape == t.shape and got.data_ptr() != t.data_ptr()
    n, first = _nbad(got, want)
    assert n == 0, (name, n, first)
    assert torch.equal(t.cpu(), torch.from_numpy(tiles.copy()))               # the input is left alone
    if name == "small2":                                                      # records 24, 25 have no op: frames 0 and 1 unchanged
        assert torch.equal(got[0, 0], t[0, 0]) and torch.equal(got[0, 1], t[0, 1]) and not torch.equal(got[0, 2], t[0, 2])
    # bit-repeatable (the reduction is an integer sum), and the records may have any leading shape
    again = ops.jitter_cameras_u8(t, torch.from_numpy(recs.copy()).to(dev).view(t.shape[0], t.shape[1], 8))
    assert torch.equal(again, got)


def test_jitter_colour_cube(dev):
    """All 2^24 colours as one 4096 x 4096 frame through hue, saturation and brightness (2048 workgroups' worth of pixels; the
    reference takes most of this test's time)."""
    from agplace_amd import ops
    v = np.arange(1 << 24, dtype=np.uint32)
    cube = np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(1, 1, 4096, 4096, 3)
    rec = np.array([[4, 3, 1, 0, 0.8, 1.0, 1.4, 77]], dtype=np.float32)
    got = ops.jitter_cameras_u8(torch.from_numpy(cube).to(dev), torch.from_numpy(rec).to(dev))
    want = colour_ref.jitter_frames(cube, rec)
    n, first = _nbad(got, want)
    assert n == 0, (n, first)


@pytest.mark.parametrize("prec", [3, 2, 4])
@pytest.mark.parametrize("norm", [None, KITTI_NORM], ids=["imagenet", "kitti"])
def test_jitter_packed_mode_equals_jitter_then_pack(dev, prec, norm):
    from agplace_amd import ops
    args = () if norm is None else norm
    for name in ("small0", "big0"):
        tiles, recs, _ = _jitter_case(name)
        t, r = torch.from_numpy(tiles.copy()).to(dev), torch.from_numpy(recs.copy()).to(dev)
        want = ops.pack_cameras_u8(ops.jitter_cameras_u8(t, r), prec, *args)
        got = ops.pack_cameras_jittered_u8(t, r, prec, *args)
        n, ncam, h, w, _ = tiles.shape
        assert (got.n, got.h, got.w, got.c, got.pad) == (n, h, ncam * w, 4, 3) and (got.lo is None) == (prec != 3)
        _same_planes(got, want)
        for a in _planes(got):                                 # the halo and the 4th channel keep SplitMap.alloc's zeros
            inner = torch.zeros_like(a, dtype=torch.bool)
            inner[:, 3:3 + h, 3:3 + ncam * w] = True
            assert int((a[~inner] != 0).sum()) == 0 and int((a[..., 3] != 0).sum()) == 0
    if norm is not None:
        assert not torch.equal(_planes(ops.pack_cameras_jittered_u8(t, r, prec))[0], _planes(got)[0])


# ------------------------------------------------------------------------------------------------ models
def _mm(dev, opt, seed=5, train=False):
    from agplace_amd.network_mm.mm import MM
    torch.manual_seed(seed)
    m = randomize_bn(MM(opt=opt)).to(dev)
    return m.train() if train else m.eval()


def _db(dev, opt, seed=6, train=False):
    from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
    torch.manual_seed(seed)
    m = randomize_bn(DBVanilla2D("db", opt.features_dim, opt=opt)).to(dev)
    return m.train() if train else m.eval()


_MODEL_REF = {}


def _ref_tiles(key, src, crop, hw, recs):
    """crop -> resize -> jitter by the numpy references, once per key"""
    if key not in _MODEL_REF:
        win = src if crop is None else colour_ref.center_crop(src, crop)
        out = colour_ref.jitter_frames(camera_ref.resize_frames(win, *hw), recs)
        out.setflags(write=False)
        _MODEL_REF[key] = out
    return _MODEL_REF[key]


def _query_pair(dev, opt, sparse, seed):
    """(data with query_frames + query_jitter, data with query_image = the reference's tiles): 2 samples x 2 cameras, 85x85 -> 64x64"""
    src = _frames((2, 2, 85, 85, 3), seed)
    recs = _records()[[3, 14, 26, 8]]                        # contrast last, second, absent and first
    tiles = _ref_tiles(("mm", seed), src, None, (64, 64), recs)
    base = nets.synth_query(2, 64, 128, opt, seed=seed)
    del base["query_image"]
    if sparse:
        for k in ("vox_levels", "voxfeatvec", "stg2voxvec", "voxvec_fuse"):
            del base[k]
        base["coords"], base["features"] = osparse.synth_cloud(2, 120, extent=20, seed=3)
    base = to_dev(base, dev)
    d_frames = dict(base, query_frames=torch.from_numpy(src).to(dev), query_jitter=torch.from_numpy(recs.copy()).to(dev))
    return d_frames, dict(base, query_image=torch.from_numpy(tiles.copy()).to(dev))


def _db_pair(dev, ndim, seed):
    """(db_frames + db_jitter, db_map = the reference's tiles) under db_cropsize = 75, db_resize = 64: 85x85 frames, origin 5"""
    shape = (3, 1, 85, 85, 3) if ndim == 5 else (2, 2, 1, 85, 85, 3)
    src = _frames(shape, seed)
    nfr = int(np.prod(shape[:-3]))
    recs = _records()[[7, 16, 29, 10][:nfr]]
    tiles = _ref_tiles(("db", ndim, seed), src, 75, (64, 64), recs)
    return ({"db_frames": torch.from_numpy(src).to(dev), "db_jitter": torch.from_numpy(recs.copy()).to(dev)},
            {"db_map": torch.from_numpy(tiles.copy()).to(dev)})


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "coords"])
def test_mm_inference_from_jittered_frames(dev, sparse):
    from agplace_amd.options import Options
    opt = Options(q_resize=64, q_jitter=0.4)
    model = _mm(dev, opt)
    d_frames, d_tiles = _query_pair(dev, opt, sparse, 71)
    want = {k: v.clone() for k, v in model(d_tiles, mode="q").items()}
    got = model(d_frames, mode="q")
    assert set(got) == set(model.OUT_KEYS)
    for k in model.OUT_KEYS:
        assert torch.equal(got[k], want[k]), k
    plain = model({k: v for k, v in d_frames.items() if k != "query_jitter"}, mode="q")
    assert not torch.equal(plain["embedding"], want["embedding"])              # (the jitter does something)


@pytest.mark.parametrize("ndim", [5, 6])
def test_dbvanilla2d_from_cropped_jittered_frames(dev, ndim):
    from agplace_amd.options import Options
    opt = Options(db_resize=64, db_cropsize=75, db_jitter=0.4)
    model = _db(dev, opt)
    d_frames, d_tiles = _db_pair(dev, ndim, 72)
    want = model(d_tiles, mode="db")["embedding"].clone()
    got = model(d_frames, mode="db")["embedding"]
    assert tuple(got.shape) == ((3, 256) if ndim == 5 else (2, 2, 256))
    assert torch.equal(got, want)
    # the crop alone (no records): the tiles of the window
    src = d_frames["db_frames"].cpu().numpy()
    tiles = camera_ref.resize_frames(colour_ref.center_crop(src, 75), 64, 64)
    want = model({"db_map": torch.from_numpy(tiles).to(dev)}, mode="db")["embedding"].clone()
    assert torch.equal(model({"db_frames": d_frames["db_frames"]}, mode="db")["embedding"], want)


def _loss_and_grads(model, d, key, G, extra=None):
    for p in model.parameters():
        p.grad = None
    out = model(d, mode=key)
    loss = (out["embedding"] * G).sum() if extra is None else (out["embedding"] * G).sum() + (out[extra] * G).sum()
    loss.backward()
    return loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


def test_mm_training_from_jittered_frames(dev):
    from agplace_amd.options import Options
    opt = Options(q_resize=64, q_jitter=0.4)
    model = _mm(dev, opt, train=True)
    d_frames, d_tiles = _query_pair(dev, opt, False, 73)
    G = torch.randn(2, 256, generator=torch.Generator().manual_seed(1)).to(dev)
    lt, gt = _loss_and_grads(model, d_tiles, "q", G, "stg2imagevec")
    lf, gf = _loss_and_grads(model, d_frames, "q", G, "stg2imagevec")
    assert torch.equal(lt, lf)
    assert "image_fe.fe.conv1.weight" in gt and set(gt) == set(gf)
    diff = [n for n in gt if not torch.equal(gt[n], gf[n])]
    assert not diff, diff[:8]


@pytest.mark.parametrize("ndim", [5, 6])
def test_dbvanilla2d_training_from_cropped_jittered_frames(dev, ndim):
    from agplace_amd.options import Options
    opt = Options(db_resize=64, db_cropsize=75, db_jitter=0.4)
    model = _db(dev, opt, train=True)
    d_frames, d_tiles = _db_pair(dev, ndim, 74)
    G = torch.randn((3, 256) if ndim == 5 else (2, 2, 256), generator=torch.Generator().manual_seed(2)).to(dev)
    lt, gt = _loss_and_grads(model, d_tiles, "db", G)
    lf, gf = _loss_and_grads(model, d_frames, "db", G)
    assert torch.equal(lt, lf)
    assert any(n.endswith("conv1.weight") for n in gt) and set(gt) == set(gf)
    diff = [n for n in gt if not torch.equal(gt[n], gf[n])]
    assert not diff, diff[:8]


def test_embed_pair_and_captured_pair_with_jitter(dev):
    from agplace_amd import pair
    from agplace_amd.options import Options
    opt = Options(q_resize=64, db_resize=64, db_cropsize=75, q_jitter=0.4, db_jitter=0.4)
    mq, mdb = _mm(dev, opt), _db(dev, opt)
    dq_frames, dq_tiles = _query_pair(dev, opt, False, 75)
    ddb_frames, ddb_tiles = _db_pair(dev, 5, 76)
    ddb_frames = {k: v[:2] for k, v in ddb_frames.items()}
    ddb_tiles = {k: v[:2] for k, v in ddb_tiles.items()}
    want_q, want_db = pair.embed_pair(mq, mdb, dq_tiles, ddb_tiles)
    want_q, want_db = {k: v.clone() for k, v in want_q.items()}, want_db["embedding"].clone()
    got_q, got_db = pair.embed_pair(mq, mdb, dq_frames, ddb_frames)
    for k in mq.OUT_KEYS:
        assert torch.equal(got_q[k], want_q[k]), k
    assert torch.equal(got_db["embedding"], want_db)
    # ---- capture once, then rewrite the records in place and replay
    dq = dict(dq_frames, query_jitter=dq_frames["query_jitter"].clone())
    ddb = dict(ddb_frames, db_jitter=ddb_frames["db_jitter"].clone())
    cp = pair.CapturedPair(mq, mdb, dq, ddb)
    recs = _records()
    for step, (qi, di) in enumerate([([0, 30, 9, 24], [18, 2]), ([35, 22, 4, 28], [31, 11])]):
        dq["query_jitter"].copy_(torch.from_numpy(recs[qi]).to(dev))
        ddb["db_jitter"].copy_(torch.from_numpy(recs[di]).to(dev))
        cp.replay()
        out_q, out_db = cp.finish()
        rep_q, rep_db = {k: v.clone() for k, v in out_q.items()}, out_db["embedding"].clone()
        eag_q, eag_db = pair.embed_pair(mq, mdb, dq, ddb)
        torch.cuda.synchronize()
        for k in mq.OUT_KEYS:
            assert torch.equal(rep_q[k], eag_q[k]), (step, k)
        assert torch.equal(rep_db, eag_db["embedding"]), step
        assert not torch.equal(rep_q["embedding"], want_q["embedding"]) and not torch.equal(rep_db, want_db)


@pytest.mark.parametrize("prec", [4, 2, 3])
def test_image_norm_reaches_the_uint8_tile_route(dev, prec):
    """Options.image_mean / image_std = 0.5 / 0.22: the trunk fed uint8 tiles (at prec 4 the walking stem reads them itself, tile
    width 64) equals the trunk fed pack_cameras_u8(tiles, mean, std) as a packed map; and differs from ImageNet's constants."""
    from agplace_amd import ops
    from agplace_amd.options import Options
    tiles = torch.from_numpy(_frames((2, 2, 64, 64, 3), 77)).to(dev)

    def last_map(model, x):
        m = model.image_fe.fe.forward_maps(x, prec=prec)[-1]
        return [p.clone() for p in _planes(m)]
    kitti = _mm(dev, Options(image_mean=KITTI_NORM[0], image_std=KITTI_NORM[1], mfma_precision=prec))
    got = last_map(kitti, tiles)
    want = last_map(kitti, ops.pack_cameras_u8(tiles, prec, *KITTI_NORM))
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    imagenet = _mm(dev, Options(mfma_precision=prec))
    assert not torch.equal(last_map(imagenet, tiles)[0], got[0])
    # the database model's trunks too
    dbk = _db(dev, Options(image_mean=KITTI_NORM[0], image_std=KITTI_NORM[1], mfma_precision=prec))
    fe = dbk.dbimage_fes[0].fe
    a = [p.clone() for p in _planes(fe.forward_maps(tiles[:, :1], prec=prec)[-1])]
    b = [p.clone() for p in _planes(fe.forward_maps(ops.pack_cameras_u8(tiles[:, :1], prec, *KITTI_NORM), prec=prec)[-1])]
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ errors
def test_errors(dev):
    from agplace_amd import ops, pair
    from agplace_amd.options import Options
    fr = torch.zeros((1, 1, 36, 72, 3), dtype=torch.uint8, device=dev)
    for f in (fr, fr.transpose(2, 3)):                       # a crop larger than the frame along either axis
        with pytest.raises(NotImplementedError, match="larger than the frame"):
            ops.resize_cameras_u8(f, 24, crop=37)
        with pytest.raises(NotImplementedError, match="larger than the frame"):
            ops.pack_cameras_resized_u8(f, 24, 4, crop=37)
    with pytest.raises(NotImplementedError, match="larger than the frame"):
        ops.center_crop_origin(36, 72, 37)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            ops.center_crop_origin(36, 72, bad)
    with pytest.raises(NotImplementedError, match="8-fold"):
        ops.resize_cameras_u8(fr, (4, 4), crop=36)            # a 9x reduction of the window
    mdb = _db(dev, Options(db_resize=24, db_cropsize=37))
    with pytest.raises(NotImplementedError, match="larger than the frame"):
        mdb({"db_frames": fr}, mode="db")
    # records: a wrong row count, a wrong width, a wrong dtype, on the host
    tiles = torch.zeros((2, 3, 8, 8, 3), dtype=torch.uint8, device=dev)
    good = torch.zeros((6, 8), dtype=torch.float32, device=dev)
    assert torch.equal(ops.jitter_cameras_u8(tiles, good), tiles)
    for bad in (good[:5], good[:, :7], good.double(), good.view(-1)):
        with pytest.raises(ValueError):
            ops.jitter_cameras_u8(tiles, bad)
        with pytest.raises(ValueError):
            ops.pack_cameras_jittered_u8(tiles, bad, 4)
    with pytest.raises(RuntimeError):
        ops.jitter_cameras_u8(tiles, good.cpu())
    with pytest.raises(ValueError):
        ops.jitter_cameras_u8(tiles.float(), good)
    # the models: a jitter key without its frames key, a wrong row count
    opt = Options(q_resize=64, db_resize=64)
    mq, mdb = _mm(dev, opt), _db(dev, opt)
    d_frames, d_tiles = _query_pair(dev, opt, False, 78)
    with pytest.raises(ValueError, match="needs `query_frames`"):
        mq(dict(d_tiles, query_jitter=d_frames["query_jitter"]), mode="q")
    with pytest.raises(ValueError, match="one record per frame"):
        mq(dict(d_frames, query_jitter=d_frames["query_jitter"][:3]), mode="q")
    dbf = torch.zeros((2, 1, 85, 85, 3), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="needs `db_frames`"):
        mdb({"db_map": torch.zeros((2, 1, 64, 64, 3), dtype=torch.uint8, device=dev), "db_jitter": good[:2]}, mode="db")
    with pytest.raises(ValueError, match="one record per frame"):
        mdb({"db_frames": dbf, "db_jitter": good[:3]}, mode="db")
    with pytest.raises(ValueError, match="needs `query_frames`"):
        pair.embed_pair(mq, mdb, dict(d_tiles, query_jitter=good[:4]), {"db_frames": dbf})
    with pytest.raises(ValueError, match="needs `db_frames`"):
        pair.embed_pair(mq, mdb, d_frames, {"db_map": torch.zeros((2, 1, 64, 64, 3), dtype=torch.uint8, device=dev), "db_jitter": good[:2]})
    with pytest.raises(ValueError):
        pair.embed_pair(mq, mdb, dict(d_frames, query_jitter=good[:3]), {"db_frames": dbf})
