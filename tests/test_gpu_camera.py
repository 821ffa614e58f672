"""-m gpu tests of the camera front end (csrc/camera.hip): decoded uint8 frames resized on the device with Pillow's
arithmetic.  Everything is exact (torch.equal): the uint8 mode against the numpy restatement tests/camera_ref.py (which
tests/test_camera_ref.py holds to Pillow itself), the fused packed mode against resize + pack_cameras_u8, and the models fed
`query_frames` / `db_frames` against the same models fed the resized uint8 tiles."""
import numpy as np
import pytest
import torch

import camera_ref
from gpu_util import randomize_bn, to_dev
from oracle import nets
from oracle import sparse as osparse

pytestmark = pytest.mark.gpu

# (n, ncam, H0, W0, h, w).  The kernel's output tile is 16 rows x 64 columns, its stage buffer holds >= 10 patch rows.
U8_GEOMETRIES = [
    (2, 2, 256, 455, 192, 341),      # the nuScenes frame under Resize(192)
    (1, 2, 37, 53, 16, 22),
    (1, 1, 20, 31, 20, 17),          # rows unchanged
    (1, 1, 9, 9, 9, 9),              # both axes unchanged
    (1, 2, 16, 24, 32, 48),          # 2x enlargement
    (1, 1, 300, 300, 256, 256),
    (1, 1, 5, 64, 3, 38),
    (1, 1, 256, 455, 256, 455),      # identity at full size
    (1, 1, 64, 64, 16, 16),          # 4x reduction, 9 taps
    (1, 1, 8, 8, 32, 32),            # 4x enlargement
    (2, 1, 70, 130, 33, 67),         # 3 x 2 tiles, neither axis a multiple of the tile
    (1, 1, 5, 7, 1, 1),              # one output row and column
    (1, 2, 136, 600, 17, 75),        # 8x reduction: 17 taps, the widest patch, staged in many chunks; 2 x 2 tiles
    (1, 1, 9, 200, 72, 25),          # 8x enlargement of the rows beside an 8x reduction of the columns
]


def _frames(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


_REF = {}


def _ref_tiles(frames, h, w, key):
    """camera_ref's resize of `frames`, computed once per key and shared (read-only)."""
    if key not in _REF:
        out = camera_ref.resize_frames(frames, h, w)
        out.setflags(write=False)
        _REF[key] = out
    return _REF[key]


@pytest.fixture(autouse=True)
def _no_grad(request):
    if "training" in request.node.name:
        yield
    else:
        with torch.no_grad():
            yield


@pytest.mark.parametrize("geo", U8_GEOMETRIES, ids=lambda g: "%dx%dx%dx%d-%dx%d" % g)
def test_u8_mode_equals_camera_ref(dev, geo):
    from agplace_amd import ops
    n, ncam, h0, w0, h, w = geo
    src = _frames((n, ncam, h0, w0, 3), 11)
    if (h0, w0) == (5, 7):
        src[:] = 255                 # the accumulator's top edge
    want = torch.from_numpy(_ref_tiles(src, h, w, ("u8",) + geo).copy())
    got = ops.resize_cameras_u8(torch.from_numpy(src).to(dev), (h, w))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (n, ncam, h, w, 3)
    diff = int((got.cpu() != want).sum())
    assert torch.equal(got.cpu(), want), (geo, diff)


def test_u8_mode_int_size_and_unaligned_base(dev):
    """Resize(int)'s rule through the op, and frames whose first byte is not 16-byte aligned (a view one byte into a buffer)."""
    from agplace_amd import ops
    src = _frames((1, 2, 37, 53, 3), 12)
    want = torch.from_numpy(_ref_tiles(src, *camera_ref.resized_size(37, 53, 16), ("int", 16)).copy())
    assert ops.resized_size(37, 53, 16) == camera_ref.resized_size(37, 53, 16) == (16, 22)
    buf = torch.zeros(src.size + 64, dtype=torch.uint8, device=dev)
    for shift in (1, 7, 16):
        fr = buf[shift:shift + src.size].view(src.shape)
        fr.copy_(torch.from_numpy(src))
        assert torch.equal(ops.resize_cameras_u8(fr, 16).cpu(), want), shift


def _planes(m):
    return [p.view(torch.int16) for p in (m.hi, m.lo) if p is not None]


@pytest.mark.parametrize("prec", [3, 2, 4])
@pytest.mark.parametrize("ncam,meanstd", [(1, None), (3, None), (3, ((0.5, 0.5, 0.5), (0.22, 0.22, 0.22)))],
                         ids=["1cam", "3cam", "3cam-kitti"])
def test_packed_mode_equals_resize_then_pack(dev, prec, ncam, meanstd):
    from agplace_amd import ops
    fr = torch.from_numpy(_frames((2, ncam, 70, 130, 3), 13)).to(dev)
    h, w = 33, 67
    kw = {} if meanstd is None else {"mean": meanstd[0], "std": meanstd[1]}
    want = ops.pack_cameras_u8(ops.resize_cameras_u8(fr, (h, w)), prec, **kw)
    got = ops.pack_cameras_resized_u8(fr, (h, w), prec, **kw)
    assert (got.n, got.h, got.w, got.c, got.pad) == (2, h, ncam * w, 4, 3) and (got.lo is None) == (prec != 3)
    for a, b in zip(_planes(got), _planes(want)):
        assert torch.equal(a, b)
        # the halo still holds the zeros SplitMap.alloc put there
        inner = torch.zeros_like(a, dtype=torch.bool)
        inner[:, 3:3 + h, 3:3 + ncam * w] = True
        assert int((a[~inner] != 0).sum()) == 0
        assert int((a[..., 3] != 0).sum()) == 0       # the 4th channel
    if meanstd is not None:                           # (and the normalisation really is another one)
        other = ops.pack_cameras_resized_u8(fr, (h, w), prec)
        assert not torch.equal(_planes(other)[0], _planes(got)[0])


def _mm(dev, opt, seed=5, train=False):
    from agplace_amd.network_mm.mm import MM
    torch.manual_seed(seed)
    m = randomize_bn(MM(opt=opt)).to(dev)
    return m.train() if train else m.eval()


def _query_pair(dev, opt, h0, w0, sparse, seed):
    """(data with query_frames, data with query_image = camera_ref's resized tiles), 2 samples x 2 cameras"""
    src = _frames((2, 2, h0, w0, 3), seed)
    h, w = camera_ref.resized_size(h0, w0, opt.q_resize)
    tiles = _ref_tiles(src, h, w, ("mm", h0, w0, seed))
    base = nets.synth_query(2, h, 2 * w, opt, seed=seed)
    del base["query_image"]
    if sparse:
        for k in ("vox_levels", "voxfeatvec", "stg2voxvec", "voxvec_fuse"):
            del base[k]
        base["coords"], base["features"] = osparse.synth_cloud(2, 120, extent=20, seed=3)
    base = to_dev(base, dev)
    return dict(base, query_frames=torch.from_numpy(src).to(dev)), dict(base, query_image=torch.from_numpy(tiles.copy()).to(dev))


@pytest.mark.parametrize("h0,w0,hw", [(85, 85, (64, 64)), (80, 120, (64, 96))], ids=["85x85", "80x120"])
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "coords"])
def test_mm_inference_from_query_frames(dev, h0, w0, hw, sparse):
    from agplace_amd.options import Options
    opt = Options(q_resize=64)
    assert camera_ref.resized_size(h0, w0, 64) == hw
    model = _mm(dev, opt)
    d_frames, d_tiles = _query_pair(dev, opt, h0, w0, sparse, 21)
    want = {k: v.clone() for k, v in model(d_tiles, mode="q").items()}
    got = model(d_frames, mode="q")
    assert set(got) == set(model.OUT_KEYS)
    for k in model.OUT_KEYS:
        assert torch.equal(got[k], want[k]), k


def _db(dev, opt, seed=6, train=False):
    from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
    torch.manual_seed(seed)
    m = randomize_bn(DBVanilla2D("db", opt.features_dim, opt=opt)).to(dev)
    return m.train() if train else m.eval()


@pytest.mark.parametrize("ndim", [5, 6])
def test_dbvanilla2d_from_db_frames(dev, ndim):
    from agplace_amd.options import Options
    opt = Options(db_resize=64)
    model = _db(dev, opt)
    shape = (3, 1, 85, 85, 3) if ndim == 5 else (2, 2, 1, 85, 85, 3)
    src = _frames(shape, 22)
    tiles = _ref_tiles(src, 64, 64, ("db", ndim))
    want = model({"db_map": torch.from_numpy(tiles.copy()).to(dev)}, mode="db")["embedding"].clone()
    got = model({"db_frames": torch.from_numpy(src).to(dev)}, mode="db")["embedding"]
    assert tuple(got.shape) == ((3, 256) if ndim == 5 else (2, 2, 256))
    assert torch.equal(got, want)


def test_mm_training_from_query_frames(dev):
    """.train() forward + backward (the default tight mode): the stem's input map is the same bits either way, and the training
    graph is bit-repeatable, so the loss and every parameter gradient are equal."""
    from agplace_amd.options import Options
    opt = Options(q_resize=64)
    model = _mm(dev, opt, train=True)
    d_frames, d_tiles = _query_pair(dev, opt, 85, 85, False, 23)
    G = torch.randn(2, 256, generator=torch.Generator().manual_seed(1)).to(dev)

    def run(d):
        for p in model.parameters():
            p.grad = None
        out = model(d, mode="q")
        loss = (out["embedding"] * G).sum() + (out["stg2imagevec"] * G).sum()
        loss.backward()
        return loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    lt, gt = run(d_tiles)
    lf, gf = run(d_frames)
    assert torch.equal(lt, lf)
    # (dense voxel stand-ins: the voxel branch has no gradients; the image trunk, which the frames feed, has all of its own)
    assert "image_fe.fe.conv1.weight" in gt and sum(n.startswith("image_fe.") for n in gt) > 40 and set(gt) == set(gf)
    diff = [n for n in gt if not torch.equal(gt[n], gf[n])]
    assert not diff, diff[:8]


def test_embed_pair_and_graph_capture_from_frames(dev):
    from agplace_amd import ops, pair
    from agplace_amd.options import Options
    opt = Options(q_resize=64, db_resize=64)
    mq, mdb = _mm(dev, opt), _db(dev, opt)
    d_frames, _ = _query_pair(dev, opt, 85, 85, False, 24)
    db = {"db_frames": torch.from_numpy(_frames((2, 1, 85, 85, 3), 25)).to(dev)}
    want_q = {k: v.clone() for k, v in mq(d_frames, mode="q").items()}
    want_db = mdb(db, mode="db")["embedding"].clone()
    got_q, got_db = pair.embed_pair(mq, mdb, d_frames, db)
    for k in mq.OUT_KEYS:
        assert torch.equal(got_q[k], want_q[k]), k
    assert torch.equal(got_db["embedding"], want_db)
    with pytest.raises(ValueError, match="not both"):
        pair.embed_pair(mq, mdb, dict(d_frames, query_image=torch.zeros(2, 3, 64, 128, device=dev)), db)
    # ---- forward_q(query_frames) in one hipGraph: tables prepared, one eager warm-up on the capture stream, the static frame
    # buffer refilled twice
    ops.prepare_resize(85, 85, 64, 64, dev)
    st = torch.cuda.Stream(device=dev)
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        mq(d_frames, mode="q")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        out = mq(d_frames, mode="q")
    for seed in (31, 32):
        new = torch.from_numpy(_frames((2, 2, 85, 85, 3), seed)).to(dev)
        d_frames["query_frames"].copy_(new)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        rep = {k: v.clone() for k, v in out.items()}
        with torch.cuda.stream(st):
            eager = mq(dict(d_frames, query_frames=new), mode="q")
        torch.cuda.synchronize()
        for k in mq.OUT_KEYS:
            assert torch.equal(rep[k], eager[k]), (seed, k)
        assert not torch.equal(rep["embedding"], want_q["embedding"])


def test_errors(dev):
    from agplace_amd import ops
    from agplace_amd.options import Options
    fr = torch.zeros((1, 1, 72, 72, 3), dtype=torch.uint8, device=dev)
    with pytest.raises(NotImplementedError, match="8-fold"):
        ops.resize_cameras_u8(fr, (8, 72))                       # a 9x reduction of the rows
    with pytest.raises(NotImplementedError, match="8-fold"):
        ops.pack_cameras_resized_u8(fr, (72, 8), 4)
    assert tuple(ops.resize_cameras_u8(fr, (9, 9)).shape) == (1, 1, 9, 9, 3)      # 8x is supported
    for bad in (fr.float(), fr[0], fr[..., :2]):
        with pytest.raises(ValueError):
            ops.resize_cameras_u8(bad, 64)
        with pytest.raises(ValueError):
            ops.pack_cameras_resized_u8(bad, 64, 4)
    opt = Options(q_resize=64)
    model = _mm(dev, opt)
    d_frames, d_tiles = _query_pair(dev, opt, 85, 85, False, 26)
    with pytest.raises(ValueError, match="not both"):
        model(dict(d_frames, query_image=d_tiles["query_image"]), mode="q")
    with pytest.raises(ValueError, match="query_frames"):
        model(dict(d_frames, query_frames=d_frames["query_frames"].float()), mode="q")
    with pytest.raises(ValueError, match="query_frames"):
        model(dict(d_frames, query_frames=d_frames["query_frames"][0]), mode="q")
    with pytest.raises(NotImplementedError):
        model(dict(d_frames, query_frames=torch.zeros((2, 2, 600, 600, 3), dtype=torch.uint8, device=dev)), mode="q")   # 600 -> 64: 9.4x
    mdb = _db(dev, Options(db_resize=64))
    with pytest.raises(ValueError, match="not both"):
        mdb({"db_frames": fr, "db_map": torch.zeros(1, 1, 3, 64, 64, device=dev)}, mode="db")
    with pytest.raises(ValueError, match="db_frames"):
        mdb({"db_frames": fr.float()}, mode="db")
    # a geometry nobody prepared, first met inside a capture: the table lookup raises before anything is launched
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="prepare_resize"):
        with torch.cuda.graph(g):
            ops.resize_tables(123, 45, dev)
    torch.cuda.synchronize()
    ops.prepare_resize(123, 77, 45, 33, dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        k, b = ops.resize_tables(123, 45, dev)                  # cached now: fine inside a capture
    assert tuple(k.shape) == (45, camera_ref.ksize(123, 45)) and tuple(b.shape) == (45, 2)
