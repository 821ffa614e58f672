"""The lidar front end on the device (csrc/coords.hip: agp_sparse_build_points; specification DESIGN.md section 1c): raw points ->
level 0 of the sparse tensor, against the numpy restatement tests/lidar_ref.py run through SparseTensor.from_coords.  Integer
outputs (keys, segment offsets, batch indices, row count) are compared bit for bit, features must be 1."""
import math

import numpy as np
import pytest
import torch

import lidar_ref as R

pytestmark = pytest.mark.gpu
SENT = 0x7fffffffffffffff


def _rot(deg):
    from agplace_amd.input_pipeline import z_rotation
    return z_rotation(math.radians(deg))


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _build(dev, pts, off, nbatch, quant, rot=None, ws=None):
    from agplace_amd import ops
    from agplace_amd.sparse import SparseTensor
    return SparseTensor.from_points_capacity(torch.as_tensor(pts, dtype=torch.float32).to(dev), torch.as_tensor(off).to(dev), nbatch, quant,
                                             ws or ops.Workspace(), None if rot is None else rot.to(dev))


def _expect(dev, pts, off, nbatch, quant, rot=None):
    """(exact-size SparseTensor of the restatement's rows, flagged)"""
    from agplace_amd.sparse import SparseTensor
    coords, flagged = R.voxelise(pts, off, quant, None if rot is None else rot.numpy())
    c = torch.from_numpy(coords).to(dev)
    return SparseTensor.from_coords(torch.ones((c.shape[0], 1), device=dev), c, nbatch=nbatch), flagged


def _check(sp, ex, flagged):
    n = int(sp.n_dev.item())
    assert n == ex.n
    assert torch.equal(sp.keys[:n], ex.keys) and bool((sp.keys[n:] == SENT).all())
    so, bi = sp.segments()
    so_e, bi_e = ex.segments()
    assert torch.equal(so, so_e) and torch.equal(bi[:n], bi_e) and bool((bi[n:] == 0).all())
    assert bool((sp.f32[:n] == 1.0).all()) and tuple(sp.f32.shape) == (sp.n, 1)
    assert int(sp.range_flag.item()) == (1 if flagged else 0)
    return n


@pytest.fixture(scope="module")
def ragged():
    """B = 4, sample sizes (0, 1, 70 000, 3 000): an empty sample, a sample of more points than agp_sparse_build accepts (65536)
    whose 70 000 points fall into fewer than 16384 voxels (the LDS sort), in a box of 80 x 80 x 8 m at quant_size 2."""
    g = np.random.default_rng(21)
    sizes = (0, 1, 70000, 3000)
    pts = (g.random((sum(sizes), 3), dtype=np.float32) * np.float32([80, 80, 8]) - np.float32([40, 40, 4])).astype(np.float32)
    off = _offsets(sizes)
    nvox = len(R.voxelise(pts[off[2]:off[3]], [0, sizes[2]], 2.0)[0])
    assert 4096 < nvox < 16384, nvox
    return pts, off


def test_ragged_samples_empty_single_and_more_points_than_the_coords_path_takes(dev, ragged):
    pts, off = ragged
    sp = _build(dev, pts, off, 4, 2.0)
    n = _check(sp, *_expect(dev, pts, off, 4, 2.0))
    so = sp.segments()[0].tolist()
    assert so[0] == so[1] == 0 and so[2] == 1 and so[4] == n and sp.n == pts.shape[0]
    # the same cloud with a shared and with a per-sample rotation, against the restatement
    r5 = _rot(5.0)
    _check(_build(dev, pts, off, 4, 2.0, r5), *_expect(dev, pts, off, 4, 2.0, r5))
    rb = torch.stack([_rot(a) for a in (0.0, -5.0, 3.3, 1.7)])
    sp_b = _build(dev, pts, off, 4, 2.0, rb)
    ex_b, fl = _expect(dev, pts, off, 4, 2.0, rb)
    _check(sp_b, ex_b, fl)
    assert not torch.equal(ex_b.keys, _expect(dev, pts, off, 4, 2.0, r5)[0].keys)        # (the matrices do differ)
    # an identity matrix is the run without rotation, bit for bit
    sp_i = _build(dev, pts, off, 4, 2.0, torch.eye(3))
    assert torch.equal(sp_i.keys, sp.keys) and torch.equal(sp_i.segments()[0], sp.segments()[0])
    assert torch.equal(sp_i.segments()[1], sp.segments()[1]) and int(sp_i.range_flag.item()) == 0


def test_same_address_contention_70000_points_in_40_voxels(dev):
    g = np.random.default_rng(22)
    pts = (g.random((70000, 3), dtype=np.float32) * np.float32([8, 10, 4])).astype(np.float32)
    off = _offsets((70000,))
    n = _check(_build(dev, pts, off, 1, 2.0), *_expect(dev, pts, off, 1, 2.0))
    assert n == 4 * 5 * 2


def test_hash_probing_near_the_design_load_and_the_global_memory_sort(dev):
    """16 000 points in 16 000 distinct voxels (a table of 2^16 slots for 36 000 rows: every insert a new key), and a second sample
    of 20 000 distinct voxels, more than one workgroup sorts in LDS."""
    g = np.random.default_rng(23)
    cells = np.stack(np.meshgrid(np.arange(-14, 14), np.arange(-14, 14), np.arange(-13, 14), indexing="ij"), -1).reshape(-1, 3)
    a = cells[g.permutation(len(cells))[:16000]]
    b = cells[g.permutation(len(cells))[:20000]]
    pts = ((np.concatenate([a, b]) + 0.5) * 2.0).astype(np.float32)
    off = _offsets((16000, 20000))
    n = _check(_build(dev, pts, off, 2, 2.0), *_expect(dev, pts, off, 2, 2.0))
    assert n == 36000
    # one sample alone at the design load: 16 000 keys in 2^15 slots
    n = _check(_build(dev, pts[:16000], off[:2], 1, 2.0), *_expect(dev, pts[:16000], off[:2], 1, 2.0))
    assert n == 16000


def test_rows_beyond_the_last_offset_are_ignored_and_raise_no_flag(dev):
    g = np.random.default_rng(24)
    pts = (g.random((5000, 3), dtype=np.float32) * 60 - 30).astype(np.float32)
    pts[3100:] = np.float32([np.nan, 1e30, -np.inf])
    pts[4000:] = np.float32(3e38)
    off = _offsets((1000, 0, 2100))
    sp = _build(dev, pts, off, 3, 2.0, _rot(-4.0))
    n = _check(sp, *_expect(dev, pts[:3100], off, 3, 2.0, _rot(-4.0)))
    assert 0 < n < 3100 and sp.n == 5000 and int(sp.range_flag.item()) == 0


@pytest.mark.parametrize("quant", [2.0, 1.0, 0.3])
def test_quantisation_equals_the_coords_path_on_host_made_coords(dev, quant):
    """Points on exact voxel boundaries (k * quant_size in fp32, both signs), just below them, negative coordinates and -0.0; at
    quant_size 0.3 the boundary points are the ones where an fp64 division lands in the neighbouring voxel."""
    from agplace_amd import ops
    from agplace_amd.sparse import SparseTensor
    g = np.random.default_rng(25)
    k = np.arange(-60, 61)
    edge = (k * quant).astype(np.float32)
    below = np.nextafter(edge, np.float32(-np.inf))
    axis = np.concatenate([edge, below, np.float32([-0.0, 0.0, 4.5, -4.5])])
    pts = np.stack([g.choice(axis, 4000), g.choice(axis, 4000), g.choice(axis, 4000)], 1).astype(np.float32)
    pts[::7] = (g.random((len(pts[::7]), 3), dtype=np.float32) * 40 - 30) * np.float32(quant)
    off = _offsets((1500, 2500))
    if quant == 0.3:
        q32 = np.floor(edge / np.float32(0.3))
        assert int((q32 != np.floor(edge.astype(np.float64) / 0.3)).sum()) >= 10
    sp = _build(dev, pts, off, 2, quant)
    n = _check(sp, *_expect(dev, pts, off, 2, quant))
    host = torch.from_numpy(R.per_point(pts, off, quant)).to(dev)
    cp = SparseTensor.from_coords_capacity(torch.ones((host.shape[0], 1), device=dev), host, 2, ops.Workspace())
    assert int(cp.n_dev.item()) == n and torch.equal(cp.keys, sp.keys)
    assert torch.equal(cp.segments()[0], sp.segments()[0]) and torch.equal(cp.segments()[1], sp.segments()[1])
    assert torch.equal(cp.f32[:n], sp.f32[:n])


def test_voxels_that_collide_after_the_rotation_merge(dev):
    cells = np.stack(np.meshgrid(np.arange(-15, 16), np.arange(-15, 16), np.arange(0, 2), indexing="ij"), -1).reshape(-1, 3)
    pts = ((cells + 0.5) * 2.0).astype(np.float32)
    pts = np.concatenate([pts, pts[::3]])                       # duplicates as well
    off = _offsets((len(pts),))
    r5 = _rot(5.0)
    rows, _ = R.voxelise(pts, off, 2.0, r5.numpy())
    assert len(rows) == len(cells) and len(R.merged(rows)) < len(rows)          # the restatement shows merges
    plain = _check(_build(dev, pts, off, 1, 2.0), *_expect(dev, pts, off, 1, 2.0))
    rotated = _check(_build(dev, pts, off, 1, 2.0, r5), *_expect(dev, pts, off, 1, 2.0, r5))
    assert plain == len(cells) and rotated == len(R.merged(rows)) < plain


def test_dropped_rows_raise_the_flag_and_leave_the_rest_untouched(dev):
    from agplace_amd import ops
    g = np.random.default_rng(26)
    good = (g.random((3000, 3), dtype=np.float32) * 50 - 25).astype(np.float32)
    good[(R.quantise(good, 2.0)[0] == 0).all(1)] = np.float32(10.0)      # nothing in the origin voxel: a dropped row must not appear there
    pts = good.copy()
    bad = np.insert(pts, [700, 2200], np.float32([[1.0, np.nan, 2.0], [1.0, 2.0, 70000.0]]), axis=0)
    off_good, off_bad = _offsets((1200, 1800)), _offsets((1201, 1801))
    ws = ops.Workspace()
    sp = _build(dev, bad, off_bad, 2, 2.0, ws=ws)
    ex, flagged = _expect(dev, bad, off_bad, 2, 2.0)
    assert flagged
    _check(sp, ex, True)
    ex_good, fl_good = _expect(dev, good, off_good, 2, 2.0)
    assert not fl_good and torch.equal(ex.keys, ex_good.keys)                    # = the cloud with those two rows removed
    assert not bool((ex.keys == ((32768 << 32) | (32768 << 16) | 32768)).any())
    # each kind alone; the flag describes THIS build: a clean cloud through the same workspace clears it
    for row in ([np.inf, 0.0, 0.0], [0.0, -65024.0, 0.0]):
        one = np.insert(pts, [5], np.float32([row]), axis=0)
        sp1 = _build(dev, one, _offsets((1201, 1800)), 2, 2.0, ws=ws)
        assert int(sp1.range_flag.item()) == 1 and torch.equal(sp1.keys[:ex_good.n], ex_good.keys)
    spc = _build(dev, np.concatenate([good, good[:2]]), off_good, 2, 2.0, ws=ws)
    _check(spc, ex_good, False)
    # a rotated voxel that leaves the key range is dropped and flagged like a raw one
    far = np.insert(pts, [9], np.float32([[60000.0, 60000.0, 0.0]]), axis=0)
    r45 = torch.tensor([[1.0, 1.0, 0.0], [-1.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    spr = _build(dev, far, _offsets((1201, 1800)), 2, 2.0, r45)
    _check(spr, *_expect(dev, far, _offsets((1201, 1800)), 2, 2.0, r45))
    assert int(spr.range_flag.item()) == 1


def test_entry_point_rejects_bad_arguments(dev):
    from agplace_amd import _lib
    from agplace_amd._lib import ptr
    L = _lib.load()
    n, nb = 64, 2
    pts = torch.zeros((n, 3), device=dev)
    off = torch.tensor([0, 10, 64], device=dev)
    keys, f = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, device=dev)
    seg, bidx = torch.empty(nb + 1, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    nbytes = L.agp_sparse_points_workspace_bytes(n, nb)
    tmp = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def call(points=pts, offsets=off, cap=n, nbatch=nb, quant=2.0, per=0, k=keys, fo=f, wsb=nbytes):
        return L.agp_sparse_build_points(ptr(points), ptr(offsets), cap, nbatch, quant, None, per, ptr(k), ptr(fo), ptr(seg), ptr(bidx),
                                         ptr(flag), ptr(tmp), wsb, _lib.stream())
    assert call() == 0
    for kw in (dict(points=None), dict(offsets=None), dict(k=None), dict(fo=None), dict(quant=0.0), dict(quant=-1.0),
               dict(quant=float("nan")), dict(quant=float("inf")), dict(nbatch=0), dict(nbatch=0x7fff), dict(cap=0), dict(cap=1 << 30),
               dict(per=2), dict(wsb=nbytes - 1)):
        assert call(**kw) == 1, kw
    torch.cuda.synchronize()


def test_training_levels_from_points_equal_those_from_coords(dev, ragged):
    from agplace_amd.sparse import SparseTensor
    pts, off = ragged
    # (the coords path takes at most 65536 points per sample: the 70 000-point sample enters it deduplicated, as the restatement's rows)
    for rot in (None, torch.stack([_rot(a) for a in (0.0, -5.0, 3.3, 1.7)])):
        a = SparseTensor.from_points_levels(torch.from_numpy(pts).to(dev), torch.from_numpy(off).to(dev), 4, 3, 2.0,
                                            None if rot is None else rot.to(dev))
        rows, _ = R.voxelise(pts, off, 2.0, None if rot is None else rot.numpy())
        c = torch.from_numpy(rows).to(dev)
        b = SparseTensor.from_coords_levels(torch.ones((c.shape[0], 1), device=dev), c, 4, 3)
        for lvl in range(4):
            assert a.n == b.n and a.stride == b.stride == 1 << lvl and torch.equal(a.keys, b.keys)
            assert torch.equal(a.segments()[0], b.segments()[0]) and torch.equal(a.segments()[1], b.segments()[1])
            if lvl == 0:
                assert torch.equal(a.f32, b.f32) and bool((a.f32 == 1.0).all())
            if lvl < 3:
                a, b = a.strided()[0], b.strided()[0]
    bad = pts.copy()
    bad[10] = np.float32([np.nan, 0, 0])
    with pytest.raises(ValueError, match="out of the"):
        SparseTensor.from_points_levels(torch.from_numpy(bad).to(dev), torch.from_numpy(off).to(dev), 4, 3, 2.0)


def _scan(seed, sizes, extent=30.0):
    g = np.random.default_rng(seed)
    pts = (g.random((sum(sizes), 3), dtype=np.float32) * np.float32([2 * extent, 2 * extent, 6]) - np.float32([extent, extent, 3]))
    return pts.astype(np.float32), _offsets(sizes)


def _query(dev, opt, seed):
    from oracle import nets
    data = nets.synth_query(2, 64, 128, opt, seed=seed)
    for k in ("vox_levels", "voxfeatvec", "stg2voxvec", "voxvec_fuse"):
        data.pop(k)
    return {k: v.to(dev) for k, v in data.items()}


def test_mm_forward_from_points_equals_forward_from_host_made_coords(dev):
    """MM.forward_q from `points` / `point_offsets` / `pc_rotation` against the same forward from the `coords` the host chain
    makes of them (one row per point, so both builds have the same capacity): every output bit-equal in eval mode; in .train()
    mode the outputs and the gradient of the voxel trunk's first convolution are equal."""
    from agplace_amd.network_mm.mm import MM
    from agplace_amd.options import Options
    opt = Options(mfma_precision=4)
    assert opt.quant_size == 2.0
    torch.manual_seed(5)
    model = MM(opt=opt).to(dev).eval()
    base = _query(dev, opt, 5)
    pts, off = _scan(31, (900, 600))
    rot = torch.stack([_rot(4.0), _rot(-2.5)])
    host = torch.from_numpy(R.per_point(pts, off, opt.quant_size, rot.numpy())).to(dev)
    d_pts = dict(base, points=torch.from_numpy(pts).to(dev), point_offsets=torch.from_numpy(off).to(dev), pc_rotation=rot.to(dev))
    d_crd = dict(base, coords=host.double(), features=torch.ones((host.shape[0], 1), device=dev))
    with torch.no_grad():
        a, b = model(d_pts, mode="q"), model(d_crd, mode="q")
        torch.cuda.synchronize()
        for k in b:
            assert torch.equal(a[k], b[k]), k
        assert float(a["voxvec_org"].abs().max()) > 0
        assert model.voxel_coords_in_range()
    model.train()
    w = model.vox_fe.conv0.kernel
    grads, outs = [], []
    for d in (d_pts, d_crd):
        model.zero_grad(set_to_none=True)
        out = model(d, mode="q")
        out["embedding"].square().sum().backward()
        grads.append(w.grad.clone())
        outs.append(out["embedding"].detach().clone())
    assert torch.equal(outs[0], outs[1]) and float(grads[0].abs().max()) > 0
    assert torch.equal(grads[0], grads[1])


def test_mm_forward_from_points_in_one_hipgraph_replays_scans_of_any_length(dev):
    """forward_q from a fixed-capacity `points` buffer captured in ONE hipGraph (warm-up on the capture stream, like
    pair.CapturedPair), replayed with three scans of different lengths copied into it.  Every replay equals the eager forward
    bit for bit.  The second scan holds one out-of-range point: an eager forward from it raises before it returns, so its replay
    is compared with the eager forward from the same scan WITHOUT that row (a dropped row leaves no trace), and
    poll_voxel_range reports that replay and no other."""
    from agplace_amd.network_mm.mm import MM
    from agplace_amd.options import Options
    opt = Options(mfma_precision=4)
    torch.manual_seed(6)
    model = MM(opt=opt).to(dev).eval()
    cap = 1500
    d = _query(dev, opt, 6)
    d["points"] = torch.full((cap, 3), float("nan"), device=dev)
    d["point_offsets"] = torch.zeros(3, dtype=torch.int64, device=dev)
    d["pc_rotation"] = _rot(3.0).to(dev)
    scans = [_scan(41, (700, 500)), _scan(42, (300, 401), extent=12.0), _scan(43, (800, 700))]
    pts_bad = np.insert(scans[1][0], [350], np.float32([[0.0, 1e6, 0.0]]), axis=0)
    off_bad = _offsets((300, 402))

    def load(dst, pts, off):
        dst["points"][:len(pts)].copy_(torch.from_numpy(pts))
        dst["point_offsets"].copy_(torch.from_numpy(off))
    with torch.no_grad():
        load(d, *scans[0])
        st = torch.cuda.Stream(device=dev)
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            for _ in range(2):
                model(d, mode="q")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            out = model(d, mode="q")
        e = dict(d, points=d["points"].clone(), point_offsets=d["point_offsets"].clone())
        seen = []
        for i, (pts, off) in enumerate([scans[0], (pts_bad, off_bad), scans[2]]):
            load(d, pts, off)
            load(e, *scans[i])
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            rep = {k: v.clone() for k, v in out.items()}
            try:
                model.poll_voxel_range()
                seen.append(False)
            except ValueError as err:
                assert "voxel coordinate" in str(err)
                seen.append(True)
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                eager = model(e, mode="q")
            torch.cuda.synchronize()
            for k in rep:
                assert torch.equal(rep[k], eager[k]), (i, k)
        assert seen == [False, True, False]
        reps = []
        for i in (0, 2):                                            # other lengths do give other descriptors
            load(d, *scans[i])
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            reps.append(out["embedding"].clone())
        assert not torch.equal(reps[0], reps[1])
        assert model.voxel_coords_in_range()


def test_drop_pc_from_points_is_one_origin_voxel_per_sample_like_zeroed_coords(dev):
    """MM(drop='pc') (reference mm.py:73: coordinates times zero) from raw scans: the points are multiplied by zero, every sample
    becomes its origin voxel -- bit-equal to the same model from the host-made coords."""
    from agplace_amd.network_mm.mm import MM
    from agplace_amd.options import Options
    opt = Options(mfma_precision=4)
    torch.manual_seed(8)
    model = MM(drop="pc", opt=opt).to(dev).eval()
    base = _query(dev, opt, 8)
    pts, off = _scan(51, (400, 300))
    host = torch.from_numpy(R.per_point(pts, off, opt.quant_size)).to(dev)
    with torch.no_grad():
        a = model(dict(base, points=torch.from_numpy(pts).to(dev), point_offsets=torch.from_numpy(off).to(dev), pc_rotation=_rot(5.0).to(dev)),
                  mode="q")
        b = model(dict(base, coords=host.double(), features=torch.ones((host.shape[0], 1), device=dev)), mode="q")
        torch.cuda.synchronize()
    for k in b:
        assert torch.equal(a[k], b[k]), k
    assert model.voxel_coords_in_range()
