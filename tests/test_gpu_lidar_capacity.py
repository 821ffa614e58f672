"""The level capacity of the raw-points route on the device (csrc/coords.hip: agp_sparse_build_points_cap).
A build that fits is compared BIT FOR BIT with the uncapped build of the same cloud (SparseTensor.from_points_capacity without the
argument, itself pinned to tests/lidar_ref.py by test_gpu_lidar.py); an overflowing build must come out empty with bit 2 of the
flag.  The cloud is the `ragged` fixture of test_gpu_lidar.py: sample sizes (0, 1, 70 000, 3 000), seed 21, a box of 80 x 80 x 8 m at
quant_size 2 -- A = 8780 distinct cells (0 / 1 / 6400 / 2379 per sample), checked against lidar_ref.voxelise below."""
import math

import numpy as np
import pytest
import torch

import lidar_ref as R

pytestmark = pytest.mark.gpu
SENT = 0x7fffffffffffffff
A_CLOUD = 8780
QUANT = 2.0


def _rot(deg):
    from agplace_amd.input_pipeline import z_rotation
    return z_rotation(math.radians(deg))


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


ROTS = {"none": lambda: None, "shared": lambda: _rot(5.0), "per_sample": lambda: torch.stack([_rot(a) for a in (0.0, -5.0, 3.3, 1.7)])}


def _build(dev, pts, off, nbatch, rot=None, cap=None, ws=None):
    from agplace_amd import ops
    from agplace_amd.sparse import SparseTensor
    kw = {} if cap is None else {"level_capacity": cap}
    return SparseTensor.from_points_capacity(torch.as_tensor(pts, dtype=torch.float32).to(dev), torch.as_tensor(off).to(dev), nbatch, QUANT,
                                             ws or ops.Workspace(), None if rot is None else rot.to(dev), **kw)


def _snap(sp):
    """the build's outputs, copied (a later build into the same workspace must not change what a test compares with)"""
    n = int(sp.n_dev.item())
    so, bi = sp.segments()
    return {"n": n, "keys": sp.keys.clone(), "seg": so.clone(), "bidx": bi.clone(), "f": sp.f32.clone(), "flag": int(sp.range_flag.item()),
            "rows": sp.n}


def _same_level(got, ref, cap):
    """got (capacity cap) == ref (uncapped) in everything a build defines: count, valid rows, segments, features, flag; padding behind"""
    n = ref["n"]
    assert got["n"] == n and got["rows"] == cap
    assert tuple(got["keys"].shape) == (cap,) and tuple(got["bidx"].shape) == (cap,) and tuple(got["f"].shape) == (cap, 1)
    assert torch.equal(got["keys"][:n], ref["keys"][:n]) and bool((got["keys"][n:] == SENT).all())
    assert torch.equal(got["seg"], ref["seg"])
    assert torch.equal(got["bidx"][:n], ref["bidx"][:n]) and bool((got["bidx"][n:] == 0).all())
    assert torch.equal(got["f"][:n], ref["f"][:n]) and bool((got["f"][:n] == 1.0).all())
    assert got["flag"] == ref["flag"]


def _is_empty(got, cap, nbatch):
    assert got["n"] == 0 and got["rows"] == cap and tuple(got["keys"].shape) == (cap,)
    assert got["seg"].tolist() == [0] * (nbatch + 1)
    assert bool((got["keys"] == SENT).all()) and bool((got["bidx"] == 0).all())


@pytest.fixture(scope="module")
def cloud():
    g = np.random.default_rng(21)
    sizes = (0, 1, 70000, 3000)
    pts = (g.random((sum(sizes), 3), dtype=np.float32) * np.float32([80, 80, 8]) - np.float32([40, 40, 4])).astype(np.float32)
    off = _offsets(sizes)
    rows, flagged = R.voxelise(pts, off, QUANT)
    assert len(rows) == A_CLOUD and not flagged
    assert np.bincount(rows[:, 0], minlength=4).tolist() == [0, 1, 6400, 2379]
    return pts, off


@pytest.fixture(scope="module")
def uncapped(dev, cloud):
    """the reference of every test below, computed once per rotation and never written again"""
    pts, off = cloud
    ref = {name: _snap(_build(dev, pts, off, 4, make())) for name, make in ROTS.items()}
    assert ref["none"]["n"] == A_CLOUD and ref["none"]["rows"] == 73001 and all(r["flag"] == 0 for r in ref.values())
    assert ref["shared"]["n"] < A_CLOUD                       # (cells that collide after the rotation merge: n < A)
    return ref


# ------------------------------------------------------------------------------------------------------------------ 1. fits
@pytest.mark.parametrize("cap", [8780, 16384, 73001, 100000])
def test_a_build_that_fits_is_bit_equal_to_the_uncapped_build(dev, cloud, uncapped, cap):
    """exact fit (A = capacity), a power of two, capacity = N and capacity > N; no, a shared and per-sample rotations.  With a
    rotation fewer rows than A survive, and A -- not the row count -- is what is held against the capacity."""
    from agplace_amd import ops
    pts, off = cloud
    for name, make in ROTS.items():
        ws = ops.Workspace()
        first = _snap(_build(dev, pts, off, 4, make(), cap, ws))
        _same_level(first, uncapped[name], cap)
        again = _snap(_build(dev, pts, off, 4, make(), cap, ws))        # a second build into the same workspace: the same bytes
        for k in ("keys", "seg", "bidx"):
            assert torch.equal(first[k], again[k]), (name, k)
        assert again["n"] == first["n"] and again["flag"] == 0 and torch.equal(first["f"][:first["n"]], again["f"][:first["n"]])


# ------------------------------------------------------------------------------------------------------------------ 2. tail rows
def test_tail_rows_of_a_larger_points_buffer_are_not_looked_at(dev, cloud, uncapped):
    pts, off = cloud
    buf = np.full((100000, 3), np.nan, dtype=np.float32)
    buf[:len(pts)] = pts
    buf[80000:] = np.float32(3e38)
    assert off[-1] == 73001
    for name, make in ROTS.items():
        _same_level(_snap(_build(dev, buf, off, 4, make(), 16384)), uncapped[name], 16384)


# ------------------------------------------------------------------------------------------------------------------ 3. overflow
class _Raw:
    """agp_sparse_build_points_cap called directly: ONE workspace and ONE flag word shared by builds of different capacities"""

    def __init__(self, dev, pts, off, nbatch, max_cap):
        from agplace_amd import _lib
        self.L, self.dev, self.nb = _lib.load(), dev, nbatch
        self.pts = torch.as_tensor(pts, dtype=torch.float32).to(dev)
        self.off = torch.as_tensor(off).to(dev)
        self.nbytes = self.L.agp_sparse_points_cap_workspace_bytes(self.pts.shape[0], max_cap, nbatch)
        self.tmp = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        self.flag = torch.full((1,), 0x55, dtype=torch.int32, device=dev)

    def build(self, cap, rot=None):
        from agplace_amd import _lib
        from agplace_amd._lib import ptr
        dev = self.dev
        assert self.L.agp_sparse_points_cap_workspace_bytes(self.pts.shape[0], cap, self.nb) <= self.nbytes
        keys = torch.full((cap,), -7, dtype=torch.int64, device=dev)
        f = torch.full((cap, 1), -7.0, device=dev)
        seg = torch.full((self.nb + 1,), -7, dtype=torch.int64, device=dev)
        bidx = torch.full((cap,), -7, dtype=torch.int32, device=dev)
        r = None if rot is None else rot.to(dev).contiguous()
        rc = self.L.agp_sparse_build_points_cap(ptr(self.pts), ptr(self.off), self.pts.shape[0], cap, self.nb, QUANT, ptr(r),
                                                1 if (r is not None and r.dim() == 3) else 0, ptr(keys), ptr(f), ptr(seg), ptr(bidx),
                                                ptr(self.flag), ptr(self.tmp), self.nbytes, _lib.stream())
        assert rc == 0
        torch.cuda.synchronize()
        return {"n": int(seg[-1].item()), "keys": keys, "seg": seg, "bidx": bidx, "f": f, "flag": int(self.flag.item()), "rows": cap}


@pytest.mark.parametrize("cap", [8779, 64])
def test_overflow_empties_the_build_and_the_next_build_in_the_same_workspace_is_clean(dev, cloud, uncapped, cap):
    """one row short of A, and a table (128 slots) far too small for the 8780 keys: the bounded probe and the early-out"""
    pts, off = cloud
    raw = _Raw(dev, pts, off, 4, 8780)
    for name, make in ROTS.items():
        got = raw.build(cap, make())
        assert got["flag"] == 4, (name, got["flag"])
        _is_empty(got, cap, 4)
        _same_level(raw.build(8780, make()), uncapped[name], 8780)          # flag 0 again: it describes THIS build


def test_overflow_through_the_sparse_tensor(dev, cloud):
    from agplace_amd import ops
    pts, off = cloud
    ws = ops.Workspace()
    got = _snap(_build(dev, pts, off, 4, None, 8779, ws))
    assert got["flag"] & 4
    _is_empty(got, 8779, 4)
    assert _snap(_build(dev, pts, off, 4, None, 8779, ws))["flag"] == 4


# ------------------------------------------------------------------------------------------------------------------ 4. flag bits
def test_flag_bits_compose(dev, cloud):
    pts, off = cloud
    bad = np.insert(pts, [40000], np.float32([[1.0, np.nan, 2.0]]), axis=0)
    off_bad = _offsets((0, 1, 70001, 3000))
    ref = _snap(_build(dev, bad, off_bad, 4))
    assert ref["flag"] == 1 and ref["n"] == A_CLOUD
    _same_level(_snap(_build(dev, bad, off_bad, 4, None, 16384)), ref, 16384)
    short = _snap(_build(dev, bad, off_bad, 4, None, 8779))
    assert short["flag"] == 5
    _is_empty(short, 8779, 4)
    # one sample of 70 000 well-separated points = 70 000 voxels (> 65536: that sample comes out empty, bit 1) beside a small one
    cells = np.stack(np.meshgrid(np.arange(-21, 21), np.arange(-21, 21), np.arange(-20, 20), indexing="ij"), -1).reshape(-1, 3)
    g = np.random.default_rng(27)
    big = ((cells[g.permutation(len(cells))[:70000]] + 0.5) * QUANT).astype(np.float32)
    both = np.concatenate([big, pts[-3000:]])
    off2 = _offsets((70000, 3000))
    ref2 = _snap(_build(dev, both, off2, 2))
    assert ref2["flag"] == 2 and ref2["n"] == 2379 and ref2["seg"].tolist() == [0, 0, 2379]
    _same_level(_snap(_build(dev, both, off2, 2, None, 80000)), ref2, 80000)


# ------------------------------------------------------------------------------------------------------------------ 5. downstream
def test_voxel_trunk_and_poolings_on_a_capped_tensor_equal_the_uncapped_ones(dev, cloud):
    from agplace_amd.sparse import ECABasicBlock, MinkFPN, MinkGeM
    from agplace_amd.sparse.modules import global_avg_pool
    pts, off = cloud
    torch.manual_seed(11)
    net = MinkFPN(1, 256, 0, 5, ECABasicBlock, [1, 1, 1], [64, 128, 256]).to(dev).eval()
    gem = MinkGeM().to(dev)
    out = []
    with torch.no_grad():
        for cap in (None, 16384):
            sp = _build(dev, pts, off, 4, _rot(5.0), cap)
            top, maps = net(sp, prec=2)
            assert top.n == (73001 if cap is None else 16384) and all(m.n == top.n for m in maps)
            out.append([gem(top).clone()] + [global_avg_pool(m).clone() for m in maps])
    torch.cuda.synchronize()
    assert float(out[0][0].abs().max()) > 0
    for a, b in zip(*out):
        assert torch.equal(a, b)


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


def _models(dev, seed, cap):
    """two models of the same weights: Options(voxel_capacity=None) and Options(voxel_capacity=cap)"""
    from agplace_amd.network_mm.mm import MM
    from agplace_amd.options import Options
    out = []
    for c in (None, cap):
        torch.manual_seed(seed)
        out.append(MM(opt=Options(mfma_precision=4, voxel_capacity=c)).to(dev).eval())
    for (ka, va), (kb, vb) in zip(out[0].state_dict().items(), out[1].state_dict().items()):
        assert ka == kb and torch.equal(va, vb)
    return out


def test_mm_forward_from_points_with_a_voxel_capacity_equals_the_forward_without(dev):
    plain, capped = _models(dev, 5, 16384)
    base = _query(dev, plain.opt, 5)
    pts, off = _scan(31, (900, 600))
    rot = torch.stack([_rot(4.0), _rot(-2.5)])
    d = dict(base, points=torch.from_numpy(pts).to(dev), point_offsets=torch.from_numpy(off).to(dev), pc_rotation=rot.to(dev))
    with torch.no_grad():
        a, b = plain(d, mode="q"), capped(d, mode="q")
        torch.cuda.synchronize()
    assert len(a) == 7 and set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert float(a["voxvec_org"].abs().max()) > 0
    assert plain.voxel_coords_in_range() and capped.voxel_coords_in_range()
    # the `coords` route ignores the option
    host = torch.from_numpy(R.per_point(pts, off, plain.opt.quant_size, rot.numpy())).to(dev)
    d_crd = dict(base, coords=host.double(), features=torch.ones((host.shape[0], 1), device=dev))
    with torch.no_grad():
        c = capped(d_crd, mode="q")
    for k in a:
        assert torch.equal(a[k], c[k]), k


# ------------------------------------------------------------------------------------------------------------------ 6. capture
def test_captured_forward_with_a_capacity_replays_other_scans_and_reports_an_overflow(dev):
    """forward_q from a points buffer of 3000 rows at voxel_capacity 2048, in one hipGraph.  A replay of another scan that fits
    equals the eager forward of that scan; a replay of a scan of more than 2048 distinct voxels completes, gives the outputs of
    the EMPTY cloud, and poll_voxel_range raises the capacity error once the flag has reached the host."""
    CAP = 2048
    plain, model = _models(dev, 6, CAP)
    del plain
    d = _query(dev, model.opt, 6)
    d["points"] = torch.full((3000, 3), float("nan"), device=dev)
    d["point_offsets"] = torch.zeros(3, dtype=torch.int64, device=dev)
    d["pc_rotation"] = _rot(3.0).to(dev)
    fit0, fit1 = _scan(41, (700, 500)), _scan(43, (800, 700))
    over = _scan(44, (1500, 1500), extent=60.0)
    assert len(R.voxelise(*fit0, 2.0)[0]) <= CAP and len(R.voxelise(*fit1, 2.0)[0]) <= CAP and len(R.voxelise(*over, 2.0)[0]) > CAP
    empty = (np.zeros((0, 3), dtype=np.float32), _offsets((0, 0)))

    def load(dst, pts, off):
        dst["points"][:len(pts)].copy_(torch.from_numpy(pts))
        dst["point_offsets"].copy_(torch.from_numpy(off))
    with torch.no_grad():
        load(d, *fit0)
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
        seen, embeddings = [], []
        for i, (scan, eager_scan) in enumerate([(fit0, fit0), (fit1, fit1), (over, empty), (fit1, fit1)]):
            load(d, *scan)
            load(e, *eager_scan)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()                       # the replay itself completes, overflow or not
            rep = {k: v.clone() for k, v in out.items()}
            try:
                model.poll_voxel_range()
                seen.append(None)
            except ValueError as err:
                seen.append(str(err))
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                eager = model(e, mode="q")
            torch.cuda.synchronize()
            for k in rep:
                assert torch.equal(rep[k], eager[k]), (i, k)
            embeddings.append(rep["embedding"])
        assert [s is not None for s in seen] == [False, False, True, False]
        assert "voxel capacity" in seen[2] and str(CAP) in seen[2] and "out of range" not in seen[2]
        assert not torch.equal(embeddings[0], embeddings[1]) and not torch.equal(embeddings[1], embeddings[2])
        assert torch.equal(embeddings[1], embeddings[3])
        assert model.voxel_coords_in_range()


# ------------------------------------------------------------------------------------------------------------------ 7. training
def test_training_levels_with_a_capacity_equal_those_without_and_an_overflow_raises(dev, cloud):
    from agplace_amd.sparse import SparseTensor
    pts, off = cloud
    p, o = torch.from_numpy(pts).to(dev), torch.from_numpy(off).to(dev)
    for make in ROTS.values():
        rot = make()
        rot = None if rot is None else rot.to(dev)
        a = SparseTensor.from_points_levels(p, o, 4, 3, QUANT, rot, level_capacity=16384)
        b = SparseTensor.from_points_levels(p, o, 4, 3, QUANT, rot)
        for lvl in range(4):
            assert a.n == b.n and a.stride == b.stride == 1 << lvl and torch.equal(a.keys, b.keys)
            assert torch.equal(a.segments()[0], b.segments()[0]) and torch.equal(a.segments()[1], b.segments()[1])
            if lvl == 0:
                assert a.n > 0 and torch.equal(a.f32, b.f32)
            if lvl < 3:
                a, b = a.strided()[0], b.strided()[0]
    with pytest.raises(ValueError, match=r"voxel capacity 8779 exceeded.*more distinct voxels"):
        SparseTensor.from_points_levels(p, o, 4, 3, QUANT, None, level_capacity=8779)
    # bits 0 / 1 alone keep their text
    bad = pts.copy()
    bad[10] = np.float32([np.nan, 0, 0])
    with pytest.raises(ValueError, match="out of the"):
        SparseTensor.from_points_levels(torch.from_numpy(bad).to(dev), o, 4, 3, QUANT, None, level_capacity=16384)


def test_one_training_step_with_a_voxel_capacity_gives_the_same_gradients(dev):
    plain, capped = _models(dev, 5, 16384)
    base = _query(dev, plain.opt, 5)
    pts, off = _scan(31, (900, 600))
    rot = torch.stack([_rot(4.0), _rot(-2.5)])
    d = dict(base, points=torch.from_numpy(pts).to(dev), point_offsets=torch.from_numpy(off).to(dev), pc_rotation=rot.to(dev))
    outs = []
    for m in (plain, capped):
        m.train()
        m.zero_grad(set_to_none=True)
        out = m(d, mode="q")
        out["embedding"].square().sum().backward()
        outs.append(out["embedding"].detach().clone())
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    ga = {k: p.grad for k, p in plain.named_parameters() if p.grad is not None}
    gb = {k: p.grad for k, p in capped.named_parameters() if p.grad is not None}
    assert set(ga) == set(gb) and "vox_fe.conv0.kernel" in ga and float(ga["vox_fe.conv0.kernel"].abs().max()) > 0
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    # an overflowing batch in .train() mode raises the capacity error of the level build
    from agplace_amd.network_mm.mm import MM
    from agplace_amd.options import Options
    torch.manual_seed(5)
    small = MM(opt=Options(mfma_precision=4, voxel_capacity=100)).to(dev).train()
    with pytest.raises(ValueError, match="voxel capacity 100 exceeded"):
        small(d, mode="q")
