"""-m gpu: the kernels of the sparse-voxel branch one by one against plain fp64 references (tests/sparse_kernel_ref.py, pinned to
oracle/sparse.py by tests/test_sparse_kernel_ref.py): the gather-GEMM agp_sparse_conv_fwd in every launch configuration the
product reaches, its tap lists (agp_sparse_tile_taps), the weight gradients agp_sparse_conv_wgrad / agp_sparse_conv_cin1_wgrad
with one and with several K splits, and the segment kernels of csrc/sparse.hip.  tests/test_gpu_sparse.py runs whole networks
on small clouds and takes one rel_l2 per feature map; here every 128 x 64 granule of an output meets the bar by itself.

Operands are drawn ALREADY ROUNDED to the storage format of the mode, so reference and kernel see the same values; the fp64
references run in torch's own ops on the device.  Gather tables come without coordinates (sparse_kernel_ref.gather_table): the
kernels take the table as given."""
import os
import re

import numpy as np
import pytest
import torch

import sparse_kernel_ref as R
from conv_sched_util import BARS, FILL_BITS, GUARD, GUARD_BITS, _bf16_pair, _f16

pytestmark = pytest.mark.gpu



def _header_code(name):
    """An AGP_* return code as include/agplace_hip.h defines it."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    m = re.search(r"#define %s (\d+)" % name, open(os.path.join(root, "include", "agplace_hip.h")).read())
    assert m, "%s not found in the header" % name
    return int(m.group(1))


BADARG = _header_code("AGP_E_BADARG")


def _L():
    from agplace_amd import _lib
    return _lib.load()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ok(rc, what):
    assert rc == 0, "%s returned %d" % (what, rc)


# ------------------------------------------------------------------------------------------------------ planes and buffers
def _planes(v, paired, dev):
    """Stored VALUES (representable in the format) -> (hi, lo) planes on the device: one fp16 plane, or a bf16 pair."""
    f = v.float()
    if not paired:
        hi = f.half()
        assert torch.equal(hi.double(), v.double()), "not an fp16 value"
        return hi.to(dev).contiguous(), None
    hi = f.bfloat16()
    lo = (f - hi.float()).bfloat16()
    assert torch.equal(hi.double() + lo.double(), v.double()), "not a bf16-pair value"
    return hi.to(dev).contiguous(), lo.to(dev).contiguous()


def _guarded(rows, c, paired, dev, zero_row=True):
    """Feature planes [rows (+ 1 zero row)][c] in the middle of larger buffers (conv_sched_util.guarded_map for a feature
    matrix): GUARD elements of one pattern on both sides, the rows pre-filled with another.  -> (hi, lo, [buffers])"""
    total = (rows + (1 if zero_row else 0)) * c
    planes, bufs = [], []
    for _ in range(2 if paired else 1):
        buf = torch.full((GUARD + total + GUARD,), GUARD_BITS, dtype=torch.int16, device=dev)
        m = buf[GUARD:GUARD + total].view(-1, c)
        m.fill_(FILL_BITS)
        if zero_row:
            m[rows] = 0
        planes.append(m.view(torch.bfloat16 if paired else torch.float16))
        bufs.append(buf)
    return planes[0], (planes[1] if paired else None), bufs


def _bits(plane):
    return plane.view(torch.int16)


def _value(hi, lo, a, b):
    v = hi[a:b].double()
    return v if lo is None else v + lo[a:b].double()


def _assert_frame(hi, lo, bufs, rows, written=(0, 0), filled=(0, 0), zero_row=True):
    """Guards and zero row untouched; no element of rows [written) still holds the fill pattern; every element of rows [filled)
    still does."""
    for plane, buf in zip([hi] + ([lo] if lo is not None else []), bufs):
        assert bool((buf[:GUARD] == GUARD_BITS).all()) and bool((buf[-GUARD:] == GUARD_BITS).all()), "guard region written"
        b = _bits(plane)
        if zero_row:
            assert not bool(b[rows].any()), "zero row written"
        miss = b[written[0]:written[1]] == FILL_BITS
        if bool(miss.any()):
            r, ch = (int(v) for v in miss.nonzero()[0])
            raise AssertionError("%d elements of rows %d..%d were not written; the first: row %d channel %d" % (
                int(miss.sum()), written[0], written[1] - 1, written[0] + r, ch))
        hit = b[filled[0]:filled[1]] != FILL_BITS
        if bool(hit.any()):
            r, ch = (int(v) for v in hit.nonzero()[0])
            raise AssertionError("%d elements of rows %d..%d were written; the first: row %d channel %d" % (
                int(hit.sum()), filled[0], filled[1] - 1, filled[0] + r, ch))


def _assert_granules(got, ref, bar, what):
    worst, where, _ = R.granule_rel(got, ref)
    whole = float((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300))
    print("%s: worst 128 x 64 granule %.3e at %s, whole map %.3e, bar %.1e" % (what, worst, where, whole, bar))
    assert worst < bar, "%s: granule %s has %.3e (bar %.1e; whole map %.3e)" % (what, where, worst, bar, whole)


# --------------------------------------------------------------------------------------------- gather-GEMM forward: problems
class Problem:
    """One gather-GEMM problem on the device: stored operands, planes, the emulated reference (sparse_kernel_ref.emulate)."""

    def __init__(self, dev, prec, cin, cout, ntaps, m, epi, seed=0, n_in=None, density=0.5, perm=False):
        from agplace_amd import _lib, ops
        self.prec, self.cin, self.cout, self.ntaps, self.m, self.dev = prec, cin, cout, ntaps, m, dev
        self.paired = prec == 3
        g = torch.Generator().manual_seed(1000 * seed + 7 * cin + cout + 31 * ntaps + m)
        n_in = n_in if n_in is not None else m * 3 // 4 + 7
        self.n_in = n_in
        ngr = (m + 127) // 128
        # granules (of GEMM rows) that lack taps, one with a single active tap, two neighbouring ones with no tap at all (a
        # whole tile without neighbours, 256-row tiles included), single rows without neighbours; an identity centre tap
        lacking, single = {}, None
        if ntaps > 4:
            lacking[0] = (0, 1, ntaps - 1)
            if ngr > 3:
                lacking[3] = tuple(range(0, ntaps, 2))
        if ngr > 7:
            lacking[4] = lacking[5] = tuple(range(ntaps))
        if ngr > 1 and ntaps > 1:
            single = (ngr - 1 if ngr < 8 else 7, ntaps - 2)
        tab = R.gather_table(ntaps, m, n_in, density, seed=seed * 77 + m + ntaps, centre=ntaps // 2 if ntaps % 2 and ntaps > 1 else None,
                             lacking=lacking, single=single, absent_rows=(m // 16 if m >= 16 else 0))
        self.perm = None
        if perm:
            # `tab` above is in GEMM-row order: GEMM row i computes output row perm[i]
            pm = torch.randperm(m, generator=g)
            t2 = np.empty_like(tab)
            t2[:, pm.numpy()] = tab
            tab, self.perm, self.perm_np = t2, pm.int().to(dev), pm.numpy()
        self.tab_np = tab
        self.tab = torch.from_numpy(tab).to(dev)
        rnd, wrnd = R.store_round(prec), R.weight_round(prec)
        x = rnd(torch.randn((n_in + 1, cin), generator=g))
        x[n_in] = 0
        w = wrnd(torch.randn((ntaps, cin, cout), generator=g) / (cin * max(1.0, density * ntaps)) ** 0.5)
        self.scale = (0.5 + torch.rand(cout, generator=g)).to(dev) if "s" in epi else None
        self.shift = (0.3 * torch.randn(cout, generator=g)).to(dev) if "s" in epi else None
        res = rnd(torch.randn((m, cout), generator=g)) if "r" in epi else None
        self.relu = "u" in epi
        self.x_hi, self.x_lo = _planes(x, self.paired, dev)
        self.r_hi, self.r_lo = _planes(res, self.paired, dev) if res is not None else (None, None)
        # weight planes as modules.MinkowskiConvolution._weights makes them: [cout][ntaps][cin] through ops.split_weight
        wk = w.float().permute(2, 0, 1).contiguous().to(dev)
        fmt = _lib.FMT_BF16 if prec == 3 else _lib.FMT_F16
        self.w_hi, self.w_lo = ops.split_weight(wk, fmt, want_lo=prec != 4)
        back = self.w_hi.double() + (self.w_lo.double() if self.w_lo is not None else 0)
        assert torch.equal(back, wk.double()), "the weight planes do not hold the stored weights"
        xd, wd, rd = x.to(dev), w.to(dev), None if res is None else res.to(dev)
        self.ref = R.emulate(prec, xd, self.tab, wd, self.scale, self.shift, rd, self.relu)
        # rows without a neighbour: relu(shift + res) in fp32, stored -- exactly
        v = torch.zeros((m, cout), dtype=torch.float32, device=dev)
        if self.shift is not None:
            v = v + self.shift
        if rd is not None:
            v = v + rd.float()
        self.absent = torch.from_numpy((tab == n_in).all(0)).to(dev)
        self.absent_value = rnd(torch.relu(v) if self.relu else v)[self.absent]

    def out(self):
        return _guarded(self.m, self.cout, self.paired, self.dev)

    def launch(self, hi, lo, n_dev=None, perm=None, taps=None):
        return _L().agp_sparse_conv_fwd(_ptr(self.x_hi), _ptr(self.x_lo), self.n_in + 1, _ptr(self.tab), self.m, self.cin, self.cout,
                                        self.ntaps, _ptr(self.w_hi), _ptr(self.w_lo), _ptr(self.scale), _ptr(self.shift),
                                        _ptr(self.r_hi), _ptr(self.r_lo), 1 if self.relu else 0, _ptr(hi), _ptr(lo), self.prec,
                                        _ptr(n_dev), _ptr(perm), _ptr(taps), _stream())

    def check(self, hi, lo, bufs, what, rows=None):
        rows = self.m if rows is None else rows
        _assert_frame(hi, lo, bufs, self.m, written=(0, rows))
        got = _value(hi, lo, 0, rows)
        assert bool(torch.isfinite(got).all())
        _assert_granules(got, self.ref[:rows], BARS[self.prec], what)
        ab = self.absent[:rows]
        assert torch.equal(got[ab], self.absent_value[:int(ab.sum())]), "%s: a row without neighbours is not relu(shift + res)" % what


@pytest.fixture(scope="module")
def problems(dev):
    """problems(prec, cin, cout, ntaps, rows, epi, ...): the Problem of these arguments, built once for the tests of this file that
    share it (reference included) and released with the module."""
    cache = {}

    def get(*key, **kw):
        k = (key, tuple(sorted(kw.items())))
        if k not in cache:
            cache[k] = Problem(dev, *key, **kw)
        return cache[k]
    yield get
    cache.clear()


# (cin, cout, ntaps, rows, epilogue: s = scale and shift, r = residual, u = ReLU).  Every (cin, cout), every tap count (1, 8, 27:
# the masked K loop; 32: the full mask word; 33, 125: the unmasked loop), every row count and both states of every epilogue part
# occur once per precision; 32 and 33 taps at cin = 32 (ONE K step per tap: a table prefetch in every stage) and at cin = 128.
SMALL = [
    (32, 64, 32, 257, "sru"),
    (32, 64, 33, 129, ""),
    (128, 256, 32, 255, ""),
    (128, 256, 33, 63, "sru"),
    (64, 64, 27, 2100, "sru"),         # 9 row tiles of 256: not a multiple of 8, a partial last tile
    (64, 128, 8, 2100, "r"),           # 17 row tiles of 128
    (256, 128, 1, 128, "su"),
    (64, 64, 125, 1, ""),
    (64, 128, 125, 257, "su"),
    (32, 64, 1, 63, "r"),
    (64, 128, 27, 129, "s"),
]


@pytest.mark.parametrize("prec", [4, 2, 3], ids=["f16", "f16w2", "bf16x3"])
@pytest.mark.parametrize("cin,cout,ntaps,m,epi", SMALL, ids=["%d-%d-taps%d-rows%d-epi_%s" % c for c in SMALL])
def test_conv_fwd_small_shapes(dev, problems, prec, cin, cout, ntaps, m, epi):
    """agp_sparse_conv_fwd in the three precisions: fp16 (4: `<4,1,32,4,EPI,2>` for 64 output channels, the gather-only choice
    of launch_igemm, and `<2,2,32,4,EPI,3>` for 128+), fp16 with a weight pair (2) and bf16 pairs (3, the residual a pair too),
    narrow (64 channels) and wide; masked (<= 32 taps), 32-tap and unmasked K loops; partial last tiles."""
    pr = problems(prec, cin, cout, ntaps, m, epi)
    hi, lo, bufs = pr.out()
    _ok(pr.launch(hi, lo), "agp_sparse_conv_fwd")
    pr.check(hi, lo, bufs, "prec %d %d->%d %d taps %d rows" % (prec, cin, cout, ntaps, m))


BIG = [
    (64, 128, 2, 130700, 511, "sru"),
    (64, 128, 2, 131000, 512, ""),
    (128, 256, 3, 65400, 512, "sru"),
    (128, 256, 3, 65000, 508, "r"),
]


@pytest.mark.parametrize("cin,cout,ntaps,m,tiles,epi", BIG,
                         ids=["%d-%d-rows%d-%s" % (c[0], c[1], c[3], "8wave_256x128" if c[4] >= 512 else "4wave_128x128") for c in BIG])
def test_conv_fwd_both_sides_of_the_8_wave_switch(dev, cin, cout, ntaps, m, tiles, epi):
    """AGP_PREC_F16 gather-GEMM with 128+ output channels: launch_igemm (csrc/igemm.hip, the `p.tap_stride && var == 0` branch,
    `if ((int64_t)((p.M + 255) / 256) * (p.N / 128) >= 512) return launch_cfg<4, 2, 32, 4, EPI, 3>`) takes the 8-wave
    256 x 128 tile from 512 such tiles on and `<2, 2, 32, 4, EPI, 3>` below.  The sizes sit on both sides of that 512: a change
    of the rule needs new sizes here.  The reference is the WHOLE output in fp64.  A second launch in capacity mode (n_dev = 70 001
    valid rows, no multiple of either tile) lets m_dev meet both tiles: the 8-wave one deals ceil(70 001 / 256) valid tiles over
    the XCDs."""
    assert (m + 255) // 256 * (cout // 128) == tiles
    pr = Problem(dev, 4, cin, cout, ntaps, m, epi, n_in=30000, density=0.6)
    hi, lo, bufs = pr.out()
    _ok(pr.launch(hi, lo), "agp_sparse_conv_fwd")
    pr.check(hi, lo, bufs, "prec 4 %d->%d %d rows (%d tiles of 256 x 128)" % (cin, cout, m, tiles))
    nv = 70001 if m > 100000 else 40001
    hi, lo, bufs = pr.out()
    _ok(pr.launch(hi, lo, n_dev=torch.tensor([nv], dtype=torch.int64, device=dev)), "agp_sparse_conv_fwd")
    _assert_frame(hi, lo, bufs, m, written=(0, nv), filled=((nv + 255) // 256 * 256, m))
    pr.check(hi, lo, bufs, "prec 4 %d->%d n_dev %d of %d rows" % (cin, cout, nv, m), rows=nv)


@pytest.mark.parametrize("n_dev", [0, 1, 130, 2099, 2100, 2107])
@pytest.mark.parametrize("prec,cin,cout,ntaps", [(4, 64, 64, 27), (4, 64, 128, 8), (3, 64, 128, 8)],
                         ids=["f16-64-64-taps27", "f16-64-128-taps8", "bf16x3-64-128-taps8"])
def test_conv_fwd_capacity_mode(dev, problems, prec, cin, cout, ntaps, n_dev):
    """m_dev: the valid row count on the device, below / at / above the capacity of 2100 rows and no multiple of a tile.  The valid
    row tiles are dealt over the XCDs inside the kernel; rows below min(n_dev, M) meet the bar, rows from the next multiple of
    256 on are not written, n_dev = 0 writes nothing."""
    m = 2100
    pr = problems(prec, cin, cout, ntaps, m, "sru")
    hi, lo, bufs = pr.out()
    nd = torch.tensor([n_dev], dtype=torch.int64, device=dev)
    _ok(pr.launch(hi, lo, n_dev=nd), "agp_sparse_conv_fwd")
    nv = min(n_dev, m)
    first_untouched = min(m, (nv + 255) // 256 * 256)
    _assert_frame(hi, lo, bufs, m, written=(0, nv), filled=(first_untouched, m))
    if nv:
        pr.check(hi, lo, bufs, "prec %d %d->%d n_dev %d of %d" % (prec, cin, cout, n_dev, m), rows=nv)


def _tile_taps(dev, tab, n_out, ntaps, zero_row, perm, n_dev, ngran):
    mask = torch.full((ngran,), -1, dtype=torch.int32, device=dev)
    _ok(_L().agp_sparse_tile_taps(_ptr(tab), n_out, ntaps, zero_row, _ptr(perm), _ptr(n_dev), _ptr(mask), ngran, _stream()),
        "agp_sparse_tile_taps")
    return mask


@pytest.mark.parametrize("m", [129, 257, 2100])
@pytest.mark.parametrize("cin,cout,ntaps", [(64, 64, 27), (64, 128, 8)], ids=["64-64-taps27", "64-128-taps8"])
@pytest.mark.parametrize("prec", [4, 2, 3], ids=["f16", "f16w2", "bf16x3"])
def test_conv_fwd_row_perm_and_tile_taps_change_no_bit(dev, problems, prec, cin, cout, ntaps, m):
    """row_perm + tile_taps (the z-plane row order and the per-tile tap lists of a centred convolution): with a random row order
    and the masks agp_sparse_tile_taps makes from the same table, the output is bit-identical to the plain launch.  The table has
    granules that lack taps, one with a single active tap and (2100 rows) a 256-row tile without any; the last tile's clamped
    rows read row_perm too.  The last launch is the call the product's centred convolutions make in capacity mode
    (modules.MinkowskiConvolution.forward): row_perm, tile_taps (made with the same n_dev) and n_dev = 130 together -- the output
    rows of the valid GEMM rows, row_perm[:130], hold the plain launch's bits, those of the GEMM rows from 256 on are not written."""
    pr = problems(prec, cin, cout, ntaps, m, "sru", seed=3, perm=True)
    ngran = (m + 255) // 256 * 2
    taps = _tile_taps(dev, pr.tab, m, ntaps, pr.n_in, pr.perm, None, ngran)
    want = R.granule_masks(pr.tab_np, pr.n_in, pr.perm_np, ngran=ngran)
    assert ((taps.cpu().numpy().astype(np.int64) & 0xffffffff) == want.astype(np.int64)).all()
    full = (1 << ntaps) - 1
    assert any(int(v) != full for v in want[:(m + 127) // 128]), "every granule has every tap: the masks skip nothing"
    if m == 2100:
        assert int(want[4]) == 0 and int(want[5]) == 0
    hi0, lo0, bufs0 = pr.out()
    _ok(pr.launch(hi0, lo0), "agp_sparse_conv_fwd")
    pr.check(hi0, lo0, bufs0, "plain, prec %d %d taps %d rows" % (prec, ntaps, m))
    hi1, lo1, bufs1 = pr.out()
    _ok(pr.launch(hi1, lo1, perm=pr.perm, taps=taps), "agp_sparse_conv_fwd")
    _assert_frame(hi1, lo1, bufs1, m, written=(0, m))
    assert torch.equal(_bits(hi0), _bits(hi1)) and (lo0 is None or torch.equal(_bits(lo0), _bits(lo1)))
    # the row order alone (every tap of every tile)
    hi2, lo2, bufs2 = pr.out()
    _ok(pr.launch(hi2, lo2, perm=pr.perm), "agp_sparse_conv_fwd")
    _assert_frame(hi2, lo2, bufs2, m, written=(0, m))
    assert torch.equal(_bits(hi0), _bits(hi2)) and (lo0 is None or torch.equal(_bits(lo0), _bits(lo2)))
    # capacity mode on top
    nv = min(130, m)
    nd = torch.tensor([130], dtype=torch.int64, device=dev)
    taps_nd = _tile_taps(dev, pr.tab, m, ntaps, pr.n_in, pr.perm, nd, ngran)
    want_nd = R.granule_masks(pr.tab_np, pr.n_in, pr.perm_np, n_valid=130, ngran=ngran)
    assert ((taps_nd.cpu().numpy().astype(np.int64) & 0xffffffff) == want_nd.astype(np.int64)).all()
    hi3, lo3, bufs3 = pr.out()
    _ok(pr.launch(hi3, lo3, n_dev=nd, perm=pr.perm, taps=taps_nd), "agp_sparse_conv_fwd")
    _assert_frame(hi3, lo3, bufs3, m)
    valid, beyond = pr.perm[:nv].long(), pr.perm[256:].long()
    for a, b in ((hi0, hi3),) + (((lo0, lo3),) if lo0 is not None else ()):
        assert torch.equal(_bits(a)[valid], _bits(b)[valid]), "a valid row differs from the plain launch"
        assert bool((_bits(b)[beyond] == FILL_BITS).all()), "a row past the valid tiles was written"


@pytest.mark.parametrize("cut", [None, 448, 1], ids=["all_rows", "n_dev_cuts_granule_3", "n_dev_1"])
@pytest.mark.parametrize("with_perm", [False, True], ids=["natural", "perm"])
@pytest.mark.parametrize("ntaps", [8, 27, 32])
def test_tile_taps_equal_the_or_over_each_granule(dev, ntaps, with_perm, cut):
    """agp_sparse_tile_taps: mask[g] bit t <=> a VALID row of GEMM granule g has a neighbour through tap t.  600 rows are 5
    granules, the 6th (ngran = ceil(600 / 256) * 2, as SparseTensor.tile_taps sizes it) and every granule past n_dev give 0; the
    kernel walks the taps nine at a time and clamps the index (8 < 9, 27 = 3 x 9, 32 = 3 x 9 + 5).  A bit too many costs only
    time in the gather-GEMM, so nothing else notices it."""
    m, n_in, ngran = 600, 400, 6
    tab = R.gather_table(ntaps, m, n_in, 0.01, seed=ntaps, lacking={1: range(ntaps), 2: (0, ntaps - 1)}, single=(4, ntaps - 1))
    g = torch.Generator().manual_seed(ntaps)
    perm = torch.randperm(m, generator=g) if with_perm else None
    nd = None if cut is None else torch.tensor([cut], dtype=torch.int64, device=dev)
    mask = _tile_taps(dev, torch.from_numpy(tab).to(dev), m, ntaps, n_in, None if perm is None else perm.int().to(dev), nd, ngran)
    want = R.granule_masks(tab, n_in, None if perm is None else perm.numpy(), n_valid=cut, ngran=ngran)
    got = mask.cpu().numpy().astype(np.int64) & 0xffffffff
    assert got.tolist() == want.astype(np.int64).tolist()
    assert want[5] == 0 and (cut is None or (want[4:] == 0).all())
    if cut is None:
        assert len(set(want[:5].tolist())) > 2                      # the granules differ: the test can tell them apart


def test_out_of_contract_arguments_are_refused_before_any_launch(dev):
    """cin % 32, cout % 64, more than 32 taps for a mask word: AGP_E_BADARG from the entry points' own checks."""
    L = _L()
    t = torch.zeros(4096, dtype=torch.int32, device=dev)
    p = _ptr(t)
    assert L.agp_sparse_conv_fwd(p, None, 9, p, 8, 48, 64, 1, p, None, None, None, None, None, 0, p, None, 4, None, None, None,
                                 _stream()) == BADARG
    assert L.agp_sparse_conv_fwd(p, None, 9, p, 8, 32, 96, 1, p, None, None, None, None, None, 0, p, None, 4, None, None, None,
                                 _stream()) == BADARG
    assert L.agp_sparse_conv_wgrad(p, p, 9, p, 8, 48, 64, 1, p, p, p, p, 1 << 20, _stream()) == BADARG
    assert L.agp_sparse_conv_wgrad_workspace_bytes(8, 48, 64, 1) == -1
    assert L.agp_sparse_tile_taps(p, 8, 33, 8, None, None, p, 2, _stream()) == BADARG
    assert L.agp_sparse_tile_taps(p, 300, 8, 8, None, None, p, 2, _stream()) == BADARG      # fewer mask words than granules
    torch.cuda.synchronize()
    assert not bool(t.any())


# ------------------------------------------------------------------------------------------------------- weight gradients
def _slab_err(got, ref):
    """The rms error of every tap slab [cin, cout] over the rms of the whole gradient -> (the largest, its tap)"""
    rms = float(ref.double().pow(2).mean().sqrt())
    e = (got.double() - ref.double()).pow(2).mean((1, 2)).sqrt() / (rms if rms > 0 else 1.0)
    return float(e.max()), int(e.argmax())


# (ntaps, cin, cout, table, rows): the tile-count branches of agp_sparse_conv_wgrad -- nb = 9 (nine or more taps), nb = 8 (eight
# A-blocks: 8 taps x 32 channels on the one-hot table of a transposed convolution, or 16 blocks of a dense one), nb = 4 (one tap,
# cin = 128), nb = 2 (one tap, cin = 64; cin = 32: the pair's second block does not exist) -- each with one K split (rows <= 1535)
# and with several (1537: 2 splits of 25 + 24 K steps; 5001: 6 splits, the last one shorter; 40 003: 51 splits, the last of ONE step)
WGRAD = [(27, 32, 64, "dense", n) for n in (1, 31, 33, 1000, 1537, 5001, 40003)] + \
        [(27, 64, 256, "dense", n) for n in (1000, 5001)] + \
        [(8, 32, 64, "one_hot", n) for n in (33, 1537, 40003)] + \
        [(8, 64, 64, "dense", n) for n in (1000, 5001)] + \
        [(1, 128, 256, "dense", n) for n in (31, 1000, 1537, 40003)] + \
        [(1, 64, 64, "dense", n) for n in (1, 1000, 5001)] + \
        [(1, 32, 64, "dense", n) for n in (33, 1537, 40003)]


def _wgrad_nb(ntaps, cin):
    nblk = ntaps * (cin // 32)
    return 9 if ntaps >= 9 else (8 if nblk >= 8 else (4 if nblk >= 4 else 2))


@pytest.mark.parametrize("ntaps,cin,cout,kind,n_out", WGRAD,
                         ids=["nb%d-taps%d-%d-%d-%s-rows%d" % (_wgrad_nb(c[0], c[1]), c[0], c[1], c[2], c[3], c[4]) for c in WGRAD])
def test_conv_wgrad_matches_fp64(dev, ntaps, cin, cout, kind, n_out):
    """agp_sparse_conv_wgrad (bf16 pairs, three MFMA products, split K + wgrad_reduce_kernel) against wgrad_ref64 on the operands as
    stored.  Workspace and gradient start as NaN: the result is finite (written, not added to) and a second call gives the same
    bits.  Bar per tap slab: max(BARS[3], 4 e32), e32 the error of the same sum in plain fp32 on the CPU (the factor 4: another,
    equally legitimate summation order).

    Measured on an MI355X (worst slab of the kernel / e32), rows above 1536:
      27 taps 32 -> 64             1537 rows 2.84e-06 / 1.97e-07   5001 rows 2.86e-06 / 2.08e-07   40 003 rows 2.88e-06 / 3.32e-07
      27 taps 64 -> 256                                            5001 rows 2.82e-06 / 2.03e-07
      8 taps 32 -> 64 (one-hot)    1537 rows 3.03e-06 / 1.21e-07                                   40 003 rows 2.80e-06 / 2.81e-07
      8 taps 64 -> 64                                              5001 rows 2.84e-06 / 2.06e-07
      1 tap 128 -> 256             1537 rows 2.81e-06 / 1.80e-07                                   40 003 rows 2.79e-06 / 3.14e-07
      1 tap 64 -> 64                                               5001 rows 2.74e-06 / 1.92e-07
      1 tap 32 -> 64               1537 rows 2.80e-06 / 1.75e-07                                   40 003 rows 2.81e-06 / 2.97e-07
    The kernel's figure is the lo x lo product that its three MFMA products leave out, the same at every size and split count
    (2.7e-06 .. 3.0e-06 with one split too); e32 grows with the rows.  The bar is BARS[3] = 2e-5 in every case."""
    L = _L()
    n_in = max(1, n_out * 2 // 3 + 3)
    g = torch.Generator().manual_seed(n_out + 13 * ntaps + cin)
    if kind == "one_hot":
        tab = R.one_hot_table(n_out, n_in, seed=n_out, ntaps=ntaps)
    else:
        tab = R.gather_table(ntaps, n_out, n_in, 0.5, seed=n_out + cin, absent_rows=n_out // 16)
    x = _bf16_pair(torch.randn((n_in + 1, cin), generator=g))
    x[n_in] = 0
    gr = _bf16_pair(torch.randn((n_out, cout), generator=g))
    x_hi, x_lo = _planes(x, True, dev)
    g_hi, g_lo = _planes(gr, True, dev)
    tab_d = torch.from_numpy(tab).to(dev)
    nbytes = L.agp_sparse_conv_wgrad_workspace_bytes(n_out, cin, cout, ntaps)
    splits = nbytes // (ntaps * cin * cout * 4)                       # (the workspace's; the launch may need one fewer)
    ksteps = (n_out + 31) // 32
    per = (ksteps + splits - 1) // splits
    used = (ksteps + per - 1) // per
    assert nbytes > 0 and (splits > 1) == (n_out > 1504)       # 48 K steps of 32 rows: two splits of 24
    outs = []
    for _ in range(2):
        ws = torch.full((max(nbytes // 4, 4),), float("nan"), dtype=torch.float32, device=dev)
        gw = torch.full((ntaps, cin, cout), float("nan"), dtype=torch.float32, device=dev)
        _ok(L.agp_sparse_conv_wgrad(_ptr(x_hi), _ptr(x_lo), n_in + 1, _ptr(tab_d), n_out, cin, cout, ntaps, _ptr(g_hi), _ptr(g_lo),
                                    _ptr(gw), _ptr(ws), nbytes, _stream()), "agp_sparse_conv_wgrad")
        outs.append(gw)
    assert bool(torch.isfinite(outs[0]).all()), "the gradient was added to its start value, or not written"
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    ref = R.wgrad_ref64(x.to(dev), tab_d, gr.to(dev))
    e32, _ = _slab_err(R.wgrad_f32(x, tab, gr), ref.cpu())
    worst, tap = _slab_err(outs[0], ref)
    bar = max(BARS[3], 4 * e32)
    print("wgrad nb %d, %d taps %d->%d, %d rows, %d splits of %d K steps (the last %d): worst slab %.3e (tap %d), e32 %.3e, "
          "bar %.1e" % (_wgrad_nb(ntaps, cin), ntaps, cin, cout, n_out, used, per, ksteps - (used - 1) * per, worst, tap, e32, bar))
    assert worst < bar, "tap %d: %.3e (e32 %.3e, bar %.1e)" % (tap, worst, e32, bar)


@pytest.mark.parametrize("nsl", [1, 2, 5, 64])
@pytest.mark.parametrize("n_out", [100, 4096, 10000])
@pytest.mark.parametrize("ntaps", [125, 27])
def test_conv_cin1_wgrad_matches_fp64(dev, ntaps, n_out, nsl):
    """agp_sparse_conv_cin1_wgrad (the first layer: fp32 voxel features, bf16-pair gradient rows) with 1 .. 64 row slices: a slice
    holds ceil(rows / slices) rows rounded up to 32, so 64 slices of 100 rows (4 used) and of 4096 rows (exactly 64) and 5 of
    10 000 (the last one shorter) include trailing EMPTY slices, whose partials must still be written (0) for the reduction.
    Same bar and NaN pre-fill as the gather wgrad; measured on an MI355X: worst tap row 6e-08 (100 rows) .. 3.4e-07 (10 000 rows in
    one slice; 7.5e-08 in 64 slices), e32 1.9e-07 .. 2.3e-06: the bar is BARS[3] = 2e-5 in every case."""
    L = _L()
    cout, n_in = 64, n_out * 2 // 3
    g = torch.Generator().manual_seed(n_out + ntaps)
    tab = R.gather_table(ntaps, n_out, n_in, 0.4, seed=n_out + ntaps, centre=ntaps // 2, absent_rows=n_out // 16)
    assert (tab == n_in).any()
    f = torch.randn(n_in, generator=g)
    gr = _bf16_pair(torch.randn((n_out, cout), generator=g))
    g_hi, g_lo = _planes(gr, True, dev)
    f_d, tab_d = f.to(dev), torch.from_numpy(tab).to(dev)
    outs = []
    for _ in range(2):
        part = torch.full((nsl, ntaps, cout), float("nan"), dtype=torch.float32, device=dev)
        gw = torch.full((ntaps, cout), float("nan"), dtype=torch.float32, device=dev)
        _ok(L.agp_sparse_conv_cin1_wgrad(_ptr(f_d), n_in, _ptr(tab_d), n_out, ntaps, _ptr(g_hi), _ptr(g_lo), cout, _ptr(gw), _ptr(part),
                                         nsl, _stream()), "agp_sparse_conv_cin1_wgrad")
        outs.append(gw)
        assert bool(torch.isfinite(part).all()), "a slice's partial was not written"
    assert bool(torch.isfinite(outs[0]).all())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    fz = torch.cat([f, torch.zeros(1)]).unsqueeze(1)
    ref = R.wgrad_ref64(fz.to(dev), tab_d, gr.to(dev))                   # [ntaps, 1, cout]
    e32, _ = _slab_err(R.wgrad_f32(fz, tab, gr), ref.cpu())
    worst, tap = _slab_err(outs[0].unsqueeze(1), ref)
    bar = max(BARS[3], 4 * e32)
    print("cin1 wgrad %d taps, %d rows, %d slices: worst tap row %.3e (tap %d), e32 %.3e, bar %.1e" % (ntaps, n_out, nsl, worst, tap,
                                                                                                      e32, bar))
    assert worst < bar, "tap %d: %.3e (e32 %.3e, bar %.1e)" % (tap, worst, e32, bar)


# --------------------------------------------------------------------------------------------------------- segment kernels
COUNTS = [0, 1, 130, 0, 70001, 0]       # empty first / middle / last, one row, about one block's worth, far more than a block
NSEG, NROWS = len(COUNTS), sum(COUNTS)
SEG_BAR = {True: 2e-5, False: 1e-3}     # bf16 pair / fp16: the tolerances test_minkfpn_matches_oracle holds these outputs to
FMT = pytest.mark.parametrize("paired", [False, True], ids=["f16", "bf16pair"])


@pytest.fixture(scope="module")
def seg(dev):
    """(seg_off int64 [NSEG + 1], bidx int32 [NROWS]) on the device"""
    off = torch.tensor([0] + list(np.cumsum(COUNTS)), dtype=torch.int64, device=dev)
    return off, R.seg_bidx(off).int()


def _rows(seed, c, paired, dev, kind="signed"):
    """[NROWS, c] stored values on the device, a function of (seed, c).  "pool": mostly positive, a tenth negative, a tenth just
    below eps = 1e-6, a few just above."""
    g = torch.Generator(device=dev).manual_seed(1000 * seed + c)
    v = torch.randn((NROWS, c), generator=g, device=dev)
    if kind == "pool":
        u = torch.randn((NROWS, c), generator=g, device=dev)
        v = torch.where(u > 1.3, -v.abs(), torch.where(u < -1.3, v.abs() * 6e-7, torch.where(u.abs() < 0.05, 1e-6 + v.abs() * 2e-6,
                                                                                              v.abs())))
    return (_bf16_pair if paired else _f16)(v)


def _per_segment(got, ref, bar, what, one_row_by_element=False):
    """rel_l2 of every non-empty segment's [C] vector by itself (the 70 001-row segment does not hide the one-row one); an empty
    segment's vector is exactly 0.  one_row_by_element: the one-row segment element by element too -- its pooled value IS the row
    (mean x, GeM max(x, eps), dot a * b), so a clamp at the wrong place shows in the channels below eps and nowhere else."""
    for b, n in enumerate(COUNTS):
        if n == 0:
            assert not bool(got[b].any()), "%s: the empty segment %d is not 0" % (what, b)
            continue
        e = float((got[b].double() - ref[b].double()).norm() / ref[b].double().norm().clamp_min(1e-300))
        print("%s: segment %d (%d rows) %.3e, bar %.1e" % (what, b, n, e, bar))
        assert e < bar, "%s: segment %d (%d rows): %.3e (bar %.1e)" % (what, b, n, e, bar)
        if n == 1 and one_row_by_element:
            bad = (got[b].double() - ref[b].double()).abs() > bar * ref[b].double().abs()
            assert not bool(bad.any()), "%s: one-row segment, channel %d: %r for %r" % (
                what, int(bad.nonzero()[0]), float(got[b][bad][0]), float(ref[b][bad][0]))


def _per_segment_rows(got, ref, bar, what):
    off = np.cumsum([0] + COUNTS)
    for b, n in enumerate(COUNTS):
        if n:
            gs, rs = got[off[b]:off[b + 1]].double(), ref[off[b]:off[b + 1]].double()
            e = float((gs - rs).norm() / rs.norm().clamp_min(1e-300))
            print("%s: rows of segment %d (%d rows) %.3e, bar %.1e" % (what, b, n, e, bar))
            assert e < bar, "%s: rows of segment %d (%d rows): %.3e (bar %.1e)" % (what, b, n, e, bar)


@FMT
@pytest.mark.parametrize("c", [64, 128, 256])
@pytest.mark.parametrize("mode,p", [("mean", 3.0), ("gem", 3.0), ("both", 2.5), ("gem", 2.5)])
def test_seg_pool_fwd(dev, seg, paired, c, mode, p):
    """agp_seg_pool_fwd (seg_pool_kernel): per-segment mean and GeM, values on both sides of eps, empty segments exactly 0."""
    off, _ = seg
    x = _rows(1, c, paired, dev, "pool")
    hi, lo = _planes(x, paired, dev)
    pt = torch.tensor([p], dtype=torch.float32, device=dev)
    mean = torch.full((NSEG, c), float("nan"), device=dev) if mode != "gem" else None
    gem = torch.full((NSEG, c), float("nan"), device=dev) if mode != "mean" else None
    _ok(_L().agp_seg_pool_fwd(_ptr(hi), _ptr(lo), _ptr(off), NSEG, c, _ptr(pt) if gem is not None else None, 1e-6, _ptr(mean), _ptr(gem),
                              _stream()), "agp_seg_pool_fwd")
    xd = x.to(dev)
    if mean is not None:
        _per_segment(mean, R.seg_mean64(xd, off), SEG_BAR[paired], "mean c %d" % c, True)
    if gem is not None:
        _per_segment(gem, R.seg_gem64(xd, off, p), SEG_BAR[paired], "GeM p %.1f c %d" % (p, c), True)


_COMBO_IDS = ["".join(n for n, on in zip(("scale_", "add_", "res_", "relu_"), (k & 1, k & 2, k & 4, k & 8)) if on) or "copy"
              for k in range(16)]


@FMT
@pytest.mark.parametrize("combo", range(16), ids=_COMBO_IDS)
def test_seg_affine_fwd(dev, seg, paired, combo):
    """agp_seg_affine_fwd: relu?(y * scale[b] + add[b] + res) with every part present or absent; on every third combination
    (1, 4, 7, 10, 13: with and without each part) n_dev cuts the rows inside the 70 001-row segment and the rows past it keep
    their fill pattern.  c walks 64 / 128 / 256 over the combinations, one step apart in the two formats.  Bar: every 128 x 64
    granule below the conv bar of the format (fp32 arithmetic on stored operands, the result stored: what the conv epilogue
    does)."""
    off, bidx = seg
    c = (64, 128, 256)[(combo // 3 + (1 if paired else 0)) % 3]
    g = torch.Generator().manual_seed(combo)
    y = _rows(2, c, paired, dev)
    res = _rows(3, c, paired, dev) if combo & 4 else None
    scale = (0.5 + torch.rand((NSEG, c), generator=g)).to(dev) if combo & 1 else None
    add = torch.randn((NSEG, c), generator=g).to(dev) if combo & 2 else None
    n_dev = 40001 if combo % 3 == 1 else None
    y_hi, y_lo = _planes(y, paired, dev)
    r_hi, r_lo = _planes(res, paired, dev) if res is not None else (None, None)
    o_hi, o_lo, bufs = _guarded(NROWS, c, paired, dev)
    nd = None if n_dev is None else torch.tensor([n_dev], dtype=torch.int64, device=dev)
    _ok(_L().agp_seg_affine_fwd(_ptr(y_hi), _ptr(y_lo), _ptr(bidx), _ptr(scale), _ptr(add), _ptr(r_hi), _ptr(r_lo), NROWS, c,
                                1 if combo & 8 else 0, _ptr(o_hi), _ptr(o_lo), _ptr(nd), _stream()), "agp_seg_affine_fwd")
    nv = NROWS if n_dev is None else n_dev
    _assert_frame(o_hi, o_lo, bufs, NROWS, written=(0, nv), filled=(nv, NROWS))
    ref = (_bf16_pair if paired else _f16)(R.seg_affine64(y.to(dev), bidx, scale, add, None if res is None else res.to(dev),
                                                               bool(combo & 8)))
    _assert_granules(_value(o_hi, o_lo, 0, nv), ref[:nv], BARS[3 if paired else 4], "seg_affine combo %d c %d" % (combo, c))


@FMT
@pytest.mark.parametrize("c", [64, 128, 256])
@pytest.mark.parametrize("second", [True, False], ids=["dot", "sum"])
def test_seg_dot_fwd(dev, seg, paired, c, second):
    """agp_seg_dot_fwd: per-segment sum of a * b (the ECA scale gradient), or of a alone (the gradient of a broadcast add)."""
    off, _ = seg
    a, b = _rows(4, c, paired, dev), (_rows(5, c, paired, dev) if second else None)
    a_hi, a_lo = _planes(a, paired, dev)
    b_hi, b_lo = _planes(b, paired, dev) if second else (None, None)
    out = torch.full((NSEG, c), float("nan"), device=dev)
    _ok(_L().agp_seg_dot_fwd(_ptr(a_hi), _ptr(a_lo), _ptr(b_hi), _ptr(b_lo), _ptr(off), NSEG, c, _ptr(out), _stream()), "agp_seg_dot_fwd")
    _per_segment(out, R.seg_dot64(a.to(dev), None if b is None else b.to(dev), off), SEG_BAR[paired], "seg_dot c %d" % c, True)


@FMT
@pytest.mark.parametrize("c", [64, 128, 256])
@pytest.mark.parametrize("case", ["base_gmean", "gmean", "gem_p3_all", "gem_p2.5_only"])
def test_seg_pool_bwd(dev, seg, paired, c, case):
    """agp_seg_pool_bwd: base + gmean / n_b + the GeM term, and dL/dp accumulated ONTO a non-zero start value, against the closed
    forms of sparse_kernel_ref.seg_pool_bwd64 and fp64 autograd of the reference GeM for dL/dp.  bidx holds no empty segment (no
    row belongs to one), as in the product.  Rows: every segment's rows by themselves (their magnitudes differ by 1 / n_b).  dL/dp:
    2e-5 of the sum of the absolute per-(segment, channel) terms (ggem is positive: little cancellation) + the fp32 spacing of
    the start value."""
    from agplace_amd import _lib
    off, bidx = seg
    p = 2.5 if "2.5" in case else 3.0
    gen = torch.Generator().manual_seed(len(case) + c)
    x = _rows(1, c, paired, dev, "pool")
    xd = x.to(dev)
    base = _rows(6, c, paired, dev) if case in ("base_gmean", "gem_p3_all") else None
    gmean = torch.randn((NSEG, c), generator=gen).to(dev) if case != "gem_p2.5_only" else None
    use_gem = case.startswith("gem")
    ggem = (0.5 + torch.rand((NSEG, c), generator=gen)).to(dev) if use_gem else None
    pt64 = torch.tensor(p, dtype=torch.float64, device=dev, requires_grad=True)
    gem64 = R.seg_gem64(xd, off, pt64)
    gem_y = gem64.detach().float().contiguous() if use_gem else None
    x_hi, x_lo = _planes(x, paired, dev)
    b_hi, b_lo = _planes(base, paired, dev) if base is not None else (None, None)
    o_hi, o_lo, bufs = _guarded(NROWS, c, paired, dev, zero_row=False)
    gp = torch.zeros(_lib.GP_FLOATS, dtype=torch.float32, device=dev)
    gp[0] = 1.25
    pt = torch.tensor([p], dtype=torch.float32, device=dev)
    _ok(_L().agp_seg_pool_bwd(_ptr(x_hi), _ptr(x_lo), _ptr(bidx), _ptr(off), _ptr(gmean), _ptr(ggem), _ptr(gem_y),
                              _ptr(pt) if use_gem else None, 1e-6, _ptr(b_hi), _ptr(b_lo), NROWS, c, _ptr(o_hi), _ptr(o_lo),
                              _ptr(gp) if use_gem else None, _stream()), "agp_seg_pool_bwd")
    _assert_frame(o_hi, o_lo, bufs, NROWS, written=(0, NROWS), zero_row=False)
    ref, _ = R.seg_pool_bwd64(xd, off, gmean, ggem, None if gem_y is None else gem_y.double(), p, base=base)
    rnd = _bf16_pair if paired else _f16
    _per_segment_rows(_value(o_hi, o_lo, 0, NROWS), rnd(ref), SEG_BAR[paired], "seg_pool_bwd " + case)
    if use_gem:
        (dp_auto,) = torch.autograd.grad((gem64 * ggem.double()).sum(), pt64)
        mag = R.gem_dp_magnitude64(xd, off, ggem, gem_y, p)
        got = float(gp[0]) - 1.25
        print("seg_pool_bwd %s c %d: dL/dp %.6e, fp64 autograd %.6e" % (case, c, got, float(dp_auto)))
        assert abs(got - float(dp_auto)) <= 2e-5 * mag + 2.0 ** -22 * max(1.25, abs(float(dp_auto)))


@pytest.mark.parametrize("c", [64, 128, 256])
@pytest.mark.parametrize("k", [3, 5])
def test_eca_scale_fwd_and_bwd(dev, seg, k, c):
    """agp_eca_scale_fwd / agp_eca_scale_bwd on the [B, C] vectors: the Conv1d over the channel axis with zero padding (the k / 2
    channels at both ends of the axis are held to the bar one by one: a window that wrapped or read the neighbouring sample's row
    would show there), the sigmoid, and the backward's dL/dmean spread over each segment's rows (0 for an empty segment) and dL/dw.
    fp32 vectors in and out: 2e-5, the bar of the pair-format rows they scale."""
    off, _ = seg
    g = torch.Generator().manual_seed(10 * k + c)
    mean = torch.randn((NSEG, c), generator=g).to(dev)
    mean[0] = mean[3] = mean[5] = 0                                          # what agp_seg_pool_fwd gives for the empty segments
    w = (0.7 * torch.randn(k, generator=g)).to(dev)
    gs = torch.randn((NSEG, c), generator=g).to(dev)
    s = torch.full((NSEG, c), float("nan"), device=dev)
    _ok(_L().agp_eca_scale_fwd(_ptr(mean), NSEG, c, _ptr(w), k, _ptr(s), _stream()), "agp_eca_scale_fwd")
    ref = R.eca64(mean, w)
    assert float((s.double() - ref).norm() / ref.norm()) < 2e-5
    ends = list(range(k // 2 + 1)) + list(range(c - k // 2 - 1, c))
    assert bool(((s.double() - ref)[:, ends].abs() <= 2e-5 * ref[:, ends].abs()).all())
    add = torch.full((NSEG, c), float("nan"), device=dev)
    gw = torch.full((k,), float("nan"), device=dev)
    _ok(_L().agp_eca_scale_bwd(_ptr(mean), _ptr(s), _ptr(gs), _ptr(off), NSEG, c, _ptr(w), k, _ptr(add), _ptr(gw), _stream()),
        "agp_eca_scale_bwd")
    add_ref, gw_ref = R.eca_bwd64(mean, s, gs, off, w)                       # (from the scale the kernel was given)
    _per_segment(add, add_ref, 2e-5, "eca_bwd add k %d c %d" % (k, c))
    for b in (1, 2, 4):
        assert bool(((add[b].double() - add_ref[b])[ends].abs() <= 2e-5 * add_ref[b].abs().max()).all())
    assert float((gw.double() - gw_ref).norm() / gw_ref.norm()) < 2e-5
