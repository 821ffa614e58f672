"""-m gpu: the COORDINATE half of the sparse-voxel branch, entry point by entry point, against references built by another method
(tests/sparse_coord_ref.py, pinned on the CPU by tests/test_sparse_coord_ref.py): agp_sparse_kernel_map_grid and
agp_sparse_kernel_map against neighbour tables from a Python dictionary (a dense occupancy volume on the 140 000-row cloud) --
exact integer equality -- and agp_sparse_conv0_fwd, which searches the keys itself, against the fp64 convolution over such a table,
every 128 x cout granule below the bar of its precision (conv_sched_util.BARS).  tests/test_gpu_sparse_kernels.py holds the
arithmetic half (the kernels that take a table as given); tests/test_gpu_sparse.py compares whole networks.

Clouds (sparse_coord_ref): `thin` (3 samples, the middle one empty, a tile across two samples), `slab` (a full 6 x 24 x 24 grid:
every tap present, search windows on both sides of conv0_mfma_kernel's 1536-key LDS copy at kernel 5), `edge` (voxels at
+-32511, sorted neighbours that are no neighbours in space), their coarsened levels, and `big` (140 000 rows: the second round of
conv0_mfma_kernel's 1024-workgroup grid, the grid-stride loop of kernel_map_kernel).  Every output lies inside a larger
pre-filled buffer; every test asserts what was written and that nothing else was.

Not reached: the grid-stride loop of kernel_map_grid_kernel starts at 8192 x 256 / ksize rows (about 420 000 at kernel 5, 700 000
at kernel 3); the product's capacity of 512 k rows at kernel 3 does not reach it, and neither does a cloud here.

The test cannot observe which search path (LDS window or global memory) conv0_mfma_kernel took for a tile: it asserts, through
sparse_coord_ref.tile_windows, that the slab's tiles lie on both sides of the kernel's rule, and that every tile's result is right.

Measured on one MI355X (worst 128 x cout granule of a case, the same in its five call forms; every table test: exact equality):
  matrix pipe, prec 4 (bar 6e-4)   thin 2.09e-4 .. 2.24e-4   slab 2.54e-4 .. 2.74e-4   edge 2.11e-4 .. 2.18e-4
                                   big 2.34e-4 .. 2.43e-4    stride 2 / 4 (levels) 2.22e-4 .. 2.85e-4   no epilogue (slab, k 5) 2.69e-4
  vector, prec 3 (bar 2e-5)        thin 2.57e-6 .. 2.66e-6   slab 3.03e-6 .. 3.21e-6   edge 2.43e-6   stride 2 2.72e-6
  vector, prec 2 (bar 4e-4)        thin 2.10e-4 .. 2.20e-4   slab 2.56e-4 .. 2.65e-4   stride 2 2.82e-4
  vector, prec 4 at kernel 7       thin 2.10e-4, 2.15e-4 (bar 6e-4)
These are the rounding of the stored output (one fp16 plane: 2^-11 / sqrt(3) = 2.8e-4 at most; a bf16 pair: about 3e-6); the fp32
accumulation of at most 343 products lies far below.  Windows of conv0_mfma_kernel by tile_windows: slab at kernel 5, 34 tiles,
156 .. 2532 keys, 11 fit the 1536 keys of the LDS copy and 23 do not; slab at kernel 3 and thin: all fit; big at kernel 5: 1094
tiles, none fits; big at kernel 3: 44 of 1094 fit.
"""
import numpy as np
import pytest
import torch

import sparse_coord_ref as C
import sparse_kernel_ref as R
from conv_sched_util import BARS, FILL_BITS, GUARD
from test_gpu_sparse_kernels import _assert_frame, _bits, _guarded, _header_code, _L, _ok, _ptr, _stream, _value

pytestmark = pytest.mark.gpu

BADARG = _header_code("AGP_E_BADARG")
UNSUPPORTED = _header_code("AGP_E_UNSUPPORTED")
SENT = -0x5A5A5A5B                      # int32 pre-fill of a table and its guard regions: no row number, no capacity


# ------------------------------------------------------------------------------------------------------- clouds and tables
def _dev64(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)


def _word(n, dev):
    return torch.tensor([n], dtype=torch.int64, device=dev)


def _up256(n):
    return (n + 255) // 256 * 256


class Cloud:
    """Sorted distinct coordinates with their keys and segment offsets, on the host and on the device."""

    def __init__(self, coords, nbatch, dev, tag):
        self.c, self.nb, self.n, self.tag, self.dev = coords, nbatch, coords.shape[0], tag, dev
        self.keys, self.seg = C.keys_of(coords), C.seg_offsets(coords, nbatch)
        self.keys_d = _dev64(self.keys if self.n else np.array([C.PAD_KEY]), dev)        # (never an empty allocation)
        self.seg_d = _dev64(self.seg, dev)

    def head(self, n):
        """The cloud of the first n rows (still sorted and distinct)"""
        return Cloud(self.c[:n], self.nb, self.dev, "%s[:%d]" % (self.tag, n))

    def padded(self, cap):
        """capacity-mode key array: `cap` rows, the padding sorts last"""
        k = np.full(cap, C.PAD_KEY, dtype=np.int64)
        k[:self.n] = self.keys
        return _dev64(k, self.dev)


class World:
    """The clouds and their reference tables, built once per module."""

    def __init__(self, dev):
        self.dev, self.clouds, self.tables = dev, {}, {}

    def cloud(self, name, stride=1):
        key = (name, stride)
        if key not in self.clouds:
            if stride == 1:
                c, nb = C.CLOUDS[name](0)
            else:
                lv, nb = C.levels(name, 0)
                c = lv[stride]
            self.clouds[key] = Cloud(c, nb, self.dev, "%s/%d" % key)
        return self.clouds[key]

    def ref(self, cin, cout, offsets, absent=None):
        """int32 [len(offsets), cout.n] on the device: the dictionary's table, the dense volume's on clouds too large for it"""
        absent = cin.n if absent is None else absent
        key = (cin.tag, cout.tag, tuple(offsets), absent)
        if key not in self.tables:
            build = C.table_dense if max(cin.n, cout.n) > 20000 else C.table_dict
            self.tables[key] = torch.from_numpy(build(cin.c, cout.c, offsets, absent)).to(self.dev)
        return self.tables[key]


@pytest.fixture(scope="module")
def world(dev):
    w = World(dev)
    yield w
    w.clouds.clear()
    w.tables.clear()


def _table_buf(ntaps, n_out, dev):
    """int32 [ntaps, n_out] in the middle of a larger buffer, everything pre-filled with SENT -> (table, whole buffer)"""
    buf = torch.full((GUARD + ntaps * n_out + GUARD,), SENT, dtype=torch.int32, device=dev)
    return buf[GUARD:GUARD + ntaps * n_out].view(ntaps, n_out), buf


def _guards_intact(buf):
    assert bool((buf[:GUARD] == SENT).all()) and bool((buf[-GUARD:] == SENT).all()), "a table's guard region was written"


def _assert_table(got, want, what):
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    t, j = (int(v) for v in bad[0])
    raise AssertionError("%s: %d of %d entries differ; the first: tap %d row %d holds %d, the reference %d" % (
        what, bad.shape[0], want.numel(), t, j, int(got[t, j]), int(want[t, j])))


def _map_grid(in_keys, n_in, out_keys, n_out, ksize, centered, stride, nbr, n_dev=None, n_in_dev=None, seg=None):
    return _L().agp_sparse_kernel_map_grid(_ptr(in_keys), n_in, _ptr(out_keys), n_out, ksize, centered, stride, _ptr(nbr), _ptr(n_dev),
                                           _ptr(n_in_dev), _ptr(seg), _stream())


def _map(in_keys, n_in, out_keys, n_out, dkey, ntaps, nbr, n_dev=None):
    return _L().agp_sparse_kernel_map(_ptr(in_keys), n_in, _ptr(out_keys), n_out, _ptr(dkey), ntaps, _ptr(nbr), _ptr(n_dev), _stream())


# ----------------------------------------------------------------------------------------------- agp_sparse_kernel_map_grid
CENTRED = [("thin", 1, 3), ("thin", 1, 5), ("slab", 1, 3), ("slab", 1, 5), ("edge", 1, 3), ("edge", 1, 5), ("thin", 2, 3),
           ("thin", 4, 3), ("slab", 2, 3), ("slab", 4, 3), ("big", 1, 3), ("big", 1, 5), ("thin", 1, 7)]


@pytest.mark.parametrize("name,stride,k", CENTRED, ids=["%s-stride%d-k%d" % c for c in CENTRED])
def test_map_grid_centred_equals_the_dictionary(dev, world, name, stride, k):
    """Exact mode (n_dev = n_in_dev = NULL): every entry of the centred k x k x k table of a level onto itself, with the input's
    segment offsets and without -- the two tables identical, every entry written, the guards not."""
    cl = world.cloud(name, stride)
    want = world.ref(cl, cl, C.offsets_centered(k, stride))
    tabs = []
    for seg in (cl.seg_d, None):
        nbr, buf = _table_buf(k ** 3, cl.n, dev)
        _ok(_map_grid(cl.keys_d, cl.n, cl.keys_d, cl.n, k, 1, stride, nbr, seg=seg), "agp_sparse_kernel_map_grid")
        _guards_intact(buf)
        assert not bool((nbr == SENT).any()), "an entry was not written"
        _assert_table(nbr, want, "%s k %d stride %d, %s" % (name, k, stride, "seg_off" if seg is not None else "no seg_off"))
        tabs.append(nbr)
    assert torch.equal(tabs[0], tabs[1])
    assert torch.equal(tabs[0][k ** 3 // 2], torch.arange(cl.n, dtype=torch.int32, device=dev))       # the centre tap: the row itself


CHILDREN = [("thin", 1), ("thin", 2), ("slab", 1), ("slab", 2)]


@pytest.mark.parametrize("name,stride", CHILDREN, ids=["%s-stride%d" % c for c in CHILDREN])
def test_map_grid_children_equals_the_dictionary(dev, world, name, stride):
    """ksize 2, centered 0: the children (level of `stride`) of every voxel of the next coarser level, in_keys != out_keys.  Every
    fine row occurs exactly once in the table."""
    fine, coarse = world.cloud(name, stride), world.cloud(name, 2 * stride)
    want = world.ref(fine, coarse, C.offsets_children(stride))
    tabs = []
    for seg in (fine.seg_d, None):
        nbr, buf = _table_buf(8, coarse.n, dev)
        _ok(_map_grid(fine.keys_d, fine.n, coarse.keys_d, coarse.n, 2, 0, stride, nbr, seg=seg), "agp_sparse_kernel_map_grid")
        _guards_intact(buf)
        _assert_table(nbr, want, "%s children of stride %d" % (name, stride))
        tabs.append(nbr)
    assert torch.equal(tabs[0], tabs[1])
    assert torch.equal(tabs[0][tabs[0] != fine.n].sort().values, torch.arange(fine.n, dtype=torch.int32, device=dev))


@pytest.mark.parametrize("rows", [None, 768, 1, 0], ids=["all_rows", "rows768", "rows1", "rows0"])
@pytest.mark.parametrize("kind", ["centred3", "centred5", "children"])
def test_map_grid_capacity_mode(dev, world, kind, rows):
    """Key arrays of `cap` > n rows padded with 0x7fff..., the valid counts in device words: rows below n hold the dictionary's
    table (absent = the capacity of the input array: its zero row), rows [n, roundup256(n)) hold that capacity too, rows beyond
    keep the pre-fill.  n = 4346 (no multiple of 256), 768 (an exact multiple: no row of the second kind), 1 and 0 (nothing is
    written).  `children`: input and output arrays of different capacities and counts."""
    slab = world.cloud("slab")
    fine = slab if rows is None else slab.head(rows)
    if kind == "children":
        out = Cloud(C.coarsen(fine.c, 2), fine.nb, dev, fine.tag + "/coarse")
        k, centered, offs = 2, 0, C.offsets_children(1)
    else:
        out = fine
        k, centered = int(kind[-1]), 1
        offs = C.offsets_centered(k, 1)
    cap_in, cap_out = _up256(fine.n) + 300, _up256(out.n) + (300 if out is fine else 427)
    want = world.ref(fine, out, offs, absent=cap_in)
    kin = fine.padded(cap_in)
    kout = kin if out is fine else out.padded(cap_out)
    tabs = []
    for seg in (fine.seg_d, None):
        nbr, buf = _table_buf(k ** 3, cap_out, dev)
        _ok(_map_grid(kin, cap_in, kout, cap_out, k, centered, 1, nbr, n_dev=_word(out.n, dev), n_in_dev=_word(fine.n, dev), seg=seg),
            "agp_sparse_kernel_map_grid")
        _guards_intact(buf)
        _assert_table(nbr[:, :out.n], want, "%s, %d of %d rows" % (kind, out.n, cap_out))
        assert bool((nbr[:, out.n:_up256(out.n)] == cap_in).all()), "a padding row of the last 256-row tile does not point at the zero row"
        assert bool((nbr[:, _up256(out.n):] == SENT).all()), "a row past the valid tiles was written"
        tabs.append(nbr)
    assert torch.equal(tabs[0], tabs[1])


def test_map_grid_refusals_write_nothing(dev, world):
    """An even centred kernel, kernel 8, stride 0 and NULL arrays return AGP_E_BADARG before a launch."""
    cl = world.cloud("thin")
    nbr, buf = _table_buf(512, cl.n, dev)
    k = cl.keys_d
    assert _map_grid(k, cl.n, k, cl.n, 2, 1, 1, nbr) == BADARG
    assert _map_grid(k, cl.n, k, cl.n, 4, 1, 1, nbr) == BADARG
    assert _map_grid(k, cl.n, k, cl.n, 8, 0, 1, nbr) == BADARG
    assert _map_grid(k, cl.n, k, cl.n, 0, 0, 1, nbr) == BADARG
    assert _map_grid(k, cl.n, k, cl.n, 3, 1, 0, nbr) == BADARG
    assert _map_grid(None, cl.n, k, cl.n, 3, 1, 1, nbr) == BADARG
    assert _map_grid(k, cl.n, None, cl.n, 3, 1, 1, nbr) == BADARG
    assert _map_grid(k, cl.n, k, cl.n, 3, 1, 1, None) == BADARG
    assert _map_grid(k, cl.n, k, 0, 3, 1, 1, nbr) == BADARG
    torch.cuda.synchronize()
    assert bool((buf == SENT).all())


# ---------------------------------------------------------------------------------------------------- agp_sparse_kernel_map
@pytest.mark.parametrize("name,stride", CHILDREN, ids=["%s-onto-stride%d" % c for c in CHILDREN])
def test_kernel_map_up_offsets_equal_the_dictionary(dev, world, name, stride):
    """The eight offsets SparseTensor.up_map passes (minus the child position) from the coarser level onto the finer one: every
    fine row has its parent through exactly one tap."""
    fine, coarse = world.cloud(name, stride), world.cloud(name, 2 * stride)
    offs = C.offsets_up(stride)
    want = world.ref(coarse, fine, offs)
    nbr, buf = _table_buf(8, fine.n, dev)
    _ok(_map(coarse.keys_d, coarse.n, fine.keys_d, fine.n, _dev64(C.key_offsets(offs), dev), 8, nbr), "agp_sparse_kernel_map")
    _guards_intact(buf)
    _assert_table(nbr, want, "%s up onto stride %d" % (name, stride))
    assert bool(((nbr != coarse.n).sum(0) == 1).all())


@pytest.mark.parametrize("name", ["big", "edge", "slab"])
def test_kernel_map_mixed_offsets_equal_the_reference(dev, world, name):
    """16 offsets of both signs in no order.  On `big`, 140 000 x 16 entries exceed the 8192 x 256 threads of the launch: the
    kernel's grid-stride loop runs its second trip."""
    cl = world.cloud(name)
    offs = C.offsets_mixed(16, seed=1)
    if name == "big":
        assert cl.n * 16 > 8192 * 256
    want = world.ref(cl, cl, offs)
    nbr, buf = _table_buf(16, cl.n, dev)
    _ok(_map(cl.keys_d, cl.n, cl.keys_d, cl.n, _dev64(C.key_offsets(offs), dev), 16, nbr), "agp_sparse_kernel_map")
    _guards_intact(buf)
    _assert_table(nbr, want, "%s, 16 mixed offsets" % name)
    assert torch.equal(nbr[offs.index((0, 0, 0))], torch.arange(cl.n, dtype=torch.int32, device=dev))


@pytest.mark.parametrize("rows", [None, 768, 1, 0], ids=["all_rows", "rows768", "rows1", "rows0"])
def test_kernel_map_capacity_mode(dev, world, rows):
    """out_keys padded to a capacity, the valid count in a device word (the input array is exact: the entry point has no
    n_in_dev): valid rows hold the dictionary's table, rows up to the next multiple of 256 hold n_in, rows beyond keep the
    pre-fill."""
    thin = world.cloud("thin")
    fine = thin if rows is None else thin.head(rows)
    coarse = world.cloud("thin", 2)
    offs = C.offsets_up(1)
    want = world.ref(coarse, fine, offs)
    cap = _up256(fine.n) + 300
    nbr, buf = _table_buf(8, cap, dev)
    _ok(_map(coarse.keys_d, coarse.n, fine.padded(cap), cap, _dev64(C.key_offsets(offs), dev), 8, nbr, n_dev=_word(fine.n, dev)),
        "agp_sparse_kernel_map")
    _guards_intact(buf)
    _assert_table(nbr[:, :fine.n], want, "up map, %d of %d rows" % (fine.n, cap))
    assert bool((nbr[:, fine.n:_up256(fine.n)] == coarse.n).all())
    assert bool((nbr[:, _up256(fine.n):] == SENT).all()), "a row past the valid tiles was written"


def test_kernel_map_without_input_rows_and_refusals(dev, world):
    """n_in = 0: every entry is absent (= n_in = 0).  NULL arrays, no taps, no output rows: AGP_E_BADARG, nothing written."""
    cl = world.cloud("thin")
    offs = C.offsets_up(1)
    dk = _dev64(C.key_offsets(offs), dev)
    nbr, buf = _table_buf(8, cl.n, dev)
    one = _dev64(np.array([C.PAD_KEY]), dev)
    _ok(_map(one, 0, cl.keys_d, cl.n, dk, 8, nbr), "agp_sparse_kernel_map")
    _guards_intact(buf)
    assert bool((nbr == 0).all())
    nbr, buf = _table_buf(8, cl.n, dev)
    assert _map(None, cl.n, cl.keys_d, cl.n, dk, 8, nbr) == BADARG
    assert _map(cl.keys_d, cl.n, None, cl.n, dk, 8, nbr) == BADARG
    assert _map(cl.keys_d, cl.n, cl.keys_d, cl.n, None, 8, nbr) == BADARG
    assert _map(cl.keys_d, cl.n, cl.keys_d, cl.n, dk, 8, None) == BADARG
    assert _map(cl.keys_d, cl.n, cl.keys_d, cl.n, dk, 0, nbr) == BADARG
    assert _map(cl.keys_d, cl.n, cl.keys_d, 0, dk, 8, nbr) == BADARG
    assert _map(cl.keys_d, -1, cl.keys_d, cl.n, dk, 8, nbr) == BADARG
    torch.cuda.synchronize()
    assert bool((buf == SENT).all())


# ----------------------------------------------------------------------------------------------------- agp_sparse_conv0_fwd
PAD_ROWS = 333          # capacity mode: the arrays have this many rows more than the cloud (no multiple of a tile)


def _conv0(keys, cap, n_dev, f, k, stride, w, cout, scale, shift, relu, hi, lo, seg, prec):
    return _L().agp_sparse_conv0_fwd(_ptr(keys), cap, _ptr(n_dev), _ptr(f), k, stride, _ptr(w), cout, _ptr(scale), _ptr(shift),
                                     1 if relu else 0, _ptr(hi), _ptr(lo), _ptr(seg), prec, _stream())


def _conv0_case(dev, world, name, stride, k, cout, prec, epi=True, f16_operands=False):
    """One problem through agp_sparse_conv0_fwd in its four call forms -- exact (cap = n, n_dev NULL) and capacity (cap = n + 333
    rows, keys padded, NaN in the padding of f, n in a device word), each with seg_off and with NULL -- plus a repeat of the first.
    Every form: the frame (rows >= n, the zero row `cap` and the guards keep their pre-fill, every element of the rows below n
    was written), every 128 x cout granule against the fp64 convolution over the dictionary's table below BARS[prec].  All five
    outputs hold the same bits (no atomics, the same tiles, the same window).  -> the worst granule"""
    cl = world.cloud(name, stride)
    n, ntaps, paired = cl.n, k ** 3, prec == 3
    g = torch.Generator().manual_seed(1000 * k + cout + 7 * prec + stride)
    f = torch.randn(n, generator=g)
    w = torch.randn((ntaps, cout), generator=g) / k ** 1.5
    if f16_operands:
        f, w = f.half().float(), w.half().float()
    scale = (0.5 + torch.rand(cout, generator=g)).to(dev) if epi else None
    shift = (0.3 * torch.randn(cout, generator=g)).to(dev) if epi else None
    f_d, w_d = f.to(dev), w.to(dev).contiguous()
    table = world.ref(cl, cl, C.offsets_centered(k, stride))
    ref = C.conv0_ref64(table, f_d, w_d, scale, shift, epi)
    cap = n + PAD_ROWS
    f_pad = torch.full((cap,), float("nan"), device=dev)
    f_pad[:n] = f_d
    forms = [("exact, seg_off", cl.keys_d, n, None, f_d, cl.seg_d), ("exact", cl.keys_d, n, None, f_d, None),
             ("capacity, seg_off", cl.padded(cap), cap, _word(n, dev), f_pad, cl.seg_d), ("capacity", cl.padded(cap), cap, _word(n, dev), f_pad, None),
             ("exact, seg_off, again", cl.keys_d, n, None, f_d, cl.seg_d)]
    what = "conv0 %s stride %d k %d cout %d prec %d%s" % (name, stride, k, cout, prec, "" if epi else " (no epilogue)")
    first, worst_all = None, 0.0
    for form, keys, rows, n_dev, fv, seg in forms:
        hi, lo, bufs = _guarded(rows, cout, paired, dev)
        _ok(_conv0(keys, rows, n_dev, fv, k, stride, w_d, cout, scale, shift, epi, hi, lo, seg, prec), "agp_sparse_conv0_fwd")
        _assert_frame(hi, lo, bufs, rows, written=(0, n), filled=(n, rows))
        got = _value(hi, lo, 0, n)
        assert bool(torch.isfinite(got).all()), "%s, %s: a non-finite output" % (what, form)
        worst, where, _ = R.granule_rel(got, ref, rows=128, cols=cout)
        worst_all = max(worst_all, worst)
        assert worst < BARS[prec], "%s, %s: granule %s has %.3e (bar %.1e)" % (what, form, where, worst, BARS[prec])
        planes = (_bits(hi)[:n].clone(),) + ((_bits(lo)[:n].clone(),) if lo is not None else ())
        if first is None:
            first = planes
            print("%s: worst 128 x %d granule %.3e at %s, bar %.1e" % (what, cout, worst, where, BARS[prec]))
        else:
            assert all(torch.equal(a, b) for a, b in zip(first, planes)), "%s: the form `%s` differs in bits from the first" % (what, form)
    return worst_all


MFMA = [(name, 1, k, cout, True) for name in ("thin", "slab", "edge", "big") for k in (3, 5) for cout in (32, 64)] + \
       [("slab", 1, 5, 64, False), ("thin", 2, 5, 64, True), ("slab", 2, 3, 32, True), ("slab", 4, 5, 32, True)]


@pytest.mark.parametrize("name,stride,k,cout,epi", MFMA, ids=["%s-stride%d-k%d-cout%d-%s" % (c[0], c[1], c[2], c[3], "bn_relu" if c[4] else "plain")
                                                                for c in MFMA])
def test_conv0_matrix_pipe_form(dev, world, name, stride, k, cout, epi):
    """AGP_PREC_F16 with out_lo = NULL and ksize <= 5: conv0_mfma_kernel.  Features and weights are drawn fp16-representable, so
    the kernel's conversions are exact and only the fp32 accumulation and the fp16 store remain.  thin: every window fits the
    LDS copy, a tile lies across two samples, no window ends on a key (sparse_coord_ref.window_end_keys_present); slab: most
    windows end on a key (a window one key short loses a tap there and nowhere on thin), at kernel 5 windows on both sides of the 1536 keys (asserted on the input,
    the kernel's own choice is not observable), interior rows with all 125 taps and the zero columns up to KP = 128; edge:
    offsets at the limit of the key fields; big: 1094 tiles on 1024 workgroups, every window in global memory."""
    cl = world.cloud(name, stride)
    win = C.tile_windows(cl.keys, k // 2, stride)
    above, below = int((win > C.C0_WK).sum()), int((win <= C.C0_WK).sum())
    print("%s stride %d k %d: %d tiles, windows %d..%d keys: %d fit the %d-key LDS copy, %d do not" % (
        name, stride, k, win.shape[0], int(win.min()), int(win.max()), below, C.C0_WK, above))
    if name == "slab" and stride == 1 and k == 5:
        assert above > 0 and below > 0
    if name == "thin":
        assert above == 0
    if name == "big":
        assert win.shape[0] > 1024
    _conv0_case(dev, world, name, stride, k, cout, 4, epi=epi, f16_operands=True)


VECTOR = [(name, 1, k, cout, prec) for prec in (3, 2) for name in ("thin", "slab") for k in (3, 5) for cout in (32, 64)] + \
         [("thin", 1, 7, 64, 4), ("thin", 1, 7, 32, 4), ("thin", 2, 3, 64, 3), ("slab", 2, 5, 32, 2), ("edge", 1, 5, 64, 3)]


@pytest.mark.parametrize("name,stride,k,cout,prec", VECTOR, ids=["%s-stride%d-k%d-cout%d-prec%d" % c for c in VECTOR])
def test_conv0_vector_form(dev, world, name, stride, k, cout, prec):
    """conv0_search_kernel: bf16-pair output (prec 3), one fp16 plane (prec 2), and AGP_PREC_F16 at kernel 7 -- past the
    `ksize <= 5` of the dispatch to the matrix-pipe form.  Unrounded fp32 features and weights: the kernel multiplies in fp32."""
    _conv0_case(dev, world, name, stride, k, cout, prec)


def test_conv0_refusals_write_nothing(dev, world):
    """cout 48: AGP_E_UNSUPPORTED; an even kernel, kernel 9, cap 0, stride 0, NULL pointers: AGP_E_BADARG -- before any launch."""
    cl = world.cloud("thin")
    hi, lo, bufs = _guarded(cl.n, 64, False, dev)
    f = torch.ones(cl.n, device=dev)
    w = torch.ones((729, 64), device=dev)
    k = cl.keys_d
    for prec in (4, 3):
        assert _conv0(k, cl.n, None, f, 5, 1, w, 48, None, None, False, hi, None, None, prec) == UNSUPPORTED
        assert _conv0(k, cl.n, None, f, 4, 1, w, 64, None, None, False, hi, None, None, prec) == BADARG
        assert _conv0(k, cl.n, None, f, 9, 1, w, 64, None, None, False, hi, None, None, prec) == BADARG
        assert _conv0(k, cl.n, None, f, 0, 1, w, 64, None, None, False, hi, None, None, prec) == BADARG
        assert _conv0(k, 0, None, f, 5, 1, w, 64, None, None, False, hi, None, None, prec) == BADARG
        assert _conv0(k, cl.n, None, f, 5, 0, w, 64, None, None, False, hi, None, None, prec) == BADARG
        assert _conv0(None, cl.n, None, f, 5, 1, w, 64, None, None, False, hi, None, None, prec) == BADARG
        assert _conv0(k, cl.n, None, None, 5, 1, w, 64, None, None, False, hi, None, None, prec) == BADARG
        assert _conv0(k, cl.n, None, f, 5, 1, None, 64, None, None, False, hi, None, None, prec) == BADARG
        assert _conv0(k, cl.n, None, f, 5, 1, w, 64, None, None, False, None, None, None, prec) == BADARG
    torch.cuda.synchronize()
    _assert_frame(hi, lo, bufs, cl.n, filled=(0, cl.n))
