"""-m gpu: the dense weight-gradient kernels of csrc/wgrad_tr.hip one by one -- wgrad_tr_kernel<0, 9> (3x3 stride 1, three bf16
products), wgrad_tr_kernel<1, NB> (stride-2 3x3, 1x1, the packed 7x7 stem), the one-pass fp16 kernels wgrad_f16_kernel and
wgrad_gather_f16_kernel<NB>, and their split-K reduction wgrad_reduce_kernel -- against the plain fp64 gradient of
tests/dense_train_ref.py (pinned to autograd by tests/test_dense_train_ref.py) on the SAME stored operands.
tests/test_gpu_train.py takes one rel_l2 over a whole weight tensor at the network's shapes; here the shapes are chosen for the
kernels (dense_train_ref.CASES: the regime of each is asserted on the CPU through the plan mirror) and every
(tap, 32 ci, 32 co) granule -- one MFMA accumulator tile -- meets the bar by itself.

Bars (not derived from the kernels): three products 1e-4 per granule; one pass 1e-3 per granule and 2e-3 per output channel,
and MORE than 3e-5 on the whole tensor (the fp16 kernel really ran) -- test_one_pass_fp16_weight_gradient's bars, per granule.
The arithmetic's own floor (test_dense_train_ref.py): 3.1e-6 / 2.4e-4 per granule.

Measured on an MI355X over every case and gradient scale (worst granule / worst output channel / whole tensor):
  three products   2.8e-6 .. 3.5e-6 / 3.5e-6 .. 6.4e-6 / 2.6e-6 .. 3.0e-6
  one pass         2.1e-4 .. 2.6e-4 / 3.2e-4 .. 5.3e-4 / 2.0e-4 .. 2.3e-4
Both kernels sit on their arithmetic's floor in every regime -- one K-step or 507 splits, exact or ragged A-block groups, gradients
of 3e-7 or 1e4: the three-product figure is the lo x lo term it leaves out, the one-pass figure the fp16 rounding of its operands."""
import ctypes as C
import os
import re

import pytest
import torch

import dense_train_ref as R
from conv_sched_util import GUARD, GUARD_BITS

pytestmark = pytest.mark.gpu

GUARD32, FILL32 = 0x7FC0DEAD, 0x7FC0BEEF        # two quiet-NaN patterns of the fp32 buffers: guard regions, pre-filled interior
WS_TAIL = 1024                                  # floats behind the workspace's splits * rows * cout that no call may touch


def _header_code(name):
    """An AGP_* return code as include/agplace_hip.h defines it."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    m = re.search(r"#define %s (\d+)" % name, open(os.path.join(root, "include", "agplace_hip.h")).read())
    assert m, "%s not found in the header" % name
    return int(m.group(1))


BADARG, UNSUPPORTED = _header_code("AGP_E_BADARG"), _header_code("AGP_E_UNSUPPORTED")


def _L():
    from agplace_amd import _lib
    return _lib.load()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------------------------ buffers
def _guard16(plane):
    """A 16-bit plane in the middle of a larger buffer of GUARD_BITS -> (the plane's view, the buffer)"""
    n = plane.numel()
    buf = torch.full((GUARD + n + GUARD,), GUARD_BITS, dtype=torch.int16, device=plane.device)
    buf[GUARD:GUARD + n] = plane.contiguous().view(torch.int16).flatten()
    return buf[GUARD:GUARD + n].view(plane.shape).view(plane.dtype), buf


def _guard32(numel, dev, start=None):
    """numel fp32 words pre-filled with FILL32 (or holding `start`) between guard regions of GUARD32 -> (view, buffer)"""
    buf = torch.full((GUARD + numel + GUARD,), GUARD32, dtype=torch.int32, device=dev)
    mid = buf[GUARD:GUARD + numel]
    if start is None:
        mid.fill_(FILL32)
    else:
        mid.copy_(start.contiguous().view(torch.int32).flatten())
    return mid.view(torch.float32), buf


def _guards_intact(buf):
    return bool((buf[:GUARD] == (GUARD32 if buf.dtype == torch.int32 else GUARD_BITS)).all()) and \
        bool((buf[-GUARD:] == (GUARD32 if buf.dtype == torch.int32 else GUARD_BITS)).all())


def _halo_is_zero(plane, pad):
    b = plane.view(torch.int16)
    return not bool(b[:, :pad].any() or b[:, -pad:].any() or b[:, :, :pad].any() or b[:, :, -pad:].any())


# ----------------------------------------------------------------------------------------------------------------- problems
class Problem:
    """One weight-gradient problem on the device: stored operands, their planes inside guard buffers, the exact per-channel
    maxima, the fp64 reference."""

    def __init__(self, dev, name, gscale=1.0, zero_channel=None):
        self.name, self.dev, self.stem = name, dev, R.is_stem(name)
        self.cin, self.cout, self.k = R.CASES[name][0][0], R.CASES[name][0][1], R.CASES[name][0][2]
        x, g = R.draw_wgrad(name, gscale, dev=dev)
        if zero_channel is not None:
            g[:, zero_channel] = 0
        self.pin = 3 if self.stem else 1
        xm = R.nhwc_map(x, self.pin, channels=4 if self.stem else None)
        gm = R.nhwc_map(g, 1)
        hi, lo = R.planes(xm, True)
        h16, _ = R.planes(xm, False)                       # the same x once more as ONE fp16 plane: both kernels see one x
        g_hi, g_lo = R.planes(gm, True)
        self.bufs = []
        for attr, p in (("x_hi", hi), ("x_lo", lo), ("x_h16", h16), ("g_hi", g_hi), ("g_lo", g_lo)):
            view, buf = _guard16(p)
            setattr(self, attr, view)
            self.bufs.append(buf)
        # the halos are zero: the kernels' contract (the K raster runs over the gradient's halo, the taps reach into x's)
        assert _halo_is_zero(self.x_hi, self.pin) and _halo_is_zero(self.x_lo, self.pin) and _halo_is_zero(self.x_h16, self.pin)
        assert _halo_is_zero(self.g_hi, 1) and _halo_is_zero(self.g_lo, 1)
        am = (self.g_hi.float() + self.g_lo.float()).abs().amax((0, 1, 2))           # exact: the kernels add the pair in fp32 too
        assert torch.equal(am.double(), g.abs().amax((0, 2, 3)))
        self.absmax = am.contiguous().view(torch.int32).clone()
        self.ref = R.reference(name, x, g)
        self.plan3, self.plan1 = R.plans(name)
        self.rows = self.plan3["rows"]
        self.shape = (7, 8, 4, self.cout) if self.stem else (self.k, self.k, self.cin, self.cout)

    def desc(self, one_pass, absmax=None, in_lo=True):
        d = R.wgrad_desc(self.name)
        d.in_hi, d.in_lo = _ptr(self.x_hi), (_ptr(self.x_lo) if in_lo else None)
        d.out_hi, d.out_lo = _ptr(self.g_hi), _ptr(self.g_lo)
        d.in_h16 = _ptr(self.x_h16) if one_pass else None
        d.out_absmax = _ptr(absmax) if one_pass else None
        return d

    def run(self, one_pass, param=None, start=None):
        """One call with the workspace and dW in guard buffers -> dW (fp32, the call's layout).  param: None = agp_conv2d_wgrad,
        0 / 1 = agp_conv2d_wgrad_param with that `accumulate` (onto `start`).  Asserts the frame of the call."""
        L, dev = _L(), self.dev
        am = torch.cat([self.absmax, torch.full((64,), 0x5A5A5A5A, dtype=torch.int32, device=dev)]) if one_pass else None
        d = self.desc(one_pass, am)
        nbytes = int(L.agp_conv2d_wgrad_workspace_bytes(C.byref(d)))
        plan = R.wgrad_plan(*R.CASES[self.name][0], f16=one_pass, stem=self.stem)
        assert nbytes == plan["splits"] * self.rows * self.cout * 4
        ws, ws_buf = _guard32(nbytes // 4 + WS_TAIL, dev)
        gw, gw_buf = _guard32(self.rows * self.cout, dev, start)
        if param is None:
            rc = L.agp_conv2d_wgrad(C.byref(d), _ptr(gw), _ptr(ws), nbytes, _stream())
        else:
            rc = L.agp_conv2d_wgrad_param(C.byref(d), _ptr(gw), param, _ptr(ws), nbytes, _stream())
        assert rc == 0, "the call returned %d" % rc
        torch.cuda.synchronize()
        for b in self.bufs + [ws_buf, gw_buf]:
            assert _guards_intact(b), "a guard region was written"
        assert bool((ws.view(torch.int32)[nbytes // 4:] == FILL32).all()), "the workspace was written past splits * rows * cout floats"
        left = int((gw.view(torch.int32) == FILL32).sum())
        assert left == 0, "%d elements of dW were not written" % left
        assert bool(torch.isfinite(gw).all()), "dW is not finite (a read outside a plane brings a guard value in)"
        if one_pass:
            runs_one_pass = plan["one_pass"]
            assert bool((am[self.cout:] == 0x5A5A5A5A).all()), "words behind out_absmax[cout] were written"
            if runs_one_pass:
                assert not bool(am[:self.cout].any()), "out_absmax is not all zero after a one-pass call"
            else:
                assert torch.equal(am[:self.cout], self.absmax), "a three-product call touched out_absmax"
        return gw

    def check(self, gw, one_pass, what):
        got = R.comparable(self.name, gw.view(self.shape))
        worst, where, _ = R.granule_rel(got, self.ref)
        chan, ch, _ = R.per_out_channel_rel(got, self.ref)
        whole = R.whole_rel(got, self.ref)
        bar = R.BAR_1P if one_pass else R.BAR_3P
        print("%s %s: worst granule %.3e at %s, worst output channel %.3e (%d), whole tensor %.3e, bar %.1e" % (
            what, "one pass" if one_pass else "three products", worst, where, chan, ch, whole, bar))
        assert worst < bar, "%s: granule %s has %.3e (bar %.1e; whole tensor %.3e)" % (what, where, worst, bar, whole)
        if one_pass:
            assert chan < R.BAR_1P_CHANNEL, "%s: output channel %d has %.3e" % (what, ch, chan)
            assert whole > R.ONE_PASS_REALLY_RAN, "%s: %.3e on the whole tensor is not an fp16 product's error" % (what, whole)
        if self.stem:
            assert not bool(gw.view(self.shape)[:, :, 3].any()), "the stem's zero channel has a gradient"


@pytest.fixture(scope="module")
def problems(dev):
    """problems(name, gscale): the Problem of a case, built once for the tests of this file that share it (reference included)"""
    cache = {}

    def get(name, gscale=1.0):
        if (name, gscale) not in cache:
            cache[(name, gscale)] = Problem(dev, name, gscale)
        return cache[(name, gscale)]
    yield get
    cache.clear()


# ------------------------------------------------------------------------------------------------------------------- parity
RUNS = [(name, gs, one_pass) for name in R.CASES for gs in R.GSCALES.get(name, (1.0,))
        for one_pass in ((False, True) if R.plans(name)[1] is not None else (False,))]


@pytest.mark.parametrize("name,gscale,one_pass", RUNS, ids=["%s-g%g-%s" % (n, g, "one_pass" if o else "three_products") for n, g, o in RUNS])
def test_wgrad_matches_fp64_in_every_granule(dev, problems, name, gscale, one_pass):
    """Every case of dense_train_ref.CASES through agp_conv2d_wgrad: the three-product kernel, and the one-pass kernel wherever the
    library takes one (in_h16 + out_absmax = the exact per-channel max |g|).  Workspace and dW lie between guard regions and
    start as a NaN pattern: dW is written everywhere (not added to), finite, the workspace untouched past the plan's partials,
    out_absmax re-zeroed by a one-pass call; a second call gives the same bits."""
    pr = problems(name, gscale)
    p = pr.plan1 if one_pass else pr.plan3
    what = "%s gscale %g (%d splits of %d K-steps, the last %d)" % (name, gscale, p["splits"], p["per"], p["last"])
    gw = pr.run(one_pass)
    pr.check(gw, one_pass, what)
    again = pr.run(one_pass)
    assert torch.equal(gw.view(torch.int32), again.view(torch.int32)), "a repeated call gives other bits"


@pytest.mark.parametrize("name", ["gx3", "one_kstep"])
def test_in_h16_on_a_shape_without_a_one_pass_kernel_runs_three_products(dev, problems, name):
    """3x3 stride 1 with cin % 64 != 0: the library takes the three-product kernel even when the descriptor carries in_h16 /
    out_absmax (conv2d_wgrad_impl) -- the result is the three-product call's, bit for bit, and out_absmax is left alone (run()
    asserts it)."""
    pr = problems(name)
    assert pr.plan1 is None
    gw = pr.run(True)
    pr.check(gw, False, name + " with in_h16")
    assert torch.equal(gw.view(torch.int32), pr.run(False).view(torch.int32))


@pytest.mark.parametrize("name", ["s1_small", "ds_ragged2", "stem"])
@pytest.mark.parametrize("one_pass", [False, True], ids=["three_products", "one_pass"])
def test_a_channel_without_gradient_gets_exact_zeros(dev, name, one_pass):
    """One output channel's gradient map is all zero: its absmax word is 0 (the one-pass scale exponent is then 0, not 13 + 127),
    and its slice of dW is exactly 0 in every kernel: wgrad_tr_kernel<0, 9> / <1, 2> / <1, 7>, wgrad_f16_kernel,
    wgrad_gather_f16_kernel<2> / <7>.  The other channels meet their bars as before."""
    zc = 37
    pr = Problem(dev, name, zero_channel=zc)
    assert int(pr.absmax[zc]) == 0 and int((pr.absmax == 0).sum()) == 1
    gw = pr.run(one_pass)
    assert bool((gw.view(pr.shape)[..., zc] == 0).all()), "the zero channel's gradient is not exactly 0"
    pr.check(gw, one_pass, "%s, channel %d zero" % (name, zc))


# --------------------------------------------------------------------------------------------------- layouts, accumulation
@pytest.mark.parametrize("name", ["s1_small", "s1_splits", "s2_entry", "s2_entry_splits", "p1_ragged4"])
@pytest.mark.parametrize("one_pass", [False, True], ids=["three_products", "one_pass"])
def test_param_layout_and_accumulate_are_bit_exact(dev, problems, name, one_pass):
    """agp_conv2d_wgrad_param writes the nn.Conv2d layout [co][ci][ky][kx] from the same partials in the same order:
    accumulate = 0 equals agp_conv2d_wgrad permuted, bit for bit; accumulate = 1 onto a non-zero tensor t0 equals t0 + fresh in
    fp32 (added exactly once); a repeated call gives the same bits.  With one split (the plain call of the three-product kernel
    stores directly, the parameter call goes through wgrad_reduce_kernel) and with several."""
    pr = problems(name)
    p = pr.plan1 if one_pass else pr.plan3
    assert (p["splits"] > 1) == name.endswith("splits")
    plain = pr.run(one_pass).view(pr.shape)
    want = plain.permute(3, 2, 0, 1).contiguous()
    fresh = pr.run(one_pass, param=0).view(want.shape)
    assert torch.equal(fresh.view(torch.int32), want.view(torch.int32)), "the parameter layout differs from the plain one"
    gen = torch.Generator(device=dev).manual_seed(5)
    t0 = torch.randn(want.shape, generator=gen, device=dev) * float(want.abs().mean())
    acc = pr.run(one_pass, param=1, start=t0).view(want.shape)
    assert torch.equal(acc.view(torch.int32), (t0 + want).view(torch.int32)), "accumulate does not add the gradient exactly once"
    again = pr.run(one_pass, param=1, start=t0).view(want.shape)
    assert torch.equal(acc.view(torch.int32), again.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_out_of_contract_calls_are_refused_before_any_launch(dev, problems):
    """Return codes only; every refused call leaves dW, the workspace and out_absmax as they were."""
    L = _L()
    pr = problems("s1_small")
    am = pr.absmax.clone()
    nbytes = int(L.agp_conv2d_wgrad_workspace_bytes(C.byref(pr.desc(False))))
    ws, _ = _guard32(nbytes // 4 + WS_TAIL, dev)
    gw, _ = _guard32(pr.rows * pr.cout, dev)

    def call(d, nb=nbytes, param=None):
        if param is None:
            return L.agp_conv2d_wgrad(C.byref(d), _ptr(gw), _ptr(ws), nb, _stream())
        return L.agp_conv2d_wgrad_param(C.byref(d), _ptr(gw), param, _ptr(ws), nb, _stream())
    assert call(pr.desc(False), nbytes - 1) == BADARG                               # a workspace one byte short
    assert call(pr.desc(False), nbytes - 1, param=0) == BADARG
    d = pr.desc(True, am)
    d.out_absmax = None
    assert call(d) == BADARG                                                        # in_h16 without out_absmax
    d = pr.desc(True, am)
    d.in_h16 = None
    assert call(d) == BADARG                                                        # ... and the reverse
    assert call(pr.desc(False, in_lo=False)) == BADARG                              # three products without in_lo
    g3 = problems("gx3")
    d = g3.desc(True, g3.absmax.clone(), in_lo=False)                               # in_h16 given, but cin = 96: three products
    n3 = int(L.agp_conv2d_wgrad_workspace_bytes(C.byref(d)))
    w3, _ = _guard32(n3 // 4 + WS_TAIL, dev)
    o3, _ = _guard32(g3.rows * g3.cout, dev)
    assert L.agp_conv2d_wgrad(C.byref(d), _ptr(o3), _ptr(w3), n3, _stream()) == BADARG
    for shape in ((48, 64, 3, 1, 13, 17, 3), (64, 96, 3, 1, 13, 17, 3), (48, 64, 1, 1, 13, 17, 3)):
        d = R.desc_of(shape)
        assert int(L.agp_conv2d_wgrad_workspace_bytes(C.byref(d))) == -1
        d.in_hi, d.in_lo, d.out_hi, d.out_lo = _ptr(pr.x_hi), _ptr(pr.x_lo), _ptr(pr.g_hi), _ptr(pr.g_lo)
        assert call(d) == UNSUPPORTED and call(d, param=0) == UNSUPPORTED
    st = problems("stem")
    ns = int(L.agp_conv2d_wgrad_workspace_bytes(C.byref(st.desc(False))))
    wst, _ = _guard32(ns // 4 + WS_TAIL, dev)
    ost, _ = _guard32(st.rows * st.cout, dev)
    for acc in (0, 1):                                                              # the packed stem's rows are not the parameter's
        assert L.agp_conv2d_wgrad_param(C.byref(st.desc(False)), _ptr(ost), acc, _ptr(wst), ns, _stream()) == UNSUPPORTED
    torch.cuda.synchronize()
    for t in (ws, gw, w3, o3, wst, ost):
        assert bool((t.view(torch.int32) == FILL32).all()), "a refused call wrote"
    assert torch.equal(am, pr.absmax)
