"""-m gpu: the global pooling kernels one by one against the fp64 closed forms of tests/pool_ref.py (pinned to fp64 autograd by
tests/test_pool_ref.py, which also evaluates the floors and bars used here on the CPU and shows that each bar discriminates).

Every map input carries garbage (-3) in the halo of every plane: a result inside the bar proves that only the interior is read.
Values are drawn in the storage format (a bf16 pair, one fp16 plane, fp32) and both sides get the stored values.  Outputs lie
between poisoned guards; refusals return the header's AGP_E_BADARG and write nothing.  Image 0, channel 1 of every map is
negative throughout: GeM = eps there and its gx must be exact zeros (the only place the [x >= eps] mask shows).

Kernels and the branches reached
  agp_pool_fwd         split-bf16 and one-fp16-plane maps; c / 8 = 1, 3, 12, 48, 256 channel groups (3, 12, 48 do not divide the 256
                       threads: ppb * groups < 256 leaves idle tail threads; 256: one pixel lane); planes of 1, 9, 65 and 99 pixels (less
                       than one trip, ragged trips, a ragged last split); pad 1 and 3; p 3 (the cube path) and 2.5 (exp2 / log2);
                       mean only (p == NULL), GeM only, both; [1, 370, 370, 8]: 2048 splits (the cap) of 67 pixels, the last 4 empty;
                       the second stage at 8 splits (one trip, fp32) and 9 (fp64) on 2048 and 8192 planes, at 256 splits with
                       c = 384 and 2048, at 258 with c = 8; there also the mean alone and GeM alone.
  agp_pool_from_conv   1, 8, 9, 32, 33, 70 blocks per image (one wave's trip, a second wave, all four, a second trip, a third);
                       c 24 and 96 (a ragged last 64-channel block) and 64.
  agp_pool_f32_fwd /   NCHW, channels_last and a sliced non-contiguous view; n * c = 21, 1 (clamped dead waves in the last block) and
  agp_gem_f32_bwd      192; planes of 1, 15 and 99 pixels; gx == NULL; two calls into one gp; 16896 blocks (> AGP_GP_SLOTS: atomics).
  agp_pool_bwd         every non-empty subset of {base, gmean, ggem}, with and without gp; c 8, 24, 96, 2048; pad 1.

Bars: pool_ref's -- the mean and the map form without GeM min(4 x floor, ceiling), floor = the float32 form on the CPU (0 ..
1.2e-7 for the mean; 2.2e-6 .. 6.9e-6 for the map form, which stores a bf16 pair); GeM 1e-5, its gx 1e-4 per (image, channel),
dL/dp 1e-3 of its value (of the subtracted sum where every plane is constant after the clamp and dL/dp analytically zero).
MEASURED on an MI355X (the worst plane over all cases, beside its bar):
  agp_pool_fwd         mean 2.2e-7 (bar 6.4e-7; [3, 9, 11, 96], 2 splits).  The second stage: 8 splits in fp32 1.8e-7 over 2048 planes
                       and 2.1e-7 over 8192 (bars 6.6e-7 and 7.8e-7); in fp64 1.8e-7 at 9 splits, 6.1e-8 and 6.6e-8 at 256 splits over
                       384 and 2048 planes, 7.5e-8 at 258 and 8.2e-8 at 2048 splits over 8 planes.  (Added in fp32, the 2048
                       partials of [1, 370, 370, 8] gave 1.25e-6 on the GPU against the bar 6.8e-7, and a CPU replay of the fp32
                       chain gives 8.1e-7 at 256 splits over the 2048 planes of [1, 128, 128, 2048], bar 6.6e-7: the finding that
                       put the fp64 sum into pool_final_kernel for every count above one trip of 8.)  GeM 2.4e-6 (bar 1e-5; on the
                       all-clamp planes, eps^p through exp2 / log2 -- just under a quarter of the ceiling).  Repeats bit-equal.
  agp_pool_from_conv   mean 2.4e-7 (bar 6.6e-7), GeM 2.2e-7; repeats bit-equal.
  agp_pool_f32_fwd     mean 1.2e-7 (bar 6.9e-7), GeM 2.4e-6 (an all-clamp plane again).
  agp_gem_f32_bwd      gx 5.9e-7 per plane (bar 1e-4); dL/dp (bar 1e-3) 2.2e-6 of the subtracted sum on the all-clamp maps [1, 1, h, w],
                       1.7e-7 of the value elsewhere and 1.5e-6 on the atomic path; two calls give exactly twice the value.
  agp_pool_bwd         base alone exact; base / gmean 7.5e-6 (bar 3.0e-5: the bf16 pair's rounding, 2^-17 at the worst); with ggem
                       1.1e-5 (bar 1e-4; one-pixel planes, the pair's rounding again); dL/dp 2.1e-7 (bar 1e-3).
"""
import os
import re

import pytest
import torch

import pool_ref as P
from conv_sched_util import assert_only_the_interior_was_written, guarded_map

pytestmark = pytest.mark.gpu

GUARD = 4096
POISON = 0x7FC0BEEF              # a quiet NaN with a payload: nothing a kernel stores


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


class Out:
    """An fp32 output of `numel` elements (viewed as `shape`) in the middle of a poisoned buffer, `spare` poisoned elements behind"""

    def __init__(self, shape, dev, spare=64):
        self.shape = tuple(shape)
        self.numel = 1
        for s in self.shape:
            self.numel *= s
        self.buf = torch.full((GUARD + self.numel + spare + GUARD,), POISON, dtype=torch.int32, device=dev)
        self.t = self.buf[GUARD:GUARD + self.numel].view(torch.float32).view(self.shape)

    def ptr(self):
        return self.t.data_ptr()

    def guards_ok(self):
        torch.cuda.synchronize()
        return bool((self.buf[:GUARD] == POISON).all()) and bool((self.buf[GUARD + self.numel:] == POISON).all())

    def value(self, what):
        assert self.guards_ok(), "%s: written outside the output" % what
        assert not bool((self.buf[GUARD:GUARD + self.numel] == POISON).any()), "%s: elements of the output were not written" % what
        return self.t.cpu()

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf == POISON).all())


def _planes_ok(got, ref, bar, what, floor=None):
    rel = P.per_plane_rel(got, ref)
    worst = float(rel.max())
    print("%s: worst plane %.3e (bar %.3e%s)" % (what, worst, bar, "" if floor is None else ", float32 floor %.3e" % floor))
    i, ch = divmod(int(rel.argmax()), rel.shape[1])
    assert worst <= bar, "%s: image %d channel %d has %.3e (bar %.3e)" % (what, i, ch, worst, bar)
    assert not bool(torch.isnan(got).any()), "%s: NaN" % what


def _dp_ok(got, ref, x, p, y, gy, what):
    mag, sub = P.dp_magnitudes(x, p, P.GEM_EPS, y, gy)
    err = P.dp_error(got, float(ref), x, sub)
    print("%s: dL/dp %.6e (fp64 %.6e, sum |terms| %.3e): error %.3e (bar %.1e)" % (what, float(got), float(ref), mag, err, P.CEIL_GP))
    assert err <= P.CEIL_GP, "%s: dL/dp error %.3e (bar %.1e)" % (what, err, P.CEIL_GP)


def _map_on(dev, v, pad, paired):
    hi, lo = P.map_planes(v, pad, paired)
    return hi.to(dev), None if lo is None else lo.to(dev)


def _scalar(p, dev):
    return None if p is None else torch.tensor([p], dtype=torch.float32, device=dev)


# -------------------------------------------------------------------------------------------------------------- agp_pool_fwd
def _pool_fwd(dev, x, fmt, pad, p, want_mean, want_gem, what):
    """one agp_pool_fwd call, repeated -> (mean, gem) on the CPU; the repeat must be bit-equal"""
    L = _L()
    n, c, h, w = x.shape
    hi, lo = _map_on(dev, x, pad, fmt == "pair")
    pd = _scalar(p, dev)
    nfl = int(L.agp_pool_workspace_floats(n, c, h, w))
    seen = []
    for _ in range(2):
        part = Out((nfl,), dev)
        mean, gem = Out((n, c), dev), Out((n, c), dev)
        _ok(L.agp_pool_fwd(_ptr(hi), _ptr(lo), n, h, w, c, pad, _ptr(pd), P.GEM_EPS, mean.ptr() if want_mean else None,
                           gem.ptr() if want_gem else None, part.ptr(), _stream()), "agp_pool_fwd")
        assert part.guards_ok(), what + ": written outside the workspace"
        seen.append((mean.value(what + " mean") if want_mean else None, gem.value(what + " gem") if want_gem else None))
        assert want_mean or mean.untouched()
        assert want_gem or gem.untouched()
    for a, b in zip(*seen):
        assert (a is None and b is None) or torch.equal(a, b), what + ": a repeat is not bit-equal"
    return seen[0]


@pytest.mark.parametrize("n,h,w", P.POOL_NHW)
@pytest.mark.parametrize("c", P.POOL_C)
def test_pool_fwd(dev, c, n, h, w):
    for fmt, pad, p, want_mean, want_gem in P.POOL_FWD_VARIANTS:
        x = P.draw_map(n, c, h, w, 1, fmt)
        what = "pool_fwd [%d, %d, %d, %d] %s pad %d p %s%s%s" % (n, h, w, c, fmt, pad, p, " mean" if want_mean else "", " gem" if want_gem else "")
        mean, gem = _pool_fwd(dev, x, fmt, pad, p, want_mean, want_gem, what)
        if want_mean:
            bar, floor = P.mean_bar(x)
            _planes_ok(mean, P.mean(x), bar, what + ": mean", floor)
        if want_gem:
            _planes_ok(gem, P.gem(x, p), P.CEIL_FWD, what + ": GeM")


@pytest.mark.parametrize("n,h,w,c", list(P.POOL_MANY_SPLITS), ids=["%dx%dx%dx%d" % s for s in P.POOL_MANY_SPLITS])
def test_pool_fwd_with_many_splits(dev, n, h, w, c):
    """The second stage of agp_pool_fwd at its threshold and beyond: 8 splits (one trip, added in fp32) and 9 (fp64) at 2048
    and 8192 planes; 256 splits at c = 384 and c = 2048, where an fp32 chain of that length loses the bar on a few of the many
    planes; 258 at c = 8; [1, 370, 370, 8]: the split count at its cap, 2048, and the last 4 splits without a pixel.  Mean and
    GeM together, and (but for the widest map) the mean alone and GeM alone: the NULL outputs of both instantiations."""
    want_splits, want_empty = P.POOL_MANY_SPLITS[(n, h, w, c)]
    splits = int(_L().agp_pool_workspace_floats(n, c, h, w)) // (n * 2 * c)
    per, empty = P.split_pixels(n, c, h, w, splits)
    assert (splits, empty) == (want_splits, want_empty), "the case tests nothing: %d splits of %d pixels, %d empty" % (splits, per, empty)
    if (n, h, w, c) == P.POOL_LARGE:
        assert empty >= 1
    x = P.draw_map(n, c, h, w, 1, "pair")
    bar, floor = P.mean_bar(x)
    ref_mean = P.mean(x)
    variants = ((2.5, True, True),) if n * c * h * w > 4_000_000 else ((2.5, True, True), (None, True, False), (3.0, False, True))
    for p, want_mean, want_gem in variants:
        what = "pool_fwd [%d, %d, %d, %d] (%d splits)%s%s" % (n, h, w, c, splits, " mean" if want_mean else "", " gem" if want_gem else "")
        mean, gem = _pool_fwd(dev, x, "pair", 1, p, want_mean, want_gem, what)
        if want_mean:
            _planes_ok(mean, ref_mean, bar, what + ": mean", floor)
        if want_gem:
            _planes_ok(gem, P.gem(x, p), P.CEIL_FWD, what + ": GeM")


def test_pool_fwd_refusals(dev):
    L = _L()
    hi = torch.zeros(2 * 5 * 5 * 2056, dtype=torch.bfloat16, device=dev)
    pd = _scalar(3.0, dev)
    part, mean, gem = Out((2 * 2 * 2056 * 4,), dev), Out((2, 2056), dev), Out((2, 2056), dev)
    call = lambda c, p: L.agp_pool_fwd(_ptr(hi), _ptr(hi), 2, 3, 3, c, 1, _ptr(p), P.GEM_EPS, mean.ptr(), gem.ptr(), part.ptr(), _stream())
    assert call(12, pd) == BADARG, "c % 8"
    assert call(2056, pd) == BADARG, "c / 8 > 256"
    assert call(8, None) == BADARG, "gem_out without p"
    assert part.untouched() and mean.untouched() and gem.untouched()


# -------------------------------------------------------------------------------------------------------- agp_pool_from_conv
@pytest.mark.parametrize("c", P.FROM_CONV_C)
@pytest.mark.parametrize("h,w", P.FROM_CONV_HW)
def test_pool_from_conv(dev, h, w, c):
    L = _L()
    n, p = 2, 2.5
    blocks = P.from_conv_blocks(h, w)
    part = P.draw_partials(n, blocks, c, 9, p)
    pd_, partd = _scalar(p, dev), part.to(dev)
    rm, rg = P.from_partials(part, h * w, p)
    floor = P.worst_plane(P.from_partials(part, h * w, p, dtype=torch.float32)[0], rm)
    for want_mean, want_gem in ((True, False), (False, True), (True, True)):
        what = "pool_from_conv %d blocks c %d%s%s" % (blocks, c, " mean" if want_mean else "", " gem" if want_gem else "")
        seen = []
        for _ in range(2):
            mean, gem = Out((n, c), dev), Out((n, c), dev)
            _ok(L.agp_pool_from_conv(_ptr(partd), n, h, w, c, _ptr(pd_) if want_gem else None, mean.ptr() if want_mean else None,
                                     gem.ptr() if want_gem else None, _stream()), "agp_pool_from_conv")
            seen.append((mean.value(what) if want_mean else None, gem.value(what) if want_gem else None))
            assert (want_mean or mean.untouched()) and (want_gem or gem.untouched())
        for a, b in zip(*seen):
            assert (a is None and b is None) or torch.equal(a, b), what + ": a repeat is not bit-equal"
        if want_mean:
            _planes_ok(seen[0][0], rm, P.bar_of(floor, P.CEIL_FWD), what + ": mean", floor)
        if want_gem:
            _planes_ok(seen[0][1], rg, P.CEIL_FWD, what + ": GeM")
    mean = Out((n, c), dev)
    assert L.agp_pool_from_conv(_ptr(partd), n, h, w, c, None, None, None, _stream()) == BADARG, "no output at all"
    assert L.agp_pool_from_conv(_ptr(partd), n, h, w, c, None, mean.ptr(), mean.ptr(), _stream()) == BADARG, "gem_out without p"
    assert mean.untouched()


# ------------------------------------------------------------------------------------ agp_pool_f32_fwd and agp_gem_f32_bwd
def _layouts(x32, dev):
    """name -> (the [n, c, h, w] fp32 view on the device, the whole buffer behind it or None)"""
    n, c, h, w = x32.shape
    big = torch.full((n, c + 2, h + 1, w + 3), P.HALO_POISON, dtype=torch.float32)
    big[:, 1:c + 1, :h, 2:w + 2] = x32
    bigd = big.to(dev)
    return {"nchw": (x32.to(dev).contiguous(), None),
            "channels_last": (x32.to(dev).contiguous(memory_format=torch.channels_last), None),
            "sliced": (bigd[:, 1:c + 1, :h, 2:w + 2], bigd)}


def _gem_bwd_call(dev, xd, pd, yd, gyd, gp, with_gx):
    """-> the gx buffer (a poisoned tensor of x's strides, or None); gp accumulates"""
    n, c, h, w = xd.shape
    gx = None
    if with_gx:
        gx = torch.empty_strided(xd.shape, xd.stride(), dtype=torch.float32, device=dev)
        gx.view(torch.int32).fill_(POISON) if gx.is_contiguous() else gx.fill_(float("nan"))
    sn, sc, sh, sw = xd.stride()
    _ok(_L().agp_gem_f32_bwd(_ptr(xd), sn, sc, sh, sw, n, c, h, w, _ptr(pd), P.GEM_EPS, _ptr(yd), _ptr(gyd), _ptr(gx), _ptr(gp), _stream()),
        "agp_gem_f32_bwd")
    return gx


@pytest.mark.parametrize("h,w", P.F32_HW)
@pytest.mark.parametrize("n,c", P.F32_NC)
def test_pool_f32_fwd_and_gem_f32_bwd(dev, n, c, h, w):
    from agplace_amd import ops
    L = _L()
    x = P.draw_map(n, c, h, w, 7, "f32")
    gy = P.draw_vec(n, c, 8, positive=True)
    gyd = gy.to(dev)
    bar, floor = P.mean_bar(x)
    blocks = (n * c + 3) // 4
    for name, (xd, whole) in _layouts(x.float(), dev).items():
        before = None if whole is None else whole.clone()
        sn, sc, sh, sw = xd.stride()
        for p in (3.0, 2.5):
            what = "[%d, %d, %d, %d] %s p %.1f" % (n, c, h, w, name, p)
            pd = _scalar(p, dev)
            mean, gem = Out((n, c), dev), Out((n, c), dev)
            _ok(L.agp_pool_f32_fwd(_ptr(xd), sn, sc, sh, sw, n, c, h, w, _ptr(pd), P.GEM_EPS, mean.ptr(), gem.ptr(), None, _stream()),
                "agp_pool_f32_fwd")
            _planes_ok(mean.value("mean"), P.mean(x), bar, "pool_f32_fwd " + what + ": mean", floor)
            y64 = P.gem(x, p)
            _planes_ok(gem.value("gem"), y64, P.CEIL_FWD, "pool_f32_fwd " + what + ": GeM")
            only = Out((n, c), dev)
            _ok(L.agp_pool_f32_fwd(_ptr(xd), sn, sc, sh, sw, n, c, h, w, None, P.GEM_EPS, only.ptr(), None, None, _stream()), "mean only")
            assert torch.equal(only.value("mean"), mean.value("mean"))
            y = y64.float()
            yd = y.to(dev)
            rx, rdp = P.gem_bwd(x, p, P.GEM_EPS, y, gy)
            gp = ops.new_gp(dev)
            gx = _gem_bwd_call(dev, xd, pd, yd, gyd, gp, True)
            torch.cuda.synchronize()
            _planes_ok(gx.cpu(), rx, P.CEIL_GX, "gem_f32_bwd " + what + ": gx")
            assert not bool(gx[0, min(1, c - 1)].any()), what + ": the all-clamp plane's gx is not exact zeros"
            once = gp.cpu()
            _dp_ok(once[0], rdp, x, p, y, gy, "gem_f32_bwd " + what)
            assert not bool(once[1 + blocks:].any()), what + ": the ticket word or slots beyond the grid are not as ops.new_gp left them"
            assert _gem_bwd_call(dev, xd, pd, yd, gyd, gp, False) is None                 # gx == NULL, into the same gp
            twice = gp.cpu()
            assert float(twice[0]) == 2.0 * float(once[0]), what + ": two calls on one gp do not give twice the value"
            assert not bool(twice[1 + blocks:].any())
            assert torch.equal(twice[1:1 + blocks], once[1:1 + blocks]), what + ": the block partials differ between two calls"
        if whole is not None:                   # nothing around the view was written, by either kernel (gx has a buffer of its own)
            assert torch.equal(whole.view(torch.int32), before.view(torch.int32))


def test_gem_f32_bwd_sliced_gx_stays_inside_its_view(dev):
    n, c, h, w = 2, 5, 3, 4
    x = P.draw_map(n, c, h, w, 7, "f32")
    gy = P.draw_vec(n, c, 8, positive=True)
    xd, _ = _layouts(x.float(), dev)["sliced"]
    p = 2.5
    y = P.gem(x, p).float()
    big = torch.full((n, c + 2, h + 1, w + 3), float("nan"), dtype=torch.float32, device=dev)
    gx = big[:, 1:c + 1, :h, 2:w + 2]
    assert gx.stride() == xd.stride()
    sn, sc, sh, sw = xd.stride()
    pd, yd, gyd = _scalar(p, dev), y.to(dev), gy.to(dev)
    _ok(_L().agp_gem_f32_bwd(_ptr(xd), sn, sc, sh, sw, n, c, h, w, _ptr(pd), P.GEM_EPS, _ptr(yd), _ptr(gyd), _ptr(gx), None, _stream()),
        "agp_gem_f32_bwd")
    torch.cuda.synchronize()
    inside = torch.zeros_like(big, dtype=torch.bool)
    inside[:, 1:c + 1, :h, 2:w + 2] = True
    assert bool(torch.isnan(big[~inside]).all()) and not bool(torch.isnan(big[inside]).any())
    _planes_ok(gx.cpu(), P.gem_bwd(x, p, P.GEM_EPS, y, gy)[0], P.CEIL_GX, "gem_f32_bwd sliced gx (gp == NULL)")


def test_gem_f32_bwd_above_the_slots_takes_the_atomic_path(dev):
    """33 x 2048 planes = 16896 blocks > AGP_GP_SLOTS: dL/dp by atomics -- held to the bar, not to bit-repeatability; the slots
    and the ticket word stay untouched."""
    from agplace_amd import ops
    n, c, h, w = P.F32_ATOMIC
    assert (n * c + 3) // 4 > P.GP_SLOTS
    x = P.draw_map(n, c, h, w, 7, "f32")
    gy = P.draw_vec(n, c, 8, positive=True)
    p = 2.5
    y = P.gem(x, p).float()
    rx, rdp = P.gem_bwd(x, p, P.GEM_EPS, y, gy)
    gp = ops.new_gp(dev)
    gx = _gem_bwd_call(dev, x.float().to(dev), _scalar(p, dev), y.to(dev), gy.to(dev), gp, True)
    torch.cuda.synchronize()
    _planes_ok(gx.cpu(), rx, P.CEIL_GX, "gem_f32_bwd [33, 2048, 1, 2]: gx")
    got = gp.cpu()
    _dp_ok(got[0], rdp, x, p, y, gy, "gem_f32_bwd [33, 2048, 1, 2] (atomic)")
    assert not bool(got[1:].any())


# -------------------------------------------------------------------------------------------------------------- agp_pool_bwd
def _interior(m):
    return P.interior(m.hi.cpu(), m.lo.cpu(), 1)


@pytest.mark.parametrize("n,h,w", P.POOL_NHW)
@pytest.mark.parametrize("c", P.POOL_BWD_C)
def test_pool_bwd(dev, c, n, h, w):
    from agplace_amd import ops
    L = _L()
    p = 3.0 if (c // 8 + h) % 2 else 2.5
    x = P.draw_map(n, c, h, w, 2, "pair")
    base = P.draw_map(n, c, h, w, 3, "pair", 1.0, 0.0)
    gm, gg = P.draw_vec(n, c, 4), P.draw_vec(n, c, 5, positive=True)
    y = P.gem(x, p).float()
    xh, xl = _map_on(dev, x, 1, True)
    bh, bl = _map_on(dev, base, 1, True)
    gmd, ggd, yd, pd = gm.to(dev), gg.to(dev), y.to(dev), _scalar(p, dev)
    for with_base, with_mean, with_gem in P.POOL_BWD_TERMS:
        for with_gp in ((False, True) if with_gem else (False,)):
            what = "pool_bwd [%d, %d, %d, %d] p %.1f%s%s%s%s" % (n, h, w, c, p, " base" if with_base else "", " gmean" if with_mean else "",
                                                                " ggem" if with_gem else "", " gp" if with_gp else "")
            out, bufs = guarded_map(n, h, w, c, 3, dev)
            gp = ops.new_gp(dev) if with_gp else None
            _ok(L.agp_pool_bwd(_ptr(xh), _ptr(xl), _ptr(gmd) if with_mean else None, _ptr(ggd) if with_gem else None,
                               _ptr(yd) if with_gem else None, _ptr(pd) if with_gem else None, P.GEM_EPS, _ptr(bh) if with_base else None,
                               _ptr(bl) if with_base else None, n, h, w, c, 1, _ptr(out.hi), _ptr(out.lo), _ptr(gp), _stream()), "agp_pool_bwd")
            torch.cuda.synchronize()
            assert_only_the_interior_was_written(out, bufs)
            got = _interior(out)
            args = (x, base if with_base else None, gm if with_mean else None)
            ref, rdp = P.pool_bwd_map(*args, gg if with_gem else None, y, p)
            if with_base and not with_mean and not with_gem:
                assert torch.equal(got, base), what + ": base alone is not hi + lo copied"
            elif not with_gem:
                bar, floor = P.linear_map_bar(*args)
                _planes_ok(got, ref, bar, what, floor)
            else:
                _planes_ok(got, ref, P.CEIL_GX, what)
                if not with_base and not with_mean:
                    assert not bool(got[0, min(1, c - 1)].any()), what + ": the all-clamp plane's gradient is not exact zeros"
            if with_gp:
                _dp_ok(gp.cpu()[0], rdp, x, p, y, gg, what)


def test_pool_bwd_refusals(dev):
    L = _L()
    n, h, w, c = 2, 3, 3, 8
    x = P.draw_map(n, c, h, w, 2, "pair")
    xh, xl = _map_on(dev, x, 1, True)
    v = P.draw_vec(n, c, 4).to(dev)
    pd = _scalar(3.0, dev)
    gp = torch.full((16386,), POISON, dtype=torch.int32, device=dev)
    out, bufs = guarded_map(n, h, w, c, 3, dev)
    before = [b.clone() for b in bufs]
    call = lambda ggem, gem_y, p, gpp, cc=c: L.agp_pool_bwd(_ptr(xh), _ptr(xl), _ptr(v), _ptr(ggem), _ptr(gem_y), _ptr(p), P.GEM_EPS, None, None,
                                                          n, h, w, cc, 1, _ptr(out.hi), _ptr(out.lo), _ptr(gpp), _stream())
    assert call(v, None, pd, None) == BADARG, "ggem without gem_y"
    assert call(v, v, None, None) == BADARG, "ggem without p"
    assert call(None, None, None, gp) == BADARG, "gp without ggem"
    assert call(None, None, None, None, 12) == BADARG, "c % 8"
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(bufs, before)) and bool((gp == POISON).all())
