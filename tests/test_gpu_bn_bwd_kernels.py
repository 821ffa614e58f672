"""-m gpu: the BatchNorm-backward passes of csrc/train.hip one by one against the closed forms of tests/dense_train_ref.py (pinned
to fp64 autograd by tests/test_dense_train_ref.py): agp_bn_bwd / agp_bn_bwd_frozen / agp_bn_bwd_from_partial, the synchronised
pair agp_bn_bwd_sums + agp_bn_bwd_apply, agp_map_affine, and the stem's fused pool passes agp_affine_maxpool3x3s2_fwd,
agp_maxpool3x3s2_bwd, agp_maxpool_bn_bwd.  tests/test_gpu_train.py reaches them through whole units at the network's shapes,
where a thread's channel group always divides the grid stride; here the maps are chosen for the kernels' branches (MAPS: the
two-items-per-trip fast paths AND the generic / per-element-atomic paths of bn_bwd_apply_kernel and affine_kernel), every
channel meets the bar by itself, and gz_absmax is compared with the true maximum -- the one-pass weight gradient scales its fp16
operand by it.

Inputs are drawn in their storage formats; mean / rstd are the exact batch statistics of the stored z rounded to fp32 and handed
to both sides; the ReLU mask is a plane of its own.

Bars: gz per channel min(4 x floor, 1e-5), floor = the same closed form in float32 on the CPU rounded to the bf16 pair
(dense_train_ref.gz_bar); ggamma / gbeta 1e-5 of the sum of the absolute terms.
Measured on an MI355X: the float32 floor is 2.5e-6 .. 6.0e-6 per channel (the pair's storage rounding; the largest on the 18-element
channels of the 2048-channel map), so the bar is 1e-5 everywhere; the kernels' worst channel is 0.19 .. 1.10 of the floor of its
own case, 6.0e-6 at most, on every path.  ggamma is at most 1.4e-7 of the sum of its absolute terms on the gathering paths and
2.2e-6 on the pooled-domain path (zhat recovered from the stored pooled value), gbeta at most 5.8e-8.  gz_absmax: the stored maximum
is at most 1 + 7.6e-6 of the word (bound 1 + 2^-16), the word at most 1 + 2.8e-7 of the true maximum (bound 1 + 1e-5)."""
import os
import re

import pytest
import torch

import dense_train_ref as R
from conv_sched_util import GUARD, _bf16_pair, _f16, assert_only_the_interior_was_written, guarded_map

pytestmark = pytest.mark.gpu

# name -> ((n, h, w, c), fixed_g): whether (c / 8) divides the grid stride of the element-wise passes, i.e. whether
# bn_bwd_apply_kernel and affine_kernel can take their fast paths (tests/test_dense_train_ref.py asserts the column through the
# grid mirror).  3 x 9 x 11 on 64 channels is 2376 items on 768 threads: a trip of pairs and a trip of single items.
MAPS = {
    "c8": ((3, 9, 11, 8), True),
    "c24": ((3, 9, 11, 24), False),              # one block: 256 threads, 3 groups
    "c64": ((3, 9, 11, 64), True),
    "c96": ((3, 9, 11, 96), False),              # four blocks: 1024 threads, 12 groups
    "small_c24": ((2, 5, 7, 24), False),
    "small_c64": ((2, 5, 7, 64), True),
    "small_c96": ((2, 5, 7, 96), False),
    "c24_fixed": ((3, 16, 16, 24), True),        # three blocks: 768 threads, 3 groups
    "c96_fixed": ((2, 9, 11, 96), True),         # three blocks: 768 threads, 12 groups
    "c2048": ((2, 3, 3, 2048), True),
}
SENTINEL = 0x5A5A5A5A


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


def _ok(rc, what):
    assert rc == 0, "%s returned %d" % (what, rc)


# --------------------------------------------------------------------------------------------------------------------- maps
def _in(v, paired):
    """[n, c, h, w] stored values -> (hi, lo) planes of the 1-pixel-halo NHWC map (lo None for one fp16 plane)"""
    return R.planes(R.nhwc_map(v, 1), paired)


def _out(n, h, w, c, paired, dev):
    """An output map between guard regions, interior pre-filled -> (map, buffers)"""
    return guarded_map(n, h, w, c, 3 if paired else 4, dev)


def _value(m):
    """the interior of a map as [n, c, h, w] fp64"""
    v = m.hi.double() if m.lo is None else m.hi.double() + m.lo.double()
    return v[:, 1:-1, 1:-1].permute(0, 3, 1, 2)


def _ws(n, h, w, c, dev):
    return torch.full((int(_L().agp_train_reduce_workspace_floats(n, h, w, c)),), float("nan"), dtype=torch.float32, device=dev)


def _absmax_words(c, dev):
    am = torch.zeros(c + 64, dtype=torch.int32, device=dev)
    am[c:] = SENTINEL
    return am


def _check_absmax(am, c, gz_map, gz64, what):
    """The word is tied to the stored value the weight gradient will read: max |hi + lo| <= absmax (1 + 2^-16), and to the truth:
    absmax <= max |gz64| (1 + 1e-5)."""
    assert bool((am[c:] == SENTINEL).all()), "words behind gz_absmax[c] were written"
    a = am[:c].view(torch.float32).double()
    stored = _value(gz_map).abs().amax((0, 2, 3))
    true = gz64.abs().amax((0, 2, 3))
    low, high = float((stored / a.clamp_min(1e-300)).max()), float((a / true.clamp_min(1e-300)).max())
    print("%s: stored max / absmax <= %.8f, absmax / true max <= %.8f" % (what, low, high))
    assert bool((stored <= a * (1 + 2.0 ** -16)).all()), "%s: a stored |gz| exceeds the recorded maximum (%.8f)" % (what, low)
    assert bool((a <= true * (1 + 1e-5)).all()), "%s: the recorded maximum exceeds the true one (%.8f)" % (what, high)


def _check_sums(gg, gb, z, g, mean, rstd, what):
    """ggamma / gbeta against fp64, SUM_BAR of the sum of the absolute terms per channel"""
    zhat = (z.double() - mean.double().view(1, -1, 1, 1)) * rstd.double().view(1, -1, 1, 1)
    tg, tb = (g * zhat).sum((0, 2, 3)), g.sum((0, 2, 3))
    mg, mb = (g * zhat).abs().sum((0, 2, 3)), g.abs().sum((0, 2, 3))
    eg, eb = (gg.double() - tg).abs(), (gb.double() - tb).abs()
    print("%s: ggamma error / sum |terms| %.3e, gbeta %.3e (bar %.1e)" % (
        what, float((eg / mg.clamp_min(1e-300)).max()), float((eb / mb.clamp_min(1e-300)).max()), R.SUM_BAR))
    assert bool((eg <= R.SUM_BAR * mg).all()), "%s: ggamma" % what
    assert bool((eb <= R.SUM_BAR * mb).all()), "%s: gbeta" % what


def _check_gz(gz_map, ref, bar, floor, what):
    worst, ch, _ = R.per_channel_rel(_value(gz_map), ref)
    print("%s: worst channel %.3e (channel %d), float32 floor %.3e, bar %.3e" % (what, worst, ch, floor, bar))
    assert worst < bar, "%s: channel %d has %.3e (bar %.3e, floor %.3e)" % (what, ch, worst, bar, floor)


# ------------------------------------------------------------------------------------------------------------ agp_bn_bwd
# (z one fp16 plane, gy one fp16 plane, ReLU, residual gradient out, gz_absmax, frozen)
VARIANTS = {
    "pair_relu_res_absmax": (False, False, True, True, True, False),
    "pair_plain": (False, False, False, False, False, False),
    "pair_relu_absmax": (False, False, True, False, True, False),
    "zf16_relu_res_absmax": (True, False, True, True, True, False),
    "gyf16_relu_res_absmax": (False, True, True, True, True, False),        # gy_lo = NULL: the generic path whatever the grid
    "frozen_relu_res_absmax": (False, False, True, True, True, True),
    "frozen_zf16_plain": (True, False, False, False, False, True),
}


class BnProblem:
    def __init__(self, dev, shape, seed, z_f16=False, gy_f16=False, relu=True):
        self.n, self.h, self.w, self.c = n, h, w, c = shape
        self.dev, self.relu = dev, relu
        self.z, self.gy, self.y, self.gamma, self.beta = R.draw_bn(n, c, h, w, seed, z_f16, gy_f16, relu, dev)
        self.mean, self.rstd = R.batch_stats(self.z)
        self.z_hi, self.z_lo = _in(self.z, not z_f16)
        self.gy_hi, self.gy_lo = _in(self.gy, not gy_f16)
        self.y_hi, self.y_lo = _in(self.y, True) if relu else (None, None)
        self.mask = (self.y > 0) if relu else None
        self.count = n * h * w

    def call(self, fn, gz, gres=None, absmax=None, gy=None):
        """agp_bn_bwd / agp_bn_bwd_frozen -> (ggamma, gbeta)"""
        gy_hi, gy_lo = (self.gy_hi, self.gy_lo) if gy is None else gy
        gg = torch.full((self.c,), float("nan"), dtype=torch.float32, device=self.dev)
        gb = torch.full_like(gg, float("nan"))
        _ok(fn(_ptr(self.z_hi), _ptr(self.z_lo), _ptr(gy_hi), _ptr(gy_lo), _ptr(self.y_hi), _ptr(self.y_lo), _ptr(self.mean),
               _ptr(self.rstd), _ptr(self.gamma), self.n, self.h, self.w, self.c, 1, 1 if self.relu else 0, _ptr(gz.hi), _ptr(gz.lo),
               _ptr(gres.hi) if gres is not None else None, _ptr(gres.lo) if gres is not None else None, _ptr(gg), _ptr(gb),
               _ptr(_ws(self.n, self.h, self.w, self.c, self.dev)), _ptr(absmax), _stream()), "agp_bn_bwd")
        return gg, gb

    def ref(self, frozen=False, gy=None):
        return R.bn_bwd64(self.z, self.gy if gy is None else gy, self.mask, self.mean, self.rstd, self.gamma, self.count, frozen)

    def bar(self, frozen=False, gy=None):
        return R.gz_bar(self.z, self.gy if gy is None else gy, self.mask, self.mean, self.rstd, self.gamma, self.count, frozen)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(MAPS))
def test_bn_bwd_matches_the_closed_form_per_channel(dev, name, variant):
    """agp_bn_bwd / agp_bn_bwd_frozen on every map of MAPS -- the fast path (fixed_g, bf16-pair gy and gz) and the generic one
    (c / 8 does not divide the grid stride: per-channel coefficient loads and the per-element atomicMax of gz_absmax; or gy as
    ONE fp16 plane) -- with z as a pair or one fp16 plane, with and without ReLU, the residual gradient and gz_absmax.  gz per
    channel against fp64; gres = gy [y > 0] exactly; ggamma / gbeta; gz_absmax against the stored and the true maximum; only the
    interiors of gz / gres written (the halo of gz stays zero: the weight gradient's K raster runs over it)."""
    shape, fixed = MAPS[name]
    z_f16, gy_f16, relu, with_res, with_am, frozen = VARIANTS[variant]
    n, h, w, c = shape
    assert R.fixed_g(n, h, w, c) == fixed
    pr = BnProblem(dev, shape, 1 + len(variant), z_f16, gy_f16, relu)
    gz, gz_bufs = _out(n, h, w, c, True, dev)
    gres, gres_bufs = _out(n, h, w, c, True, dev) if with_res else (None, None)
    am = _absmax_words(c, dev) if with_am else None
    gg, gb = pr.call(_L().agp_bn_bwd_frozen if frozen else _L().agp_bn_bwd, gz, gres, am)
    torch.cuda.synchronize()
    what = "%s %s (%s path)" % (name, variant, "fast" if fixed and not gy_f16 else "generic")
    assert_only_the_interior_was_written(gz, gz_bufs)
    ref_gz, ref_g, _, _, _ = pr.ref(frozen)
    bar, floor = pr.bar(frozen)
    _check_gz(gz, ref_gz, bar, floor, what)
    _check_sums(gg, gb, pr.z, ref_g, pr.mean, pr.rstd, what)
    if with_res:
        assert_only_the_interior_was_written(gres, gres_bufs)
        assert torch.equal(_value(gres), ref_g), "%s: gres is not gy [y > 0] bit for bit" % what
    if with_am:
        _check_absmax(am, c, gz, ref_gz, what)


@pytest.mark.parametrize("name", ["c64", "c24", "c96", "c96_fixed", "c2048"])
def test_gz_absmax_keeps_the_maximum_over_launches(dev, name):
    """gz_absmax is an atomic maximum that only the weight gradient re-zeroes: a launch with half the gradient after a launch
    with the whole one leaves the word where it was, the other order raises it to the same bits -- on the fast path's LDS-folded
    flush and on the generic path's per-element atomics."""
    shape, fixed = MAPS[name]
    n, h, w, c = shape
    pr = BnProblem(dev, shape, 3)
    half = _in(pr.gy * 0.5, True)
    words = []
    for order in ((None, half), (half, None, half)):
        am = _absmax_words(c, dev)
        seen = []
        for gy in order:
            gz, bufs = _out(n, h, w, c, True, dev)
            pr.call(_L().agp_bn_bwd, gz, None, am, gy)
            torch.cuda.synchronize()
            seen.append(am[:c].clone())
        words.append(seen)
    (full, after_half), (first_half, raised, still) = words
    assert torch.equal(full, after_half) and torch.equal(raised, full) and torch.equal(still, full)
    assert bool((first_half < full).all()) and bool((first_half > 0).all())
    gz, bufs = _out(n, h, w, c, True, dev)
    am = _absmax_words(c, dev)
    pr.call(_L().agp_bn_bwd, gz, None, am)
    torch.cuda.synchronize()
    assert torch.equal(am[:c], full)
    _check_absmax(am, c, gz, pr.ref()[0], "%s (%s)" % (name, "fixed_g" if fixed else "not fixed_g"))


@pytest.mark.parametrize("name", ["c64", "c96", "small_c24", "c96_fixed"])
def test_synchronised_sums_and_apply(dev, name):
    """agp_bn_bwd_sums + agp_bn_bwd_apply: the local map is the first half of a batch of two maps; the fp64 sums of both halves are
    added on the host and the global count handed over on the device.  gz of the local half against bn_bwd64 over the WHOLE batch,
    sums[0 : 2c] against the fp64 local sums."""
    (n, h, w, c), _ = MAPS[name]
    L = _L()
    z, gy, y, gamma, _ = R.draw_bn(2 * n, c, h, w, 5, dev=dev)
    mean, rstd = R.batch_stats(z)
    count = 2 * n * h * w
    whole = R.bn_bwd64(z, gy, y > 0, mean, rstd, gamma, count)
    sums, halves = [], []
    for sl in (slice(0, n), slice(n, 2 * n)):
        pl = [_in(t[sl], True) for t in (z, gy, y)]
        s = torch.full((2 * c + 1,), float("nan"), dtype=torch.float64, device=dev)
        gg = torch.full((c,), float("nan"), dtype=torch.float32, device=dev)
        gb = torch.full_like(gg, float("nan"))
        ws = _ws(n, h, w, c, dev)
        _ok(L.agp_bn_bwd_sums(_ptr(pl[0][0]), _ptr(pl[0][1]), _ptr(pl[1][0]), _ptr(pl[1][1]), _ptr(pl[2][0]), _ptr(pl[2][1]), _ptr(mean),
                              _ptr(rstd), n, h, w, c, 1, 1, _ptr(s), _ptr(gg), _ptr(gb), _ptr(ws), _stream()), "agp_bn_bwd_sums")
        local = R.bn_bwd64(z[sl], gy[sl], y[sl] > 0, mean, rstd, gamma, count)
        _check_sums(s[c:2 * c], s[:c], z[sl], local[1], mean, rstd, "%s sums of images %d.." % (name, sl.start))
        _check_sums(gg, gb, z[sl], local[1], mean, rstd, "%s fp32 sums of images %d.." % (name, sl.start))
        sums.append(s)
        halves.append((pl, ws))
    total = (sums[0] + sums[1])[:2 * c].contiguous()
    cnt = torch.tensor([float(count)], dtype=torch.float64, device=dev)
    (pz, pg, py), ws = halves[0]
    gz, gz_bufs = _out(n, h, w, c, True, dev)
    gres, gres_bufs = _out(n, h, w, c, True, dev)
    _ok(L.agp_bn_bwd_apply(_ptr(pz[0]), _ptr(pz[1]), _ptr(pg[0]), _ptr(pg[1]), _ptr(py[0]), _ptr(py[1]), _ptr(mean), _ptr(rstd),
                           _ptr(gamma), _ptr(total), _ptr(cnt), n, h, w, c, 1, 1, _ptr(gz.hi), _ptr(gz.lo), _ptr(gres.hi), _ptr(gres.lo),
                           _ptr(ws), _stream()), "agp_bn_bwd_apply")
    torch.cuda.synchronize()
    assert_only_the_interior_was_written(gz, gz_bufs)
    assert_only_the_interior_was_written(gres, gres_bufs)
    bar, floor = R.gz_bar(z, gy, y > 0, mean, rstd, gamma, count)
    _check_gz(gz, whole[0][:n], bar, floor, "%s synchronised" % name)
    assert torch.equal(_value(gres), whole[1][:n])


@pytest.mark.parametrize("frozen", [False, True], ids=["train", "frozen"])
@pytest.mark.parametrize("name", ["c64", "c24", "c96_fixed"])
def test_bn_bwd_from_partial(dev, name, frozen):
    """agp_bn_bwd_from_partial with the test's own per-image fp32 sums as `partial` (tiles = n): gz equals agp_bn_bwd's on the same
    inputs to the bar, and the closed form's."""
    shape, _ = MAPS[name]
    n, h, w, c = shape
    L = _L()
    pr = BnProblem(dev, shape, 7)
    ref_gz, ref_g, _, _, _ = pr.ref(frozen)
    zhat = (pr.z - pr.mean.double().view(1, -1, 1, 1)) * pr.rstd.double().view(1, -1, 1, 1)
    partial = torch.stack([ref_g.sum((2, 3)), (ref_g * zhat).sum((2, 3))], 1).float().contiguous()       # [n][2][c]
    gz, gz_bufs = _out(n, h, w, c, True, dev)
    am = _absmax_words(c, dev)
    gg = torch.full((c,), float("nan"), dtype=torch.float32, device=dev)
    gb = torch.full_like(gg, float("nan"))
    _ok(L.agp_bn_bwd_from_partial(_ptr(partial), n, _ptr(pr.z_hi), _ptr(pr.z_lo), _ptr(pr.gy_hi), _ptr(pr.gy_lo), _ptr(pr.y_hi),
                                  _ptr(pr.y_lo), _ptr(pr.mean), _ptr(pr.rstd), _ptr(pr.gamma), n, h, w, c, 1, 1, 1 if frozen else 0,
                                  _ptr(gz.hi), _ptr(gz.lo), None, None, _ptr(gg), _ptr(gb), _ptr(am), _stream()),
        "agp_bn_bwd_from_partial")
    gz2, gz2_bufs = _out(n, h, w, c, True, dev)
    pr.call(L.agp_bn_bwd_frozen if frozen else L.agp_bn_bwd, gz2)
    torch.cuda.synchronize()
    assert_only_the_interior_was_written(gz, gz_bufs)
    bar, floor = pr.bar(frozen)
    _check_gz(gz, ref_gz, bar, floor, "%s from_partial" % name)
    _check_gz(gz, _value(gz2), bar, floor, "%s from_partial against agp_bn_bwd" % name)
    _check_sums(gg, gb, pr.z, ref_g, pr.mean, pr.rstd, "%s from_partial" % name)
    _check_absmax(am, c, gz, ref_gz, "%s from_partial" % name)


# --------------------------------------------------------------------------------------------------------- agp_map_affine
# (a one fp16 plane, residual: None / "pair" / "f16", ReLU, outputs: "pair" / "pair+h16" / "f16", scale and shift given)
AFFINE = {
    "pair_res_relu_pair_h16": (False, "pair", True, "pair+h16", True),
    "pair_plain_pair": (False, None, False, "pair", True),
    "pair_copy_pair_h16": (False, None, False, "pair+h16", False),          # no scale / shift: the pass that makes an fp16 plane
    "f16_relu_pair_h16": (True, None, True, "pair+h16", True),
    "f16_res_f16out": (True, "pair", False, "f16", True),
    "pair_relu_f16out": (False, None, True, "f16", True),
    "pair_resf16_relu_pair": (False, "f16", True, "pair", True),            # r_lo = NULL: the generic path whatever the grid
}


@pytest.mark.parametrize("variant", list(AFFINE))
@pytest.mark.parametrize("name", ["c64", "c24", "c96", "c96_fixed", "small_c64", "c2048"])
def test_map_affine(dev, name, variant):
    """agp_map_affine: relu?(a scale + shift + r) on both paths of affine_kernel.  The stored value is within one rounding of the
    fp64 result (+ the fp32 arithmetic: 2^-22 of the terms' magnitude); o_h16 is half() of the fp32 value, bit for bit, from a
    float32 reference (the fma, the residual added in fp32)."""
    (n, h, w, c), fixed = MAPS[name]
    a_f16, res, relu, outs, coeffs = AFFINE[variant]
    gen = torch.Generator(device=dev).manual_seed(len(variant) + c)
    a = (_f16 if a_f16 else _bf16_pair)(torch.randn((n, c, h, w), generator=gen, device=dev) * 2)
    r = None if res is None else (_f16 if res == "f16" else _bf16_pair)(torch.randn((n, c, h, w), generator=gen, device=dev))
    scale = (0.5 + torch.rand(c, generator=gen, device=dev)).float() if coeffs else None
    shift = (0.3 * torch.randn(c, generator=gen, device=dev)).float() if coeffs else None
    a_hi, a_lo = _in(a, not a_f16)
    r_hi, r_lo = _in(r, res == "pair") if r is not None else (None, None)
    out, out_bufs = _out(n, h, w, c, outs != "f16", dev)
    h16, h16_bufs = _out(n, h, w, c, False, dev) if outs == "pair+h16" else (None, None)
    _ok(_L().agp_map_affine(_ptr(a_hi), _ptr(a_lo), _ptr(scale), _ptr(shift), _ptr(r_hi), _ptr(r_lo), n, h, w, c, 1, 1 if relu else 0,
                            _ptr(out.hi), _ptr(out.lo), _ptr(h16.hi) if h16 is not None else None, _stream()), "agp_map_affine")
    torch.cuda.synchronize()
    assert_only_the_interior_was_written(out, out_bufs)
    sc = scale.double().view(1, -1, 1, 1) if coeffs else 1.0
    sh = shift.double().view(1, -1, 1, 1) if coeffs else 0.0
    v64 = a * sc + sh + (r if r is not None else 0.0)
    terms = (a * sc).abs() + abs(sh) + (r.abs() if r is not None else 0.0)
    v32 = (a * sc + sh).float()
    if r is not None:
        v32 = v32 + r.float()
    if relu:
        v64, v32 = v64.clamp_min(0), v32.clamp_min(0)
    ulp = 2.0 ** -10 if outs == "f16" else 2.0 ** -16
    err = (_value(out) - v64).abs()
    tol = ulp * v64.abs() + 2.0 ** -22 * terms + (2.0 ** -24 if outs == "f16" else 0.0)
    print("%s %s (%s): worst error / tolerance %.3f" % (name, variant, "fixed_g" if fixed else "not fixed_g", float((err / tol).max())))
    assert bool((err <= tol).all()), "%s %s: a stored value is more than one rounding from the fp64 result" % (name, variant)
    if h16 is not None:
        assert_only_the_interior_was_written(h16, h16_bufs)
        want = v32.half().permute(0, 2, 3, 1)
        got = h16.hi[:, 1:-1, 1:-1]
        diff = int((got.view(torch.int16) != want.contiguous().view(torch.int16)).sum())
        assert diff == 0, "%s %s: %d elements of o_h16 differ from half() of the fp32 value" % (name, variant, diff)


# ------------------------------------------------------------------------------------------------------- the stem's pool
def _argmax_buf(n, ho, wo, c, dev):
    buf = torch.full((GUARD + n * ho * wo * c + GUARD,), 0xEE, dtype=torch.uint8, device=dev)
    return buf[GUARD:GUARD + n * ho * wo * c].view(n, ho, wo, c), buf


POOL_MAPS = [(2, 9, 11, 64), (2, 8, 10, 64), (1, 9, 10, 8), (3, 5, 6, 24), (1, 6, 7, 96)]


@pytest.mark.parametrize("z_f16", [False, True], ids=["z_pair", "z_f16"])
@pytest.mark.parametrize("n,h,w,c", POOL_MAPS, ids=["%dx%dx%dx%d" % s for s in POOL_MAPS])
def test_affine_maxpool_fwd(dev, n, h, w, c, z_f16):
    """agp_affine_maxpool3x3s2_fwd, odd and even h and w: the pooled map within storage rounding of affine_maxpool64 (it IS the
    fp32 activation, so the bf16 pair of it), the argmax bytes equal, o_h16 = half() of the fp32 maximum; channel 1's activations
    are all zero: every window of it records position 4 and pools 0."""
    beta0 = (0.3 * torch.randn(c, generator=torch.Generator().manual_seed(c + w))).float().to(dev)
    beta0[1] = -60.0
    z, mean, rstd, gamma, beta, scale, shift = R.draw_pool(n, c, h, w, 3, z_f16, None, beta0, dev=dev)
    assert not bool(R.pool_decision_ties(z, scale, shift).any())
    pooled, pos, act = R.affine_maxpool64(z, scale, shift)
    assert not bool(act[:, 1].any()) and bool((pos[:, 1] == 4).all()) and bool((pos != 4).any())
    ho, wo = pooled.shape[2], pooled.shape[3]
    z_hi, z_lo = _in(z, not z_f16)
    out, out_bufs = _out(n, ho, wo, c, True, dev)
    h16, h16_bufs = _out(n, ho, wo, c, False, dev)
    idx, idx_buf = _argmax_buf(n, ho, wo, c, dev)
    L = _L()
    args = lambda hh, ww: (_ptr(z_hi), _ptr(z_lo), _ptr(scale), _ptr(shift), n, h, w, c, 1, _ptr(out.hi), _ptr(out.lo), hh, ww, 1,
                           _ptr(idx), _ptr(h16.hi), _stream())
    assert L.agp_affine_maxpool3x3s2_fwd(*args(ho + 1, wo)) == BADARG and L.agp_affine_maxpool3x3s2_fwd(*args(ho, wo - 1)) == BADARG
    _ok(L.agp_affine_maxpool3x3s2_fwd(*args(ho, wo)), "agp_affine_maxpool3x3s2_fwd")
    torch.cuda.synchronize()
    assert_only_the_interior_was_written(out, out_bufs)
    assert_only_the_interior_was_written(h16, h16_bufs)
    assert bool((idx_buf[:GUARD] == 0xEE).all()) and bool((idx_buf[-GUARD:] == 0xEE).all())
    wrong = int((idx.permute(0, 3, 1, 2) != pos).sum())
    assert wrong == 0, "%d argmax bytes differ" % wrong
    assert bool(((_value(out) - pooled).abs() <= 2.0 ** -17 * pooled.abs()).all())
    assert torch.equal(_value(out), _bf16_pair(pooled))
    want = pooled.float().half().permute(0, 2, 3, 1).contiguous()
    assert torch.equal(h16.hi[:, 1:-1, 1:-1].contiguous().view(torch.int16), want.view(torch.int16))
    assert not bool(_value(out)[:, 1].any())


@pytest.mark.parametrize("gy_f16", [False, True], ids=["gy_pair", "gy_f16"])
@pytest.mark.parametrize("n,h,w,c", POOL_MAPS, ids=["%dx%dx%dx%d" % s for s in POOL_MAPS])
def test_maxpool_bwd(dev, n, h, w, c, gy_f16):
    """agp_maxpool3x3s2_bwd: every input pixel receives the pooled gradient of the (at most four) windows that recorded it -- an
    element with one contribution (or none) holds it exactly, one with several the fp32 sum of stored values: within one ulp of
    the pair (2^-16) of the sum of their magnitudes."""
    z, mean, rstd, gamma, beta, scale, shift = R.draw_pool(n, c, h, w, 4, dev=dev)
    pooled, pos, _ = R.affine_maxpool64(z, scale, shift)
    ho, wo = pooled.shape[2], pooled.shape[3]
    gen = torch.Generator(device=dev).manual_seed(h * w + c)
    gp = (_f16 if gy_f16 else _bf16_pair)(torch.randn(pooled.shape, generator=gen, device=dev))
    gp_hi, gp_lo = _in(gp, not gy_f16)
    idx = pos.permute(0, 2, 3, 1).contiguous()
    gx, gx_bufs = _out(n, h, w, c, True, dev)
    _ok(_L().agp_maxpool3x3s2_bwd(_ptr(idx), _ptr(gp_hi), _ptr(gp_lo), n, h, w, c, 1, ho, wo, 1, _ptr(gx.hi), _ptr(gx.lo), _stream()),
        "agp_maxpool3x3s2_bwd")
    torch.cuda.synchronize()
    assert_only_the_interior_was_written(gx, gx_bufs)
    ref = R.maxpool_route64(gp, pos, h, w)
    count = R.maxpool_route64(torch.ones_like(gp), pos, h, w)
    mag = R.maxpool_route64(gp.abs(), pos, h, w)
    got = _value(gx)
    assert int(count.max()) >= 2 and bool((count == 0).any())
    assert torch.equal(got[count <= 1], ref[count <= 1]), "an element with one contribution does not hold it exactly"
    assert bool(((got - ref).abs() <= 2.0 ** -16 * mag).all())


# (the sums path: "y" a stored output plane, "recompute" the mask from scale / shift, "pooled" the pooled-domain sums)
@pytest.mark.parametrize("frozen", [False, True], ids=["train", "frozen"])
@pytest.mark.parametrize("z_f16", [False, True], ids=["z_pair", "z_f16"])
@pytest.mark.parametrize("path", ["y", "recompute", "pooled"])
@pytest.mark.parametrize("n,h,w,c", [(2, 9, 11, 64), (2, 8, 10, 64), (3, 12, 15, 8)], ids=["2x9x11x64", "2x8x10x64", "3x12x15x8"])
def test_maxpool_bn_bwd(dev, n, h, w, c, path, z_f16, frozen):
    """agp_maxpool_bn_bwd on its three sums paths, frozen and not: gz, ggamma, gbeta and gz_absmax against maxpool_bn_bwd64.  On
    the pooled-domain path channel 3 has gamma = 5e-5 (|gamma| < 1e-4) and channel 5 beta = 20 gamma (|beta / gamma| > 16): the
    "slow channel" branch of pool_bn_bwd_sums_pooled_kernel, which reads z at the recorded argmax."""
    gamma0 = (0.5 + torch.rand(c, generator=torch.Generator().manual_seed(c + h))).float().to(dev)
    beta0 = (0.3 * torch.randn(c, generator=torch.Generator().manual_seed(c + w))).float().to(dev)
    gamma0[3], beta0[3] = 5e-5, 0.3
    beta0[5] = 20.0 * gamma0[5]
    gamma0[6] = -gamma0[6]
    z, mean, rstd, gamma, beta, scale, shift = R.draw_pool(n, c, h, w, 6, z_f16, gamma0, beta0, dev=dev)
    assert not bool(R.pool_decision_ties(z, scale, shift).any())
    assert abs(float(gamma[3])) < 1e-4 and abs(float(beta[5] / gamma[5])) > 16
    pooled, pos, act = R.affine_maxpool64(z, scale, shift)
    ho, wo = pooled.shape[2], pooled.shape[3]
    gen = torch.Generator(device=dev).manual_seed(h * w + c)
    gp = _bf16_pair(torch.randn(pooled.shape, generator=gen, device=dev))
    gp_hi, gp_lo = _in(gp, True)
    z_hi, z_lo = _in(z, not z_f16)
    y_hi, y_lo = _in(_bf16_pair(act), True) if path == "y" else (None, None)
    pv_hi, pv_lo = _in(_bf16_pair(pooled), True) if path == "pooled" else (None, None)
    idx = pos.permute(0, 2, 3, 1).contiguous()
    L = _L()

    def call(gz, am, gg, gb, cc=c, hh=ho):
        return L.agp_maxpool_bn_bwd(_ptr(idx), _ptr(gp_hi), _ptr(gp_lo), hh, wo, 1, _ptr(z_hi), _ptr(z_lo), _ptr(y_hi), _ptr(y_lo),
                                    _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(scale) if path != "y" else None,
                                    _ptr(shift) if path != "y" else None, _ptr(pv_hi), _ptr(pv_lo), _ptr(beta), n, h, w, cc, 1, 1,
                                    1 if frozen else 0, _ptr(gz.hi), _ptr(gz.lo), _ptr(gg), _ptr(gb), _ptr(_ws(n, h, w, c, dev)),
                                    _ptr(am), _stream())
    gz, gz_bufs = _out(n, h, w, c, True, dev)
    am = _absmax_words(c, dev)
    gg = torch.full((c,), float("nan"), dtype=torch.float32, device=dev)
    gb = torch.full_like(gg, float("nan"))
    assert call(gz, am, gg, gb, hh=ho + 1) == BADARG                              # a wrong pooled height
    assert call(gz, am, gg, gb, cc=24) == UNSUPPORTED                              # 256 % (24 / 8) != 0
    _ok(call(gz, am, gg, gb), "agp_maxpool_bn_bwd")
    torch.cuda.synchronize()
    what = "%dx%dx%dx%d %s %s %s" % (n, h, w, c, path, "z_f16" if z_f16 else "z_pair", "frozen" if frozen else "train")
    assert_only_the_interior_was_written(gz, gz_bufs)
    ref_gz, ref_g, _, _, _ = R.maxpool_bn_bwd64(gp, pos, act, z, mean, rstd, gamma, frozen)
    routed = R.maxpool_route64(gp, pos, h, w)
    bar, floor = R.gz_bar(z, routed, act > 0, mean, rstd, gamma, n * h * w, frozen)
    _check_gz(gz, ref_gz, bar, floor, what)
    _check_sums(gg, gb, z, ref_g, mean, rstd, what)
    _check_absmax(am, c, gz, ref_gz, what)
