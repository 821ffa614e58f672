"""-m gpu: the map pack, split, halo and layout kernels one by one against the bit-exact CPU references of tests/map_ref.py
(pinned by tests/test_map_ref.py to an integer round-to-nearest-even, to torch.flip / permute, to max_pool2d and to
dense_train_ref.affine_maxpool64; that file also shows that every comparison made here rejects a wrong variant, and evaluates the
float32 floor of the channel sum).  The entry points are called directly through ctypes.

Rules of the file
  * every output lies between poisoned guards (GUARD elements; 0x7FC0BEEF, 0x7FC0 in 16-bit planes -- a NaN in bf16 and in fp16,
    nothing these kernels store from finite inputs -- and 0xEF in the argmax bytes);
  * a map output is poisoned throughout (interior and halo; the halo zeroed where a kernel is specified against a zero halo) and
    the WHOLE plane is compared with the expected one: the documented region holds the reference's bits, everything else what was
    there -- "written" and "not written" in one comparison;
  * map inputs carry garbage (-3) in the halo (the pooling input: zeros in the ring its windows read, 7 outside it);
  * refusals return AGP_E_BADARG / AGP_E_UNSUPPORTED as include/agplace_hip.h defines them, and write nothing;
  * everything is compared as bit patterns, -0 distinct from +0; the one exception is agp_map_chan_sum (1e-5 of sum |terms|);
  * inputs: magnitudes 2^-60 .. 6e4 log-uniform with exact zeros, -0, rounding ties of hi and of lo, the largest finite bf16 and,
    for fp16 planes, values beyond +-65504 and below 2^-14 planted in every case (map_ref.specials); no NaN, no infinity.

Departures from the issue that asked for this file
  * agp_pack_u8_cams_to_nhwc: none of the three shapes has 256 pixels, so none can hold every byte value in every channel;
    they hold a ramp, and a fourth shape (1, 2, 8, 16) holds every byte value in every channel.
  * the additions to the cpad == 4 coverage (pad 0 and 1, the h16 plane, its AGP_E_UNSUPPORTED answers) are a test of this file,
    test_pack_cpad4_pads_and_the_h16_plane; test_pack_stem_input_fast_and_generic_paths of test_gpu_kernels.py stays as it was.
  * the pooling input holds no -0: it is a post-ReLU map.
  * sums of two planted values are kept finite: the operands of the add kernels are clamped to +-1e38 (no infinity, see above).

MEASURED on an MI355X (all 76 cases of this file, 3.4 s):
  agp_split_f32                  bit-equal over all cases, both formats, with and without lo: the fp16 vector path (pack8_h) and the
                                 scalar tail (split_f16) agree with the reference on both sides of +-65504 and in the subnormal range.
  agp_split_conv_weight[_both]   bit-equal over all cases; chunk_major 0 of the _both entry bit-equal to the two single calls; dgrad
                                 2, 3 and -1 refused, nothing written.
  agp_pack_f32_to_nhwc[4_h16]    bit-equal over all cases (four source layouts, the stride loop, cpad 4 at pad 0 and 1, the h16 plane).
  agp_pack_u8_cams_to_nhwc       bit-equal over all cases: the device's fp32 division is the correctly rounded one, no ulp allowance
                                 is made.
  agp_unpack_nhwc_to_f32, agp_map_zero_halo, agp_maxpool3x3s2_fwd (values and argmax), agp_bcast_add_fwd, agp_map_add (the
  subnormal mask values count as positive), agp_upsample2_zero: bit-equal over all cases, nothing outside the documented region
  written, nothing inside it left unwritten.
  agp_map_chan_sum               worst 2.8e-7 of sum |terms| ([3, 9, 11, 8], pair; bar 1e-5; the float32 floor of the cases on the
                                 CPU is 1.6e-7); one fp16 plane 6.5e-8 at the worst (the fp32 chains of such values are exact, what
                                 is left is the final rounding); two calls bit-equal in every case.
  agp_bn_frozen_coeffs           bit-equal to float(the fp64 formula): 0 of 1 / 255 / 256 / 257 channels differ in mean, rstd, scale
                                 and shift, with gamma / beta and without; no ulp allowance is made.
"""
import os
import re

import pytest
import torch

import map_ref as M
import pool_ref as P

pytestmark = pytest.mark.gpu

GUARD = 4096
POISON = 0x7FC0BEEF              # a quiet NaN with a payload
POISON16 = 0x7FC0                # its 16-bit counterpart: a quiet NaN as bf16 and as fp16
POISON8 = 0xEF
_POISON_OF = {torch.uint8: POISON8, torch.int16: POISON16, torch.int32: POISON}


def _header_code(name):
    """An AGP_* return code as include/agplace_hip.h defines it."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    m = re.search(r"#define %s (\d+)" % name, open(os.path.join(root, "include", "agplace_hip.h")).read())
    assert m, "%s not found in the header" % name
    return int(m.group(1))


OK = _header_code("AGP_OK")
BADARG = _header_code("AGP_E_BADARG")
UNSUPPORTED = _header_code("AGP_E_UNSUPPORTED")


def _L():
    from agplace_amd import _lib
    return _lib.load()


def _ptr(t):
    if t is None:
        return None
    return t.ptr() if isinstance(t, Buf) else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ok(rc, what):
    assert rc == OK, "%s returned %d" % (what, rc)


class Buf:
    """An integer tensor of `shape` (1, 2 or 4 bytes per element) in the middle of a poisoned buffer, itself poisoned or
    holding `init`; `before` is what it held before the call."""

    def __init__(self, shape, dev, dtype=torch.int16, init=None):
        self.poison = _POISON_OF[dtype]
        numel = 1
        for s in shape:
            numel *= int(s)
        self.numel = numel
        self.buf = torch.full((GUARD + numel + GUARD,), self.poison, dtype=dtype, device=dev)
        self.t = self.buf[GUARD:GUARD + numel].view(tuple(shape))
        if init is not None:
            self.t.copy_(init.to(dev))
        self.before = self.t.cpu().clone()

    def ptr(self):
        return self.t.data_ptr()

    def bits(self, what):
        torch.cuda.synchronize()
        assert bool((self.buf[:GUARD] == self.poison).all()) and bool((self.buf[GUARD + self.numel:] == self.poison).all()), \
            what + ": written outside the buffer"
        return self.t.cpu()

    def untouched(self, what="refusal"):
        return torch.equal(self.bits(what), self.before)


def _same(got, want, what):
    """bit equality of two integer tensors, with the first difference named"""
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if torch.equal(got, want):
        return
    diff = (got != want)
    idx = tuple(int(v) for v in diff.nonzero()[0])
    mask = (1 << (8 * got.element_size())) - 1
    raise AssertionError("%s: %d of %d elements differ; the first at %s: got 0x%X, expected 0x%X" % (
        what, int(diff.sum()), got.numel(), idx, int(got[idx]) & mask, int(want[idx]) & mask))


def _map_bufs(n, h, w, c, pad, paired, dev, zero_halo=False):
    """the (hi, lo or None) output planes of a map [n, h + 2 pad, w + 2 pad, c]: poison everywhere, or a zero halo round it"""
    shape = (n, h + 2 * pad, w + 2 * pad, c)
    init = None
    if zero_halo:
        init = torch.full(shape, POISON16, dtype=torch.int16)
        init[M.halo_mask(n, h, w, c, pad)] = 0
    return Buf(shape, dev, init=init), (Buf(shape, dev, init=init) if paired else None)


def _expect_interior(buf, inner, pad, what):
    """the plane holds `inner` [n, h, w, c] in its interior and what it held before everywhere else"""
    assert not bool((inner == POISON16).any()), what + ": the reference holds the poison pattern"
    _same(buf.bits(what), M.put_interior(buf.before, inner, pad), what)


def _expect_map(hi, lo, ref, pad, what):
    _expect_interior(hi, ref[0], pad, what + " hi")
    if lo is not None:
        _expect_interior(lo, ref[1], pad, what + " lo")


def _in_planes(v, pad, paired, dev):
    """stored values [n, c, h, w] -> device planes with garbage in the halo, and the fp32 values map_load8 reads of them (NCHW)"""
    hi, lo = P.map_planes(v, pad, paired)
    a = M.load_map(hi, lo)
    if pad:
        a = a[:, pad:-pad, pad:-pad]
    return hi.to(dev), None if lo is None else lo.to(dev), a.permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _fmt(paired):
    return M.BF16 if paired else M.F16


def _name(paired):
    return "pair" if paired else "f16"


def _draw_stored(shape, seed, paired, roll=0):
    """stored values of a map in its format, sums of two of them finite"""
    x = M.draw_values(shape, seed, M.F16).clamp(-1e38, 1e38)
    if roll:
        x = x.roll(roll, 3)
    return M.stored(x, paired)


# ------------------------------------------------------------------------------------------------------------ agp_split_f32
@pytest.mark.parametrize("n", M.SPLIT_N)
@pytest.mark.parametrize("fmt", [M.BF16, M.F16])
def test_split_f32(dev, fmt, n):
    """The scalar tail alone (1, 7), one whole vector (8), vector + tail (9, 2055: a 7-element tail that holds the saturation
    boundary, as the first vectors do) and 8 (4096 * 256) + 8 * 300 + 5: past the grid cap, a second trip of the stride loop that
    ends in a ragged tail.  pack8_h (vector) and split_f16 (tail) must give the reference's bits on both sides of +-65504."""
    L = _L()
    x = M.draw_values((n,), 1, fmt, scatter=False)
    if fmt == M.F16 and n >= 2055:
        assert bool((x[8 * (n // 8):].abs() > 65504).any()) and bool((x[:8 * (n // 8)].abs() > 65504).any())
    xd = x.to(dev)
    want = M.split(x, fmt)
    hi, lo = Buf((n,), dev), Buf((n,), dev)
    _ok(L.agp_split_f32(_ptr(xd), _ptr(hi), _ptr(lo), n, M.FMT_CODE[fmt], _stream()), "agp_split_f32")
    _same(hi.bits("hi"), want[0], "split_f32 %s n %d hi" % (fmt, n))
    _same(lo.bits("lo"), want[1], "split_f32 %s n %d lo" % (fmt, n))
    only, spare = Buf((n,), dev), Buf((n,), dev)
    _ok(L.agp_split_f32(_ptr(xd), _ptr(only), None, n, M.FMT_CODE[fmt], _stream()), "agp_split_f32 (lo == NULL)")
    _same(only.bits("hi"), want[0], "split_f32 %s n %d hi alone" % (fmt, n))
    assert spare.untouched()


def test_split_f32_empty_and_refusals(dev):
    L = _L()
    x = M.draw_values((64,), 2, M.F16, scatter=False).to(dev)
    hi, lo = Buf((64,), dev), Buf((64,), dev)
    for fmt in (0, 1):
        _ok(L.agp_split_f32(_ptr(x), _ptr(hi), _ptr(lo), 0, fmt, _stream()), "agp_split_f32 n = 0")
    assert hi.untouched("n = 0") and lo.untouched("n = 0")
    assert L.agp_split_f32(_ptr(x), _ptr(hi), _ptr(lo), 64, 2, _stream()) == BADARG, "fmt 2"
    assert L.agp_split_f32(_ptr(x), _ptr(hi), _ptr(lo), 64, -1, _stream()) == BADARG, "fmt -1"
    assert L.agp_split_f32(None, _ptr(hi), _ptr(lo), 64, 0, _stream()) == BADARG, "x == NULL"
    assert L.agp_split_f32(_ptr(x), None, _ptr(lo), 64, 0, _stream()) == BADARG, "hi == NULL"
    assert L.agp_split_f32(_ptr(x), _ptr(hi), _ptr(lo), -1, 0, _stream()) == BADARG, "n < 0"
    assert hi.untouched() and lo.untouched()


# ---------------------------------------------------------------------------------------------------- agp_split_conv_weight
@pytest.mark.parametrize("cout,cin,kh,kw", M.WEIGHT_SHAPES)
def test_split_conv_weight(dev, cout, cin, kh, kw):
    """Both layouts through the single entry, every chunk_major the %32 rule allows through the _both entry, and the _both entry
    with chunk_major 0 against the two single calls.  Every weight holds a value of its own (hi plane included)."""
    L = _L()
    w = M.distinct_weights(cout, cin, kh, kw)
    wd = w.to(dev)
    numel = w.numel()
    single = {}
    for dgrad in (0, 1):
        hi, lo = Buf((numel,), dev), Buf((numel,), dev)
        _ok(L.agp_split_conv_weight(_ptr(wd), cout, cin, kh, kw, dgrad, _ptr(hi), _ptr(lo), _stream()), "agp_split_conv_weight")
        want = M.conv_weight_planes(w, dgrad, False)
        what = "split_conv_weight %s dgrad %d (%d threads)" % ((cout, cin, kh, kw), dgrad, M.split_threads(cout, cin, kh, kw, dgrad))
        _same(hi.bits(what), want[0], what + " hi")
        _same(lo.bits(what), want[1], what + " lo")
        single[dgrad] = (hi.bits(what), lo.bits(what))
    modes = M.chunk_major_modes(cout, cin)
    assert 0 in modes
    for cm in modes:
        bufs = [Buf((numel,), dev) for _ in range(4)]
        _ok(L.agp_split_conv_weight_both(_ptr(wd), cout, cin, kh, kw, *[_ptr(b) for b in bufs], cm, _stream()), "agp_split_conv_weight_both")
        what = "split_conv_weight_both %s chunk_major %d (%d threads)" % ((cout, cin, kh, kw), cm, M.split_threads(cout, cin, kh, kw, 2))
        got = [b.bits(what) for b in bufs]
        wf, wd_ = M.conv_weight_planes(w, 0, bool(cm & 1)), M.conv_weight_planes(w, 1, bool(cm & 2))
        for g, r, name in zip(got, (wf[0], wf[1], wd_[0], wd_[1]), ("hi", "lo", "hi_d", "lo_d")):
            _same(g, r, what + " " + name)
        if cm == 0:
            assert torch.equal(got[0], single[0][0]) and torch.equal(got[1], single[0][1]) and torch.equal(got[2], single[1][0]) and \
                torch.equal(got[3], single[1][1]), what + ": not bit-equal to two single calls"


def test_split_conv_weight_refusals(dev):
    L = _L()
    w = M.distinct_weights(64, 64, 3, 3).to(dev)
    bufs = [Buf((64 * 64 * 9,), dev) for _ in range(4)]
    p = [_ptr(b) for b in bufs]
    one = lambda cout, cin, dgrad, hi=p[0], lo=p[1], wp=_ptr(w): L.agp_split_conv_weight(wp, cout, cin, 3, 3, dgrad, hi, lo, _stream())
    assert one(8, 12, 0) == BADARG, "dgrad 0: cin % 8"
    assert one(12, 8, 1) == BADARG, "dgrad 1: cout % 8"
    assert M.split_threads(16, 40, 3, 3, 0) % 256 and M.split_threads(64, 32, 3, 3, 0) % 256 == 0
    for dgrad in (2, 3, -1):         # 2 is the kernel's both-planes mode: this entry has no second pair to give it
        assert one(16, 40, dgrad) == BADARG and one(64, 32, dgrad) == BADARG, "dgrad %d" % dgrad
    assert one(8, 8, 0, hi=None) == BADARG and one(8, 8, 0, lo=None) == BADARG and one(8, 8, 0, wp=None) == BADARG, "NULL"
    both = lambda cout, cin, cm, q=p: L.agp_split_conv_weight_both(_ptr(w), cout, cin, 3, 3, q[0], q[1], q[2], q[3], cm, _stream())
    assert both(8, 12, 0) == BADARG and both(12, 8, 0) == BADARG, "_both: % 8"
    assert both(16, 40, 1) == BADARG, "chunk_major bit 0: cin % 32"
    assert both(16, 64, 2) == BADARG, "chunk_major bit 1: cout % 32"
    assert both(64, 32, 4) == BADARG and both(64, 32, 7) == BADARG and both(64, 32, -4) == BADARG, "chunk_major & ~3"
    for k in range(4):
        assert both(64, 32, 0, [None if j == k else p[j] for j in range(4)]) == BADARG, "_both: NULL plane %d" % k
    assert all(b.untouched() for b in bufs)


# ----------------------------------------------------------------------------------------------------- agp_pack_f32_to_nhwc
def _source(x, layout, dev):
    """-> the [n, c, h, w] fp32 view on the device in one of the source layouts (garbage -3 between the elements of a view)"""
    n, c, h, w = x.shape
    if layout == "nchw":
        return x.to(dev).contiguous()
    if layout == "channels_last":                # sc == 1: the kernel's other thread order
        t = x.to(dev).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert t.stride(1) == 1 or c == 1
        return t
    if layout == "width_strided":
        big = torch.full((n, c, h, 2 * w), P.HALO_POISON)
        big[..., ::2] = x
        return big.to(dev)[..., ::2]
    assert layout == "channel_sliced"
    big = torch.full((n, c + 2, h, w), P.HALO_POISON)
    big[:, 1:c + 1] = x
    return big.to(dev)[:, 1:c + 1]


def _pack(L, t, c, cpad, pad, hi, lo):
    n, _, h, w = t.shape
    sn, sc, sh, sw = t.stride()
    return L.agp_pack_f32_to_nhwc(_ptr(t), sn, sc, sh, sw, n, c, h, w, cpad, pad, _ptr(hi), _ptr(lo), _stream())


@pytest.mark.parametrize("n,c,h,w,cpad", M.PACK_SHAPES)
def test_pack_f32_to_nhwc_generic(dev, n, c, h, w, cpad):
    """The 8-channel kernel: four source layouts (channels_last takes the sc == 1 thread order; the strided views show that sw
    and sc are honoured), pad 0 / 1 / 3, a pair and one fp16 plane.  Channels c .. cpad - 1 are exact +0, the halo stays poison."""
    L = _L()
    for paired in (True, False):
        x = M.draw_values((n, c, h, w), 2, _fmt(paired))
        for layout in M.PACK_LAYOUTS:
            t = _source(x, layout, dev)
            for pad in (0, 1, 3):
                what = "pack [%d, %d, %d, %d] cpad %d %s pad %d %s" % (n, c, h, w, cpad, layout, pad, _name(paired))
                hi, lo = _map_bufs(n, h, w, cpad, pad, paired, dev)
                _ok(_pack(L, t, c, cpad, pad, hi, lo), "agp_pack_f32_to_nhwc")
                ref = M.pack_nhwc(x, c, cpad, pad, paired)
                assert not bool(ref[0][..., c:].any())
                _expect_map(hi, lo, ref, pad, what)


def test_pack_f32_to_nhwc_stride_loop(dev):
    n, c, h, w, cpad = M.PACK_LARGE
    assert n * h * w * (cpad // 8) > M.GRID_CAP
    L = _L()
    x = M.draw_values((n, c, h, w), 3, M.F16)
    hi, _ = _map_bufs(n, h, w, cpad, 1, False, dev)
    _ok(_pack(L, x.to(dev), c, cpad, 1, hi, None), "agp_pack_f32_to_nhwc")
    _expect_interior(hi, M.pack_nhwc(x, c, cpad, 1, False)[0], 1, "pack %s f16 pad 1" % (M.PACK_LARGE,))


def test_pack_f32_to_nhwc_refusals(dev):
    L = _L()
    x = M.draw_values((2, 8, 3, 4), 4, M.F16).to(dev)
    hi, lo = _map_bufs(2, 3, 4, 16, 1, True, dev)
    assert _pack(L, x, 8, 4, 1, hi, lo) == BADARG, "cpad < c"
    assert _pack(L, x[:, :3], 3, 12, 1, hi, lo) == BADARG, "cpad 12: neither 4 nor a multiple of 8"
    assert _pack(L, x[:, :3], 3, 6, 1, hi, lo) == BADARG, "cpad 6"
    assert hi.untouched() and lo.untouched()


@pytest.mark.parametrize("n,c,h,w", M.PACK4_SHAPES)
def test_pack_cpad4_pads_and_the_h16_plane(dev, n, c, h, w):
    """cpad == 4 at pad 0 and 1 (test_gpu_kernels.py holds pad 3): the four-pixel kernel (unit stride, w % 4 == 0, aligned) and
    the generic one (w % 4 != 0, a width-strided view, a source 4 bytes off alignment); agp_pack_f32_to_nhwc4_h16's operand plane
    h16 == half(x) bit for bit on the fast path and AGP_E_UNSUPPORTED, nothing written, everywhere else."""
    L = _L()
    for paired in (True, False):
        x = M.draw_values((n, c, h, w), 5, _fmt(paired))
        off = torch.full((x.numel() + 4,), P.HALO_POISON)
        off[1:1 + x.numel()] = x.reshape(-1)
        offd = off.to(dev)
        sources = {"nchw": _source(x, "nchw", dev), "width_strided": _source(x, "width_strided", dev),
                   "misaligned": offd[1:1 + x.numel()].view(n, c, h, w)}
        assert sources["misaligned"].data_ptr() % 16 == 4 and sources["nchw"].data_ptr() % 16 == 0
        for name, t in sources.items():
            fast = name == "nchw" and w % 4 == 0
            for pad in (0, 1):
                what = "pack4 [%d, %d, %d, %d] %s pad %d %s" % (n, c, h, w, name, pad, _name(paired))
                ref = M.pack_nhwc(x, c, 4, pad, paired)
                hi, lo = _map_bufs(n, h, w, 4, pad, paired, dev)
                _ok(_pack(L, t, c, 4, pad, hi, lo), "agp_pack_f32_to_nhwc")
                _expect_map(hi, lo, ref, pad, what)
                hi, lo = _map_bufs(n, h, w, 4, pad, paired, dev)
                h16, _ = _map_bufs(n, h, w, 4, pad, False, dev)
                sn, sc, sh, sw = t.stride()
                rc = L.agp_pack_f32_to_nhwc4_h16(_ptr(t), sn, sc, sh, sw, n, c, h, w, pad, _ptr(hi), _ptr(lo), _ptr(h16), _stream())
                if fast:
                    _ok(rc, "agp_pack_f32_to_nhwc4_h16")
                    _expect_map(hi, lo, ref, pad, what + " (h16 entry)")
                    _expect_interior(h16, M.pack_nhwc(x, c, 4, pad, False)[0], pad, what + " h16")
                else:
                    assert rc == UNSUPPORTED, "%s: agp_pack_f32_to_nhwc4_h16 returned %d" % (what, rc)
                    assert hi.untouched() and (lo is None or lo.untouched()) and h16.untouched()


# ------------------------------------------------------------------------------------------------- agp_pack_u8_cams_to_nhwc
CAM_SWEEP = (1, 2, 8, 16)            # 256 pixels: every byte value in every channel


def _cam_image(n, ncam, h, w):
    idx = torch.arange(n * ncam * h * w, dtype=torch.int64)
    img = torch.stack([(idx * k + o) % 256 for k, o in ((37, 0), (101, 85), (203, 170))], -1)
    return img.to(torch.uint8).view(n, ncam, h, w, 3)


@pytest.mark.parametrize("n,ncam,h,w", M.CAM_SHAPES + (CAM_SWEEP,))
def test_pack_u8_cams(dev, n, ncam, h, w):
    """(u8 / 255 - mean) / std in fp32 in that order, then the split: bit-equal to torch's correctly rounded fp32 division on the
    CPU; tiles side by side, the 4th channel +0, the halo left alone."""
    import ctypes as C
    L = _L()
    img = _cam_image(n, ncam, h, w)
    if (n, ncam, h, w) == CAM_SWEEP:
        for ch in range(3):
            assert len(torch.unique(img[..., ch])) == 256
    imgd = img.to(dev)
    m, s = (C.c_float * 3)(*M.CAM_MEAN), (C.c_float * 3)(*M.CAM_STD)
    for paired in (True, False):
        for pad in (0, 3):
            what = "pack_u8_cams [%d, %d, %d, %d] pad %d %s" % (n, ncam, h, w, pad, _name(paired))
            rh, rl, v = M.u8_cams(img, M.CAM_MEAN, M.CAM_STD, pad, paired)
            hi, lo = _map_bufs(n, h, ncam * w, 4, pad, paired, dev)
            _ok(L.agp_pack_u8_cams_to_nhwc(_ptr(imgd), n, ncam, h, w, m, s, pad, _ptr(hi), _ptr(lo), _stream()), "agp_pack_u8_cams_to_nhwc")
            assert not bool(rh[..., 3].any())
            _expect_map(hi, lo, (rh, rl), pad, what)


# --------------------------------------------------------------------------------------------------- agp_unpack_nhwc_to_f32
@pytest.mark.parametrize("c", M.UNPACK_C)
def test_unpack_nhwc_to_f32(dev, c):
    """Planes built on the CPU, garbage in the halo: the output is float(hi) + float(lo) bit for bit, in NHWC order."""
    L = _L()
    n, h, w = M.UNPACK_NHW
    for paired in (True, False):
        v = M.stored(M.draw_values((n, c, h, w), 6, _fmt(paired)), paired)
        for pad in (0, 1, 3):
            hi, lo, a = _in_planes(v, pad, paired, dev)
            out = Buf((n, h, w, c), dev, torch.int32)
            _ok(L.agp_unpack_nhwc_to_f32(_ptr(hi), _ptr(lo), n, h, w, c, pad, _ptr(out), _stream()), "agp_unpack_nhwc_to_f32")
            _same(out.bits("unpack"), _nhwc(a).view(torch.int32), "unpack c %d pad %d %s" % (c, pad, _name(paired)))


def test_unpack_refusals(dev):
    L = _L()
    hi, lo, _ = _in_planes(M.stored(M.draw_values((2, 16, 3, 5), 6, M.BF16), True), 1, True, dev)
    out = Buf((2, 3, 5, 16), dev, torch.int32)
    call = lambda h_, n=2, c=16, o=_ptr(out): L.agp_unpack_nhwc_to_f32(h_, _ptr(lo), n, 3, 5, c, 1, o, _stream())
    assert call(_ptr(hi), c=12) == BADARG, "c % 8"
    assert call(None) == BADARG and call(_ptr(hi), o=None) == BADARG, "NULL"
    assert call(_ptr(hi), n=0) == BADARG, "n = 0"
    assert out.untouched()


# -------------------------------------------------------------------------------------------------------- agp_map_zero_halo
@pytest.mark.parametrize("c", M.HALO_C)
def test_map_zero_halo(dev, c):
    """16-byte (c 8, 64), 8-byte (4, 12) and 2-byte (3, 5) pieces: after the call exactly the halo is zero and the interior
    still poison, in both planes; pad 0 is accepted and writes nothing."""
    L = _L()
    for n, h, w in M.HALO_NHW:
        for pad in (0, 1, 2, 3):
            for paired in (True, False):
                what = "zero_halo [%d, %d, %d, %d] pad %d%s" % (n, h, w, c, pad, " hi + lo" if paired else "")
                hi, lo = _map_bufs(n, h, w, c, pad, paired, dev)
                spare = Buf((8,), dev)
                _ok(L.agp_map_zero_halo(_ptr(hi), _ptr(lo), n, h, w, c, pad, _stream()), "agp_map_zero_halo")
                mask = M.halo_mask(n, h, w, c, pad)
                for b in (hi, lo) if paired else (hi,):
                    want = b.before.clone()
                    want[mask] = 0
                    _same(b.bits(what), want, what)
                    assert pad or b.untouched()
                assert spare.untouched()


# ----------------------------------------------------------------------------------------------------- agp_maxpool3x3s2_fwd
@pytest.mark.parametrize("paired", [True, False], ids=["pair", "f16"])
@pytest.mark.parametrize("n,h,w,c", M.POOL_SHAPES)
def test_maxpool3x3s2_fwd(dev, n, h, w, c, paired):
    """Odd and even sizes, input halo 1 and 3, output halo 0 and 1, with and without the argmax.  The values are max_pool2d of the
    stored values, re-stored; the argmax is the first strictly positive maximum in window order, 4 for an all-zero window."""
    L = _L()
    v = M.draw_relu_map(n, c, h, w, 3, paired)
    vals, pos = M.maxpool_first_positive(v)
    ho, wo = M.pool_out(h, w)
    ref = M.store_map(_nhwc(vals.float()), paired)
    for pin in (1, 3):
        ih, il = M.maxpool_input_planes(v, pin, paired)
        ihd, ild = ih.to(dev), None if il is None else il.to(dev)
        for pout in (0, 1):
            for with_idx in (True, False):
                what = "maxpool [%d, %d, %d, %d] %s pin %d pout %d%s" % (n, h, w, c, _name(paired), pin, pout, " argmax" if with_idx else "")
                hi, lo = _map_bufs(n, ho, wo, c, pout, paired, dev)
                idx = Buf((n, ho, wo, c), dev, torch.uint8)
                _ok(L.agp_maxpool3x3s2_fwd(_ptr(ihd), _ptr(ild), n, h, w, c, pin, _ptr(hi), _ptr(lo), ho, wo, pout,
                                           _ptr(idx) if with_idx else None, _stream()), "agp_maxpool3x3s2_fwd")
                _expect_map(hi, lo, ref, pout, what)
                if with_idx:
                    _same(idx.bits(what), _nhwc(pos), what + " argmax")
                else:
                    assert idx.untouched()


def test_maxpool_refusals(dev):
    L = _L()
    n, h, w, c = 2, 5, 7, 16
    v = M.draw_relu_map(n, c, h, w, 3, True)
    ih, il = (t.to(dev) for t in M.maxpool_input_planes(v, 1, True))
    hi, lo = _map_bufs(n, 3, 4, c, 1, True, dev)
    idx = Buf((n, 3, 4, c), dev, torch.uint8)
    call = lambda pin=1, ho=3, wo=4, cc=c: L.agp_maxpool3x3s2_fwd(_ptr(ih), _ptr(il), n, h, w, cc, pin, _ptr(hi), _ptr(lo), ho, wo, 1,
                                                                 _ptr(idx), _stream())
    assert call(pin=0) == BADARG, "pin == 0"
    assert call(ho=2) == BADARG and call(ho=4) == BADARG, "hout"
    assert call(wo=3) == BADARG and call(wo=5) == BADARG, "wout"
    assert call(cc=12) == BADARG, "c % 8"
    assert hi.untouched() and lo.untouched() and idx.untouched()


# --------------------------------------------------------------------------------------------------------- agp_bcast_add_fwd
@pytest.mark.parametrize("n,h,w,c", M.ADD_SHAPES)
def test_bcast_add_fwd(dev, n, h, w, c):
    """pin != pout, pair -> pair and f16 -> f16: bit-equal to store_map(fp32(a) + vec)."""
    L = _L()
    for paired in (True, False):
        v = _draw_stored((n, c, h, w), 7, paired)
        vec = M.draw_values((n, c), 8, M.F16).clamp(-1e38, 1e38)
        vecd = vec.to(dev)
        for pin, pout in ((1, 3), (3, 1), (0, 1), (1, 0)):
            ah, al, a = _in_planes(v, pin, paired, dev)
            hi, lo = _map_bufs(n, h, w, c, pout, paired, dev)
            _ok(L.agp_bcast_add_fwd(_ptr(ah), _ptr(al), _ptr(vecd), n, h, w, c, pin, _ptr(hi), _ptr(lo), pout, _stream()), "agp_bcast_add_fwd")
            ref = M.store_map(_nhwc(M.bcast_add(a, vec)), paired)
            _expect_map(hi, lo, ref, pout, "bcast_add [%d, %d, %d, %d] %s pin %d pout %d" % (n, h, w, c, _name(paired), pin, pout))


# --------------------------------------------------------------------------------------------------------------- agp_map_add
@pytest.mark.parametrize("n,h,w,c", M.ADD_SHAPES)
def test_map_add(dev, n, h, w, c):
    """a alone (a copy of the loaded values), a + b, a [mask > 0], a [mask > 0] + b; the mask holds zeros, -0, negatives and the
    smallest positive values of its format: bit-equal to store_map of the fp32 expression, mask first, then the add."""
    L = _L()
    shape = (n, c, h, w)
    for paired in (True, False):
        ah, al, a = _in_planes(_draw_stored(shape, 9, paired), 1, paired, dev)
        bh, bl, b = _in_planes(_draw_stored(shape, 10, paired, roll=1), 1, paired, dev)
        mv = M.mask_values(shape, 1) if paired else M.mask_values_f16(shape, 1)
        mh, ml, m = _in_planes(mv, 1, paired, dev)
        assert torch.equal(m.double(), mv)
        for with_b in (False, True):
            for with_mask in (False, True):
                what = "map_add [%d, %d, %d, %d] %s%s%s" % (n, h, w, c, _name(paired), " mask" if with_mask else "", " + b" if with_b else "")
                hi, lo = _map_bufs(n, h, w, c, 1, paired, dev)
                _ok(L.agp_map_add(_ptr(ah), _ptr(al), _ptr(bh) if with_b else None, _ptr(bl) if with_b else None,
                                  _ptr(mh) if with_mask else None, _ptr(ml) if with_mask else None, n, h, w, c, 1, _ptr(hi), _ptr(lo),
                                  _stream()), "agp_map_add")
                ref = M.store_map(_nhwc(M.map_add(a, b if with_b else None, m if with_mask else None)), paired)
                _expect_map(hi, lo, ref, 1, what)


# -------------------------------------------------------------------------------------------------------- agp_upsample2_zero
@pytest.mark.parametrize("src,dst", M.UPSAMPLE, ids=["%dx%d-%dx%d" % (s + d) for s, d in M.UPSAMPLE])
def test_upsample2_zero(dev, src, dst):
    """The source halo holds garbage; the output interior is poisoned beforehand and must be written throughout (values at the even
    coordinates, exact +0 elsewhere); its zero halo stays zero."""
    L = _L()
    (ho, wo), (hu, wu) = src, dst
    n = 2
    for c in (8, 24):
        for paired in (True, False):
            v = _draw_stored((n, c, ho, wo), 11, paired)
            for gpad in (0, 1):
                gh, gl, g = _in_planes(v, gpad, paired, dev)
                hi, lo = _map_bufs(n, hu, wu, c, 1, paired, dev, zero_halo=True)
                _ok(L.agp_upsample2_zero(_ptr(gh), _ptr(gl), n, ho, wo, c, gpad, _ptr(hi), _ptr(lo), hu, wu, 1, _stream()), "agp_upsample2_zero")
                u = M.upsample2_zero(g, hu, wu)
                ref = M.store_map(_nhwc(u), paired)
                off = torch.ones((hu, wu), dtype=torch.bool)
                off[::2, ::2] = False
                assert not bool(ref[0][:, off].any()), "the reference's odd coordinates are not +0"
                _expect_map(hi, lo, ref, 1, "upsample2_zero %s -> %s c %d %s gpad %d" % (src, dst, c, _name(paired), gpad))


# ---------------------------------------------------------------------------------------------------------- agp_map_chan_sum
@pytest.mark.parametrize("n,h,w", M.CHAN_SUM_NHW)
@pytest.mark.parametrize("c", M.CHAN_SUM_C)
def test_map_chan_sum(dev, c, n, h, w):
    """The one inexact kernel: fp32 chains per thread and per block, an fp64 finalize.  Bar 1e-5 of sum |terms| per channel (the
    float32 floor of these cases is below a quarter of it: test_map_ref.py); two calls bit-equal; the workspace starts as NaN."""
    L = _L()
    nfl = int(L.agp_train_reduce_workspace_floats(n, h, w, c))
    for paired in (True, False):
        v = M.draw_chan_sum(n, c, h, w, paired)
        ref, mag = M.chan_sum64(v)
        hi, lo, _ = _in_planes(v, 1, paired, dev)
        seen = []
        for _ in range(2):
            ws, out = Buf((nfl,), dev, torch.int32), Buf((c,), dev, torch.int32)
            _ok(L.agp_map_chan_sum(_ptr(hi), _ptr(lo), n, h, w, c, 1, _ptr(out), _ptr(ws), _stream()), "agp_map_chan_sum")
            ws.bits("workspace")
            got = out.bits("chan_sum")
            assert not bool((got == POISON).any()), "channels were not written"
            seen.append(got)
        assert torch.equal(seen[0], seen[1]), "two calls are not bit-equal"
        got = seen[0].view(torch.float32).double()
        err = ((got - ref).abs() / mag)
        print("chan_sum [%d, %d, %d, %d] %s: worst %.3e of sum |terms| (bar %.1e)" % (n, h, w, c, _name(paired), float(err.max()), M.CHAN_SUM_BAR))
        assert not bool(torch.isnan(got).any()) and float(err.max()) <= M.CHAN_SUM_BAR, "channel %d: %.3e" % (int(err.argmax()), float(err.max()))


def test_map_chan_sum_refusal(dev):
    L = _L()
    c = 2056
    hi = torch.zeros((1, 3, 3, c), dtype=torch.bfloat16, device=dev)
    ws, out = Buf((int(L.agp_train_reduce_workspace_floats(1, 1, 1, c)),), dev, torch.int32), Buf((c,), dev, torch.int32)
    assert L.agp_map_chan_sum(_ptr(hi), _ptr(hi), 1, 1, 1, c, 1, _ptr(out), _ptr(ws), _stream()) == BADARG, "c / 8 > 256"
    assert L.agp_map_chan_sum(_ptr(hi), _ptr(hi), 1, 1, 1, 12, 1, _ptr(out), _ptr(ws), _stream()) == BADARG, "c % 8"
    assert ws.untouched() and out.untouched()


# ------------------------------------------------------------------------------------------------------ agp_bn_frozen_coeffs
@pytest.mark.parametrize("c", M.FROZEN_C)
def test_bn_frozen_coeffs(dev, c):
    """The block edge (255, 256, 257 channels), gamma / beta given and NULL, variances 0 and 1e-12 beside eps 1e-5: float(the
    fp64 formula) bit for bit."""
    L = _L()
    rm, rv, gamma, beta = M.draw_frozen(c)
    rmd, rvd, gd, bd = (t.to(dev) for t in (rm, rv, gamma, beta))
    for affine in (True, False):
        outs = [Buf((c,), dev, torch.int32) for _ in range(4)]
        _ok(L.agp_bn_frozen_coeffs(_ptr(rmd), _ptr(rvd), _ptr(gd) if affine else None, _ptr(bd) if affine else None, c, M.FROZEN_EPS,
                                   *[_ptr(o) for o in outs], _stream()), "agp_bn_frozen_coeffs")
        ref = M.frozen_coeffs64(rm, rv, gamma if affine else None, beta if affine else None, M.FROZEN_EPS)
        for o, r, name in zip(outs, ref, ("mean", "rstd", "scale", "shift")):
            got = o.bits(name)
            d = M.ulp_distance(got.view(torch.float32), r)
            print("bn_frozen_coeffs c %d%s %s: %d of %d differ, at most %d ulp" % (c, " affine" if affine else "", name, int((d > 0).sum()), c, int(d.max())))
            _same(got, r.view(torch.int32), "bn_frozen_coeffs c %d%s %s" % (c, " affine" if affine else "", name))
