"""References, plan mirror and problem builders of the dense training-kernel tests (tests/test_dense_train_ref.py pins them to
fp64 autograd and to the library's own workspace query on the CPU; tests/test_gpu_wgrad_kernels.py and
tests/test_gpu_bn_bwd_kernels.py hold the HIP kernels of csrc/wgrad_tr.hip and csrc/train.hip against them): plain fp64 forms
of the dense weight gradient (the packed 7x7 stem included), of the BatchNorm backward and of the fused affine + ReLU +
max-pool, a Python restatement of make_plan() for choosing and naming shapes, the emulations of the two weight-gradient
arithmetics, and the per-granule error.  Every function works on the device of its arguments (torch's own ops only)."""
import torch
import torch.nn.functional as F

from conv_sched_util import _bf16_pair, _f16

# ------------------------------------------------------------------------------------------------------------------- bars
BAR_3P = 1e-4                    # the three-product kernel (tests/test_gpu_train.py test_one_pass_fp16_weight_gradient: e3 < 1e-4)
BAR_1P, BAR_1P_CHANNEL = 1e-3, 2e-3          # the one-pass kernels: TOL per granule, 2e-3 per output channel (the same test)
ONE_PASS_REALLY_RAN = 3e-5       # ... whose whole-tensor error lies ABOVE this (an fp16-sized error, not the three products')
BN_BAR_MAX = 1e-5                # gz / gres per channel: never above the bar of test_bn_stats_matches_torch_batchnorm
SUM_BAR = 1e-5                   # ggamma / gbeta: |got - ref| <= SUM_BAR * sum |terms| (fp32 chains of a few dozen terms: ~2^-24 per
#                                  term, an fp64 finalize; the bound is about ten times that)


# ----------------------------------------------------------------------------------------------------------- shapes, plans
def out_hw(h, w, k, stride, stem=False):
    if stem:
        k, stride = 7, 2
    pad = k // 2
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def wgrad_plan(cin, cout, k, stride, h, w, n, f16=False, stem=False):
    """What make_plan() of csrc/wgrad_tr.hip decides for a k x k conv (pad k // 2, 1-pixel-halo maps; stem: the packed 7x7 / 2
    stem), restated: f16 = the descriptor carries in_h16 / out_absmax.  None where the library refuses the shape.
      mode 0 the 3x3 stride-1 raster kernels, 1 the gather kernels; nb A-blocks per workgroup; gx, gy the tile grid
      one_pass        a one-product fp16 kernel runs (mode 0 with cin % 64 == 0, every mode-1 plan) -- only with f16
      P, kpix, ksteps raster positions per K-step, raster length n (ho + 2)(wo + 2), its K-steps
      per, splits     K-steps per split, splits;  last: K-steps of the last split;  kpix_mod_p: kpix % P
      last_group      A-blocks of the last workgroup along x (nb where the blocks divide)
      slots           (mode-0 one-pass) workgroup slots per tile of the XCD-ordered grid, 8 * ceil(splits / 8) >= splits"""
    if stem:
        cin_d, kh, kw, stride = 32, 7, 1, 2
    else:
        cin_d, kh, kw = cin, k, k
    if cout % 64 or cin_d % 32 or n <= 0:
        return None
    ho, wo = out_hw(h, w, k, stride, stem)
    taps, cblocks = kh * kw, cin_d // 32
    kxr = (not stem) and k == 3 and stride == 1
    if kxr or taps == 9:
        nb, gx = 9, cblocks
    elif taps == 7 and cblocks == 1:
        nb, gx = 7, 1
    elif taps == 1:
        nb = 8 if cblocks >= 8 else (4 if cblocks >= 4 else 2)
        gx = (cblocks + nb - 1) // nb
    else:
        return None
    gy = cout // 64
    kpix = n * (ho + 2) * (wo + 2)
    P = 64 if kxr else 32
    ksteps = (kpix + P - 1) // P
    tiles = gx * gy
    f16_raster = bool(kxr and f16 and cin_d % 64 == 0)
    if f16_raster:
        splits = max(1, 512 // ((cin_d // 64) * gy))
        splits = min(splits, ksteps // 8)
    else:
        splits = min((1024 + tiles - 1) // tiles, ksteps // 24)
    splits = min(max(splits, 1), 1024)
    per = (ksteps + splits - 1) // splits
    splits = (ksteps + per - 1) // per
    nblk = taps * cblocks
    return dict(mode=0 if kxr else 1, nb=nb, gx=gx, gy=gy, kpix=kpix, P=P, ksteps=ksteps, per=per, splits=splits,
                last=ksteps - (splits - 1) * per, kpix_mod_p=kpix % P, last_group=nblk - (gx - 1) * nb if not kxr else 9,
                one_pass=bool(f16 and (f16_raster or not kxr)), slots=8 * ((splits + 7) // 8) if f16_raster else None,
                rows=taps * cin_d, ho=ho, wo=wo)


def smallest_n(cin, cout, k, stride, h, w, f16, want, most=1024):
    """The smallest batch whose plan satisfies `want(plan)`."""
    for n in range(1, most):
        if want(wgrad_plan(cin, cout, k, stride, h, w, n, f16)):
            return n
    raise AssertionError("no batch below %d qualifies" % most)


def _many_splits(p):             # the reduce kernel's second trip, a last trip that is not full, a partial last split
    return p["splits"] > 32 and p["splits"] % 4 != 0 and p["last"] < p["per"]


def _many_chunks(p):
    return p["splits"] > 32 and p["splits"] % 8 != 0


N_MANY_SPLITS = smallest_n(64, 64, 3, 1, 62, 94, False, _many_splits)
N_MANY_CHUNKS = smallest_n(64, 64, 3, 1, 56, 56, True, _many_chunks)

# name -> ((cin, cout, k, stride, h, w, n), the regime: a predicate on (three-product plan, one-pass plan or None)).  Both test
# files take the shapes from here and the host test asserts every regime through wgrad_plan, which it holds to the library's own
# workspace query: a heuristic that moves fails there instead of silently losing the coverage.
CASES = {
    "one_kstep": ((32, 64, 3, 1, 5, 7, 1),
                  lambda t, o: t["mode"] == 0 and t["kpix"] == 63 and t["ksteps"] == 1 and t["splits"] == 1 and o is None),
    "gx3": ((96, 64, 3, 1, 9, 11, 3), lambda t, o: t["mode"] == 0 and t["gx"] == 3 and o is None),
    "s1_small": ((64, 64, 3, 1, 13, 17, 3), lambda t, o: t["splits"] == 1 and o["splits"] == 1 and o["mode"] == 0),
    "s1_splits": ((64, 64, 3, 1, 30, 45, 5),
                  lambda t, o: (t["splits"], t["per"], t["last"], t["kpix_mod_p"]) == (4, 30, 28, 32) and
                  (o["splits"], o["slots"], o["last"]) == (14, 16, 1)),
    "s1_128": ((128, 128, 3, 1, 15, 22, 4),
               lambda t, o: (o["splits"], o["per"], o["last"]) == (3, 9, 8) and t["splits"] == 1 and t["gx"] * t["gy"] == 8),
    "s1_wide": ((256, 512, 3, 1, 7, 9, 2), lambda t, o: t["gx"] == 8 and t["gy"] == 8 and t["ksteps"] == 4),
    "s1_many_splits": ((64, 64, 3, 1, 62, 94, N_MANY_SPLITS), lambda t, o: _many_splits(t)),
    "f16_many_chunks": ((64, 64, 3, 1, 56, 56, N_MANY_CHUNKS), lambda t, o: _many_chunks(o)),
    "s2_entry": ((64, 128, 3, 2, 29, 37, 2), lambda t, o: t["mode"] == 1 and t["nb"] == 9 and o["one_pass"]),
    "s2_entry_splits": ((64, 128, 3, 2, 56, 84, 3), lambda t, o: t["mode"] == 1 and t["nb"] == 9 and t["splits"] > 1 and
                        o["splits"] == t["splits"]),
    "ds_one_block": ((32, 64, 1, 2, 12, 15, 1), lambda t, o: t["nb"] == 2 and t["gx"] == 1 and t["last_group"] == 1),
    "ds_ragged2": ((96, 64, 1, 2, 13, 21, 2), lambda t, o: t["nb"] == 2 and t["gx"] == 2 and t["last_group"] == 1),
    "p1_ragged4": ((160, 64, 1, 1, 9, 11, 3), lambda t, o: t["nb"] == 4 and t["gx"] == 2 and t["last_group"] == 1),
    "p1_ragged8": ((288, 128, 1, 1, 9, 11, 3), lambda t, o: t["nb"] == 8 and t["gx"] == 2 and t["last_group"] == 1),
    "p1_exact8": ((256, 64, 1, 1, 6, 6, 2), lambda t, o: t["nb"] == 8 and t["last_group"] == 8 and t["kpix_mod_p"] == 0),
    "p1_many_splits": ((32, 64, 1, 1, 96, 128, 6), lambda t, o: (t["splits"], t["per"], t["last"]) == (96, 25, 14) and
                       (o["splits"], o["last"]) == (96, 14)),
    "stem": ((3, 64, 7, 2, 37, 53, 2), lambda t, o: t["nb"] == 7 and t["splits"] == 1 and t["kpix_mod_p"] == 2 and o["one_pass"]),
    "stem_splits": ((3, 64, 7, 2, 64, 96, 3), lambda t, o: (t["splits"], t["per"], t["last"]) == (6, 27, 25)),
}
GSCALES = {"s1_splits": (3e-7, 1.0, 1e4), "s2_entry": (3e-7, 1.0, 1e4), "stem_splits": (3e-7, 1.0, 1e4)}


def is_stem(name):
    return name.startswith("stem")


def plans(name):
    """(three-product plan, one-pass plan or None) of a case"""
    shape = CASES[name][0]
    t = wgrad_plan(*shape, f16=False, stem=is_stem(name))
    o = wgrad_plan(*shape, f16=True, stem=is_stem(name))
    return t, (o if o["one_pass"] else None)


def wgrad_desc(name, f16=False):
    return desc_of(CASES[name][0], is_stem(name), f16)


def desc_of(shape, stem=False, f16=False):
    """The agp_conv_desc of (cin, cout, k, stride, h, w, n) as train_graph.ConvBNUnit._wgrad fills it: geometry, and the pointer
    fields the entry points look at as NULL / non-NULL set to 1 (the workspace query dereferences nothing; the GPU tests put their
    planes in)."""
    from agplace_amd import _lib
    cin, cout, k, stride, h, w, n = shape
    d = _lib.ConvDesc()
    d.in_hi = d.in_lo = d.out_hi = d.out_lo = 1
    d.n, d.hin, d.win = n, h, w
    d.hout, d.wout = out_hw(h, w, k, stride, stem)
    d.cout, d.pout = cout, 1
    if stem:
        d.cin, d.in_w_step, d.pin, d.kh, d.kw, d.stride, d.pad = 32, 4, 3, 7, 1, 2, 3
    else:
        d.cin, d.in_w_step, d.pin, d.kh, d.kw, d.stride, d.pad = cin, cin, 1, k, k, stride, k // 2
    d.prec = _lib.PREC_BF16X3
    if f16:
        d.in_h16 = d.out_absmax = 1
    return d


# ---------------------------------------------------------------------------------------------------------------- operands
def draw_wgrad(name, gscale=1.0, seed=0, dev="cpu", n=None):
    """(x [n, cin, h, w], g [n, cout, ho, wo]) as fp64 STORED values: x = relu(randn) as fp16 values (a bf16 pair holds them
    exactly too), g = randn * gscale with the first quarter of the channels 1e-3 as large, rounded to a bf16 pair."""
    cin, cout, k, stride, h, w, n0 = CASES[name][0]
    n = n0 if n is None else n
    ho, wo = out_hw(h, w, k, stride, is_stem(name))
    gen = torch.Generator(device=dev).manual_seed(1000 * seed + 7 * cin + cout + 31 * h + w + n)
    x = _f16(torch.randn((n, cin, h, w), generator=gen, device=dev).relu_())
    g = torch.randn((n, cout, ho, wo), generator=gen, device=dev) * gscale
    g[:, :cout // 4] *= 1e-3
    return x, _bf16_pair(g)


def nhwc_map(v, pad, channels=None):
    """[n, c, h, w] values -> the halo-padded NHWC map [n, h + 2 pad, w + 2 pad, channels or c], halo and extra channels zero."""
    n, c, h, w = v.shape
    m = torch.zeros((n, h + 2 * pad, w + 2 * pad, channels or c), dtype=v.dtype, device=v.device)
    m[:, pad:pad + h, pad:pad + w, :c] = v.permute(0, 2, 3, 1)
    return m


def planes(v, paired):
    """Stored VALUES -> (hi, lo) planes: one fp16 plane, or a bf16 pair; asserts that the format holds the values exactly."""
    f = v.float()
    if not paired:
        hi = f.half()
        assert torch.equal(hi.double(), v.double()), "not an fp16 value"
        return hi.contiguous(), None
    hi = f.bfloat16()
    lo = (f - hi.float()).bfloat16()
    assert torch.equal(hi.double() + lo.double(), v.double()), "not a bf16-pair value"
    return hi.contiguous(), lo.contiguous()


def split_bf16(v):
    """fp64 values of a bf16 pair -> (hi, lo) as fp64"""
    hi = v.float().bfloat16().double()
    return hi, v.double() - hi


# --------------------------------------------------------------------------------------------------- weight gradient, fp64
def _taps(x, g, k, stride, pad, shifted=None):
    """The per-tap operand pairs of dW[ky][kx] = X_tap^T G: yields (tap, X_tap [ci, n ho wo]); G is [n ho wo, co].
    shifted: a tap whose strip is read one pixel to the right (a planted defect)."""
    n, ci, h, w = x.shape
    ho, wo = g.shape[2], g.shape[3]
    xp = F.pad(x, (pad, pad + stride + 1, pad, pad + stride))
    for ky in range(k):
        for kx in range(k):
            sx = kx + (1 if shifted == ky * k + kx else 0)
            xs = xp[:, :, ky:ky + stride * (ho - 1) + 1:stride, sx:sx + stride * (wo - 1) + 1:stride]
            yield ky * k + kx, xs.permute(1, 0, 2, 3).reshape(ci, -1)


def wgrad64(x, g, k, stride, pad, shifted=None):
    """dW[ky][kx][ci][co] = sum over output pixels x[img][s oy + ky - pad][s ox + kx - pad][ci] g[img][oy][ox][co] in fp64, one
    matrix product per tap (an explicit unfold)."""
    x, g = x.double(), g.double()
    gm = g.permute(0, 2, 3, 1).reshape(-1, g.shape[1])
    return torch.stack([xt @ gm for _, xt in _taps(x, g, k, stride, pad, shifted)]).view(k, k, x.shape[1], g.shape[1])


def wgrad64_stem_packed(x, g, shifted=None):
    """The packed 7x7 / stride-2 / pad-3 stem as ConvBNUnit._wgrad describes it (cin, in_w_step = 32, 4; kh, kw = 7, 1): the image
    is an NHWC map of 4 channels (RGB + a zero channel) with a 3-pixel halo and a "tap" is one ky with 32 "channels" = 8 pixels x
    4 channels -> [7][8][4][cout].  [:, :7, :3] is the real gradient, [:, :, 3] is exactly zero, [:, 7] belongs to a tap that does
    not exist (the window's eighth column: whatever lies there; the host drops it) and is NaN here."""
    real = wgrad64(x, g, 7, 2, 3, shifted)                          # [7][7][3][cout]
    out = torch.full((7, 8, 4, g.shape[1]), float("nan"), dtype=torch.float64, device=x.device)
    out[:, :7, :3] = real
    out[:, :7, 3] = 0
    return out


def comparable(name, gw):
    """A kernel's or a reference's gradient as [taps, rows, cout], the rows that mean something: [k k, cin, cout], or the stem's
    [7, 7 x 3, cout] out of its packed [7][8][4][cout]."""
    if is_stem(name):
        return gw.reshape(7, 8, 4, -1)[:, :7, :3].reshape(7, 21, -1)
    return gw.reshape(-1, CASES[name][0][0], gw.shape[-1])


def reference(name, x, g, shifted=None):
    """wgrad64 of a case's operands as comparable() gives it"""
    _, _, k, stride, _, _, _ = CASES[name][0]
    return comparable(name, wgrad64_stem_packed(x, g, shifted) if is_stem(name) else wgrad64(x, g, k, stride, k // 2, shifted))


def granule_rel(got, ref):
    """rel-L2 of every (tap, 32 ci, 32 co) granule -- one MFMA accumulator tile -- of [taps, rows, cout] gradients ->
    (the worst, "tap t ci a..b co c..d", the [taps, row blocks, co blocks] tensor).  A granule whose reference is all zero
    counts its absolute error (an all-zero channel block must come out as zeros)."""
    got, ref = got.double(), ref.double()
    t, r, c = ref.shape
    rb, cb = (r + 31) // 32, (c + 31) // 32

    def blocks(v):
        p = torch.zeros((t, rb * 32, cb * 32), dtype=torch.float64, device=ref.device)
        p[:, :r, :c] = v
        return p.view(t, rb, 32, cb, 32).sum((2, 4))
    num, den = blocks((got - ref) ** 2), blocks(ref ** 2)
    rel = torch.where(den > 0, num / den.clamp_min(1e-300), num).sqrt()
    rel = torch.nan_to_num(rel, nan=float("inf"))
    i = int(rel.argmax())
    tap, j = divmod(i, rb * cb)
    b, cc = divmod(j, cb)
    where = "tap %d ci %d..%d co %d..%d" % (tap, 32 * b, min(r, 32 * b + 32) - 1, 32 * cc, min(c, 32 * cc + 32) - 1)
    return float(rel.max()), where, rel


def per_out_channel_rel(got, ref):
    """The same per output channel -> (the worst, the channel, the [cout] vector)"""
    got, ref = got.double(), ref.double()
    num, den = ((got - ref) ** 2).sum((0, 1)), (ref ** 2).sum((0, 1))
    rel = torch.nan_to_num(torch.where(den > 0, num / den.clamp_min(1e-300), num).sqrt(), nan=float("inf"))
    return float(rel.max()), int(rel.argmax()), rel


def whole_rel(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------ the two arithmetics, emulated
def emulate_three_product(name, x, g, drop_xl_block=None, shifted=None):
    """The three-product kernel's arithmetic in fp64: xh gh + xh gl + xl gh of the bf16 pairs, the lo x lo term dropped.
    drop_xl_block: a 32-channel block whose xl gh product is missing (a planted defect)."""
    xh, xl = split_bf16(x)
    gh, gl = split_bf16(g)
    if drop_xl_block is not None:
        xl = xl.clone()
        xl[:, 32 * drop_xl_block:32 * drop_xl_block + 32] = 0
    return reference(name, xh, gh, shifted) + reference(name, xh, gl, shifted) + reference(name, xl, gh, shifted)


def scale_exponents(absmax):
    """s[co] of the one-pass kernels from the exact per-channel max |g| (fp32): max 2^s in [2^13, 2^14), 0 for an all-zero channel,
    clamped to +-100 -- from the exponent field, as the kernels take it."""
    bits = absmax.float().contiguous().view(torch.int32).long()
    ex = 13 - (((bits >> 23) & 0xff) - 127)
    return torch.where(bits == 0, torch.zeros_like(ex), ex.clamp(-100, 100))


def channel_absmax(g):
    """exact per-channel max |g| of [n, cout, ho, wo] stored bf16-pair values, as fp32"""
    return g.abs().amax((0, 2, 3)).float()


def scaled_f16_operand(g, s):
    """g 2^s[co] rounded to fp16 (fp64 values; inf where fp16 overflows)"""
    return (g.double() * torch.pow(2.0, s.double()).view(1, -1, 1, 1)).float().half().double()


def emulate_one_pass(name, x, g, s=None):
    """The one-pass kernels' arithmetic in fp64: x as its fp16 plane, g times 2^s[co] rounded to fp16, the scale divided out."""
    s = scale_exponents(channel_absmax(g)) if s is None else s
    return reference(name, _f16(x), scaled_f16_operand(g, s)) * torch.pow(2.0, -s.double()).view(1, 1, -1)


def raster_mask(name, n, lo, hi, dev="cpu"):
    """[n, 1, ho, wo] of 0 / 1: the interior pixels whose position in the kernels' K raster (the halo-padded gradient plane,
    (img, y in [0, ho + 2), x in [0, wo + 2)) linear) lies OUTSIDE [lo, hi) -- multiply g by it to drop those K positions."""
    cin, cout, k, stride, h, w, _ = CASES[name][0]
    ho, wo = out_hw(h, w, k, stride, is_stem(name))
    pos = torch.arange(n * (ho + 2) * (wo + 2), device=dev).view(n, ho + 2, wo + 2)[:, 1:-1, 1:-1]
    return (~((pos >= lo) & (pos < hi))).double().unsqueeze(1)


# ---------------------------------------------------------------------------------------------------- BatchNorm backward
def grid_for(items):
    """blocks of the element-wise passes of csrc/train.hip (256 threads each)"""
    return min(max((items + 1023) // 1024, 1), 8192)


def fixed_g(n, h, w, c):
    """bn_bwd_apply_kernel / affine_kernel keep a thread's channel group over the grid-stride loop (their fast paths) when the
    groups divide the grid stride"""
    return (grid_for(n * h * w * (c // 8)) * 256) % (c // 8) == 0


def batch_stats(z, eps=1e-5):
    """exact batch statistics of [n, c, h, w] stored values, rounded to fp32: (mean, rstd)"""
    z = z.double()
    mean = z.mean((0, 2, 3))
    var = ((z - mean.view(1, -1, 1, 1)) ** 2).mean((0, 2, 3))
    return mean.float(), (1.0 / (var + eps).sqrt()).float()


def _cv(v):
    return v.double().view(1, -1, 1, 1)


def bn_bwd64(z, gy, ymask, mean, rstd, gamma, count, frozen=False, sums=None):
    """BatchNorm (+ ReLU) backward in closed form, fp64: g = gy [y > 0] (ymask None: no ReLU),
         gz = gamma rstd (g - sum(g) / N - zhat sum(g zhat) / N),  zhat = (z - mean) rstd,  N = count
    without the two mean terms when frozen.  sums: (sum g, sum g zhat) [c] of a LARGER batch than z (synchronised BatchNorm).
    -> (gz, gres = g, ggamma = sum g zhat, gbeta = sum g, absmax = max |gz| per channel); the sums are those of THIS map."""
    z, g = z.double(), gy.double()
    if ymask is not None:
        g = g * ymask.to(g.dtype)
    zhat = (z - _cv(mean)) * _cv(rstd)
    sg, sgz = g.sum((0, 2, 3)), (g * zhat).sum((0, 2, 3))
    coef = _cv(gamma) * _cv(rstd) if gamma is not None else _cv(rstd)
    if frozen:
        gz = coef * g
    else:
        tg, tgz = (sg, sgz) if sums is None else sums
        gz = coef * (g - _cv(tg) / count - zhat * _cv(tgz) / count)
    return gz, g, sgz, sg, gz.abs().amax((0, 2, 3))


def bn_bwd_f32(z, gy, ymask, mean, rstd, gamma, count, frozen=False, paired=True):
    """The same closed form evaluated in float32 with torch's ops (sums taken from fp64, rounded) and rounded to the output's
    storage format: the yardstick of the gz bar -> gz as fp64 values."""
    _, _, sgz, sg, _ = bn_bwd64(z, gy, ymask, mean, rstd, gamma, count, frozen)
    cv = lambda v: v.float().view(1, -1, 1, 1)
    g = gy.float() * (ymask.float() if ymask is not None else 1.0)
    coef = cv(gamma) * cv(rstd) if gamma is not None else cv(rstd)
    if frozen:
        gz = coef * g
    else:
        zhat = (z.float() - cv(mean)) * cv(rstd)
        gz = coef * (g - cv(sg) / float(count) - zhat * cv(sgz) / float(count))
    return (_bf16_pair if paired else _f16)(gz)


def per_channel_rel(got, ref):
    """rel-L2 of every channel of [n, c, h, w] maps -> (the worst, its channel, the [c] vector)"""
    got, ref = got.double(), ref.double()
    num, den = ((got - ref) ** 2).sum((0, 2, 3)), (ref ** 2).sum((0, 2, 3))
    rel = torch.nan_to_num(torch.where(den > 0, num / den.clamp_min(1e-300), num).sqrt(), nan=float("inf"))
    return float(rel.max()), int(rel.argmax()), rel


def gz_bar(z, gy, ymask, mean, rstd, gamma, count, frozen=False):
    """(bar, floor): floor = the worst per-channel error of bn_bwd_f32 against bn_bwd64; the kernel gets four times that (another
    association of the fp32 operations, fma contraction), never more than BN_BAR_MAX."""
    ref = bn_bwd64(z, gy, ymask, mean, rstd, gamma, count, frozen)[0]
    floor, _, _ = per_channel_rel(bn_bwd_f32(z, gy, ymask, mean, rstd, gamma, count, frozen), ref)
    return min(4 * floor, BN_BAR_MAX), floor


def draw_bn(n, c, h, w, seed, z_f16=False, gy_f16=False, relu=True, dev="cpu"):
    """A BatchNorm-backward problem in its storage formats (fp64 values): z (bf16 pair, or one fp16 plane), gy, the post-ReLU
    output y whose sign is the mask (a plane of its own: no pre-activation near the kink decides anything), gamma, beta."""
    gen = torch.Generator(device=dev).manual_seed(100003 * seed + 17 * c + 131 * h + w + n)
    rz, rg = (_f16 if z_f16 else _bf16_pair), (_f16 if gy_f16 else _bf16_pair)
    chan = 0.5 + torch.rand(c, generator=gen, device=dev) * 2
    z = rz(torch.randn((n, c, h, w), generator=gen, device=dev) * chan.view(1, -1, 1, 1) +
           torch.randn(c, generator=gen, device=dev).view(1, -1, 1, 1))
    gy = rg(torch.randn((n, c, h, w), generator=gen, device=dev) * (0.25 + 4 * torch.rand(c, generator=gen, device=dev)).view(1, -1, 1, 1))
    y = _bf16_pair(torch.randn((n, c, h, w), generator=gen, device=dev).relu_()) if relu else None
    gamma = (0.5 + torch.rand(c, generator=gen, device=dev)) * torch.where(torch.rand(c, generator=gen, device=dev) < 0.25, -1.0, 1.0)
    beta = 0.3 * torch.randn(c, generator=gen, device=dev)
    return z, gy, y, gamma.float(), beta.float()


# ------------------------------------------------------------------------------------------ affine + ReLU + max-pool 3x3/2
def stem_act32(z, scale, shift):
    """fmaxf(fmaf(z, sc, sh), 0) as float32: the product and sum exact in fp64 (z holds at most 17 significant bits), rounded
    ONCE -- a correctly rounded fma short of a double-rounding tie."""
    return (z.double() * _cv(scale) + _cv(shift)).float().clamp_min(0.0)


def _windows(a, fill):
    """[n, c, h, w] -> [n, c, ho, wo, 9]: the 3x3 / stride-2 / pad-1 windows, out-of-map taps = fill"""
    n, c, h, w = a.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    ap = F.pad(a, (1, 2, 1, 2), value=fill)
    return torch.stack([ap[:, :, ky:ky + 2 * ho - 1:2, kx:kx + 2 * wo - 1:2] for ky in range(3) for kx in range(3)], -1)


def pool_decision_ties(z, scale, shift, rel=1e-6):
    """bool [n, c, h, w]: True where an element takes part in a decision that another rounding could flip -- its activation within
    `rel` relative of zero, or within `rel` of another positive tap of one of its windows.  The tests draw inputs with none."""
    pre = z.double() * _cv(scale) + _cv(shift)
    near0 = pre.abs() <= rel * (z.double() * _cv(scale)).abs().clamp_min(_cv(shift).abs())
    a = pre.clamp_min(0.0)
    n, c, h, w = a.shape
    ids = torch.arange(n * c * h * w, device=a.device, dtype=torch.float64).view(n, c, h, w)
    wa, wi = _windows(a, -1.0), _windows(ids, -1.0).long()
    bad = near0.clone().view(-1)
    for i in range(9):
        for j in range(i + 1, 9):
            ai, aj = wa[..., i], wa[..., j]
            close = (ai > 0) & (aj > 0) & ((ai - aj).abs() <= rel * torch.maximum(ai, aj))
            bad[wi[..., i][close]] = True
            bad[wi[..., j][close]] = True
    return bad.view(n, c, h, w)


def affine_maxpool64(z, scale, shift):
    """MaxPool2d(3, 2, 1)(relu(z scale + shift)) with the kernel's rule: the activation in fp32 (stem_act32), the window walked in
    (ky, kx) order with strict `>`, start value 0 at position 4, out-of-map taps skipped.
    -> (pooled [n, c, ho, wo] fp32 values as fp64, position uint8 in 0..8, the activations [n, c, h, w] fp32)"""
    act = stem_act32(z, scale, shift)
    win = _windows(act, -1.0)
    best = torch.zeros(win.shape[:-1], dtype=torch.float32, device=z.device)
    pos = torch.full(win.shape[:-1], 4, dtype=torch.uint8, device=z.device)
    for t in range(9):
        better = win[..., t] > best
        best = torch.where(better, win[..., t], best)
        pos = torch.where(better, torch.full_like(pos, t), pos)
    return best.double(), pos, act


def maxpool_route64(gp, pos, h, w):
    """The pooled gradient [n, c, ho, wo] routed to the recorded positions -> [n, c, h, w] fp64.  (A window of all-zero
    activations records position 4, its centre 2 oy, 2 ox: always inside the map.)"""
    n, c, ho, wo = gp.shape
    oy = torch.arange(ho, device=gp.device).view(1, 1, -1, 1)
    ox = torch.arange(wo, device=gp.device).view(1, 1, 1, -1)
    p = pos.long()
    iy, ix = 2 * oy - 1 + p // 3, 2 * ox - 1 + p % 3
    assert bool((iy >= 0).all() and (iy < h).all() and (ix >= 0).all() and (ix < w).all())
    ni = torch.arange(n, device=gp.device).view(-1, 1, 1, 1).expand_as(p)
    ci = torch.arange(c, device=gp.device).view(1, -1, 1, 1).expand_as(p)
    out = torch.zeros((n, c, h, w), dtype=torch.float64, device=gp.device)
    out.index_put_((ni, ci, iy, ix), gp.double(), accumulate=True)
    return out


def maxpool_bn_bwd64(gp, pos, act, z, mean, rstd, gamma, frozen=False):
    """Backward of conv -> BatchNorm -> ReLU -> max-pool from the pooled gradient: routed through the positions, masked by the
    activations' sign, then bn_bwd64 over the full-size map -> bn_bwd64's tuple."""
    n, c, h, w = z.shape
    return bn_bwd64(z, maxpool_route64(gp, pos, h, w), act > 0, mean, rstd, gamma, n * h * w, frozen)


def draw_pool(n, c, h, w, seed, z_f16=False, gamma=None, beta=None, dev="cpu"):
    """A stem-pool problem: stored z, its exact batch statistics, gamma / beta (given ones are kept), the forward's scale / shift in
    fp32, and NO element for which pool_decision_ties objects (offenders are redrawn; the statistics are taken afterwards)."""
    gen = torch.Generator(device=dev).manual_seed(7919 * seed + 17 * c + 131 * h + w + n)
    rz = _f16 if z_f16 else _bf16_pair
    z = rz(torch.randn((n, c, h, w), generator=gen, device=dev) * 1.5 + 0.2)
    if gamma is None:
        gamma = (0.5 + torch.rand(c, generator=gen, device=dev)).float()
    if beta is None:
        beta = (0.3 * torch.randn(c, generator=gen, device=dev)).float()
    for _ in range(64):
        mean, rstd = batch_stats(z)
        scale = (gamma.double() * rstd.double()).float()
        shift = (beta.double() - mean.double() * scale.double()).float()
        bad = pool_decision_ties(z, scale, shift)
        if not bool(bad.any()):
            return z, mean, rstd, gamma, beta, scale, shift
        z = torch.where(bad, rz(torch.randn((n, c, h, w), generator=gen, device=dev) * 1.5 + 0.2), z)
    raise AssertionError("no tie-free draw")
