"""CPU references of the map pack, split, halo and layout kernels (csrc/pack.hip: agp_split_f32, agp_split_conv_weight[_both],
agp_pack_f32_to_nhwc[4_h16], agp_pack_u8_cams_to_nhwc, agp_unpack_nhwc_to_f32, agp_map_zero_halo, agp_maxpool3x3s2_fwd,
agp_bcast_add_fwd; csrc/train.hip: agp_map_add, agp_upsample2_zero, agp_map_chan_sum, agp_bn_frozen_coeffs).  Plain torch on the
CPU.  These kernels round and move: apart from the channel sum every one of them is exact, so the references return BIT PATTERNS
(int16 views of the bf16 / fp16 planes, -0 distinct from +0) and tests/test_gpu_map_kernels.py compares bits.
tests/test_map_ref.py pins the roundings to an integer round-to-nearest-even on the raw fp32 bits, the layouts to torch.flip /
permute, the pooling to max_pool2d and dense_train_ref.affine_maxpool64, and shows that every comparison rejects a wrong variant.

    split          hi = rn(x), lo = rn(x - float(hi)) in bf16; in fp16 after the clamp to +-65504 of common.hpp's f2h
    store_map      common.hpp map_store8: the bf16 split of a pair, or the saturating fp16 of one plane (lo absent)
    load_map       common.hpp map_load8: float(hi) + float(lo) in fp32, or float(hi)

The case tables of the GPU file are at the end, so that the CPU file walks the same cases."""
import torch
import torch.nn.functional as F

from conv_sched_util import _bf16_pair, _f16
from dense_train_ref import nhwc_map, planes

F16_MAX = 65504.0
BF16, F16 = "bf16", "f16"            # AGP_FMT_BF16 = 0, AGP_FMT_F16 = 1
FMT_CODE = {BF16: 0, F16: 1}


# ------------------------------------------------------------------------------------------------------------- roundings
def _bits(t):
    return t.contiguous().view(torch.int16)


def f2h(x):
    """common.hpp f2h: the saturating fp16 of fp32 values, as an fp16 tensor"""
    return x.float().clamp(-F16_MAX, F16_MAX).half()


def split(x, fmt, truncate=False):
    """fp32 -> the (hi, lo) bit patterns (int16).  truncate: the wrong variant that chops the mantissa instead of rounding."""
    x = x.float()
    if truncate:
        assert fmt == BF16
        chop = lambda v: ((v.contiguous().view(torch.int32) >> 16) << 16).view(torch.float32).bfloat16()
        hi = chop(x)
        return _bits(hi), _bits(chop(x - hi.float()))
    if fmt == BF16:
        hi = x.bfloat16()
        return _bits(hi), _bits((x - hi.float()).bfloat16())
    assert fmt == F16
    hi = f2h(x)
    return _bits(hi), _bits(f2h(x - hi.float()))


def store_map(v, paired):
    """map_store8 -> (hi bits, lo bits or None)"""
    if paired:
        return split(v, BF16)
    return _bits(f2h(v)), None


def load_map(hi, lo):
    """map_load8 of bf16 / fp16 planes (tensors of that dtype) -> fp32"""
    return hi.float() if lo is None else hi.float() + lo.float()


def stored(x, paired):
    """fp32 values -> the values a map of that format holds of them (fp64), what dense_train_ref.planes takes"""
    return _bf16_pair(x) if paired else _f16(x.float().clamp(-F16_MAX, F16_MAX))


# ---------------------------------------------------------------------------------------------------------------- weights
def conv_weight_values(w, dgrad, flip=True):
    """w [cout][cin][kh][kw] -> [nn][kh][kw][cc] by the index formulas of pack.hip: dgrad 0 out[n][ky][kx][c] = w[n][c][ky][kx];
    dgrad 1 out[n][ky][kx][c] = w[c][n][kh-1-ky][kw-1-kx].  flip=False: the wrong variant, a transpose without the flip."""
    cout, cin, kh, kw = w.shape
    nn, cc = (cin, cout) if dgrad else (cout, cin)
    n, ky, kx, c = torch.meshgrid(torch.arange(nn), torch.arange(kh), torch.arange(kw), torch.arange(cc), indexing="ij")
    if not dgrad:
        return w[n, c, ky, kx]
    return w[c, n, kh - 1 - ky, kw - 1 - kx] if flip else w[c, n, ky, kx]


def chunk_major_order(v, swapped=False):
    """[nn][taps...][cc] -> [K/32][nn][32] flat, K = tap * cc + channel.  swapped: the wrong variant [nn][K/32][32]."""
    nn = v.shape[0]
    k = v.reshape(nn, -1)
    assert k.shape[1] % 32 == 0
    k = k.view(nn, -1, 32)
    return (k if swapped else k.permute(1, 0, 2)).reshape(-1)


def conv_weight_planes(w, dgrad, chunk_major):
    """-> the flat (hi, lo) bit patterns of agp_split_conv_weight's planes"""
    v = conv_weight_values(w, dgrad)
    v = chunk_major_order(v) if chunk_major else v.reshape(-1)
    return split(v, BF16)


def distinct_weights(cout, cin, kh, kw, seed=0):
    """weights in which every (n, c, ky, kx) holds its own value, hi plane included: an index code on a 2^-7 grid (exact in
    bf16 up to 256) times 2^k, plus a small random part that fills the lo plane"""
    g = torch.Generator().manual_seed(977 * seed + 31 * cout + 7 * cin + kh)
    numel = cout * cin * kh * kw
    code = torch.arange(numel, dtype=torch.float64)
    base = (1.0 + (code % 128) / 128.0) * torch.pow(2.0, (code // 128) - 40.0)        # bf16 values, all distinct
    w = base * (1.0 + (torch.rand(numel, generator=g, dtype=torch.float64) - 0.5) * 2.0 ** -10)
    sign = torch.where(torch.rand(numel, generator=g) < 0.5, -1.0, 1.0).double()
    return (w * sign).float().view(cout, cin, kh, kw)


# ------------------------------------------------------------------------------------------------------------------- maps
def pack_nhwc(x, c, cpad, pad, paired):
    """x [n, c, h, w] fp32 -> the interior [n, h, w, cpad] (hi, lo) bit patterns; channels c .. cpad - 1 are +0.  (The kernel
    leaves the halo as it was: the test keeps what was there.)"""
    assert x.shape[1] == c
    return store_map(nhwc_map(x.float(), 0, cpad), paired)


def u8_cams(img, mean, std, pad, paired):
    """uint8 [n][ncam][h][w][3] -> the interior [n, h, ncam w, 4] bit patterns: (u8 / 255 - m) / s in fp32, in that order, tiles
    side by side, the 4th channel zero -> (hi, lo, the fp32 values before the split)"""
    n, ncam, h, w, _ = img.shape
    m = torch.tensor(mean, dtype=torch.float32)
    s = torch.tensor(std, dtype=torch.float32)
    v = (img.float() / torch.tensor(255.0) - m) / s
    v = v.permute(0, 2, 1, 3, 4).reshape(n, h, ncam * w, 3)
    v = torch.cat([v, torch.zeros((n, h, ncam * w, 1))], -1)
    hi, lo = store_map(v, paired)
    return hi, lo, v


def halo_mask(n, h, w, c, pad, short=False):
    """bool [n, h + 2 pad, w + 2 pad, c]: True on the halo.  short: the wrong variant that misses the last column."""
    m = torch.ones((n, h + 2 * pad, w + 2 * pad, c), dtype=torch.bool)
    m[:, pad:pad + h, pad:pad + w] = False
    if short and pad:
        m[:, :, -1] = False
    return m


def put_interior(whole, inner, pad):
    """a copy of the plane [n, h + 2 pad, w + 2 pad, c] with its interior replaced"""
    out = whole.clone()
    n, h, w, c = inner.shape
    out[:, pad:pad + h, pad:pad + w] = inner
    return out


def pool_out(h, w):
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


def maxpool_first_positive(v, last=False):
    """MaxPool2d(3, 2, 1) of non-negative [n, c, h, w] values by the rule stated in pack.hip -> (values, position uint8): the
    position 3 ky + kx of the FIRST strictly positive maximum in row-major window order, 4 where the window holds no positive
    value.  last: the wrong variant that keeps the last maximum."""
    n, c, h, w = v.shape
    ho, wo = pool_out(h, w)
    vp = F.pad(v.double(), (1, 2, 1, 2))                               # zeros: never a positive maximum
    win = vp.unfold(2, 3, 2).unfold(3, 3, 2)[:, :, :ho, :wo].reshape(n, c, ho, wo, 9)
    m = win.amax(-1)
    hit = (win == m.unsqueeze(-1)) & (win > 0)
    order = torch.arange(9).view(1, 1, 1, 1, 9)
    if last:
        idx = torch.where(hit, order, torch.full_like(order, -1)).amax(-1)
        pos = torch.where(idx < 0, torch.full_like(idx, 4), idx)
    else:
        idx = torch.where(hit, order, torch.full_like(order, 9)).amin(-1)
        pos = torch.where(idx > 8, torch.full_like(idx, 4), idx)
    return torch.where(m > 0, m, torch.zeros_like(m)), pos.to(torch.uint8)


def bcast_add(a, vec):
    """fp32: a [n, c, h, w] + vec [n, c]"""
    return a.float() + vec.float()[:, :, None, None]


def map_add(a, b=None, mask=None, mask_ge=False):
    """fp32, in the kernel's order: a where mask > 0 (else +0), then + b.  mask_ge: the wrong variant with mask >= 0."""
    a = a.float()
    if mask is not None:
        keep = (mask.float() >= 0) if mask_ge else (mask.float() > 0)
        a = torch.where(keep, a, torch.zeros_like(a))
    if b is not None:
        a = a + b.float()
    return a


def upsample2_zero(g, hu, wu):
    """g [n, c, ho, wo] fp32 -> u [n, c, hu, wu]: u[2 oy][2 ox] = g[oy][ox], +0 elsewhere"""
    n, c, ho, wo = g.shape
    u = torch.zeros((n, c, hu, wu), dtype=torch.float32)
    sub = u[:, :, ::2, ::2]
    hh, ww = min(ho, sub.shape[2]), min(wo, sub.shape[3])
    sub[:, :, :hh, :ww] = g.float()[:, :, :hh, :ww]
    return u


def chan_sum64(v):
    """[n, c, h, w] stored values -> (sum [c], sum |terms| [c]) in fp64"""
    v = v.double()
    return v.sum((0, 2, 3)), v.abs().sum((0, 2, 3))


def frozen_coeffs64(running_mean, running_var, gamma, beta, eps):
    """agp_bn_frozen_coeffs in fp64 from the fp32 inputs (eps as the fp32 the entry takes), rounded once to fp32:
    mean, rstd = 1 / sqrt(var + eps), scale = gamma rstd, shift = beta - mean scale"""
    m, v = running_mean.double(), running_var.double()
    e = torch.tensor(eps, dtype=torch.float32).double()
    rs = 1.0 / torch.sqrt(v + e)
    sc = rs if gamma is None else gamma.double() * rs
    sh = (0.0 if beta is None else beta.double()) - m * sc
    return m.float(), rs.float(), sc.float(), sh.float()


def ulp_distance(a, b):
    """fp32 tensors -> int64: how many representable values apart (finite values of one sign, or across zero)"""
    def key(t):
        i = t.contiguous().view(torch.int32).long()
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return (key(a) - key(b)).abs()


# ----------------------------------------------------------------------------------------------------------------- inputs
def specials(fmt):
    """what every case plants: exact zeros, -0, rounding ties and their neighbours; for fp16 planes values beyond +-65504 and
    below 2^-14.  The last seven are the ones a 7-element scalar tail must see."""
    t8, t11 = 2.0 ** -8, 2.0 ** -11
    s = [0.0, 1.0, -1.0, 3.0e-5, -2.5e3,
         1 + t8, 1 + 3 * t8, -(1 + t8), 1 + t8 + 2.0 ** -23, 1 + t8 - 2.0 ** -23,          # bf16 hi ties (to even: down, up) and neighbours
         1 + 2.0 ** -7 + 2.0 ** -16, 1 + 2.0 ** -7 + 3 * 2.0 ** -16,                        # ties of the lo plane
         3.3895313892515355e38]                                                           # the largest finite bf16
    if fmt == F16:
        s += [1 + t11, 1 + 3 * t11, 1 + t11 + 2.0 ** -23, 1 + t11 - 2.0 ** -23, 2049.0, 2051.0,      # fp16 ties
              2.0 ** -14, 2.0 ** -15, 3 * 2.0 ** -24, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -20),   # subnormals
              2.0 ** -26, -(2.0 ** -24), 65504.0, -65504.0, 65519.0, 7.0e4, -7.0e4]
        tail = [65520.0, 1.0e6, -1.0e6, -0.0, 1 + t11, 2.0 ** -25, 65519.996]
    else:
        tail = [65520.0, 1.0e6, -1.0e6, -0.0, 1 + t8, 2.0 ** -25, 3.0e38]
    return torch.tensor(s + tail, dtype=torch.float64).float()


def draw_values(shape, seed, fmt, scatter=True):
    """fp32 values spread over the magnitudes 2^-60 .. 6e4 (log-uniform, random sign) with specials(fmt) planted: scattered
    through the tensor, or (scatter=False, flat tensors) at the start and once more at the very end."""
    g = torch.Generator().manual_seed(1000003 * seed + sum((i + 1) * int(s) for i, s in enumerate(shape)))
    numel = 1
    for s in shape:
        numel *= int(s)
    e = torch.rand(numel, generator=g, dtype=torch.float64) * (15.87 + 60.0) - 60.0
    x = torch.pow(2.0, e) * torch.where(torch.rand(numel, generator=g) < 0.5, -1.0, 1.0).double()
    x = x.float()
    sp = specials(fmt)
    if scatter:
        pos = (torch.arange(len(sp)) * 7919 + 3) % numel
        x[pos] = sp                                  # (a tensor smaller than the list keeps the last writes)
    else:
        k = min(len(sp), numel)
        x[:k] = sp[:k]
        x[numel - k:] = sp[len(sp) - k:]
    return x.view(*shape)


def draw_relu_map(n, c, h, w, seed, paired):
    """A post-ReLU map as stored values (fp64): about 40 % exact zeros, the rest in (0, 4]; in image 0 the first window is all
    zero in every channel, and where the map has a window (1, 1) its taps (a, b) of channel ch are one planted maximum 50: ties."""
    g = torch.Generator().manual_seed(7919 * seed + 131 * h + 17 * w + c + n)
    v = torch.rand((n, c, h, w), generator=g) * 4.0 + 2.0 ** -8
    v = torch.where(torch.rand((n, c, h, w), generator=g) < 0.4, torch.zeros(()), v)
    v[0, :, :2, :2] = 0.0
    if h >= 4 and w >= 4:
        pairs = ((0, 8), (2, 6), (1, 3), (4, 5), (7, 8), (3, 5), (0, 1))
        for ch in range(c):
            for t in pairs[ch % len(pairs)]:
                v[:, ch, 1 + t // 3, 1 + t % 3] = 50.0
    return stored(v, paired)


def maxpool_input_planes(v, pin, paired):
    """The planes of a pooling input: the halo ring the windows read is zero (the padding value), the rings outside it hold 7 (a
    window that reached them would return it)"""
    hi, lo = planes(nhwc_map(v, pin), paired)
    if pin > 1:
        for p in (hi,) if lo is None else (hi, lo):
            inner = p[:, pin - 1:p.shape[1] - pin + 1, pin - 1:p.shape[2] - pin + 1].clone()
            p[:] = 7.0
            p[:, pin - 1:p.shape[1] - pin + 1, pin - 1:p.shape[2] - pin + 1] = inner
    return hi, lo


def mask_values(shape, seed):
    """A ReLU mask map (bf16 values, exact in either format's terms where used): positives, exact zeros, -0, negatives, the
    smallest positive bf16 (2^-133, a subnormal) and the smallest normal (2^-126)"""
    g = torch.Generator().manual_seed(31337 * seed + sum(int(s) for s in shape))
    pick = torch.randint(0, 6, shape, generator=g)
    table = torch.tensor([1.5, 0.0, -0.0, -2.0, 2.0 ** -133, 2.0 ** -126], dtype=torch.float64)
    return table[pick]


def mask_values_f16(shape, seed):
    """the same for one fp16 plane: the smallest positive fp16 (2^-24) and the smallest normal (2^-14)"""
    g = torch.Generator().manual_seed(31337 * seed + sum(int(s) for s in shape))
    pick = torch.randint(0, 6, shape, generator=g)
    table = torch.tensor([1.5, 0.0, -0.0, -2.0, 2.0 ** -24, 2.0 ** -14], dtype=torch.float64)
    return table[pick]


# ------------------------------------------------------------------------------------------- the cases of the GPU tests
GRID_CAP = 4096 * 256                # pack.hip grid_for: at most 4096 blocks of 256 threads
SPLIT_N = (1, 7, 8, 9, 2055, 8 * GRID_CAP + 8 * 300 + 5)
WEIGHT_SHAPES = ((8, 8, 1, 1), (16, 40, 3, 3), (64, 32, 3, 3), (32, 96, 1, 1), (24, 8, 7, 7))        # (cout, cin, kh, kw)
PACK_SHAPES = ((2, 8, 3, 5, 8), (1, 13, 4, 3, 16), (3, 64, 2, 2, 64), (1, 1, 1, 1, 8))              # (n, c, h, w, cpad)
PACK_LAYOUTS = ("nchw", "channels_last", "width_strided", "channel_sliced")
PACK_LARGE = (2, 1024, 64, 66, 1024)
PACK4_SHAPES = ((2, 3, 5, 8), (1, 1, 2, 4), (2, 4, 3, 12), (1, 3, 4, 6))       # (n, c, h, w); w % 4 == 0 takes the fast kernel
CAM_SHAPES = ((1, 1, 1, 1), (2, 3, 5, 7), (1, 6, 3, 4))                         # (n, ncam, h, w)
CAM_MEAN, CAM_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
UNPACK_C = (8, 24, 64)
UNPACK_NHW = (2, 3, 5)
HALO_C = (8, 64, 4, 12, 3, 5)
HALO_NHW = ((1, 1, 1), (2, 3, 5), (3, 1, 7), (2, 6, 1))
POOL_SHAPES = ((1, 1, 1, 8), (2, 5, 7, 8), (1, 6, 4, 24), (2, 7, 7, 64))        # (n, h, w, c)
ADD_SHAPES = ((1, 1, 1, 8), (3, 2, 5, 24), (2, 3, 3, 64))                        # (n, h, w, c)
UPSAMPLE = (((1, 1), (1, 1)), ((2, 3), (4, 6)), ((2, 3), (3, 5)), ((4, 4), (7, 8)))
CHAN_SUM_C = (8, 24, 2048)
CHAN_SUM_NHW = ((1, 1, 1), (3, 9, 11), (2, 5, 13))
CHAN_SUM_BAR = 1e-5                  # of sum |terms| per channel: the column-sum bar of tests/test_gpu_head_kernels.py
FROZEN_C = (1, 255, 256, 257)
FROZEN_EPS = 1e-5


def split_threads(cout, cin, kh, kw, dgrad):
    """threads agp_split_conv_weight launches: one per 8 innermost channels; dgrad 2: both planes (the _both entry)"""
    f, d = cout * kh * kw * (cin // 8), cin * kh * kw * (cout // 8)
    return (f, d, f + d)[dgrad]


def chunk_major_modes(cout, cin):
    """the chunk_major values agp_split_conv_weight_both accepts: bit 0 needs cin % 32 == 0, bit 1 cout % 32 == 0"""
    return [cm for cm in range(4) if not ((cm & 1) and cin % 32) and not ((cm & 2) and cout % 32)]


def draw_chan_sum(n, c, h, w, paired):
    """stored values with mean 1 and spread 0.5: sum |terms| ~ |sum|"""
    g = torch.Generator().manual_seed(1000003 * 11 + 8191 * c + 131 * h + 17 * w + n)
    return stored(torch.randn((n, c, h, w), generator=g) * 0.5 + 1.0, paired)


def draw_frozen(c, seed=0):
    """(running_mean, running_var, gamma, beta) fp32; the variances include 0 and 1e-12"""
    g = torch.Generator().manual_seed(4099 * seed + c)
    rm = torch.randn(c, generator=g)
    rv = torch.rand(c, generator=g) * 2.0 + 1e-3
    rv[0] = 0.0
    if c > 2:
        rv[c // 2] = 1e-12
        rv[-1] = 0.0
    gamma = (0.5 + torch.rand(c, generator=g)) * torch.where(torch.rand(c, generator=g) < 0.25, -1.0, 1.0)
    beta = 0.3 * torch.randn(c, generator=g)
    return rm.float(), rv.float(), gamma.float(), beta.float()

