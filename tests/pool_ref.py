"""fp64 closed forms of the global pooling kernels (csrc/pool.hip: agp_pool_fwd, agp_pool_from_conv, agp_pool_f32_fwd,
agp_gem_f32_bwd; csrc/train.hip: agp_pool_bwd): the mean, GeM, GeM's backward with dL/dp, and the map form of the backward.
Plain torch on the CPU, no autograd: tests/test_pool_ref.py pins them to fp64 autograd through oracle/nets.gem and evaluates the
floors and bars tests/test_gpu_pool_kernels.py holds the kernels to.

    mean[n][c] = sum(x) / HW
    y = GeM    = S^(1/p),  S = mean(c_i^p),  c_i = max(x_i, eps)
    dy/dx_i    = y^(1-p) c_i^(p-1) [x_i >= eps] / HW
    dy/dp      = y (-ln(S) / p^2 + mean(c_i^p ln c_i) / (p S))
    map form:    out = base + gmean / HW + ggem dy/dx

Bars (every one per (image, channel) plane, built from the reference alone):
  * the mean and the map form without a GeM term: min(4 x floor, ceiling), floor = the same form in float32 on the CPU (rounded
    to the bf16 pair where the kernel stores one), its worst plane, never below 2^-24; ceilings 1e-5 forward, 1e-4 backward;
  * GeM goes through the device's exp2 / log2: the project's ceilings, 1e-5 forward, 1e-4 gx, 1e-3 of the value of dL/dp.  Where
    every plane is constant after the clamp (one pixel per plane) dL/dp is analytically zero, its two terms cancel: there the
    error is taken relative to the sum the kernel subtracts, sum |ggem y ln(S) / p^2|.
"""
import torch

from conv_sched_util import _bf16_pair, _f16
from dense_train_ref import nhwc_map, planes

GEM_EPS = 1e-6
CEIL_FWD, CEIL_GX, CEIL_GP = 1e-5, 1e-4, 1e-3
MARGIN = 4.0
ONE_ROUNDING = 2.0 ** -24
HALO_POISON = -3.0               # finite, non-zero, and both an fp16 and a bf16 value: a kernel that reads the halo shows it


# ------------------------------------------------------------------------------------------------------------------ forms
def mean(x, dtype=torch.float64, extra_divisor=0):
    """[n, c, h, w] -> [n, c].  extra_divisor=1: the wrong variant that divides by HW + 1."""
    x = x.to(dtype)
    return x.sum((2, 3)) / float(x.shape[2] * x.shape[3] + extra_divisor)


def gem(x, p, eps=GEM_EPS, dtype=torch.float64):
    """[n, c, h, w] -> [n, c]"""
    p = float(p)
    c = x.to(dtype).clamp_min(eps)
    return c.pow(p).mean((2, 3)).pow(1.0 / p)


def _dp_parts(x, p, eps, y, gy, dtype):
    """the two terms of dL/dp per plane: (gy y mean(c^p ln c) / (p S), gy y ln(S) / p^2), S = y^p"""
    p = float(p)
    c = x.to(dtype).clamp_min(eps)
    y, gy = y.to(dtype), gy.to(dtype)
    S = y.pow(p)
    a = gy * y * (c.pow(p) * c.log()).mean((2, 3)) / (p * S)
    b = gy * y * S.log() / (p * p)
    return a, b


def gem_bwd(x, p, eps, y, gy, dtype=torch.float64, mask=True, ln_term=True):
    """-> (gx [n, c, h, w], dL/dp scalar) from the forward output y [n, c] and gy [n, c].  Wrong variants: mask=False forgets
    [x >= eps], ln_term=False forgets -ln(S) / p^2."""
    p = float(p)
    xd = x.to(dtype)
    c = xd.clamp_min(eps)
    coef = gy.to(dtype) * y.to(dtype).pow(1.0 - p) / float(x.shape[2] * x.shape[3])
    gx = coef[:, :, None, None] * c.pow(p - 1.0)
    if mask:
        gx = gx * (xd >= eps).to(dtype)
    a, b = _dp_parts(x, p, eps, y, gy, dtype)
    return gx, (a.sum() - b.sum()) if ln_term else a.sum()


def dp_magnitudes(x, p, eps, y, gy):
    """(sum |a| + sum |b|, sum |b|): what an error of dL/dp is relative to where its terms cancel; b is what the kernels subtract"""
    a, b = _dp_parts(x, p, eps, y, gy, torch.float64)
    return float(a.abs().sum() + b.abs().sum()), float(b.abs().sum())


def dp_error(got, ref, x, sub_mag, eps=GEM_EPS):
    """The relative error of dL/dp the CEIL_GP bar applies to: of the value itself -- or, where every plane is constant after
    the clamp (one pixel per plane; a plane that is all clamp), so that GeM is that constant whatever p is and dL/dp
    analytically zero, of the sum the kernel subtracts."""
    c = x.double().clamp_min(eps)
    flat = bool((c.amax((2, 3)) == c.amin((2, 3))).all())
    return abs(float(got) - ref) / max(sub_mag if flat else abs(ref), 1e-300)


def pool_bwd_map(x, base=None, gmean=None, ggem=None, gem_y=None, p=None, eps=GEM_EPS, dtype=torch.float64):
    """The map form: base + gmean / HW + ggem dGeM/dx -> (out [n, c, h, w], dL/dp or None)"""
    n, c, h, w = x.shape
    out = torch.zeros((n, c, h, w), dtype=dtype)
    if base is not None:
        out = out + base.to(dtype)
    if gmean is not None:
        out = out + (gmean.to(dtype) / float(h * w))[:, :, None, None]
    dp = None
    if ggem is not None:
        gx, dp = gem_bwd(x, p, eps, gem_y, ggem, dtype)
        out = out + gx
    return out, dp


def from_partials(partial, hw, p=None, dtype=torch.float64):
    """agp_pool_from_conv: partial [n][blocks][2][c] (sum x, sum max(x, eps)^p per 64-row block) -> (mean, gem) [n, c]"""
    s = partial.to(dtype).sum(1)
    m = s[:, 0] / float(hw)
    return m, None if p is None else (s[:, 1] / float(hw)).pow(1.0 / float(p))


# ------------------------------------------------------------------------------------------------------------------- bars
def per_plane_rel(got, ref):
    """[n, c, h, w] -> [n, c] rel_l2 of every plane ([n, c] inputs: the relative error of every value); a plane whose reference
    is all zero must be zero: inf otherwise"""
    g, r = got.double(), ref.double()
    if g.dim() == 2:
        g, r = g[:, :, None, None], r[:, :, None, None]
    num, den = ((g - r) ** 2).sum((2, 3)).sqrt(), (r ** 2).sum((2, 3)).sqrt()
    return torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num > 0, torch.full_like(num, float("inf")), torch.zeros_like(num)))


def worst_plane(got, ref):
    return float(per_plane_rel(got, ref).max())


def bar_of(floor, ceiling):
    return min(MARGIN * max(float(floor), ONE_ROUNDING), ceiling)


def mean_bar(x):
    """(bar, floor) of the mean of these stored values"""
    floor = worst_plane(mean(x, torch.float32), mean(x))
    return bar_of(floor, CEIL_FWD), floor


def linear_map_bar(x, base, gmean):
    """(bar, floor) of the map form WITHOUT a GeM term: float32, rounded to the bf16 pair the kernel stores"""
    ref, _ = pool_bwd_map(x, base, gmean)
    f32, _ = pool_bwd_map(x, base, gmean, dtype=torch.float32)
    floor = worst_plane(_bf16_pair(f32), ref)
    return bar_of(floor, CEIL_GX), floor


# ---------------------------------------------------------------------------------------------------------------- layouts
def draw_map(n, c, h, w, seed, fmt="pair", scale=0.5, shift=1.0):
    """[n, c, h, w] stored values (fp64) of a map in its storage format ("pair": split bf16, "f16": one fp16 plane, "f32"): mostly
    positive, about one in forty below eps -- the clamp and the mask of GeM meet both sides, the mean stays well conditioned --
    the first pixel of channel 1 of every image is -0.25 and that plane of image 0 is negative throughout: all clamp, GeM = eps
    and gx = 0 exactly.  (A clamped pixel beside live ones carries eps^(p-1) of their gradient: only an all-clamp plane shows
    whether the [x >= eps] mask is there.)"""
    g = torch.Generator().manual_seed(1000003 * seed + 8191 * c + 131 * h + 17 * w + n)
    v = torch.randn((n, c, h, w), generator=g) * scale + shift
    ch = min(1, c - 1)
    v[:, ch, 0, 0] = -0.25
    v[0, ch] = -v[0, ch].abs() - 0.25
    return {"pair": _bf16_pair, "f16": _f16, "f32": lambda t: t.float().double()}[fmt](v)


def draw_vec(n, c, seed, positive=False):
    """[n, c] fp32 values (a gradient of a pooled vector).  positive: the gradient of the GeM vector in the cases that check
    dL/dp -- a power mean grows with p, so every plane then adds to dL/dp with the same sign and the sum over the planes does not
    cancel (with mixed signs |dL/dp| falls to 1e-5 of its terms and a relative error of it measures nothing)."""
    g = torch.Generator().manual_seed(7919 * seed + 31 * c + n)
    v = torch.randn((n, c), generator=g).float()
    return v.abs() + 0.1 if positive else v


def poison_halo(plane, pad, value=HALO_POISON):
    """fill the halo of an NHWC plane [n, h + 2 pad, w + 2 pad, c] in place"""
    if pad:
        plane[:, :pad] = value
        plane[:, -pad:] = value
        plane[:, :, :pad] = value
        plane[:, :, -pad:] = value
    return plane


def map_planes(v, pad, paired, halo=HALO_POISON):
    """[n, c, h, w] stored values -> the (hi, lo) planes of the halo-`pad` NHWC map (lo None for one fp16 plane) with garbage in
    the halo of every plane: a result that matches proves that only the interior is read"""
    hi, lo = planes(nhwc_map(v, pad), paired)
    poison_halo(hi, pad, halo)
    if lo is not None:
        poison_halo(lo, pad, halo)
    return hi, lo


def interior(plane_hi, plane_lo, pad):
    """the interior of NHWC planes as [n, c, h, w] fp64 values (hi + lo)"""
    v = plane_hi.double() if plane_lo is None else plane_hi.double() + plane_lo.double()
    if pad:
        v = v[:, pad:-pad, pad:-pad]
    return v.permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------- the cases of the GPU tests
# Shared by tests/test_pool_ref.py (floors, bars, discrimination: on the CPU) and tests/test_gpu_pool_kernels.py.
POOL_C = (8, 24, 96, 384, 2048)      # c / 8 = 1, 3, 12, 48, 256 channel groups: 3, 12 and 48 do not divide the 256 threads (idle tail
                                     # threads: 255, 252 and 240 of them work), 256 groups leave one pixel lane
POOL_NHW = ((1, 1, 1), (2, 3, 3), (3, 9, 11), (2, 5, 13))      # a plane smaller than one trip; 9, 99 and 65 pixels: ragged trips and splits
# (format, pad, p, mean wanted, GeM wanted); p None: agp_pool_fwd's p == NULL
POOL_FWD_VARIANTS = (("pair", 1, 3.0, True, True), ("pair", 3, 2.5, True, True), ("pair", 3, 3.0, False, True),
                     ("pair", 1, None, True, False), ("f16", 3, 3.0, True, True), ("f16", 1, 2.5, True, True),
                     ("f16", 3, None, True, False), ("f16", 1, 2.5, False, True))
POOL_LARGE = (1, 370, 370, 8)        # 136900 pixels: the split count is at its cap and the last splits get no pixel
# (n, h, w, c) -> (splits, empty splits).  The second stage adds one trip of up to POOL_F32_SPLITS = 8 partials in fp32 and
# more in fp64: 8 and 9 splits at the widest map (2048 planes: the worst plane of many), 256 splits at c = 384 and 2048 (an fp32
# chain of that length loses the bar on a few of so many planes), 258 at c = 8, and the capped 2048 with empty splits
POOL_MANY_SPLITS = {(1, 16, 32, 2048): (8, 0), (4, 16, 32, 2048): (8, 0), (1, 16, 33, 2048): (9, 0), (1, 128, 128, 384): (256, 0),
                    (1, 128, 128, 2048): (256, 0), (1, 127, 130, 8): (258, 0), POOL_LARGE: (2048, 4)}
POOL_F32_SPLITS = 8                  # csrc/pool.hip
POOL_BWD_C = (8, 24, 96, 2048)
POOL_BWD_TERMS = tuple((b, m, g) for b in (False, True) for m in (False, True) for g in (False, True) if b or m or g)
F32_NC = ((3, 7), (1, 1), (2, 96))   # n * c = 21 and 1: no multiple of 4, the last block has clamped dead waves
F32_HW = ((1, 1), (3, 5), (9, 11))
F32_ATOMIC = (33, 2048, 1, 2)        # 67584 waves = 16896 blocks, above AGP_GP_SLOTS = 16384: the atomic form of the dL/dp sum
FROM_CONV_HW = ((1, 1), (8, 62), (9, 62), (32, 62), (33, 62), (70, 62))      # (h (w + 2) + 63) / 64 = 1, 8, 9, 32, 33, 70 blocks per image
FROM_CONV_C = (24, 64, 96)
GP_SLOTS = 16384


def from_conv_blocks(h, w):
    """64-row blocks per image of the 3x3 kernels' padded-width raster"""
    return (h * (w + 2) + 63) // 64


def split_pixels(n, c, h, w, splits):
    """(pixels per split, splits that get no pixel) of agp_pool_fwd's first stage"""
    per = (h * w + splits - 1) // splits
    return per, sum(1 for s in range(splits) if s * per >= h * w)


def draw_partials(n, blocks, c, seed, p):
    """fp32 partial sums [n][blocks][2][c] as the conv epilogue leaves them: per block the sum of 64 rows' x and max(x, eps)^p"""
    g = torch.Generator().manual_seed(104729 * seed + 613 * c + blocks + n)
    x = torch.randn((n, blocks, 64, c), generator=g) * 0.5 + 1.0
    return torch.stack([x.sum(2), x.clamp_min(GEM_EPS).pow(float(p)).sum(2)], 2).float().contiguous()
