"""Host tests of tests/map_ref.py (no GPU): the split against an integer round-to-nearest-even on the raw fp32 bits (numpy uint32
arithmetic: ties, their neighbours, +-0, the largest finite bf16, 65504 / 65520 / 1e6 and the subnormal range in fp16); the weight
layouts against torch.flip + permute; the pooling rule against dense_train_ref.affine_maxpool64 and max_pool2d; for every
comparison tests/test_gpu_map_kernels.py makes a wrong variant of the same form that the comparison must reject (a transpose
without the flip, a chunk-major order with n and chunk swapped, the last maximum instead of the first, a mask taken as >= 0, a
halo mask one column short, a split that truncates); and the float32 floor of the channel sum at the GPU file's cases.

The channel-sum floor on the CPU (torch's float32 sum of the stored values against fp64, as a fraction of sum |terms| per channel):
at most 1.6e-7 over all cases ([3, 9, 11, 2048], pair), under a quarter (2.5e-6) of the bar 1e-5."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dense_train_ref as R
import map_ref as M


# ---------------------------------------------------------------------------------------- the integer rounding, numpy only
def _u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)


def rne_bf16_bits(x):
    """fp32 -> bf16 bit patterns: add 0x7FFF plus the kept part's last bit, drop 16 bits (finite inputs)"""
    u = _u32(x)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def rne_f16_bits(x):
    """fp32 -> saturating fp16 bit patterns in integers: the magnitude clamped to 65504's pattern, the mantissa (with its hidden
    bit below 2^-14) shifted down and rounded to nearest, ties to even"""
    u = _u32(x)
    sign = ((u >> 31) & 1) << 15
    a = np.minimum(u & 0x7FFFFFFF, np.uint64(0x477FE000))            # 65504.0f
    exp, man = a >> 23, a & 0x7FFFFF
    normal = exp >= 113
    shift = np.where(normal, 13, np.clip(126 - exp.astype(np.int64), 14, 25)).astype(np.uint64)
    m = np.where(normal, man, man | 0x800000)
    kept, rem, half = m >> shift, m & ((np.uint64(1) << shift) - 1), np.uint64(1) << (shift - 1)
    h = np.where(normal, ((exp - 112) << 10) | kept, kept)
    h = h + ((rem > half) | ((rem == half) & ((h & 1) == 1)))
    return (sign | h).astype(np.uint16)


def _bf16_to_f32(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def int_split(x, fmt):
    x = np.ascontiguousarray(x, dtype=np.float32)
    if fmt == M.BF16:
        hi = rne_bf16_bits(x)
        lo = rne_bf16_bits(x - _bf16_to_f32(hi))
    else:
        hi = rne_f16_bits(x)
        lo = rne_f16_bits(x - hi.view(np.float16).astype(np.float32))
    return hi.view(np.int16), lo.view(np.int16)


def _hex(v):
    return int(v) & 0xFFFF


def test_the_integer_rounding_itself_on_known_patterns():
    f = lambda *v: np.array(v, dtype=np.float32)
    assert [_hex(b) for b in rne_bf16_bits(f(1.0, -0.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 3.3895313892515355e38))] == \
        [0x3F80, 0x8000, 0x3F80, 0x3F82, 0x7F7F]
    assert [_hex(b) for b in rne_f16_bits(f(1.0, -0.0, 65504, 65520, 1e6, -1e6, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25,
                                            1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2.0 ** -60))] == \
        [0x3C00, 0x8000, 0x7BFF, 0x7BFF, 0x7BFF, 0xFBFF, 0x0400, 0x0001, 0x0000, 0x0002, 0x3C00, 0x3C02, 0x0000]


@pytest.mark.parametrize("fmt", [M.BF16, M.F16])
def test_split_matches_the_integer_round_to_nearest_even(fmt):
    edge = [0.0, -0.0, 3.3895313892515355e38, -3.3895313892515355e38, 65504.0, 65520.0, 1e6, -65520.0, -1e6,
            65519.996, 65504.004, 2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -11), 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -23), 2.0 ** -26]
    ties = []
    for e in (-20, -1, 0, 3, 14):
        for frac, ulp in ((2.0 ** -8, 2.0 ** -23), (3 * 2.0 ** -8, 2.0 ** -23), (2.0 ** -11, 2.0 ** -23), (3 * 2.0 ** -11, 2.0 ** -23)):
            for d in (-ulp, 0.0, ulp):
                ties += [(1 + frac + d) * 2.0 ** e, -(1 + frac + d) * 2.0 ** e]
    sub = [k * 2.0 ** -26 for k in range(0, 70)] + [2.0 ** -14 + k * 2.0 ** -26 for k in range(-9, 9)]     # fp16's subnormal range in quarter steps
    drawn = [M.draw_values((4099,), s, fmt, scatter=False).numpy() for s in (1, 2)]
    x = np.concatenate([np.array(edge + ties + sub, dtype=np.float32), M.specials(fmt).numpy()] + drawn)
    hi, lo = M.split(torch.from_numpy(x), fmt)
    ih, il = int_split(x, fmt)
    assert np.array_equal(hi.numpy(), ih), "hi differs at %s" % x[hi.numpy() != ih][:4]
    assert np.array_equal(lo.numpy(), il), "lo differs at %s" % x[lo.numpy() != il][:4]
    zero = M.split(torch.tensor([0.0, -0.0]), fmt)[0]
    assert [_hex(b) for b in zero] == [0x0000, 0x8000], "-0 is not kept distinct from +0"
    print("split %s: %d values bit-equal to the integer round-to-nearest-even (hi and lo)" % (fmt, len(x)))


def test_store_map_is_the_split_or_the_saturating_fp16():
    x = M.draw_values((3001,), 3, M.F16, scatter=False)
    hi, lo = M.store_map(x, True)
    ih, il = int_split(x.numpy(), M.BF16)
    assert np.array_equal(hi.numpy(), ih) and np.array_equal(lo.numpy(), il)
    hi, lo = M.store_map(x, False)
    assert lo is None and np.array_equal(hi.numpy(), rne_f16_bits(x.numpy()).view(np.int16))
    assert bool((hi.view(torch.float16).float().abs() <= 65504).all()) and bool((x.abs() > 65504).any())
    h16, l16 = M.planes(M.stored(x, False), False)
    assert l16 is None and torch.equal(h16.view(torch.int16), hi)
    assert torch.equal(M.load_map(*M.planes(M.stored(x, True), True)).double(), M.stored(x, True))


# ---------------------------------------------------------------------------------------------------------------- weights
@pytest.mark.parametrize("cout,cin,kh,kw", M.WEIGHT_SHAPES)
def test_weight_layouts_match_flip_and_permute(cout, cin, kh, kw):
    w = M.distinct_weights(cout, cin, kh, kw)
    hi = M.split(w.reshape(-1), M.BF16)[0]
    assert len(torch.unique(hi)) == w.numel(), "the hi plane alone does not tell the elements apart"
    fwd = w.permute(0, 2, 3, 1)
    dg = torch.flip(w, (2, 3)).permute(1, 2, 3, 0)
    assert torch.equal(M.conv_weight_values(w, 0), fwd) and torch.equal(M.conv_weight_values(w, 1), dg)
    for dgrad, ref in ((0, fwd), (1, dg)):
        want = M.split(ref.reshape(-1), M.BF16)
        got = M.conv_weight_planes(w, dgrad, False)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        nn, cc = ref.shape[0], ref.shape[3]
        if cc % 32 == 0:
            K = kh * kw * cc
            flat = ref.reshape(nn, K)
            cm = torch.stack([flat[:, 32 * j:32 * j + 32] for j in range(K // 32)]).reshape(-1)       # [K/32][n][32], spelled out
            got = M.conv_weight_planes(w, dgrad, True)
            assert torch.equal(got[0], M.split(cm, M.BF16)[0]) and torch.equal(got[1], M.split(cm, M.BF16)[1])
            swapped = M.split(M.chunk_major_order(ref, swapped=True), M.BF16)
            if nn > 1 and K > 32:
                assert not torch.equal(got[0], swapped[0]), "n and chunk swapped is not rejected"
    if kh * kw > 1:
        noflip = M.split(M.conv_weight_values(w, 1, flip=False).reshape(-1), M.BF16)
        assert not torch.equal(M.conv_weight_planes(w, 1, False)[0], noflip[0]), "a transpose without the flip is not rejected"
    else:
        assert not torch.equal(M.conv_weight_planes(w, 1, False)[0], M.conv_weight_planes(w, 0, False)[0]) or cout == cin == 1


def test_weight_cases_reach_both_kinds_of_last_block_and_every_chunk_major_mode():
    counts = [M.split_threads(*s, d) for s in M.WEIGHT_SHAPES for d in (0, 1, 2)]
    assert any(t % 256 == 0 for t in counts) and any(t % 256 for t in counts), counts
    assert any(M.split_threads(*s, 2) % 256 for s in M.WEIGHT_SHAPES), "no _both case with idle tail threads"
    modes = [M.chunk_major_modes(s[0], s[1]) for s in M.WEIGHT_SHAPES]
    assert [0, 1, 2, 3] in modes and [0] in modes, modes


# ------------------------------------------------------------------------------------------------------------------- maps
def test_pack_reference_layout_and_zero_channels():
    n, c, h, w, cpad = 2, 13, 4, 3, 16
    x = M.draw_values((n, c, h, w), 5, M.F16)
    for paired in (True, False):
        hi, lo = M.pack_nhwc(x, c, cpad, 1, paired)
        assert hi.shape == (n, h, w, cpad) and not bool(hi[..., c:].any()) and (lo is None or not bool(lo[..., c:].any()))
        want = M.store_map(x, paired)[0]
        assert torch.equal(hi[..., :c].permute(0, 3, 1, 2), want)
        whole = torch.full((n, h + 2, w + 2, cpad), 0x7FC0, dtype=torch.int16)
        put = M.put_interior(whole, hi, 1)
        assert torch.equal(put[:, 1:-1, 1:-1], hi) and bool((put[M.halo_mask(n, h, w, cpad, 1)] == 0x7FC0).all())


def test_u8_cams_reference_formula_and_layout():
    n, ncam, h, w = 2, 3, 5, 7
    img = torch.arange(n * ncam * h * w * 3, dtype=torch.int64).remainder(256).to(torch.uint8).view(n, ncam, h, w, 3)
    hi, lo, v = M.u8_cams(img, M.CAM_MEAN, M.CAM_STD, 3, True)
    assert v.shape == (n, h, ncam * w, 4) and not bool(v[..., 3].any())
    i, cam, y, x, ch = 1, 2, 4, 6, 1
    one = (np.float32(int(img[i, cam, y, x, ch])) / np.float32(255) - np.float32(M.CAM_MEAN[ch])) / np.float32(M.CAM_STD[ch])
    assert float(v[i, y, cam * w + x, ch]) == float(one) and isinstance(one, np.float32)
    ih, il = int_split(v.numpy().reshape(-1), M.BF16)
    assert np.array_equal(hi.numpy().reshape(-1), ih) and np.array_equal(lo.numpy().reshape(-1), il)


@pytest.mark.parametrize("n,h,w", M.HALO_NHW)
def test_halo_mask_counts_and_rejects_a_short_column(n, h, w):
    for pad in (1, 2, 3):
        for c in (3, 8):
            m = M.halo_mask(n, h, w, c, pad)
            assert int(m.sum()) == n * c * ((h + 2 * pad) * (w + 2 * pad) - h * w) and not bool(m[:, pad:pad + h, pad:pad + w].any())
            assert not torch.equal(m, M.halo_mask(n, h, w, c, pad, short=True)), "a halo mask one column short is not rejected"
    assert not bool(M.halo_mask(n, h, w, 8, 0).any())


@pytest.mark.parametrize("n,h,w,c", M.POOL_SHAPES)
@pytest.mark.parametrize("paired", [True, False])
def test_maxpool_rule_matches_affine_maxpool64_and_max_pool2d(n, h, w, c, paired):
    v = M.draw_relu_map(n, c, h, w, 3, paired)
    assert bool((v >= 0).all())
    zeros = float((v == 0).double().mean())
    vals, pos = M.maxpool_first_positive(v)
    ones, nought = torch.ones(c), torch.zeros(c)
    rv, rp, act = R.affine_maxpool64(v, ones, nought)
    assert torch.equal(act.double(), v), "scale 1, shift 0 changes the stored values"
    assert torch.equal(vals, rv) and torch.equal(pos, rp)
    assert torch.equal(vals, F.max_pool2d(v, 3, 2, 1))
    if h * w > 1:
        assert 0.3 < zeros < 0.55, zeros
        assert sorted(set(pos.reshape(-1).tolist())) == list(range(9)), "not every window position holds a maximum somewhere"
        assert bool((vals == 0).any()), "no all-zero window"
        wrong = M.maxpool_first_positive(v, last=True)
        assert torch.equal(wrong[0], vals) and not torch.equal(wrong[1], pos), "the last maximum instead of the first is not rejected"
    else:
        assert pos.reshape(-1).tolist() == [4] * c
    hi, lo = M.maxpool_input_planes(v, 3, paired)
    assert torch.equal(M.load_map(hi, lo)[:, 3:-3, 3:-3].double(), v.permute(0, 2, 3, 1))
    assert not bool(hi[:, 2, 2:-2].any()) and not bool(hi[:, 2:-2, 2].any()) and bool((hi[:, 1].float() == 7).all())


def test_map_add_order_and_the_mask_rule():
    shape = (3, 24, 2, 5)
    for paired, mv in ((True, M.mask_values(shape, 1)), (False, M.mask_values_f16(shape, 1))):
        a = M.stored(M.draw_values(shape, 6, M.F16).clamp(-1e38, 1e38), paired).float()
        b = M.stored(M.draw_values(shape, 7, M.F16).clamp(-1e38, 1e38).roll(1, 3), paired).float()
        assert torch.equal(M.stored(mv, paired), mv), "the mask values are not values of the format"
        assert bool((mv > 0).any()) and bool((mv < 0).any()) and bool((mv == 0).any()) and bool(torch.signbit(mv[mv == 0]).any())
        assert 0 < float(mv[mv > 0].min()) < 1e-4
        got = M.map_add(a, b, mv)
        assert torch.equal(got, torch.where(mv > 0, a, torch.zeros(())) + b)
        assert torch.equal(M.map_add(a), a) and torch.equal(M.map_add(a, b), a + b)
        assert bool(torch.isfinite(got).all())
        ge = M.store_map(M.map_add(a, b, mv, mask_ge=True), paired)[0]
        assert not torch.equal(ge, M.store_map(got, paired)[0]), "a mask taken as >= 0 is not rejected"


def test_upsample_reference():
    for (ho, wo), (hu, wu) in M.UPSAMPLE:
        g = torch.arange(1, 1 + 2 * 8 * ho * wo, dtype=torch.float32).view(2, 8, ho, wo)
        u = M.upsample2_zero(g, hu, wu)
        assert u.shape == (2, 8, hu, wu)
        for y in range(hu):
            for x in range(wu):
                want = g[:, :, y // 2, x // 2] if (y % 2 == 0 and x % 2 == 0 and y // 2 < ho and x // 2 < wo) else torch.zeros(2, 8)
                assert torch.equal(u[:, :, y, x], want)
        assert (hu + 1) // 2 <= ho and (wu + 1) // 2 <= wo, "a case whose every even pixel has a source"


def test_truncating_split_is_rejected():
    for seed in (1, 2):
        x = M.draw_values((2, 8, 3, 5), seed, M.BF16)
        good, bad = M.split(x, M.BF16), M.split(x, M.BF16, truncate=True)
        assert not torch.equal(good[0], bad[0]) and not torch.equal(good[1], bad[1]), "a split that truncates is not rejected"


def test_frozen_coeffs_reference_and_ulp_distance():
    rm, rv, gamma, beta = M.draw_frozen(257)
    assert float(rv[0]) == 0 and float(rv[128]) == pytest.approx(1e-12) and bool((rv >= 0).all())
    mean, rstd, scale, shift = M.frozen_coeffs64(rm, rv, gamma, beta, M.FROZEN_EPS)
    eps32 = float(np.float32(M.FROZEN_EPS))
    i = 128
    rs = 1.0 / np.sqrt(float(rv[i]) + eps32)
    assert float(rstd[i]) == float(np.float32(rs)) and float(scale[i]) == float(np.float32(float(gamma[i]) * rs))
    assert float(shift[i]) == float(np.float32(float(beta[i]) - float(rm[i]) * (float(gamma[i]) * rs)))
    assert torch.equal(mean, rm) and bool(torch.isfinite(rstd).all())
    _, _, s1, sh1 = M.frozen_coeffs64(rm, rv, None, None, M.FROZEN_EPS)
    assert torch.equal(s1, rstd) and torch.equal(sh1, (-(rm.double() * (1.0 / torch.sqrt(rv.double() + eps32)))).float())
    one = torch.tensor([1.0, -1.0, 0.0])
    nxt = torch.tensor([1.0 + 2.0 ** -23, -1.0 - 2.0 ** -23, 1.4e-45])
    assert M.ulp_distance(one, nxt).tolist() == [1, 1, 1] and M.ulp_distance(one, one).tolist() == [0, 0, 0]


# ------------------------------------------------------------------------------------------------- the channel sum's floor
def test_chan_sum_float32_floor_is_below_a_quarter_of_the_bar():
    worst = 0.0
    for c in M.CHAN_SUM_C:
        for n, h, w in M.CHAN_SUM_NHW:
            for paired in (True, False):
                v = M.draw_chan_sum(n, c, h, w, paired)
                ref, mag = M.chan_sum64(v)
                assert bool((ref.abs() > 0.5 * mag).all()), "sum |terms| is not about |sum|"
                f32 = v.float().sum((0, 2, 3))
                floor = float(((f32.double() - ref).abs() / mag).max())
                print("chan_sum floor [%d, %d, %d, %d] %s: %.3e of sum |terms|" % (n, h, w, c, "pair" if paired else "f16", floor))
                worst = max(worst, floor)
    print("chan_sum float32 floor, the worst case: %.3e (bar %.1e, a quarter of it %.2e)" % (worst, M.CHAN_SUM_BAR, M.CHAN_SUM_BAR / 4))
    assert worst < M.CHAN_SUM_BAR / 4
