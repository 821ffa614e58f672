"""Host tests of tests/pool_ref.py (no GPU): the closed forms of the mean, GeM, GeM's backward with dL/dp and the map form
against fp64 autograd through oracle/nets.gem to 1e-12; the layout helpers; the float32 floors the bars of
tests/test_gpu_pool_kernels.py are built from, at that file's cases; and for every bar a deliberately wrong variant of the same
closed form that must exceed it: GeM backward without the [x >= eps] mask, dL/dp without the -ln(S) / p^2 term, the mean with the
divisor HW + 1.

Floors on the CPU: the float32 mean 0 .. 1.2e-7 per plane (bars 2.4e-7 .. 4.7e-7); the float32 map form base + gmean / HW rounded
to the bf16 pair 2.2e-6 .. 6.9e-6 (the pair's rounding, 2^-17 at the worst: the largest on one-pixel planes; bars 0.9e-5 .. 2.8e-5)."""
import pytest
import torch

import pool_ref as P
from oracle import nets

TIGHT = 1e-12


def _close(got, ref, what):
    got, ref = got.detach().double(), ref.detach().double()
    err = float((got - ref).norm() / ref.norm().clamp_min(1e-300))
    assert err < TIGHT, "%s: %.3e" % (what, err)


# ------------------------------------------------------------------------------------------------------- pinned to autograd
@pytest.mark.parametrize("p", [3.0, 2.5])
@pytest.mark.parametrize("n,c,h,w", [(2, 5, 3, 4), (3, 2, 1, 1)])
def test_pooling_forms_match_autograd(n, c, h, w, p):
    x = P.draw_map(n, c, h, w, 1, "f32")
    assert bool((x < P.GEM_EPS).any())
    gm, gg = P.draw_vec(n, c, 2).double(), P.draw_vec(n, c, 3).double()
    base = P.draw_map(n, c, h, w, 4, "pair", 1.0, 0.0)
    xl = x.clone().requires_grad_(True)
    pl = torch.tensor([p], dtype=torch.float64, requires_grad=True)
    mean, gem = nets.avgpool_vec(xl), nets.gem_flat(xl, pl, P.GEM_EPS)
    _close(P.mean(x), mean, "mean"), _close(P.gem(x, p), gem, "gem")
    ((base * xl).sum() + (gm * mean).sum() + (gg * gem).sum()).backward()
    y = gem.detach()
    out, dp = P.pool_bwd_map(x, base, gm, gg, y, p)
    _close(out, xl.grad, "the map form")
    mag, sub = P.dp_magnitudes(x, p, P.GEM_EPS, y, gg)
    assert abs(float(dp) - float(pl.grad)) <= TIGHT * mag, "dL/dp"
    gx, dp2 = P.gem_bwd(x, p, P.GEM_EPS, y, gg)
    assert float(dp2) == float(dp) and sub <= mag
    _close(gx, out - base - (gm / (h * w))[:, :, None, None], "gem_bwd's gx")
    if h * w == 1:
        assert abs(float(dp)) <= TIGHT * mag, "one pixel per plane: GeM = max(x, eps) whatever p is"
        assert P.dp_error(1e-4 * sub, float(dp), x, sub) == pytest.approx(1e-4, rel=1e-6)


def test_from_partials_is_the_pooling_of_the_summed_blocks():
    x = P.draw_map(2, 24, 16, 16, 5, "f32")
    blocks = x.permute(0, 2, 3, 1).reshape(2, 4, 64, 24)
    partial = torch.stack([blocks.sum(2), blocks.clamp_min(P.GEM_EPS).pow(2.5).sum(2)], 2)
    m, g = P.from_partials(partial, 256, 2.5)
    _close(m, P.mean(x), "mean"), _close(g, P.gem(x, 2.5), "gem")
    assert P.from_partials(partial, 256)[1] is None
    assert [P.from_conv_blocks(h, w) for h, w in P.FROM_CONV_HW] == [1, 8, 9, 32, 33, 70]


@pytest.mark.parametrize("paired", [True, False])
@pytest.mark.parametrize("pad", [1, 3])
def test_layout_helpers(pad, paired):
    v = P.draw_map(2, 8, 3, 5, 6, "pair" if paired else "f16")
    hi, lo = P.map_planes(v, pad, paired)
    assert tuple(hi.shape) == (2, 3 + 2 * pad, 5 + 2 * pad, 8) and (lo is None) == (not paired)
    assert torch.equal(P.interior(hi, lo, pad), v)
    for plane in [hi] + ([lo] if paired else []):
        inner = torch.zeros_like(plane, dtype=torch.bool)
        inner[:, pad:-pad, pad:-pad] = True
        assert bool((plane[~inner] == P.HALO_POISON).all()) and int((~inner).sum()) > 0


def test_the_large_map_has_empty_splits_and_the_atomic_case_is_above_the_slots():
    from agplace_amd import _lib
    for (n, h, w, c), want in P.POOL_MANY_SPLITS.items():
        splits = int(_lib.load().agp_pool_workspace_floats(n, c, h, w)) // (n * 2 * c)
        assert (splits, P.split_pixels(n, c, h, w, splits)[1]) == want
    assert {P.POOL_F32_SPLITS, P.POOL_F32_SPLITS + 1, 256, 2048} <= {s for s, _ in P.POOL_MANY_SPLITS.values()}
    assert {384, 2048} <= {c for (n, h, w, c), (s, _) in P.POOL_MANY_SPLITS.items() if s == 256}
    assert P.split_pixels(*[P.POOL_LARGE[i] for i in (0, 3, 1, 2)], 2048) == (67, 4)
    n, c, h, w = P.F32_ATOMIC
    assert (n * c + 3) // 4 > P.GP_SLOTS == _lib.GP_FLOATS - 2
    for nn, cc in P.F32_NC[:2]:
        assert (nn * cc) % 4


# ------------------------------------------------------------------------------------------- floors, bars, discrimination
@pytest.mark.parametrize("n,h,w,c", [(n, h, w, c) for c in P.POOL_C for n, h, w in P.POOL_NHW] + list(P.POOL_MANY_SPLITS))
def test_forward_floors_and_the_wrong_divisor(c, n, h, w):
    big = n * c * h * w > 4_000_000           # (the widest many-split maps: one format, the mean alone)
    for fmt in ("pair",) if big else ("pair", "f16"):
        x = P.draw_map(n, c, h, w, 1, fmt)
        bar, floor = P.mean_bar(x)
        print("mean [%d, %d, %d, %d] %s: float32 floor %.3e, bar %.3e" % (n, h, w, c, fmt, floor, bar))
        assert floor < 5e-7 and bar < P.CEIL_FWD / 10
        wrong = P.per_plane_rel(P.mean(x, extra_divisor=1), P.mean(x))
        assert bool((wrong > bar).all()), "the mean with the divisor HW + 1 passes the bar"
        for p in () if big else (3.0, 2.5):
            y = P.gem(x, p)
            f32 = P.worst_plane(P.gem(x, p, dtype=torch.float32), y)
            assert f32 < P.CEIL_FWD / 4, "the float32 form of GeM is not well inside the ceiling: %.3e" % f32


@pytest.mark.parametrize("n,h,w", P.POOL_NHW)
@pytest.mark.parametrize("c", P.POOL_BWD_C)
def test_backward_bars_catch_the_missing_mask_and_the_missing_log_term(c, n, h, w):
    x = P.draw_map(n, c, h, w, 2, "pair")
    base = P.draw_map(n, c, h, w, 3, "pair", 1.0, 0.0)
    gm, gg = P.draw_vec(n, c, 4), P.draw_vec(n, c, 5, positive=True)
    bar, floor = P.linear_map_bar(x, base, gm)
    bar_m, floor_m = P.linear_map_bar(x, None, gm)
    print("[%d, %d, %d, %d]: base + gmean floor %.3e bar %.3e, gmean alone floor %.3e bar %.3e" % (n, h, w, c, floor, bar, floor_m, bar_m))
    assert floor <= 2.0 ** -17 and floor_m <= 2.0 ** -17          # one rounding of the pair, at the worst
    ref, _ = P.pool_bwd_map(x, base, gm)
    wrong = base + (gm.double() / (h * w + 1))[:, :, None, None]
    assert P.worst_plane(wrong, ref) > bar, "gmean / (HW + 1) passes the bar"
    for p in (3.0, 2.5):
        y = P.gem(x, p).float()
        gx, dp = P.gem_bwd(x, p, P.GEM_EPS, y, gg)
        f32x, f32p = P.gem_bwd(x, p, P.GEM_EPS, y, gg, dtype=torch.float32)
        mag, sub = P.dp_magnitudes(x, p, P.GEM_EPS, y, gg)
        assert P.worst_plane(P._bf16_pair(f32x), gx) < P.CEIL_GX / 4
        assert P.dp_error(f32p, float(dp), x, sub) < P.CEIL_GP / 4, "the float32 form of dL/dp is not well inside its bar"
        clamped = (x < P.GEM_EPS).all(3).all(2) & (gg != 0)       # the planes that are all clamp: their gx is zero
        assert bool(clamped.any()) and not bool(gx[clamped].any())
        bad, _ = P.gem_bwd(x, p, P.GEM_EPS, y, gg, mask=False)
        rel = P.per_plane_rel(bad, gx)
        assert bool((rel[clamped] > P.CEIL_GX).all()), "GeM backward without the [x >= eps] mask passes the bar"
        _, bad_dp = P.gem_bwd(x, p, P.GEM_EPS, y, gg, ln_term=False)
        assert P.dp_error(float(bad_dp), float(dp), x, sub) > P.CEIL_GP, "dL/dp without the -ln(S) / p^2 term passes the bar"


@pytest.mark.parametrize("h,w", P.F32_HW)
@pytest.mark.parametrize("n,c", P.F32_NC + (P.F32_ATOMIC[:2],))
def test_f32_floors(n, c, h, w):
    if (n, c) == P.F32_ATOMIC[:2]:
        if (h, w) != P.F32_HW[0]:
            return
        h, w = P.F32_ATOMIC[2:]
    x = P.draw_map(n, c, h, w, 7, "f32")
    gy = P.draw_vec(n, c, 8, positive=True)
    bar, floor = P.mean_bar(x)
    assert floor < 5e-7
    for p in (3.0, 2.5):
        y = P.gem(x, p).float()
        gx, dp = P.gem_bwd(x, p, P.GEM_EPS, y, gy)
        f32x, f32p = P.gem_bwd(x, p, P.GEM_EPS, y, gy, dtype=torch.float32)
        mag, sub = P.dp_magnitudes(x, p, P.GEM_EPS, y, gy)
        assert P.worst_plane(f32x, gx) < P.CEIL_GX / 4
        err = P.dp_error(f32p, float(dp), x, sub)
        print("[%d, %d, %d, %d] p %.1f: float32 dL/dp error %.3e (|dL/dp| / sum |terms| %.3e)" % (n, c, h, w, p, err, abs(float(dp)) / mag))
        assert err < P.CEIL_GP / 4
        _, bad_dp = P.gem_bwd(x, p, P.GEM_EPS, y, gy, ln_term=False)
        assert P.dp_error(float(bad_dp), float(dp), x, sub) > P.CEIL_GP


@pytest.mark.parametrize("c", P.FROM_CONV_C)
@pytest.mark.parametrize("h,w", P.FROM_CONV_HW)
def test_from_conv_floors(h, w, c):
    blocks = P.from_conv_blocks(h, w)
    part = P.draw_partials(2, blocks, c, 9, 2.5)
    m, g = P.from_partials(part, h * w, 2.5)
    m32, g32 = P.from_partials(part, h * w, 2.5, dtype=torch.float32)
    floor = P.worst_plane(m32, m)
    assert floor < 5e-7 and P.worst_plane(g32, g) < P.CEIL_FWD / 4
    bar = P.bar_of(floor, P.CEIL_FWD)
    if blocks > 1:
        m_bad, g_bad = P.from_partials(part[:, :-1], h * w, 2.5)
        assert bool((P.per_plane_rel(m_bad, m) > bar).all()) and bool((P.per_plane_rel(g_bad, g) > P.CEIL_FWD).all()), \
            "a sum that loses its last block passes"
