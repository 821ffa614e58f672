"""The references of tests/dense_train_ref.py pinned on the CPU: the fp64 weight gradient and BatchNorm backward against fp64
autograd, the plan mirror against the library's own workspace query (the library loads without a GPU), the regime every named
shape is there for, the error floors of the two weight-gradient arithmetics against the bars the GPU tests hold the kernels to,
and planted defects that those bars must catch.  tests/test_gpu_wgrad_kernels.py and tests/test_gpu_bn_bwd_kernels.py stand on
these functions."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import dense_train_ref as R
from conv_sched_util import _bf16_pair, _f16

TOL = 1e-12
HOST_N = 8          # images of the two many-split shapes on the CPU (their batches exist for the split count alone: the plan is
#                     asserted at the full batch, the arithmetic's error floor does not depend on it)


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------- the fp64 weight gradient
@pytest.mark.parametrize("k,stride", [(3, 1), (3, 2), (1, 1), (1, 2), (7, 2)], ids=["3x3s1", "3x3s2", "1x1s1", "1x1s2", "7x7s2"])
def test_wgrad64_equals_autograd(k, stride):
    gen = torch.Generator().manual_seed(10 * k + stride)
    cin, cout, n, h, w = (3 if k == 7 else 5), 6, 2, 11, 14
    x = torch.randn((n, cin, h, w), generator=gen, dtype=torch.float64)
    wt = torch.randn((cout, cin, k, k), generator=gen, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, wt, None, stride, k // 2)
    g = torch.randn(y.shape, generator=gen, dtype=torch.float64)
    (y * g).sum().backward()
    got = R.wgrad64(x, g, k, stride, k // 2)
    assert got.shape == (k, k, cin, cout)
    assert _rel(got.permute(3, 2, 0, 1), wt.grad) < TOL
    if k == 7:
        packed = R.wgrad64_stem_packed(x, g)
        assert packed.shape == (7, 8, 4, cout)
        assert torch.equal(packed[:, :7, :3], got) and not bool(packed[:, :7, 3].any()) and bool(packed[:, 7].isnan().all())


def test_shifted_tap_is_the_neighbouring_column():
    """The planted strip shift: tap (ky, kx) read one pixel to the right is tap (ky, kx + 1) wherever that exists."""
    gen = torch.Generator().manual_seed(3)
    x = torch.randn((2, 4, 9, 10), generator=gen, dtype=torch.float64)
    g = torch.randn((2, 5, 9, 10), generator=gen, dtype=torch.float64)
    clean, bent = R.wgrad64(x, g, 3, 1, 1), R.wgrad64(x, g, 3, 1, 1, shifted=3)
    assert torch.equal(bent[1, 0], clean[1, 1]) and torch.equal(bent[0], clean[0]) and torch.equal(bent[1, 1:], clean[1, 1:])


# ------------------------------------------------------------------------------------------------------ BatchNorm backward
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("relu,residual", [(True, True), (True, False), (False, False)], ids=["relu_res", "relu", "plain"])
def test_bn_bwd64_equals_autograd(train, relu, residual):
    """y = relu?(BN(z) + res?) as test_conv_bn_unit_backward builds it; gres is the gradient of the residual branch."""
    gen = torch.Generator().manual_seed(7)
    n, c, h, w, eps = 3, 8, 5, 7, 1e-5
    z = torch.randn((n, c, h, w), generator=gen, dtype=torch.float64, requires_grad=True)
    res = torch.randn((n, c, h, w), generator=gen, dtype=torch.float64, requires_grad=True)
    gam = (0.5 + torch.rand(c, generator=gen, dtype=torch.float64)).requires_grad_(True)
    bet = torch.randn(c, generator=gen, dtype=torch.float64, requires_grad=True)
    G = torch.randn((n, c, h, w), generator=gen, dtype=torch.float64)
    if train:
        mean = z.detach().mean((0, 2, 3))
        var = ((z.detach() - mean.view(1, -1, 1, 1)) ** 2).mean((0, 2, 3))
        y = F.batch_norm(z, None, None, gam, bet, True, 0.0, eps)
    else:
        mean = torch.randn(c, generator=gen, dtype=torch.float64)
        var = 0.5 + torch.rand(c, generator=gen, dtype=torch.float64)
        y = F.batch_norm(z, mean, var, gam, bet, False, 0.0, eps)
    if residual:
        y = y + res
    if relu:
        y = torch.relu(y)
    (y * G).sum().backward()
    rstd = 1.0 / (var + eps).sqrt()
    gz, gres, gg, gb, am = R.bn_bwd64(z.detach(), G, (y.detach() > 0) if relu else None, mean, rstd, gam.detach(), n * h * w,
                                      frozen=not train)
    assert _rel(gz, z.grad) < 1e-11 and _rel(gg, gam.grad) < 1e-11 and _rel(gb, bet.grad) < 1e-11
    if residual:
        assert _rel(gres, res.grad) < TOL
    assert torch.equal(am, z.grad.abs().amax((0, 2, 3))) or _rel(am, z.grad.abs().amax((0, 2, 3))) < 1e-11


def test_synchronised_form_is_the_whole_batch():
    """bn_bwd64 on the first half of a batch with the whole batch's sums and count = the first half of bn_bwd64 on the whole."""
    z, gy, y, gamma, _ = R.draw_bn(4, 8, 5, 7, seed=1)
    mean, rstd = R.batch_stats(z)
    cnt = 4 * 5 * 7
    whole = R.bn_bwd64(z, gy, y > 0, mean, rstd, gamma, cnt)
    half = R.bn_bwd64(z[:2], gy[:2], y[:2] > 0, mean, rstd, gamma, cnt, sums=(whole[3], whole[2]))
    assert _rel(half[0], whole[0][:2]) < TOL


@pytest.mark.parametrize("h,w", [(9, 11), (8, 10), (5, 6)])
@pytest.mark.parametrize("frozen", [False, True], ids=["train", "frozen"])
def test_maxpool_bn_bwd64_equals_autograd(h, w, frozen):
    n, c, eps = 2, 8, 1e-5
    z, mean, rstd, gamma, beta, scale, shift = R.draw_pool(n, c, h, w, seed=h)
    assert not bool(R.pool_decision_ties(z, scale, shift).any())
    pooled, pos, act = R.affine_maxpool64(z, scale, shift)
    gen = torch.Generator().manual_seed(h * w)
    gp = torch.randn(pooled.shape, generator=gen, dtype=torch.float64)
    zr = z.clone().requires_grad_(True)
    gam, bet = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    m64, v64 = mean.double(), 1.0 / rstd.double() ** 2 - eps
    if frozen:
        bn = F.batch_norm(zr, m64, v64, gam, bet, False, 0.0, eps)
    else:
        bn = F.batch_norm(zr, None, None, gam, bet, True, 0.0, eps)
    yp = F.max_pool2d(torch.relu(bn), 3, 2, 1)
    (yp * gp).sum().backward()
    # the fp32 activations and the fp64 ones order every window the same way (no ties by construction): same routing
    assert _rel(pooled, yp.detach()) < 1e-6
    gz, _, gg, gb, _ = R.maxpool_bn_bwd64(gp, pos, act, z, mean, rstd, gamma, frozen)
    # (mean / rstd rounded to fp32 against autograd's exact ones: 1e-6, not 1e-12)
    assert _rel(gz, zr.grad) < 2e-6 and _rel(gg, gam.grad) < 2e-6 and _rel(gb, bet.grad) < 2e-6


def test_affine_maxpool64_follows_the_kernels_rule():
    """Strict `>` from a start value of 0 at position 4: a window without a positive activation records 4 and pools 0; the first
    of the maxima wins; out-of-map taps never do."""
    z = torch.full((1, 8, 5, 6), -1.0, dtype=torch.float64)
    one, zero = torch.ones(8), torch.zeros(8)
    pooled, pos, _ = R.affine_maxpool64(z, one, zero)
    assert not bool(pooled.any()) and bool((pos == 4).all())
    z[0, :, 0, 0] = 2.0                 # window (0, 0): tap (ky, kx) = (1, 1) -> 4; no other window sees pixel (0, 0)
    z[0, :, 2, 3] = 3.0                 # windows (1, 1) and (1, 2): taps (1, 2) = 5 and (1, 0) = 3
    z[0, :, 3, 3] = 3.0                 # the same windows one row lower (a later tap: no strict improvement), and row 2's windows
    pooled, pos, _ = R.affine_maxpool64(z, one, zero)
    assert int(pos[0, 0, 0, 0]) == 4 and float(pooled[0, 0, 0, 0]) == 2.0
    assert int(pos[0, 0, 1, 1]) == 5 and int(pos[0, 0, 1, 2]) == 3
    assert int(pos[0, 0, 2, 1]) == 2 and int(pos[0, 0, 2, 2]) == 0           # window row 2: pixel row 3 is its ky = 0
    assert bool(R.pool_decision_ties(z, one, zero).any())                      # the equal pair above IS such a tie
    routed = R.maxpool_route64(torch.ones_like(pooled), pos, 5, 6)
    assert float(routed.sum()) == pooled.numel() and float(routed[0, 0, 2, 3]) == 2.0


# ------------------------------------------------------------------------------------------------------- the grid mirror
def test_fixed_g_of_the_bn_maps():
    """Which path bn_bwd_apply_kernel / affine_kernel take on the maps of tests/test_gpu_bn_bwd_kernels.py."""
    import test_gpu_bn_bwd_kernels as T
    for (n, h, w) in ((3, 9, 11), (2, 5, 7)):
        assert R.fixed_g(n, h, w, 8) and R.fixed_g(n, h, w, 64)
        assert not R.fixed_g(n, h, w, 24) and not R.fixed_g(n, h, w, 96)
    assert R.grid_for(3 * 9 * 11 * 3) == 1 and R.grid_for(3 * 9 * 11 * 12) == 4 and R.grid_for(2 * 5 * 7 * 12) == 1
    assert R.fixed_g(2, 3, 3, 2048)
    assert 3 * 9 * 11 * 8 == 2376 and R.grid_for(2376) == 3       # 768 threads: a trip of pairs (1536 items), a trip of single items
    for (n, h, w, c), want in T.MAPS.values():
        assert R.fixed_g(n, h, w, c) == want, (n, h, w, c)
    assert any(want and c in (24, 96) for (_, _, _, c), want in T.MAPS.values())
    assert R.grid_for(10 ** 9) == 8192


def test_gz_floor_of_a_float32_evaluation():
    """The yardstick of the gz bar: the closed form in float32 on the CPU, rounded to the bf16 pair, against fp64 -- per channel.
    The kernels get four times the floor and never more than 1e-5."""
    worst = 0.0
    for (n, h, w, c) in ((3, 9, 11, 64), (2, 5, 7, 24), (3, 9, 11, 96), (2, 3, 3, 2048)):
        for frozen in (False, True):
            z, gy, y, gamma, _ = R.draw_bn(n, c, h, w, seed=2)
            mean, rstd = R.batch_stats(z)
            bar, floor = R.gz_bar(z, gy, y > 0, mean, rstd, gamma, n * h * w, frozen)
            print("gz floor %d x %d x %d x %d frozen %d: %.3e, bar %.3e" % (n, h, w, c, frozen, floor, bar))
            assert 0 < floor < R.BN_BAR_MAX and bar <= R.BN_BAR_MAX
            worst = max(worst, floor)
    assert worst < 2.0 ** -17       # the storage rounding of the pair bounds every element by that: so does it a channel's rms


# ----------------------------------------------------------------------------------------------------------- the plan mirror
@pytest.mark.parametrize("name", list(R.CASES))
def test_wgrad_plan_equals_the_library_and_reports_the_intended_regime(name):
    from agplace_amd import _lib
    L = _lib.load()
    t, o = R.plans(name)
    for f16, p in ((False, t), (True, R.wgrad_plan(*R.CASES[name][0], f16=True, stem=R.is_stem(name)))):
        d = R.wgrad_desc(name, f16=f16)
        assert int(L.agp_conv2d_wgrad_workspace_bytes(C.byref(d))) == p["splits"] * p["rows"] * d.cout * 4, (name, f16, p)
        assert p["rows"] == d.kh * d.kw * d.cin
    assert R.CASES[name][1](t, o), (name, t, o)
    assert (o is None) == (name in ("one_kstep", "gx3"))           # mode 0 with cin % 64 != 0: three products only
    assert t["splits"] <= t["ksteps"] and t["last"] >= 1


def test_wgrad_plan_over_a_sweep_of_shapes():
    """The mirror against the library on shapes around the cases: every (kernel, cin) family, batches 1 .. 40."""
    from agplace_amd import _lib
    L = _lib.load()
    for (cin, cout, k, stride, h, w) in ((64, 64, 3, 1, 30, 45), (128, 64, 3, 1, 14, 20), (96, 128, 3, 1, 9, 9), (64, 128, 3, 2, 29, 37),
                                         (160, 64, 1, 1, 20, 31), (32, 64, 1, 2, 40, 51), (512, 64, 1, 1, 7, 9)):
        for n in (1, 2, 3, 7, 16, 40):
            for f16 in (False, True):
                p = R.wgrad_plan(cin, cout, k, stride, h, w, n, f16)
                d = R.desc_of((cin, cout, k, stride, h, w, n), f16=f16)
                assert int(L.agp_conv2d_wgrad_workspace_bytes(C.byref(d))) == p["splits"] * p["rows"] * cout * 4
    assert R.wgrad_plan(48, 64, 3, 1, 9, 9, 1) is None and R.wgrad_plan(64, 96, 3, 1, 9, 9, 1) is None
    assert R.wgrad_plan(64, 64, 5, 1, 9, 9, 1) is None


def test_the_many_split_batches_are_the_smallest():
    assert not R._many_splits(R.wgrad_plan(64, 64, 3, 1, 62, 94, R.N_MANY_SPLITS - 1))
    assert not R._many_chunks(R.wgrad_plan(64, 64, 3, 1, 56, 56, R.N_MANY_CHUNKS - 1, True))
    t, _ = R.plans("s1_many_splits")
    assert t["splits"] > 32 and t["splits"] % 32 != 0      # the reduce's last trip is not full: clamped loads, skipped adds


# -------------------------------------------------------------------------------------------------------- the error floors
def _host_operands(name, gscale):
    n = min(R.CASES[name][0][6], HOST_N)
    return R.draw_wgrad(name, gscale, seed=1, n=n)


FLOOR_CASES = [(name, gs) for name in R.CASES for gs in R.GSCALES.get(name, (1.0,))]


@pytest.mark.parametrize("name,gscale", FLOOR_CASES, ids=["%s-g%g" % c for c in FLOOR_CASES])
def test_error_floor_of_both_arithmetics_is_at_most_half_the_bar(name, gscale):
    """emulate_three_product and emulate_one_pass (exact arithmetic on the operands the kernels multiply) against wgrad64 on the
    stored operands: at most half of what the GPU tests allow the kernels, per granule and per output channel."""
    x, g = _host_operands(name, gscale)
    ref = R.reference(name, x, g)
    e3 = R.emulate_three_product(name, x, g)
    g3, where3, _ = R.granule_rel(e3, ref)
    c3, _, _ = R.per_out_channel_rel(e3, ref)
    e1 = R.emulate_one_pass(name, x, g)
    g1, where1, _ = R.granule_rel(e1, ref)
    c1, _, _ = R.per_out_channel_rel(e1, ref)
    print("%s gscale %g: three-product floor %.2e per granule (%s) %.2e per channel; one-pass %.2e (%s) %.2e; whole %.2e" % (
        name, gscale, g3, where3, c3, g1, where1, c1, R.whole_rel(e1, ref)))
    assert g3 <= R.BAR_3P / 2 and c3 <= R.BAR_3P / 2
    assert g1 <= R.BAR_1P / 2 and c1 <= R.BAR_1P_CHANNEL / 2
    assert R.whole_rel(e1, ref) > R.ONE_PASS_REALLY_RAN            # the one-pass arithmetic is told from the three products'
    assert R.whole_rel(e3, ref) < R.ONE_PASS_REALLY_RAN


def test_operands_are_exact_in_both_formats():
    x, g = R.draw_wgrad("s1_small")
    assert torch.equal(_f16(x), x) and torch.equal(_bf16_pair(x), x) and torch.equal(_bf16_pair(g), g)
    R.planes(x, False), R.planes(x, True), R.planes(g, True)
    assert float(g[:, :16].abs().max()) < 0.01 < float(g[:, 16:].abs().max())


# ------------------------------------------------------------------------------------------------------------ sensitivity
def test_planted_defects_cross_the_bars():
    """What a subtly wrong kernel would produce lies above the bars: the last K-step of one split dropped, one tap's x strip
    shifted by one pixel, the xl gh product of one 32-channel block missing."""
    name = "s1_splits"
    x, g = R.draw_wgrad(name, seed=1)
    ref = R.reference(name, x, g)
    t, o = R.plans(name)
    for p, bar in ((t, R.BAR_3P), (o, R.BAR_1P)):
        hi = 2 * p["per"] * p["P"]                                 # the end of split 1
        worst, where, _ = R.granule_rel(R.reference(name, x, g * R.raster_mask(name, x.shape[0], hi - p["P"], hi)), ref)
        print("last K-step of split 1 of %d dropped: worst granule %.2e (%s)" % (p["splits"], worst, where))
        assert worst > bar
    worst, where, rel = R.granule_rel(R.reference(name, x, g, shifted=5), ref)
    assert worst > R.BAR_1P and where.startswith("tap 5") and float(rel[:5].max()) == 0
    e3 = R.emulate_three_product(name, x, g, drop_xl_block=1)
    worst, where, rel = R.granule_rel(e3, ref)
    print("xl gh of channel block 1 missing: worst granule %.2e (%s)" % (worst, where))
    assert worst > R.BAR_3P and "ci 32..63" in where and float(rel[:, 0].max()) < R.BAR_3P / 2
    # a gather shape and the stem too
    for other in ("ds_ragged2", "stem"):
        xo, go = R.draw_wgrad(other, seed=1)
        ro = R.reference(other, xo, go)
        po = R.plans(other)[0]
        lo = po["kpix"] - po["kpix_mod_p"] - po["P"]           # the last full K-step and the partial one (which holds halo alone)
        assert R.granule_rel(R.reference(other, xo, go * R.raster_mask(other, xo.shape[0], lo, po["kpix"])), ro)[0] > R.BAR_1P
        assert R.granule_rel(R.emulate_three_product(other, xo, go, drop_xl_block=0), ro)[0] > R.BAR_3P


def test_a_wrong_scale_exponent_overflows_fp16():
    """gscale = 1e4: the exponents put every channel's maximum into [2^13, 2^14).  One step more leaves two binades of headroom
    by design (the result stays finite and exact to fp16); a channel that takes its NEIGHBOUR's exponent -- an index off by one
    at the boundary between the small and the large channels -- sends its operand to inf."""
    name = "s2_entry"
    x, g = R.draw_wgrad(name, 1e4, seed=1)
    s = R.scale_exponents(R.channel_absmax(g))
    top = R.scaled_f16_operand(g, s).abs().amax((0, 2, 3))
    assert bool((top >= 2.0 ** 13).all()) and bool((top < 2.0 ** 14).all())
    assert bool(torch.isfinite(R.scaled_f16_operand(g, s + 1)).all())
    c = g.shape[1] // 4
    bad = s.clone()
    bad[c] = s[c - 1]
    assert int(bad[c]) >= int(s[c]) + 3
    op = R.scaled_f16_operand(g, bad)
    assert bool(torch.isinf(op[:, c]).any()) and bool(torch.isfinite(op[:, :c]).all()) and bool(torch.isfinite(op[:, c + 1:]).all())
    assert not bool(torch.isfinite(R.emulate_one_pass(name, x, g, bad)[:, :, c]).all())
    # an all-zero channel: exponent 0, operand and gradient exactly 0
    g0 = g.clone()
    g0[:, 5] = 0
    s0 = R.scale_exponents(R.channel_absmax(g0))
    assert int(s0[5]) == 0 and not bool(R.emulate_one_pass(name, x, g0)[:, :, 5].any())
