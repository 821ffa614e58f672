"""Host tests of tests/head_ref.py (no GPU): every closed form against fp64 autograd -- F.linear, F.layer_norm, F.normalize and
the fixed-grid solver of oracle/ode.py -- to 1e-12; the floors the bars of tests/test_gpu_head_kernels.py are built from,
evaluated at that file's cases; and, for every bar, a deliberately wrong variant of the same closed form (in fp64) that must
exceed it at those cases -- a bar that a wrong kernel would pass is no bar.

Floors on the CPU: the three-product form 3.0e-6 .. 6.7e-6 per row for K = 32 .. 1024 (the dropped lo*lo term; the larger ones
on rows a ReLU or tanh shortened), so the Linear bars come to 1.2e-5 .. 2e-5; the float32 row-wise forms 3e-8 .. 2e-7."""
import pytest
import torch
import torch.nn.functional as F

import head_ref as H
from oracle import ode

TIGHT = 1e-12
_ACT = {"id": lambda v: v, "relu": torch.relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid}


def _close(got, ref, what):
    got, ref = got.detach().double(), ref.detach().double()
    err = float((got - ref).norm() / ref.norm().clamp_min(1e-300))
    assert err < TIGHT, "%s: %.3e" % (what, err)


def _leaf(t):
    return t.double().clone().requires_grad_(True)


# ------------------------------------------------------------------------------------------------------- pinned to autograd
@pytest.mark.parametrize("act", H.ACTS)
def test_linear_forms_match_autograd(act):
    x, a1, a2, w, bias, gy = H.draw_linear(5, 96, 40, seed=1)
    xl, wl, bl = _leaf(x), _leaf(w), _leaf(bias)
    y = _ACT[act](F.linear(xl + a1.double() + a2.double(), wl, bl))
    _close(H.linear(x, a1, a2, w, bias, act), y, "linear " + act)
    _close(H.linear(x, None, None, w, None, act), _ACT[act](F.linear(x.double(), w.double())), "linear without adds / bias")
    y.backward(gy.double())
    gx, gw, gb = H.linear_bwd(x.double() + a1.double() + a2.double(), y.detach(), gy, w, act)
    _close(gx, xl.grad, "gx"), _close(gw, wl.grad, "gw"), _close(gb, bl.grad, "gb")


@pytest.mark.parametrize("variant", list(H.LN_VARIANTS))
def test_layernorm_forms_match_autograd(variant):
    affine, relu, with_res, _ = H.LN_VARIANTS[variant]
    x, res, gy, gamma, beta = H.draw_rows(5, 100, seed=2)
    xl, rl, gl, bl = _leaf(x), _leaf(res), _leaf(gamma), _leaf(beta)
    y = F.layer_norm(xl, (100,), gl if affine else None, bl if affine else None, H.LN_EPS)
    if with_res:
        y = y + rl
    if relu:
        y = torch.relu(y)
    mine = H.layernorm(x, gamma if affine else None, beta if affine else None, H.LN_EPS, relu, res if with_res else None)
    _close(mine, y, "layernorm")
    y.backward(gy.double())
    gx, gres, gg, gb = H.layernorm_bwd(x, gamma if affine else None, y.detach(), gy, H.LN_EPS, relu)
    _close(gx, xl.grad, "gx")
    if with_res:
        _close(gres, rl.grad, "gres")
    if affine:
        _close(gg, gl.grad, "ggamma"), _close(gb, bl.grad, "gbeta")
    tg, tb, mg = H.layernorm_param_terms(x, y.detach(), gy, H.LN_EPS, relu)
    _close(tg.sum(0), gg, "the terms of ggamma"), _close(tb.sum(0), gb, "the terms of gbeta")
    assert bool((mg * (1 + 1e-12) >= tg.abs()).all())


def test_l2normalize_forms_match_autograd_and_the_clamped_row():
    x, _, gy, _, _ = H.draw_rows(5, 100, seed=3, zero_row=2)
    xl = _leaf(x)
    y = F.normalize(xl, dim=1, eps=H.L2_CLAMP)
    _close(H.l2normalize(x), y, "l2normalize")
    y.backward(gy.double())
    gx = H.l2normalize_bwd(x, gy)
    live = [0, 1, 3, 4]
    _close(gx[live], xl.grad[live], "gx of the live rows")
    assert not bool(H.l2normalize(x)[2].any())
    assert torch.equal(gx[2], gy[2].double() / 1e-12), "a clamped row: gx = gy / 1e-12"
    _close(gx[2], xl.grad[2], "autograd on the clamped row")
    tiny = torch.full((1, 8), 1e-14)
    assert torch.equal(H.l2normalize_bwd(tiny, gy[:1, :8]), gy[:1, :8].double() / 1e-12)


def test_wsum_and_dot():
    g = torch.Generator().manual_seed(4)
    xs = [torch.randn(7, 9, generator=g) for _ in range(6)]
    ws = [torch.randn(1, generator=g) for _ in range(6)]
    ws[2] = None
    ref = sum(x.double() * (1.0 if w is None else w.double()) for x, w in zip(xs, ws))
    _close(H.wsum(xs, ws), ref, "wsum")
    _close(H.wsum(xs[:1]), xs[0], "wsum of one term")
    _close(H.dot(xs[0], xs[1]), torch.dot(xs[0].double().reshape(-1), xs[1].double().reshape(-1)), "dot")
    assert float(H.dot(xs[0][:0], xs[1][:0])) == 0.0


@pytest.mark.parametrize("act", H.FCODE_ACTS)
@pytest.mark.parametrize("method,step", H.FCODE_SOLVERS)
def test_fcode_forms_match_the_oracle_solver_and_its_autograd(method, step, act):
    x, a1, a2, w, bias, gy = H.draw_fcode(3, seed=5)
    dts = H.grid_dts(step)
    assert len(dts) == {1.0: 1, 0.1: 10, 0.3: 4, 0.25: 4}[step] and abs(sum(dts) - 1) < 1e-6
    xl, wl, bl = _leaf(x.double() + a1.double()), _leaf(w), _leaf(bias)
    ref = ode.odeint_fixed(lambda v: ode.fc(v, wl, bl, act), xl, method, step, dt_dtype=torch.float32)
    y, traj = H.fcode_traj(x, w, bias, act, method, dts, add1=a1)
    _close(y, ref, "fcode y")
    nst = H.stages(method)
    assert tuple(traj.shape) == (len(dts), 1 + nst, 3, 256)
    assert torch.equal(traj[0, 0], x.double() + a1.double())
    _close(traj[0, 1], ode.fc(traj[0, 0], w.double(), bias.double(), act), "k1 of the first step")
    if len(dts) > 1:            # the next state is the step's update of the recorded stages
        bw = H.TABLEAUS[method][1]
        _close(traj[1, 0], traj[0, 0] + dts[0] * sum(bi * traj[0, 1 + i] for i, bi in enumerate(bw)), "the second state")
    ref.backward(gy.double())
    gx, gw, gb = H.fcode_bwd(traj, gy, w, act, method, dts)
    _close(gx, xl.grad, "gx"), _close(gw, wl.grad, "gw"), _close(gb, bl.grad, "gb")


def test_three_product_is_the_sum_of_the_three_partial_products():
    x, _, _, w, _, _ = H.draw_linear(4, 64, 8, seed=6)
    xh, xl = H.bf16_pair(x)
    wh, wl = H.bf16_pair(w)
    assert torch.equal(xh.float().bfloat16().double(), xh) and torch.equal(xl.float().bfloat16().double(), xl)
    full = (xh + xl) @ (wh + wl).t()
    assert torch.allclose(H.three_product(x, w), full - xl @ wl.t(), rtol=0, atol=1e-15)
    assert float((xh + xl - x.double()).abs().max()) <= 2.0 ** -16 * float(x.abs().max())


# ------------------------------------------------------------------------------------------- floors, bars, discrimination
def test_the_case_tables_cover_what_they_claim():
    cases = H.linear_fwd_cases()
    assert len(cases) == 24 and {(b, k) for b, k, *_ in cases} == {(b, k) for b in H.LINEAR_B for k in H.LINEAR_K}
    for k in H.LINEAR_K:
        mine = [c for c in cases if c[1] == k]
        assert {c[3] for c in mine} == set(H.ACTS), "every K meets every activation"
        assert {c[2] for c in mine} == {256, 512}
    assert {c[4] for c in cases} == {0, 1, 2} and {c[5] for c in cases} == {True, False}
    assert {(c[1], c[5]) for c in cases} >= {(288, False), (320, False)}, "bias == NULL on the ragged second chunk"
    fc = H.fcode_cases()
    assert len(fc) == 16 and len({(m, s, a) for _, m, s, a in fc}) == 16
    for b in H.LINEAR_B:
        mine = [c for c in fc if c[0] == b]
        assert {(m, s) for _, m, s, _ in mine} == set(H.FCODE_SOLVERS) and {a for *_, a in mine} == set(H.FCODE_ACTS)


@pytest.mark.parametrize("b,k,n,act,adds,with_bias", H.linear_fwd_cases())
def test_linear_forward_floor_and_bar(b, k, n, act, adds, with_bias):
    """The three-product floor per row, and what the bar catches: weights rounded to ONE bf16 (the lo plane ignored) or an add
    operand forgotten are errors of 1e-3 and more."""
    x, a1, a2, w, bias, _ = H.draw_linear(b, k, n)
    a1, a2, bias = (a1 if adds >= 1 else None), (a2 if adds == 2 else None), (bias if with_bias else None)
    ref, bars, floor = H.linear_fwd_bars(x, a1, a2, w, bias, act)
    print("K %d act %s: floor %.3e .. %.3e, bar %.3e .. %.3e" % (k, act, float(floor.min()), float(floor.max()),
                                                                 float(bars.min()), float(bars.max())))
    assert 1e-6 < float(floor.min()) and float(floor.max()) < 1e-5
    assert float(bars.max()) <= H.CEIL_LINEAR_FWD
    hi_only = H.linear(x, a1, a2, w.bfloat16().float(), bias, act)
    assert bool((H.per_row_rel(hi_only, ref) > bars).all()), "weights as one bf16 plane pass the bar"
    if adds:
        assert bool((H.per_row_rel(H.linear(x, None, a2, w, bias, act), ref) > bars).all()), "a forgotten add passes the bar"


@pytest.mark.parametrize("act", H.ACTS)
@pytest.mark.parametrize("b,k,n", H.LINEAR_BWD_SHAPES)
def test_linear_backward_bars_catch_a_dropped_batch_row(b, k, n, act):
    x, _, _, w, bias, gy = H.draw_linear(b, k, n)
    y = H.linear(x, None, None, w, bias, act).float()
    (gx, gw, gb), bx, bw, gz = H.linear_bwd_bars(x, y, gy, w, act)
    print("(%d, %d, %d) %s: gx bars %.3e .. %.3e, gw bars %.3e .. %.3e" % (b, k, n, act, float(bx.min()), float(bx.max()),
                                                                         float(bw.min()), float(bw.max())))
    assert float(bx.max()) <= H.CEIL_DATA and float(bw.max()) <= H.CEIL_DATA
    assert H.sum_check(gb, gz)[1]
    _, gw_bad, gb_bad = H.linear_bwd(x, y, gy, w, act, drop_row=b - 1)
    rel = H.per_row_rel(gw_bad, gw)
    hit = gz[b - 1] != 0                  # (a unit the ReLU switched off in that batch row loses nothing)
    assert int(hit.sum()) >= n // 4 and not bool(rel[~hit].any())
    assert bool((rel[hit] > bw[hit]).all()), "gw with a batch row dropped passes the bar in some row"
    assert not H.sum_check(gb_bad, gz)[1], "gb with a batch row dropped passes"
    # act' from the output: forgetting it is caught wherever it is not 1
    if act != "id":
        plain = H.linear_bwd(x, y, gy, w, "id")[0]
        assert bool((H.per_row_rel(plain, gx) > bx).any())


@pytest.mark.parametrize("b", H.LN_B)
@pytest.mark.parametrize("d", H.LN_D)
def test_rowwise_floors_and_bars(d, b):
    """LayerNorm and L2-normalise at every (d, b) of the GPU tests: the float32 floors, and the wrong variants -- LayerNorm
    backward without the xhat * s2 term, ggamma / gbeta without the ReLU mask -- above the bars."""
    x, res, gy, gamma, beta = H.draw_rows(b, d)
    for name, (affine, relu, with_res, _) in H.LN_VARIANTS.items():
        ga, be, rs = (gamma if affine else None), (beta if affine else None), (res if with_res else None)
        y64 = H.layernorm(x, ga, be, H.LN_EPS, relu, rs)
        bar, floor = H.rowwise_bar(H.layernorm(x, ga, be, H.LN_EPS, relu, rs, dtype=torch.float32), y64, H.CEIL_ROW_FWD)
        y = y64.float()
        ref = H.layernorm_bwd(x, ga, y, gy, H.LN_EPS, relu)
        f32 = H.layernorm_bwd(x, ga, y, gy, H.LN_EPS, relu, dtype=torch.float32)
        gbar, gfloor = H.rowwise_bar(f32[0], ref[0], H.CEIL_ROW_BWD)
        print("layernorm d %d b %d %s: forward floor %.3e bar %.3e, gx floor %.3e bar %.3e" % (d, b, name, floor, bar, gfloor, gbar))
        assert floor < 5e-7 and gfloor < 2e-6 and bar < H.CEIL_ROW_FWD and gbar < H.CEIL_ROW_BWD
        wrong = H.layernorm_bwd(x, ga, y, gy, H.LN_EPS, relu, drop_s2=True)[0]
        assert bool((H.per_row_rel(wrong, ref[0]) > gbar).all()), "gx without the xhat * s2 term passes the bar"
        tg, tb, mg = H.layernorm_param_terms(x, y, gy, H.LN_EPS, relu)
        assert H.sum_check(f32[2], tg, mg)[1] and H.sum_check(f32[3], tb)[1], "the float32 sums miss their own bar"
        if relu:
            _, _, gg_bad, gb_bad = H.layernorm_bwd(x, ga, y, gy, H.LN_EPS, relu, mask_params=False)
            assert bool((y <= 0).any())
            assert not H.sum_check(gg_bad, tg, mg)[1] and not H.sum_check(gb_bad, tb)[1], "ggamma / gbeta without the mask pass"
    y64 = H.l2normalize(x)
    bar, floor = H.rowwise_bar(H.l2normalize(x, torch.float32), y64, H.CEIL_ROW_FWD)
    ref = H.l2normalize_bwd(x, gy)
    gbar, gfloor = H.rowwise_bar(H.l2normalize_bwd(x, gy, torch.float32), ref, H.CEIL_ROW_BWD)
    print("l2normalize d %d b %d: forward floor %.3e bar %.3e, gx floor %.3e bar %.3e" % (d, b, floor, bar, gfloor, gbar))
    assert floor < 5e-7 and gfloor < 2e-6
    no_projection = gy.double() / x.double().norm(dim=1, keepdim=True)
    assert bool((H.per_row_rel(no_projection, ref) > gbar).all()), "gx without the y (y . gy) term passes the bar"


def test_wsum_and_dot_floors():
    g = torch.Generator().manual_seed(8)
    xs = [torch.randn(255, generator=g) for _ in range(6)]
    ws = [torch.randn(1, generator=g) for _ in range(6)]
    ref = H.wsum(xs, ws)
    bar, floor = H.rowwise_bar(H.wsum(xs, ws, torch.float32)[None], ref[None], H.CEIL_ROW_FWD)
    assert floor < 5e-7
    assert H.worst_row(H.wsum(xs[:5], ws[:5])[None], ref[None]) > bar, "a weighted sum that loses its last term passes"
    ws[1] = None
    assert H.worst_row(H.wsum(xs, [ws[0], None, None] + ws[3:])[None], H.wsum(xs, ws)[None]) > bar, "a NULL weight that ends the list"


@pytest.mark.parametrize("b,method,step,act", H.fcode_cases())
def test_fcode_bars_catch_the_classic_rk4_and_a_dropped_row(b, method, step, act):
    """The FCODE bars at the GPU cases.  Forward: the classic rk4 weights in place of the 3/8 rule change every recorded stage
    from k2 on (for act = id the END state is the same polynomial in dt W: only the trajectory check tells the two apart).
    Backward: gw / gb with one batch row dropped."""
    x, a1, a2, w, bias, gy = H.draw_fcode(b)
    dts = H.grid_dts(step)
    y, traj, by, bt = H.fcode_fwd_bars(x, a1, a2, w, bias, act, method, dts)
    print("fcode b %d %s %.2f %s: y bars %.3e .. %.3e, traj bars %.3e .. %.3e" % (b, method, step, act, float(by.min()),
                                                                                  float(by.max()), float(bt.min()), float(bt.max())))
    assert float(by.max()) <= H.CEIL_DATA and float(bt.max()) <= H.CEIL_DATA
    if method == "rk4":
        y_bad, traj_bad = H.fcode_traj(x, w, bias, act, "rk4_classic", dts, a1, a2)
        rel = H.per_row_rel(traj_bad, traj).reshape(bt.shape)
        assert bool((rel[:, 2:] > bt[:, 2:]).all()), "a classic-rk4 trajectory passes the bar"
    t32 = traj.float()
    (gx, gw, gb), bx, bw, bb = H.fcode_bwd_bars(t32, gy, w, act, method, dts)
    print("    gx bars %.3e .. %.3e, gw bars %.3e .. %.3e, gb bar %.3e" % (float(bx.min()), float(bx.max()), float(bw.min()),
                                                                         float(bw.max()), bb))
    assert float(bx.max()) <= H.CEIL_DATA and float(bw.max()) <= H.CEIL_PARAM and bb <= H.CEIL_PARAM
    _, gw_bad, gb_bad = H.fcode_bwd(t32, gy, w, act, method, dts, drop_row=b - 1)
    rel = H.per_row_rel(gw_bad, gw)
    hit = (gw_bad - gw).norm(dim=1) > 0   # (a unit whose act' is zero in that batch row at every stage loses nothing)
    assert int(hit.sum()) >= 64 and bool((rel[hit] > bw[hit]).all()), "gw with a batch row dropped passes"
    assert H.worst_row(gb_bad[None], gb[None]) > bb, "gb with a batch row dropped passes"
    if method == "rk4":
        gw_bad = H.fcode_bwd(t32, gy, w, act, "rk4_classic", dts)[1]
        assert bool((H.per_row_rel(gw_bad, gw) > bw).any()), "the classic-rk4 backward passes the gw bar"
