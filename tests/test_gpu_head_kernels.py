"""-m gpu: the row-wise descriptor head kernel by kernel against the fp64 closed forms of tests/head_ref.py (pinned to fp64
autograd by tests/test_head_ref.py, which also evaluates every floor and bar used here on the CPU and shows that each bar
discriminates).  Entry points are called directly (or through the thin ops.* wrappers), no modules.

Rules of the file: every output lies between poisoned guard regions and is allocated with spare rows -- the guards and the rows
at and beyond b must keep the poison; refusals return the header's AGP_E_BADARG and write nothing; a backward kernel receives the
fp64 reference's forward outputs rounded to fp32 (y for Linear and LayerNorm, traj for FCODE), so both sides take act' and the
ReLU mask from identical numbers and no element is left out of any comparison.

Kernels and the branches reached
  agp_linear_fwd      b 1 / 16 / 17 / 33 (one row, a full block, a block with 15 dead rows, three blocks); K 32 .. 1024: nks = 1, 3, 8
                      (one whole fetch chunk), 9 and 10 (the ragged second chunk: the ks clamp and the k0 + j < nks guard), 32 = MAXK
                      (66 KB of LDS); N 256 / 512; every activation; 0, 1, 2 add operands; bias == NULL.
  agp_linear_bwd      n % 32 != 0 (zero-padded gz columns: 100, 40), k not a multiple of 64 (96, 320) in gemm_tn_f32_kernel, b > 32 in
                      colsum_kernel (33, 70), kp > k (gx rows 256 / 512 wide), each output switched off, a NaN workspace.
  agp_layernorm_*     d 32 (half a wave idle) / 64 / 100 (ragged) / 256 / 4096 (the limit; 64 column blocks of the parameter kernel);
                      b 1 / 3 / 4 / 5 / 9 (dead waves in the last block; 1 .. 3 rows per wave of the parameter kernel); gamma / beta
                      NULL, relu, res / gres, ggamma / gbeta NULL; ggamma / gbeta bit-equal over two calls.
  agp_l2normalize_*   the same d and b; an all-zero row: forward exact zeros, backward the clamped branch gy / 1e-12f.
  agp_wsum_fwd        1 .. 6 terms, a NULL weight between two given ones, n 1 / 255 / 256 * 2048 + 17 (beyond the grid cap: the stride
                      loop's second trip); ops.wsum's chaining at 7 and 12 terms.  agp_dot_f32: n 0 / 1 / 1023 / 1025 / 100000.
  agp_fcode_fwd/_bwd  every solver (euler 1 and 10 steps, midpoint 4, rk4 4) with every activation, b through a Latin square;
                      traj recorded and every slot checked; backward from the reference trajectory with a NaN workspace (b = 1, 17,
                      33: the dead rows of a block must be written as zeros) and with gw / gb NULL.
  agp_vecprog_run     LINEAR from memory K 32 .. 256 with / without scale, from registers with both adds, dst == src; FCODE; LAYERNORM;
                      L2NORM with a zero row; WSUM of 1 and 6; exactly AGP_VECPROG_MAXOPS ops.  Also against the per-op kernels.
  agp_vecprog_run2    a rider with fewer (5) and with more (33) rows than program A (17, with an FCODE): bit-equal to solo runs.

Bars: head_ref's -- min(4 x floor, ceiling); floors on the CPU: three-product 3.0e-6 .. 6.7e-6 per row, float32 row-wise forms
3e-8 .. 2e-7; ceilings 2e-5 (Linear forward), 1e-4 (FCODE forward, data gradients, row-wise backward), 1e-3 (FCODE parameter
gradients), 1e-5 (row-wise forward); tanh / sigmoid: the ceiling.  Column sums: 1e-5 of the sum of the absolute terms.
Two bars depart from the issue's wording, both to the looser side:
  * ggamma is held to 1e-5 of sum |g| (|x| + |mean|) rstd, not of sum |g xhat| (1x to 5x looser).  A term g (x - mean) rstd is a
    difference: where x is close to the row's mean, float32 loses 2^-24 of |x| + |mean|, not of the term, and the float32 closed
    form itself misses 1e-5 of sum |g xhat| in 10 of the 75 cases (by up to 1.5e-3).  The looser bound still catches the missing
    mask (tests/test_head_ref.py).
  * every gw row of an FCODE case takes the worst row's floor of its case, not its own (head_ref.fcode_bwd_bars says why).  This is
    weaker than a per-row floor: at b = 1 the rows' own floors run from 5e-8 over a median of 1e-6 to 7e-5, so most rows are held
    to 50 .. 200 times their own floor (bars up to 3.7e-4; the ceiling is 1e-3).  An error of a few percent in a row is still caught.

MEASURED on an MI355X (the worst row over all cases, beside the bar of that row):
  agp_linear_fwd       6.7e-6 (bar 2e-5) for id / relu, 1.02 x the three-product floor of the same row at the most: the kernel IS
                       the floor, the dropped lo*lo term.  That is a third of the 2e-5 ceiling -- above a quarter of it, and it
                       cannot be less.  tanh / sigmoid 5.8e-6 against the ceiling 2e-5 (also above a quarter: the same floor).
  agp_linear_bwd       gx 6.0e-6 (bar 2.4e-5), gw 2.0e-7 (bar 6.7e-7), gb 1.2e-7 of the sum of its absolute terms (bar 1e-5).
  agp_layernorm_*      y 1.7e-7 (bar 6.3e-7; 2.1 x the float32 floor at the most), gx 1.4e-7 (bar 4.2e-7; 1.7 x), gres bit-equal,
                       ggamma 2.6e-7 and gbeta 1.4e-7 of the sums of their terms (bar 1e-5), bit-equal over two calls.
  agp_l2normalize_*    y 8.2e-8 (bar 2.6e-7), gx 8.8e-8 (bar 3.5e-7); the zero row exact / gy / 1e-12f to the bit.
  agp_wsum_fwd         6.5e-8 (bar 3.0e-7, 0.9 x the floor).  agp_dot_f32 1.4e-7 (bar 2.4e-7: the floor clamp 2^-24, x 4).
  agp_fcode_fwd        y 2.9e-6 (id / relu: bar 1.1e-5; tanh / sigmoid: the ceiling 1e-4), traj 5.5e-6 (bar 2.1e-5) and 6.5e-6 (1e-4).
  agp_fcode_bwd        gx 3.1e-6 (bar 1.2e-5), gw 9.1e-5 at b = 1 (bar 3.7e-4; 4.7e-6 and less for b >= 16), gb 1.6e-6 (bar 6.3e-6).
  agp_vecprog_run      LINEAR 6.4e-6 (bar 2e-5; 1.04 x the floor) and 1.9e-7 from agp_linear_fwd; FCODE 2.9e-6, bit-equal to
                       agp_fcode_fwd; LAYERNORM 3.4e-7 (bar 7.5e-7) and 3.5e-7 from agp_layernorm_fwd; L2NORM 1.3e-7 (bar 2.4e-7);
                       WSUM 7.2e-8 (bar 3.7e-7), bit-equal to agp_wsum_fwd.
  agp_vecprog_run2     bit-equal to the solo runs, with the smaller and with the larger rider.
"""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest
import torch

import head_ref as H

pytestmark = pytest.mark.gpu

GUARD = 4096                     # elements before and after every output
POISON = 0x7FC0BEEF              # a quiet NaN with a payload: nothing a kernel stores
SPARE_ROWS = 32                  # rows behind the b a kernel is given: two more 16-row blocks


def _header_code(name):
    """An AGP_* return code as include/agplace_hip.h defines it."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    m = re.search(r"#define %s (\d+)" % name, open(os.path.join(root, "include", "agplace_hip.h")).read())
    assert m, "%s not found in the header" % name
    return int(m.group(1))


BADARG = _header_code("AGP_E_BADARG")
MAXOPS = _header_code("AGP_VECPROG_MAXOPS")


def _L():
    from agplace_amd import _lib
    return _lib.load()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ok(rc, what):
    assert rc == 0, "%s returned %d" % (what, rc)


def _act(name):
    from agplace_amd import _lib
    return _lib.ACT[name]


def _ode(name):
    from agplace_amd import _lib
    return _lib.ODE[name]


class Out:
    """An fp32 output [rows, cols] in the middle of a poisoned buffer, with SPARE_ROWS poisoned rows behind it."""

    def __init__(self, rows, cols, dev, spare=SPARE_ROWS):
        self.rows, self.cols = rows, cols
        total = (rows + spare) * cols
        self.buf = torch.full((GUARD + total + GUARD,), POISON, dtype=torch.int32, device=dev)
        self.t = self.buf[GUARD:GUARD + total].view(torch.float32).view(rows + spare, cols)

    def ptr(self):
        return self.t.data_ptr()

    def value(self, what):
        """the [rows, cols] result on the CPU; asserts that nothing else was written and that no element of it was left out"""
        torch.cuda.synchronize()
        live = slice(GUARD, GUARD + self.rows * self.cols)
        assert bool((self.buf[:GUARD] == POISON).all()), "%s: the guard in front was written" % what
        assert bool((self.buf[live.stop:] == POISON).all()), "%s: rows at or beyond b, or the guard behind, were written" % what
        assert not bool((self.buf[live] == POISON).any()), "%s: elements of the output were not written" % what
        return self.t[:self.rows].cpu()

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf == POISON).all())


def _nan(nbytes, dev):
    """a NaN-poisoned workspace of at least nbytes"""
    return torch.full(((int(nbytes) + 3) // 4,), float("nan"), dtype=torch.float32, device=dev)


def _rows_ok(got, ref, bars, what, floor=None):
    """per-row rel_l2 against per-row bars: prints the worst figure, asserts every row"""
    rel = H.per_row_rel(got, ref)
    bars = torch.as_tensor(bars, dtype=torch.float64).reshape(-1)
    bars = bars.expand_as(rel) if bars.numel() == 1 else bars
    assert bars.shape == rel.shape
    i = int((rel / bars).argmax()) if rel.numel() else 0
    extra = "" if floor is None else ", %.2f x floor" % float((rel / torch.as_tensor(floor).reshape(-1).clamp_min(H.ONE_ROUNDING)).max())
    print("%s: worst row %.3e (bar %.3e%s)" % (what, float(rel[i]) if rel.numel() else 0.0, float(bars[i]) if rel.numel() else 0.0, extra))
    assert bool((rel <= bars).all()), "%s: row %d has %.3e (bar %.3e)" % (what, i, float(rel[i]), float(bars[i]))
    assert not bool(torch.isnan(got).any()), "%s: NaN" % what


def _sum_ok(got, terms, what, mags=None):
    worst, ok = H.sum_check(got, terms, mags)
    print("%s: error / sum |terms| %.3e (bar %.1e)" % (what, worst, H.SUM_BAR))
    assert ok, "%s: %.3e of the sum of the absolute terms" % (what, worst)


def _weights(w, bias, dev, transpose=False):
    from agplace_amd import ops
    return ops.LinearWeights(w.to(dev), None if bias is None else bias.to(dev), with_transpose=transpose)


def _d(t, dev):
    return None if t is None else t.float().contiguous().to(dev)


# ------------------------------------------------------------------------------------------------------------ agp_linear_fwd
@pytest.mark.parametrize("b,k,n,act,adds,with_bias", H.linear_fwd_cases())
def test_linear_fwd(dev, b, k, n, act, adds, with_bias):
    x, a1, a2, w, bias, _ = H.draw_linear(b, k, n)
    a1, a2, bias = (a1 if adds >= 1 else None), (a2 if adds == 2 else None), (bias if with_bias else None)
    ref, bars, floor = H.linear_fwd_bars(x, a1, a2, w, bias, act)
    lw = _weights(w, bias, dev)
    y = Out(b, n, dev)
    xd, a1d, a2d = _d(x, dev), _d(a1, dev), _d(a2, dev)
    _ok(_L().agp_linear_fwd(_ptr(xd), _ptr(a1d), _ptr(a2d), _ptr(lw.w_hi), _ptr(lw.w_lo), _ptr(lw.bias), b, k, n, _act(act), y.ptr(),
                            _stream()), "agp_linear_fwd")
    _rows_ok(y.value("y"), ref, bars, "linear_fwd b %d K %d N %d %s adds %d bias %d" % (b, k, n, act, adds, with_bias), floor)


def test_linear_fwd_refusals(dev):
    x, _, _, w, bias, _ = H.draw_linear(4, 1056, 256)
    lw = _weights(w, bias, dev)
    xd = _d(x, dev)
    y = Out(4, 256, dev)
    call = lambda k, n, act: _L().agp_linear_fwd(_ptr(xd), None, None, _ptr(lw.w_hi), _ptr(lw.w_lo), _ptr(lw.bias), 4, k, n, act, y.ptr(),
                                                 _stream())
    assert call(48, 256, 0) == BADARG, "k % 32"
    assert call(1056, 256, 0) == BADARG, "k > 1024"
    assert call(64, 128, 0) == BADARG, "n % 256"
    assert call(64, 256, -1) == BADARG and call(64, 256, 4) == BADARG, "act out of range"
    assert y.untouched(), "a refused call wrote"


# ------------------------------------------------------------------------------------------------------------ agp_linear_bwd
def _linear_bwd_call(dev, lw, xd, yd, gyd, b, k, n, act, want, ws=None, ws_bytes=None):
    """-> (rc, gx Out [b, kp], gw Out [n, k], gb Out [1, n]); want: (gx, gw, gb) switches"""
    L = _L()
    kp = (k + 255) // 256 * 256
    need = int(L.agp_linear_bwd_workspace_bytes(b, k, n))
    assert need == b * ((n + 31) // 32 * 32) * 4
    ws = _nan(need, dev) if ws is None else ws
    gx, gw, gb = Out(b, kp, dev), Out(n, k, dev, spare=4), Out(1, n, dev, spare=1)
    rc = L.agp_linear_bwd(_ptr(xd), _ptr(yd), _ptr(gyd), _ptr(lw.wt_hi), _ptr(lw.wt_lo), b, k, n, _act(act), gx.ptr() if want[0] else None,
                          gw.ptr() if want[1] else None, gb.ptr() if want[2] else None, _ptr(ws), need if ws_bytes is None else ws_bytes,
                          _stream())
    return rc, gx, gw, gb


@pytest.mark.parametrize("act", H.ACTS)
@pytest.mark.parametrize("b,k,n", H.LINEAR_BWD_SHAPES)
def test_linear_bwd(dev, b, k, n, act):
    x, _, _, w, bias, gy = H.draw_linear(b, k, n)
    y = H.linear(x, None, None, w, bias, act).float()
    (rx, rw, rb), bx, bw, gz = H.linear_bwd_bars(x, y, gy, w, act)
    lw = _weights(w, bias, dev, transpose=True)
    xd, yd, gyd = _d(x, dev), _d(y, dev), _d(gy, dev)
    what = "linear_bwd (%d, %d, %d) %s" % (b, k, n, act)
    rc, gx, gw, gb = _linear_bwd_call(dev, lw, xd, yd, gyd, b, k, n, act, (True, True, True))
    _ok(rc, "agp_linear_bwd")
    full = gx.value("gx"), gw.value("gw"), gb.value("gb")
    assert not bool(full[0][:, k:].any()), "%s: the padding columns of gx (W^T's zero rows) are not zero" % what
    _rows_ok(full[0][:, :k], rx, bx, what + " gx per batch row")
    _rows_ok(full[1], rw, bw, what + " gw per output row")
    _sum_ok(full[2][0], gz, what + " gb")
    for off in range(3):          # each output switched off in turn: the others are the same bits, the one left out is not written
        want = tuple(i != off for i in range(3))
        rc, gx, gw, gb = _linear_bwd_call(dev, lw, xd, yd, gyd, b, k, n, act, want)
        _ok(rc, "agp_linear_bwd")
        for i, o in enumerate((gx, gw, gb)):
            if want[i]:
                assert torch.equal(o.value("output %d" % i), full[i]), "%s: output %d changes when output %d is switched off" % (what, i, off)
            else:
                assert o.untouched(), "%s: output %d written although it was switched off" % (what, i)


def test_linear_bwd_refusals(dev):
    b, k, n = 4, 64, 64
    x, _, _, w, bias, gy = H.draw_linear(b, k, n)
    lw = _weights(w, bias, dev, transpose=True)
    y = H.linear(x, None, None, w, bias, "relu").float()
    xd, yd, gyd = _d(x, dev), _d(y, dev), _d(gy, dev)
    need = int(_L().agp_linear_bwd_workspace_bytes(b, k, n))
    ws = torch.full((need // 4 + 64,), POISON, dtype=torch.int32, device=dev)
    rc, gx, gw, gb = _linear_bwd_call(dev, lw, xd, yd, gyd, b, k, n, "relu", (True, True, True), ws=ws, ws_bytes=need - 4)
    assert rc == BADARG, "a short workspace"
    assert gx.untouched() and gw.untouched() and gb.untouched() and bool((ws == POISON).all())
    rc, gx, gw, gb = _linear_bwd_call(dev, lw, xd, None, gyd, b, k, n, "relu", (True, True, True), ws=ws)
    assert rc == BADARG, "act != id without y"
    assert gx.untouched() and gw.untouched() and gb.untouched() and bool((ws == POISON).all())
    big = torch.full((b * 1056 + 64,), POISON, dtype=torch.int32, device=dev)           # np = 1056 > 1024
    gyb = torch.zeros((b, 1056), dtype=torch.float32, device=dev)
    gxo = Out(b, 256, dev)
    rc = _L().agp_linear_bwd(_ptr(xd), None, _ptr(gyb), _ptr(lw.wt_hi), _ptr(lw.wt_lo), b, k, 1056, 0, gxo.ptr(), None, None, _ptr(big),
                             big.numel() * 4, _stream())
    assert rc == BADARG, "np > 1024"
    torch.cuda.synchronize()
    assert gxo.untouched() and bool((big == POISON).all())


# ------------------------------------------------------------------------------------------------------ LayerNorm, L2-normalise
@pytest.mark.parametrize("b", H.LN_B)
@pytest.mark.parametrize("d", H.LN_D)
def test_layernorm_fwd_and_bwd(dev, d, b):
    L = _L()
    x, res, gy, gamma, beta = H.draw_rows(b, d)
    xd, gyd = _d(x, dev), _d(gy, dev)
    for name, (affine, relu, with_res, want_params) in H.LN_VARIANTS.items():
        ga, be, rs = (gamma if affine else None), (beta if affine else None), (res if with_res else None)
        gad, bed, rsd = _d(ga, dev), _d(be, dev), _d(rs, dev)
        what = "layernorm d %d b %d %s" % (d, b, name)
        y64 = H.layernorm(x, ga, be, H.LN_EPS, relu, rs)
        bar, floor = H.rowwise_bar(H.layernorm(x, ga, be, H.LN_EPS, relu, rs, dtype=torch.float32), y64, H.CEIL_ROW_FWD)
        yo = Out(b, d, dev)
        _ok(L.agp_layernorm_fwd(_ptr(xd), _ptr(gad), _ptr(bed), _ptr(rsd), b, d, H.LN_EPS, int(relu), yo.ptr(), _stream()), "agp_layernorm_fwd")
        _rows_ok(yo.value("y"), y64, bar, what + " y", floor)
        y = y64.float()
        yd = _d(y, dev)
        rx, rres, rgg, rgb = H.layernorm_bwd(x, ga, y, gy, H.LN_EPS, relu)
        f32 = H.layernorm_bwd(x, ga, y, gy, H.LN_EPS, relu, dtype=torch.float32)
        gbar, gfloor = H.rowwise_bar(f32[0], rx, H.CEIL_ROW_BWD)
        params = []
        for _ in range(2):
            gx, gres = Out(b, d, dev), Out(b, d, dev)
            gg, gb = Out(1, d, dev, spare=1), Out(1, d, dev, spare=1)
            _ok(L.agp_layernorm_bwd(_ptr(xd), _ptr(gad), _ptr(yd), _ptr(gyd), b, d, H.LN_EPS, int(relu), gx.ptr(),
                                    gres.ptr() if with_res else None, gg.ptr() if want_params else None,
                                    gb.ptr() if want_params else None, _stream()), "agp_layernorm_bwd")
            _rows_ok(gx.value("gx"), rx, gbar, what + " gx", gfloor)
            if with_res:
                assert torch.equal(gres.value("gres").double(), rres), what + ": gres is not gy [y > 0] bit for bit"
            else:
                assert gres.untouched()
            if want_params:
                params.append((gg.value("ggamma")[0], gb.value("gbeta")[0]))
            else:
                assert gg.untouched() and gb.untouched()
        if want_params:
            tg, tb, mg = H.layernorm_param_terms(x, y, gy, H.LN_EPS, relu)
            _sum_ok(params[0][0], tg, what + " ggamma", mg)
            _sum_ok(params[0][1], tb, what + " gbeta")
            assert torch.equal(params[0][0], params[1][0]) and torch.equal(params[0][1], params[1][1]), \
                what + ": ggamma / gbeta differ between two calls (the kernel promises a fixed order)"


def test_layernorm_fwd_refuses_d_4097(dev):
    x = torch.zeros((2, 4097), dtype=torch.float32, device=dev)
    y = Out(2, 4097, dev)
    assert _L().agp_layernorm_fwd(_ptr(x), None, None, None, 2, 4097, H.LN_EPS, 0, y.ptr(), _stream()) == BADARG
    assert _L().agp_layernorm_fwd(_ptr(x), None, None, None, 0, 64, H.LN_EPS, 0, y.ptr(), _stream()) == BADARG
    assert y.untouched()


@pytest.mark.parametrize("b", H.LN_B)
@pytest.mark.parametrize("d", H.LN_D)
def test_l2normalize_fwd_and_bwd(dev, d, b):
    L = _L()
    zero = b // 2 if b > 1 else None                      # one all-zero row among live ones
    x, _, gy, _, _ = H.draw_rows(b, d, seed=1, zero_row=zero)
    xd, gyd = _d(x, dev), _d(gy, dev)
    what = "l2normalize d %d b %d" % (d, b)
    y64 = H.l2normalize(x)
    bar, floor = H.rowwise_bar(H.l2normalize(x, torch.float32), y64, H.CEIL_ROW_FWD)
    yo, gxo = Out(b, d, dev), Out(b, d, dev)
    _ok(L.agp_l2normalize_fwd(_ptr(xd), b, d, yo.ptr(), _stream()), "agp_l2normalize_fwd")
    _ok(L.agp_l2normalize_bwd(_ptr(xd), _ptr(gyd), b, d, gxo.ptr(), _stream()), "agp_l2normalize_bwd")
    y, gx = yo.value("y"), gxo.value("gx")
    _rows_ok(y, y64, bar, what + " y", floor)
    ref = H.l2normalize_bwd(x, gy)
    gbar, gfloor = H.rowwise_bar(H.l2normalize_bwd(x, gy, torch.float32), ref, H.CEIL_ROW_BWD)
    live = [i for i in range(b) if i != zero]
    _rows_ok(gx[live], ref[live], gbar, what + " gx", gfloor)
    assert not bool(torch.isnan(y).any()) and not bool(torch.isnan(gx).any()) and not bool(torch.isinf(gx).any())
    if zero is not None:
        assert not bool(y[zero].any()), what + ": the zero row does not normalise to exact zeros"
        want = gy[zero] / torch.tensor(1e-12, dtype=torch.float32)              # gy / 1e-12f in float32
        ulp = (torch.nextafter(want.abs(), torch.full_like(want, float("inf"))) - want.abs())
        assert bool(((gx[zero] - want).abs() <= ulp).all()), what + ": the clamped row is not gy / 1e-12f to 1 ulp"


# ----------------------------------------------------------------------------------------------------------------- wsum, dot
WSUM_N = (1, 255, 256 * 2048 + 17)


def _as_rows(v):
    """a flat vector as rows of 256 (+ one ragged last row) for the per-row rule"""
    n = v.numel()
    full = n // 256 * 256
    return ([v[:full].reshape(-1, 256)] if full else []) + ([v[full:].reshape(1, -1)] if n > full else [])


def _flat_ok(got, ref, f32, what):
    for g, r, f in zip(_as_rows(got), _as_rows(ref), _as_rows(f32)):
        bar, floor = H.rowwise_bar(f, r, H.CEIL_ROW_FWD)
        _rows_ok(g, r, bar, what, floor)


@pytest.mark.parametrize("n", WSUM_N)
def test_wsum_fwd(dev, n):
    L = _L()
    g = torch.Generator().manual_seed(n)
    xs = [torch.randn(n, generator=g) for _ in range(6)]
    ws = [torch.randn(1, generator=g) for _ in range(6)]
    xd, wd = [_d(x, dev) for x in xs], [_d(w, dev) for w in ws]
    for terms in (range(1, 7) if n < 1000 else (1, 6)):
        for null in ((None, 1) if terms >= 3 else (None,)):           # a NULL weight between two given ones counts 1
            w_cpu = [None if i == null else ws[i] for i in range(terms)]
            w_dev = [None if i == null else wd[i] for i in range(terms)]
            y = Out(1, n, dev, spare=1)
            px = [_ptr(t) for t in xd[:terms]] + [None] * (6 - terms)
            pw = [_ptr(t) for t in w_dev] + [None] * (6 - terms)
            _ok(L.agp_wsum_fwd(*px, *pw, n, y.ptr(), _stream()), "agp_wsum_fwd")
            _flat_ok(y.value("y")[0], H.wsum(xs[:terms], w_cpu), H.wsum(xs[:terms], w_cpu, torch.float32),
                     "wsum n %d, %d terms%s" % (n, terms, "" if null is None else ", weight 1 NULL"))
    y = Out(1, n, dev, spare=1)
    assert L.agp_wsum_fwd(None, *([None] * 11), n, y.ptr(), _stream()) == BADARG and y.untouched()


@pytest.mark.parametrize("terms", [7, 12])
def test_ops_wsum_chains_beyond_six_terms(dev, terms):
    from agplace_amd import ops
    g = torch.Generator().manual_seed(terms)
    xs = [torch.randn(255, generator=g) for _ in range(terms)]
    ws = [None if i == 3 else torch.randn(1, generator=g) for i in range(terms)]
    got = ops.wsum([_d(x, dev) for x in xs], [_d(w, dev) for w in ws]).cpu()
    _flat_ok(got, H.wsum(xs, ws), H.wsum(xs, ws, torch.float32), "ops.wsum of %d terms" % terms)


@pytest.mark.parametrize("n", [0, 1, 1023, 1025, 100000])
def test_dot_f32(dev, n):
    """positive terms: the sum is well conditioned and its relative error means something"""
    g = torch.Generator().manual_seed(n + 1)
    a, b = torch.randn(n, generator=g).abs() + 0.1, torch.randn(n, generator=g).abs() + 0.1
    ad, bd = (_d(a, dev), _d(b, dev)) if n else (torch.zeros(4, device=dev), torch.zeros(4, device=dev))
    outs = []
    for _ in range(2):
        o = Out(1, 1, dev, spare=1)
        _ok(_L().agp_dot_f32(_ptr(ad), _ptr(bd), n, o.ptr(), _stream()), "agp_dot_f32")
        outs.append(o.value("dot"))
    assert torch.equal(outs[0], outs[1]), "two calls differ"
    ref = H.dot(a, b)
    if n == 0:
        assert float(outs[0]) == 0.0
        return
    bar, floor = H.rowwise_bar(H.dot(a, b, torch.float32).reshape(1, 1), ref.reshape(1, 1), H.CEIL_ROW_FWD)
    _rows_ok(outs[0].reshape(1, 1), ref.reshape(1, 1), bar, "dot n %d" % n, floor)


# --------------------------------------------------------------------------------------------------------------------- FCODE
def _dt_array(dts):
    return (C.c_float * max(1, len(dts)))(*dts)


@pytest.mark.parametrize("b,method,step,act", H.fcode_cases())
def test_fcode_fwd_with_traj(dev, b, method, step, act):
    L = _L()
    x, a1, a2, w, bias, _ = H.draw_fcode(b)
    dts = H.grid_dts(step)
    y64, traj64, by, bt = H.fcode_fwd_bars(x, a1, a2, w, bias, act, method, dts)
    lw = _weights(w, bias, dev)
    nslot = 1 + H.stages(method)
    assert int(L.agp_fcode_traj_floats(b, _ode(method), len(dts))) == len(dts) * nslot * b * 256
    y, traj = Out(b, 256, dev), Out(len(dts) * nslot * b, 256, dev)
    xd, a1d, a2d = _d(x, dev), _d(a1, dev), _d(a2, dev)
    _ok(L.agp_fcode_fwd(_ptr(xd), _ptr(a1d), _ptr(a2d), _ptr(lw.w_hi), _ptr(lw.w_lo), _ptr(lw.bias), b, _act(act), _ode(method),
                        _dt_array(dts), len(dts), y.ptr(), traj.ptr(), _stream()), "agp_fcode_fwd")
    what = "fcode_fwd b %d %s %.2f %s" % (b, method, step, act)
    _rows_ok(y.value("y"), y64, by, what + " y")
    _rows_ok(traj.value("traj"), traj64.reshape(-1, 256), bt.reshape(-1), what + " traj (every slot)")
    y2 = Out(b, 256, dev)                                    # without traj: the same bits
    _ok(L.agp_fcode_fwd(_ptr(xd), _ptr(a1d), _ptr(a2d), _ptr(lw.w_hi), _ptr(lw.w_lo), _ptr(lw.bias), b, _act(act), _ode(method),
                        _dt_array(dts), len(dts), y2.ptr(), None, _stream()), "agp_fcode_fwd")
    assert torch.equal(y2.value("y"), y.value("y"))


@pytest.mark.parametrize("b,method,step,act", H.fcode_cases())
def test_fcode_bwd_from_the_reference_trajectory(dev, b, method, step, act):
    """The backward kernel alone: its input is head_ref.fcode_traj's trajectory rounded to fp32.  The workspace starts as NaN: with
    b = 1, 17 or 33 the GZ / S rows of a block's dead batch rows are summed into gw / gb, so they must have been written as zeros."""
    L = _L()
    x, a1, a2, w, bias, gy = H.draw_fcode(b)
    dts = H.grid_dts(step)
    _, traj64 = H.fcode_traj(x, w, bias, act, method, dts, a1, a2)
    t32 = traj64.float()
    (rx, rw, rb), bx, bw, bb = H.fcode_bwd_bars(t32, gy, w, act, method, dts)
    lw = _weights(w, bias, dev, transpose=True)
    need = int(L.agp_fcode_bwd_workspace_bytes(b, _ode(method), len(dts)))
    assert need == 2 * len(dts) * H.stages(method) * ((b + 15) // 16 * 16) * 256 * 4
    td, gyd = _d(t32, dev), _d(gy, dev)
    what = "fcode_bwd b %d %s %.2f %s" % (b, method, step, act)
    gx, gw, gb = Out(b, 256, dev), Out(256, 256, dev, spare=4), Out(1, 256, dev, spare=1)
    _ok(L.agp_fcode_bwd(_ptr(td), _ptr(gyd), _ptr(lw.wt_hi), _ptr(lw.wt_lo), b, _act(act), _ode(method), _dt_array(dts), len(dts), gx.ptr(),
                        gw.ptr(), gb.ptr(), _ptr(_nan(need, dev)), need, _stream()), "agp_fcode_bwd")
    vx, vw, vb = gx.value("gx"), gw.value("gw"), gb.value("gb")
    assert bool(torch.isfinite(vw).all()) and bool(torch.isfinite(vb).all()), what + ": gw / gb took in workspace rows nobody wrote"
    _rows_ok(vx, rx, bx, what + " gx per batch row")
    _rows_ok(vw, rw, bw, what + " gw per output row")
    _rows_ok(vb, rb[None], bb, what + " gb")
    gx2, gw2, gb2 = Out(b, 256, dev), Out(256, 256, dev, spare=4), Out(1, 256, dev, spare=1)
    _ok(L.agp_fcode_bwd(_ptr(td), _ptr(gyd), _ptr(lw.wt_hi), _ptr(lw.wt_lo), b, _act(act), _ode(method), _dt_array(dts), len(dts), gx2.ptr(),
                        None, None, _ptr(_nan(need, dev)), need, _stream()), "agp_fcode_bwd")
    assert torch.equal(gx2.value("gx"), vx) and gw2.untouched() and gb2.untouched(), what + ": gw / gb NULL"


def test_fcode_refusals(dev):
    L = _L()
    b = 4
    x, _, _, w, bias, gy = H.draw_fcode(b)
    lw = _weights(w, bias, dev, transpose=True)
    xd, gyd = _d(x, dev), _d(gy, dev)
    y, traj = Out(b, 256, dev), Out(2 * 2 * b, 256, dev)
    fwd = lambda method, nsteps: L.agp_fcode_fwd(_ptr(xd), None, None, _ptr(lw.w_hi), _ptr(lw.w_lo), _ptr(lw.bias), b, 1, method,
                                                 (C.c_float * 65)(*([0.5] * 65)), nsteps, y.ptr(), traj.ptr(), _stream())
    assert fwd(0, 0) == BADARG and fwd(0, 65) == BADARG, "nsteps 0 and 65"
    assert fwd(3, 2) == BADARG and fwd(-1, 2) == BADARG, "a bad method"
    assert y.untouched() and traj.untouched()
    need = int(L.agp_fcode_bwd_workspace_bytes(b, 0, 2))
    ws = torch.full((need // 4 + 64,), POISON, dtype=torch.int32, device=dev)
    td = torch.zeros((2 * 2 * b, 256), dtype=torch.float32, device=dev)
    gx, gw, gb = Out(b, 256, dev), Out(256, 256, dev, spare=4), Out(1, 256, dev, spare=1)
    bwd = lambda method, nsteps, nbytes: L.agp_fcode_bwd(_ptr(td), _ptr(gyd), _ptr(lw.wt_hi), _ptr(lw.wt_lo), b, 1, method,
                                                         (C.c_float * 65)(*([0.5] * 65)), nsteps, gx.ptr(), gw.ptr(), gb.ptr(), _ptr(ws),
                                                         nbytes, _stream())
    assert bwd(0, 2, need - 4) == BADARG, "a short workspace"
    assert bwd(0, 0, need) == BADARG and bwd(0, 65, 1 << 40) == BADARG, "nsteps 0 and 65"
    assert bwd(3, 2, 1 << 40) == BADARG and bwd(-1, 2, 1 << 40) == BADARG, "a bad method"
    assert gx.untouched() and gw.untouched() and gb.untouched() and bool((ws == POISON).all())


# ------------------------------------------------------------------------------------------------------------ agp_vecprog_run
VP_B = (1, 16, 17, 37)


def _program(b, dev):
    from agplace_amd.vecprog import VecProgram
    return VecProgram(b, dev)


def _store(vp, reg, b, dev):
    """a store target carved out of a poisoned buffer"""
    o = Out(b, 256, dev)
    vp.store(reg, o.t[:b])
    return o


def _fcode_standin(lw, method, dts, act):
    return SimpleNamespace(adaptive=False, _prep=SimpleNamespace(get=lambda: lw), method=method, dts=list(dts), act_name=act)


def _ln_standin(gamma, beta, dev):
    return SimpleNamespace(normalized_shape=(256,), weight=_d(gamma, dev), bias=_d(beta, dev), eps=H.LN_EPS)


@pytest.mark.parametrize("b", VP_B)
def test_vecprog_linear(dev, b):
    """LINEAR from memory at K 32 / 64 / 128 / 256 (scale on 64 and 256, every activation), from a register with both adds, and
    with dst == src; every result against fp64 and against agp_linear_fwd's on the same inputs."""
    from agplace_amd import ops
    vp = _program(b, dev)
    checks = []
    scale = torch.tensor([0.75], dtype=torch.float32)
    sd = _d(scale, dev)
    for i, k in enumerate((32, 64, 128, 256)):
        x, a1, a2, w, bias, _ = H.draw_linear(b, k, 256, seed=3)
        act, sc = H.ACTS[(i + 1) % 4], (k in (64, 256))
        lw = _weights(w, bias if k != 128 else None, dev)
        xd = _d(x, dev)
        vp.linear(i % 3, lw, xd, act=act, scale=sd if sc else None)
        xs = x * scale if sc else x                                    # (the load multiplies in fp32)
        checks.append((_store(vp, i % 3, b, dev), (xs, None, None, w, bias if k != 128 else None, act),
                       ops.linear(_d(xs, dev), lw, act=act), "from memory K %d %s%s" % (k, act, " scaled" if sc else "")))
    x, a1, a2, w, bias, _ = H.draw_linear(b, 256, 256, seed=4)
    lw = _weights(w, bias, dev)
    xd, a1d, a2d = _d(x, dev), _d(a1, dev), _d(a2, dev)
    for r, t in enumerate((xd, a1d, a2d)):
        vp.load(r, t)
    vp.linear(3, lw, 0, add1=1, add2=2, act="tanh")
    checks.append((_store(vp, 3, b, dev), (x, a1, a2, w, bias, "tanh"), ops.linear(xd, lw, act="tanh", add1=a1d, add2=a2d),
                   "from a register with both adds"))
    vp.linear(0, lw, 0, act="relu")                                     # dst == src
    checks.append((_store(vp, 0, b, dev), (x, None, None, w, bias, "relu"), ops.linear(xd, lw, act="relu"), "dst == src"))
    vp.run()
    for out, args, per_op, what in checks:
        ref, bars, floor = H.linear_fwd_bars(*args)
        got = out.value(what)
        _rows_ok(got, ref, bars, "vecprog LINEAR b %d %s" % (b, what), floor)
        _rows_ok(got, per_op.cpu(), bars, "vecprog LINEAR b %d %s against agp_linear_fwd" % (b, what))


@pytest.mark.parametrize("b,method,step,act", H.fcode_cases())
def test_vecprog_fcode(dev, b, method, step, act):
    from agplace_amd import ops
    x, a1, a2, w, bias, _ = H.draw_fcode(b)
    dts = H.grid_dts(step)
    y64, _, by, _ = H.fcode_fwd_bars(x, a1, a2, w, bias, act, method, dts)
    lw = _weights(w, bias, dev)
    xd, a1d, a2d = _d(x, dev), _d(a1, dev), _d(a2, dev)
    vp = _program(b, dev)
    for r, t in enumerate((xd, a1d, a2d)):
        vp.load(r, t)
    vp.fcode(4, _fcode_standin(lw, method, dts, act), 0, add1=1, add2=2)
    out = _store(vp, 4, b, dev)
    vp.run()
    got = out.value("y")
    what = "vecprog FCODE b %d %s %.2f %s" % (b, method, step, act)
    _rows_ok(got, y64, by, what)
    _rows_ok(got, ops.fcode(xd, lw, act, method, dts, add1=a1d, add2=a2d).cpu(), by, what + " against agp_fcode_fwd")


@pytest.mark.parametrize("b", VP_B)
def test_vecprog_rowwise_ops(dev, b):
    """LAYERNORM with and without affine, relu and residual; L2NORM with a zero row; WSUM of 1 and of 6 terms with device weights."""
    from agplace_amd import ops
    zero = b // 2 if b > 1 else None
    x, res, gy, gamma, beta = H.draw_rows(b, 256, seed=2, zero_row=zero)
    x2 = H.draw_rows(b, 256, seed=3)[0]
    xd, rd, gd, x2d = _d(x, dev), _d(res, dev), _d(gy, dev), _d(x2, dev)
    vp = _program(b, dev)
    vp.load(0, x2d), vp.load(1, rd), vp.load(2, xd), vp.load(3, gd)
    checks = []
    for name, (affine, relu, with_res, _) in H.LN_VARIANTS.items():
        ga, be = (gamma if affine else None), (beta if affine else None)
        vp.layernorm(4, _ln_standin(ga, be, dev), 0, relu=relu, residual=1 if with_res else -1)
        rs = res if with_res else None
        y64 = H.layernorm(x2, ga, be, H.LN_EPS, relu, rs)
        bar, floor = H.rowwise_bar(H.layernorm(x2, ga, be, H.LN_EPS, relu, rs, dtype=torch.float32), y64, H.CEIL_ROW_FWD)
        checks.append((_store(vp, 4, b, dev), y64, bar, floor, ops.layernorm(x2d, _d(ga, dev), _d(be, dev), H.LN_EPS, relu, _d(rs, dev)),
                       "LAYERNORM " + name))
    vp.l2norm(4, 2)
    y64 = H.l2normalize(x)
    bar, floor = H.rowwise_bar(H.l2normalize(x, torch.float32), y64, H.CEIL_ROW_FWD)
    l2 = _store(vp, 4, b, dev)
    checks.append((l2, y64, bar, floor, ops.l2normalize(xd), "L2NORM"))
    g = torch.Generator().manual_seed(b)
    ws = [torch.randn(1, generator=g) for _ in range(6)]
    wd = [_d(t, dev) for t in ws]
    terms = [x2, res, x, gy, x2, x]
    regs = [0, 1, 2, 3, 0, 2]
    vp.wsum(5, regs, wd)
    y64 = H.wsum(terms, ws)
    bar, floor = H.rowwise_bar(H.wsum(terms, ws, torch.float32), y64, H.CEIL_ROW_FWD)
    checks.append((_store(vp, 5, b, dev), y64, bar, floor, ops.wsum([x2d, rd, xd, gd, x2d, xd], wd), "WSUM of 6"))
    vp.wsum(5, [3], [wd[0]])
    y64 = H.wsum([gy], [ws[0]])
    bar, floor = H.rowwise_bar(H.wsum([gy], [ws[0]], torch.float32), y64, H.CEIL_ROW_FWD)
    checks.append((_store(vp, 5, b, dev), y64, bar, floor, ops.wsum([gd], [wd[0]]), "WSUM of 1"))
    vp.run()
    for out, ref, bar, floor, per_op, what in checks:
        got = out.value(what)
        _rows_ok(got, ref, bar, "vecprog b %d %s" % (b, what), floor)
        _rows_ok(got, per_op.cpu(), bar, "vecprog b %d %s against the per-op kernel" % (b, what))
    if zero is not None:
        assert not bool(l2.value("L2NORM")[zero].any()), "the zero row does not normalise to exact zeros"


def test_vecprog_runs_exactly_maxops_ops_and_refuses_one_more(dev):
    from agplace_amd.vecprog import VecProgramUnfit
    b = 17
    x = H.draw_rows(b, 256, seed=5)[0]
    vp = _program(b, dev)
    vp.load(0, _d(x, dev))
    for _ in range(MAXOPS - 2):
        vp.wsum(0, [0, 0])                                   # r0 <- r0 + r0: exact
    out = _store(vp, 0, b, dev)
    assert len(vp.ops) == MAXOPS
    vp.run()
    assert torch.equal(out.value("y"), x * 2.0 ** (MAXOPS - 2)), "a program of exactly AGP_VECPROG_MAXOPS ops"
    with pytest.raises(VecProgramUnfit):
        vp.wsum(0, [0, 0])


# ----------------------------------------------------------------------------------------------------------- agp_vecprog_run2
def _program_a(dev, b=17):
    """(program, [store targets]): load, FCODE (rk4, tanh), LINEAR, LAYERNORM, two stores"""
    x, a1, a2, w, bias, _ = H.draw_fcode(b, seed=6)
    _, res, _, gamma, beta = H.draw_rows(b, 256, seed=6)
    lw = _weights(w, bias, dev)
    vp = _program(b, dev)
    vp.load(0, _d(x, dev)), vp.load(1, _d(a1, dev)), vp.load(2, _d(res, dev))
    vp.fcode(3, _fcode_standin(lw, "rk4", H.grid_dts(0.25), "tanh"), 0, add1=1)
    outs = [_store(vp, 3, b, dev)]
    vp.linear(4, lw, 3, add1=0, act="relu")
    vp.layernorm(5, _ln_standin(gamma, beta, dev), 4, relu=True, residual=2)
    outs.append(_store(vp, 5, b, dev))
    return vp, outs


def _rider(dev, b):
    """(program, [store targets]) of a different op list: LINEAR from memory (K 64), L2NORM with a zero row, WSUM"""
    x, _, _, w, bias, _ = H.draw_linear(b, 64, 256, seed=7)
    x2 = H.draw_rows(b, 256, seed=7, zero_row=0)[0]
    lw = _weights(w, bias, dev)
    wt = _d(torch.tensor([1.5]), dev)
    vp = _program(b, dev)
    vp.linear(0, lw, _d(x, dev), act="sigmoid")
    vp.load(1, _d(x2, dev))
    vp.l2norm(2, 1)
    outs = [_store(vp, 2, b, dev)]
    vp.wsum(3, [0, 2, 1], [wt, None, wt])
    outs.append(_store(vp, 3, b, dev))
    return vp, outs


@pytest.mark.parametrize("b_rider", [5, 33])
def test_vecprog_run2_is_bit_equal_to_running_each_program_alone(dev, b_rider):
    solo = []
    for build in (lambda: _program_a(dev), lambda: _rider(dev, b_rider)):
        vp, outs = build()
        vp.run()
        solo.append([o.value("solo") for o in outs])
    vpa, outs_a = _program_a(dev)
    vpb, outs_b = _rider(dev, b_rider)
    assert vpa.fits_beside(vpb) and [o.op for o in vpa.ops] != [o.op for o in vpb.ops]
    vpa.run(rider=vpb)
    for alone, outs, who in ((solo[0], outs_a, "program A"), (solo[1], outs_b, "the rider")):
        for i, (want, o) in enumerate(zip(alone, outs)):
            got = o.value("%s output %d" % (who, i))
            assert bool(torch.isfinite(got).all())
            assert torch.equal(got, want), "%s (rider of %d rows): output %d differs from its solo run" % (who, b_rider, i)


def test_vecprog_run2_refusals(dev):
    from agplace_amd import _lib
    vpa, outs_a = _program_a(dev)
    vpb, outs_b = _rider(dev, 5)
    na, nb = len(vpa.ops), len(vpb.ops)
    arr_a = (_lib.VecProgOp * MAXOPS)(*(vpa.ops + [vpa.ops[-1]] * (MAXOPS - na)))
    arr_b = (_lib.VecProgOp * nb)(*vpb.ops)
    method, dts = vpa.ode
    dt = _dt_array(dts)
    run2 = lambda n_a, n_b, b_b: _L().agp_vecprog_run2(arr_a, n_a, 17, arr_b, n_b, b_b, method, dt, len(dts), _stream())
    assert run2(MAXOPS, 1, 5) == BADARG, "nops_a + nops_b > AGP_VECPROG_MAXOPS"
    assert run2(MAXOPS - nb + 1, nb, 5) == BADARG
    assert run2(na, nb, 0) == BADARG and run2(na, nb, -3) == BADARG, "a rider with b_b <= 0"
    assert _L().agp_vecprog_run(arr_a, MAXOPS + 1, 17, method, dt, len(dts), _stream()) == BADARG
    assert all(o.untouched() for o in outs_a + outs_b), "a refused launch wrote"
