"""fp64 restatement of FCODE's adaptive solve over a Butcher table (TEST INFRASTRUCTURE; the specification is DESIGN.md
section 2, "Adaptive solver").  tests/dopri5_ref.py restates torchdiffeq's controller for Dormand-Prince 5(4); every other
embedded FSAL member of that family runs the same controller with another table, and this module is dopri5_ref.solve with
the table as an argument: with TABLES["dopri5"] it computes, operation for operation, what dopri5_ref computes
(tests/test_rk_adaptive_host.py holds it to equality).  The norm, the constants of the controller, the log and the input law are
dopri5_ref's own.

A table: S stages, A (row i = the weights of stage i + 1's input; the last row is CS, so the last stage is f(y1): FSAL), the
solution weights CS, the error weights CE (they sum to 0), the mid-point weights MID of the quartic interpolant, and ORDER
(the step factor is ratio^(-1/ORDER), the first step (0.01 / max(d1, d2))^(1/ORDER)).

solve(f, y0, tol, table) -> (y(1), log); fcode(x, weight, bias, act, tol, method) -> (y, log); log.f_evals = 2 + (S - 1) attempts.
relu_kinks: the elements at which relu's derivative is beyond the device's resolution (gradient comparisons)."""
import torch

import dopri5_ref as R
from dopri5_ref import DFACTOR, IFACTOR, SAFETY, Log, act_fn, input_law, linear_exact, rms  # noqa: F401  (re-exported)


class Table:
    def __init__(self, A, CS, CE, MID, ORDER):
        self.A, self.CS, self.CE, self.MID, self.ORDER, self.S = A, CS, CE, MID, ORDER, len(CS)
        assert len(A) == self.S and len(CE) == self.S and len(MID) == self.S and all(len(A[i]) == i for i in range(self.S))
        assert list(A[-1]) == list(CS[:-1]) and CS[-1] == 0, "FSAL: the last stage is f(y1)"


TABLES = {
    "dopri5": Table(R.A, R.CS, R.CE, R.MID, R.ORDER),
    # Bogacki-Shampine 3(2); MID as torchdiffeq ships it (y_mid = y + dt k2 / 2)
    "bosh3": Table([[], [1 / 2], [0, 3 / 4], [2 / 9, 1 / 3, 4 / 9]], [2 / 9, 1 / 3, 4 / 9, 0],
                   [2 / 9 - 7 / 24, 1 / 3 - 1 / 4, 4 / 9 - 1 / 3, -1 / 8], [0, 1 / 2, 0, 0], 3),
}


def first_step(f, y0, f0, rtol, atol, tb):
    """torchdiffeq's _select_initial_step for a method of order tb.ORDER."""
    scale = atol + y0.detach().abs() * rtol
    d0, d1 = rms(y0 / scale), rms(f0 / scale)
    h0 = 1e-6 if (d0 < 1e-5 or d1 < 1e-5) else 0.01 * d0 / d1
    f1 = f(y0.detach() + h0 * f0.detach())
    d2 = rms((f1 - f0) / scale) / h0
    if d1 <= 1e-15 and d2 <= 1e-15:
        h1 = max(1e-6, h0 * 1e-3)
    else:
        h1 = (0.01 / max(d1, d2)) ** (1.0 / tb.ORDER)
    return min(100 * h0, h1)


def stages(f, y, k1, dt, tb):
    """k1 .. kS of one attempted step; kS = f(y1)."""
    k = [k1]
    for i in range(1, tb.S):
        k.append(f(y + dt * sum(a * kk for a, kk in zip(tb.A[i], k) if a != 0)))
    return k


def error_ratio(y, y1, k, dt, rtol, atol, tb):
    err = dt * sum(c * kk.detach() for c, kk in zip(tb.CE, k) if c != 0)
    return rms(err / (atol + rtol * torch.max(y.detach().abs(), y1.detach().abs())))


def step_factor(ratio, tb):
    if ratio == 0:
        return IFACTOR
    return min(IFACTOR, max(SAFETY / ratio ** (1.0 / tb.ORDER), 1.0 if ratio < 1 else DFACTOR))


def interp_poly(y, y1, k, dt, x, tb):
    """The quartic through y, ymid, y1 with end slopes k1, kS at x in [0, 1]."""
    ymid = R.combine(y, k, dt, tb.MID)
    f0, f1 = k[0], k[-1]
    a = 2 * dt * (f1 - f0) - 8 * (y1 + y) + 16 * ymid
    b = dt * (5 * f0 - 3 * f1) + 18 * y + 14 * y1 - 32 * ymid
    c = dt * (f1 - 4 * f0) - 11 * y - 5 * y1 + 16 * ymid
    d = dt * f0
    return (((a * x + b) * x + c) * x + d) * x + y


def beta(x, tb):
    """interp_poly(...) == y + dt * sum_j beta(x)[j] * k[j]; beta(1) == CS."""
    out = []
    for j in range(tb.S):
        d1, dS = float(j == 0), float(j == tb.S - 1)
        out.append(x ** 4 * (16 * tb.MID[j] - 8 * tb.CS[j] + 2 * (dS - d1)) + x ** 3 * (14 * tb.CS[j] - 32 * tb.MID[j] + 5 * d1 - 3 * dS)
                   + x ** 2 * (16 * tb.MID[j] - 5 * tb.CS[j] + dS - 4 * d1) + x * d1)
    return out


def one_step(f, y, dt, tb):
    """(y1, error estimate) of a single step of size dt from y."""
    k = stages(f, y, f(y), dt, tb)
    return R.combine(y, k, dt, tb.CS), dt * sum(c * kk for c, kk in zip(tb.CE, k) if c != 0)


def solve(f, y0, tol, tb, max_steps=10000, dtype=torch.float64):
    """y(1) of y' = f(y), y(0) = y0 with rtol = atol = tol.  Differentiable in y0 and in whatever f closes over."""
    rtol = atol = float(tol)
    y = y0.to(dtype)
    log = Log()
    k1 = f(y)
    dt = first_step(f, y, k1, rtol, atol, tb)
    log.first_dt, log.f_evals = dt, 2
    t = 0.0
    while True:
        if len(log.steps) >= max_steps:
            raise RuntimeError("rk_adaptive_ref: step cap")
        if t + dt == t:
            raise RuntimeError("rk_adaptive_ref: step size underflow")
        k = stages(f, y, k1, dt, tb)
        log.f_evals += tb.S - 1
        y1 = R.combine(y, k, dt, tb.CS)
        ratio = error_ratio(y, y1, k, dt, rtol, atol, tb)
        accepted = ratio <= 1
        log.steps.append((t, dt, ratio, accepted))
        if accepted:
            t1 = t + dt
            if t1 >= 1.0:
                return interp_poly(y, y1, k, dt, (1.0 - t) / (t1 - t), tb), log
            t, y, k1 = t1, y1, k[-1]
        dt = dt * step_factor(ratio, tb)


def fcode(x, weight, bias, act, tol, method, dtype=torch.float64, relu_slope=None):
    """FCODE.forward with odeint_method = method, rtol = atol = tol: (y, log).  log.inp / log.pre: the input and the
    pre-activation of every evaluation of f, in order (0 = f(y0), 1 = the probe of the first-step choice, then S - 1 per
    attempted step), detached.  relu_slope (relu only, see relu_kinks): {evaluation: (mask, slope)} -- at the masked elements of
    that evaluation relu's derivative is `slope` instead of [z > 0]; values are untouched."""
    g = act_fn(act)
    w, b = weight.to(dtype), bias.to(dtype)
    inp, pre = [], []

    def f(v):
        z = torch.nn.functional.linear(v, w, b)
        k = g(z)
        if relu_slope and len(pre) in relu_slope:
            mask, slope = relu_slope[len(pre)]
            k = torch.where(mask, k.detach() + slope * (z - z.detach()), k)
        inp.append(v.detach())
        pre.append(z.detach())
        return k
    y, log = solve(f, x, tol, TABLES[method], dtype=dtype)
    log.inp, log.pre = inp, pre
    return y, log


def relu_kinks(log, weight, ring, method, bits=17):
    """relu is not differentiable at 0, and a pre-activation z the device cannot tell from 0 has no derivative the device could
    be held to: there the gradient comparison takes the device's own choice, everywhere else fp64's.  The device forms
    z = sum_j w_j v_j from two bf16 planes of W (each product resolved to 2^-18 of its size: two roundings of 2^-9) in fp32
    sums, on a stage input that itself carries the solve's 1e-6 of error; |z| < 2^-bits sum_j |w_j| |v_j|, bits = 17, is
    twice the planes' resolution of the absolute sum.  ring = the device's record [step][0 = y, i = k_i][b][D] of the same
    solve (CPU tensor): its k_i > 0 is the choice the device's backward makes.  Only accepted steps carry gradient.
    Returns the relu_slope argument of fcode and (elements in the band, of those the device chose against fp64's sign)."""
    S = TABLES[method].S
    absw = weight.detach().double().abs()
    out, inband, flipped = {}, 0, 0
    where = {0: (0, 1)}                                      # evaluation -> (accepted step, stage) in the ring
    n = 0
    for a, ok in enumerate(log.accepted):
        if ok:
            for i in range(2, S + 1):
                where[2 + (S - 1) * a + (i - 2)] = (n, i)
            n += 1
    for e, (n, i) in where.items():
        z = log.pre[e]
        mask = z.abs() < 2.0 ** -bits * (log.inp[e].abs() @ absw.T)
        if bool(mask.any()):
            slope = (ring[n, i].double() > 0).double()
            out[e] = (mask, slope)
            inband += int(mask.sum())
            flipped += int((mask & ((z > 0).double() != slope)).sum())
    return out, (inband, flipped)
