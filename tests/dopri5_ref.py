"""fp64 restatement of the adaptive dopri5 solve of FCODE (TEST INFRASTRUCTURE; the specification is DESIGN.md section 2,
"Adaptive solver").  torchdiffeq is not available, so like the fixed-grid oracle (oracle/ode.py) this restates its
published algorithm: Dormand-Prince 5(4) with FSAL, one RMS error norm over the whole batch, steps not clipped to the end
time, the result read off the last step's quartic interpolant.  Step sizes, the error ratio and the first-step choice are
plain Python floats: constants to autograd, as torchdiffeq computes them without a tape.

solve(f, y0, tol) -> (y(1), log); log.first_dt, log.steps = [(t, dt, ratio, accepted)] per ATTEMPTED step, log.f_evals."""
import torch

A = [[], [1 / 5], [3 / 40, 9 / 40], [44 / 45, -56 / 15, 32 / 9], [19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729],
     [9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656], [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84]]
CS = [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84, 0]
CE = [35 / 384 - 1951 / 21600, 0, 500 / 1113 - 22642 / 50085, 125 / 192 - 451 / 720, -2187 / 6784 + 12231 / 42400,
      11 / 84 - 649 / 6300, -1 / 60]
MID = [0.5 * v for v in (6025192743 / 30085553152, 0, 51252292925 / 65400821598, -2691868925 / 45128329728,
                         187940372067 / 1594534317056, -1776094331 / 19743644256, 11237099 / 235043384)]
SAFETY, IFACTOR, DFACTOR, ORDER = 0.9, 10.0, 0.2, 5


class Log:
    def __init__(self):
        self.first_dt, self.steps, self.f_evals = None, [], 0

    @property
    def accepted(self):
        return [s[3] for s in self.steps]

    @property
    def dts(self):
        return [s[1] for s in self.steps]

    @property
    def ratios(self):
        return [s[2] for s in self.steps]


def rms(v):
    """sqrt(mean(v^2)) over ALL elements, as a float (no tape)."""
    return float(v.detach().double().pow(2).mean().sqrt())


def first_step(f, y0, f0, rtol, atol):
    """(dt, f evaluations used) of torchdiffeq's _select_initial_step for an order-5 method's embedded order 4."""
    scale = atol + y0.detach().abs() * rtol
    d0, d1 = rms(y0 / scale), rms(f0 / scale)
    h0 = 1e-6 if (d0 < 1e-5 or d1 < 1e-5) else 0.01 * d0 / d1
    f1 = f(y0.detach() + h0 * f0.detach())
    d2 = rms((f1 - f0) / scale) / h0
    if d1 <= 1e-15 and d2 <= 1e-15:
        h1 = max(1e-6, h0 * 1e-3)
    else:
        h1 = (0.01 / max(d1, d2)) ** (1.0 / ORDER)
    return min(100 * h0, h1)


def stages(f, y, k1, dt):
    """k1 .. k7 of one attempted step; k7 = f(y1)."""
    k = [k1]
    for i in range(1, 7):
        k.append(f(y + dt * sum(a * kk for a, kk in zip(A[i], k) if a != 0)))
    return k


def combine(y, k, dt, w):
    return y + dt * sum(c * kk for c, kk in zip(w, k) if c != 0)


def error_ratio(y, y1, k, dt, rtol, atol):
    err = dt * sum(c * kk.detach() for c, kk in zip(CE, k) if c != 0)
    return rms(err / (atol + rtol * torch.max(y.detach().abs(), y1.detach().abs())))


def step_factor(ratio):
    if ratio == 0:
        return IFACTOR
    return min(IFACTOR, max(SAFETY / ratio ** (1.0 / ORDER), 1.0 if ratio < 1 else DFACTOR))


def interp_poly(y, y1, k, dt, x):
    """The quartic through y, ymid, y1 with end slopes k1, k7 (torchdiffeq _interp_fit / _interp_evaluate) at x in [0, 1]."""
    ymid = combine(y, k, dt, MID)
    f0, f1 = k[0], k[6]
    a = 2 * dt * (f1 - f0) - 8 * (y1 + y) + 16 * ymid
    b = dt * (5 * f0 - 3 * f1) + 18 * y + 14 * y1 - 32 * ymid
    c = dt * (f1 - 4 * f0) - 11 * y - 5 * y1 + 16 * ymid
    d = dt * f0
    return (((a * x + b) * x + c) * x + d) * x + y


def beta(x):
    """interp_poly(...) == y + dt * sum_j beta(x)[j] * k[j]; beta(1) == CS."""
    out = []
    for j in range(7):
        d1, d7 = float(j == 0), float(j == 6)
        out.append(x ** 4 * (16 * MID[j] - 8 * CS[j] + 2 * (d7 - d1)) + x ** 3 * (14 * CS[j] - 32 * MID[j] + 5 * d1 - 3 * d7)
                   + x ** 2 * (16 * MID[j] - 5 * CS[j] + d7 - 4 * d1) + x * d1)
    return out


def solve(f, y0, tol, max_steps=10000, dtype=torch.float64):
    """y(1) of y' = f(y), y(0) = y0 with rtol = atol = tol.  Differentiable in y0 and in whatever f closes over."""
    rtol = atol = float(tol)
    y = y0.to(dtype)
    log = Log()
    k1 = f(y)
    dt = first_step(f, y, k1, rtol, atol)
    log.first_dt, log.f_evals = dt, 2
    t = 0.0
    while True:
        if len(log.steps) >= max_steps:
            raise RuntimeError("dopri5_ref: step cap")
        if t + dt == t:
            raise RuntimeError("dopri5_ref: step size underflow")
        k = stages(f, y, k1, dt)
        log.f_evals += 6
        y1 = combine(y, k, dt, CS)
        ratio = error_ratio(y, y1, k, dt, rtol, atol)
        accepted = ratio <= 1
        log.steps.append((t, dt, ratio, accepted))
        if accepted:
            t1 = t + dt
            if t1 >= 1.0:
                return interp_poly(y, y1, k, dt, (1.0 - t) / (t1 - t)), log
            t, y, k1 = t1, y1, k[6]
        dt = dt * step_factor(ratio)


def act_fn(name):
    return {None: lambda v: v, "id": lambda v: v, "relu": torch.relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid}[name]


def fcode(x, weight, bias, act, tol, dtype=torch.float64):
    """FCODE.forward with odeint_method='dopri5', rtol = atol = tol: (y, log)."""
    g = act_fn(act)
    w, b = weight.to(dtype), bias.to(dtype)
    return solve(lambda v: g(torch.nn.functional.linear(v, w, b)), x, tol, dtype=dtype)


def input_law(b, gain=1.0, seed=11):
    """The inputs of tests/test_gpu_kernels.py::test_fcode_matches_oracle (x, add1, w = randn / 16, bias), w times `gain`."""
    g = torch.Generator().manual_seed(seed)
    x, a1 = torch.randn(b, 256, generator=g), torch.randn(b, 256, generator=g) * 0.5
    w = torch.randn(256, 256, generator=g) / 16 * gain
    bias = torch.randn(256, generator=g) * 0.1
    return x, a1, w, bias


def linear_exact(y0, w, bias):
    """y(1) of y' = W y + bias in fp64 by the matrix exponential of the augmented system."""
    n = w.shape[0]
    m = torch.zeros(n + 1, n + 1, dtype=torch.float64)
    m[:n, :n], m[:n, n] = w.double(), bias.double()
    e = torch.linalg.matrix_exp(m)
    return y0.double() @ e[:n, :n].T + e[:n, n]
