"""Known-answer tests of the fp64 restatement of the adaptive dopri5 solve (tests/dopri5_ref.py), and the host-side
behaviour of the dopri5 option that needs no GPU."""
import math
import types

import pytest
import torch

import dopri5_ref as R


def test_tableau_is_consistent():
    for i in range(1, 7):
        assert abs(sum(R.A[i]) - (0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1, 1)[i]) < 1e-15
    assert abs(sum(R.CS) - 1) < 1e-15 and abs(sum(R.CE)) < 1e-15 and abs(sum(R.MID) - 0.5) < 1e-15
    assert R.A[6] == R.CS[:6]


@pytest.mark.parametrize("z", [0.3, -0.7, 1.0])
def test_one_step_of_the_linear_test_equation(z):
    """y' = lambda y: y1 / y0 = 1 + z + ... + z^5 / 120 + z^6 / 600 (order 5, and dopri5's own sixth-order coefficient)."""
    lam = -2.0
    dt = z / lam
    y0 = torch.tensor([1.5, -0.25], dtype=torch.float64)

    def f(v):
        return lam * v
    k = R.stages(f, y0, f(y0), dt)
    y1 = R.combine(y0, k, dt, R.CS)
    want = 1 + z + z ** 2 / 2 + z ** 3 / 6 + z ** 4 / 24 + z ** 5 / 120 + z ** 6 / 600
    assert float((y1 / y0 - want).abs().max()) < 1e-14
    assert float((k[6] - f(y1)).abs().max()) < 1e-14          # FSAL: k7 = f(y1)


def test_interpolant_hits_its_nodes_and_equals_the_beta_form():
    g = torch.Generator().manual_seed(0)
    w = torch.randn(6, 6, generator=g, dtype=torch.float64) / 3
    y0 = torch.randn(4, 6, generator=g, dtype=torch.float64)

    def f(v):
        return torch.tanh(v @ w.T)
    dt = 0.37
    k = R.stages(f, y0, f(y0), dt)
    y1, ymid = R.combine(y0, k, dt, R.CS), R.combine(y0, k, dt, R.MID)
    assert float((R.interp_poly(y0, y1, k, dt, 0.0) - y0).abs().max()) < 1e-14
    assert float((R.interp_poly(y0, y1, k, dt, 0.5) - ymid).abs().max()) < 1e-14
    assert float((R.interp_poly(y0, y1, k, dt, 1.0) - y1).abs().max()) < 1e-14
    assert max(abs(a - b) for a, b in zip(R.beta(1.0), R.CS)) < 1e-15
    for x in (0.0, 0.123, 0.5, 0.9, 1.0):
        assert float((R.interp_poly(y0, y1, k, dt, x) - R.combine(y0, k, dt, R.beta(x))).abs().max()) < 1e-14


def test_constant_right_hand_side_grows_the_step_tenfold():
    """f = 0: ratio exactly 0, the degenerate first step (h0 = 1e-6, h1 = max(1e-6, 1e-3 h0)), dt grows tenfold per step.
    f = a non-zero constant: the error is dt c sum(CE), rounding of a sum that is zero in exact arithmetic."""
    y0 = torch.tensor([1.0, 2.0], dtype=torch.float64)
    y, log = R.solve(lambda v: 0 * v, y0, 1e-3)
    assert log.first_dt == 1e-6 and len(log.steps) == 7 and all(r == 0 for r in log.ratios) and all(log.accepted)
    for a, b in zip(log.dts[:-1], log.dts[1:]):
        assert abs(b / a - 10) < 1e-14
    assert float((y - y0).abs().max()) == 0
    c = torch.tensor([3.0, -4.0], dtype=torch.float64)
    y, log = R.solve(lambda v: c + 0 * v, y0, 1e-3)
    assert len(log.steps) == 2 and all(r < 1e-12 for r in log.ratios) and all(log.accepted)
    assert abs(log.dts[1] / log.dts[0] - 10) < 1e-14
    assert float((y - (y0 + c)).abs().max()) < 1e-13           # the interpolant of a straight line is exact


def test_first_step_by_hand():
    """y' = -y, y0 = (1, 2), rtol = atol = 1e-3: scale = (2e-3, 3e-3), d0 = d1 = rms(500, 2000 / 3) = 589.2556...,
    h0 = 0.01; f1 - f0 = h0 y0, so d2 = d0 as well; h1 = (0.01 / d0)^(1/5) = 0.11116...; dt = min(100 h0, h1) = h1."""
    y0 = torch.tensor([1.0, 2.0], dtype=torch.float64)

    def f(v):
        return -v
    d0 = math.sqrt((500.0 ** 2 + (2000.0 / 3) ** 2) / 2)
    assert abs(d0 - 589.2556509887896) < 1e-9
    dt = R.first_step(f, y0, f(y0), 1e-3, 1e-3)
    assert abs(dt - (0.01 / d0) ** 0.2) < 1e-12 and abs(dt - 0.1111576) < 1e-6
    _, log = R.solve(f, y0, 1e-3)
    assert log.first_dt == dt and log.steps[0][0] == 0.0 and log.steps[0][1] == dt


def test_step_factor_limits():
    assert R.step_factor(0.0) == 10 and R.step_factor(1e-12) == 10
    assert R.step_factor(0.5) == pytest.approx(0.9 / 0.5 ** 0.2)
    assert R.step_factor(0.9) == 1.0                            # accepted steps never shrink
    assert R.step_factor(2.0) == pytest.approx(0.9 / 2 ** 0.2) and R.step_factor(1e9) == 0.2


@pytest.mark.parametrize("tol,lo,hi", [(1e-3, 5e-5, 5e-4), (1e-4, 5e-6, 1e-4)])
def test_linear_system_against_the_matrix_exponential(tol, lo, hi):
    """act = id: the restatement's own error against expm -- the yardstick of the GPU test
    (tests/test_gpu_dopri5.py::test_identity_against_the_matrix_exponential).  Measured: 1.9e-4 .. 2.0e-4 at tol = 1e-3,
    4.2e-5 at tol = 1e-4; the band asserts the order of magnitude (a solver that ignores tol leaves it)."""
    for b in (3, 16, 37, 64):
        x, a1, w, bias = R.input_law(b)
        y, log = R.fcode((x + a1).double(), w, bias, "id", tol)
        ex = R.linear_exact(x + a1, w, bias)
        err = float((y - ex).norm() / ex.norm())
        print(f"DOPRI5 REF id tol {tol} b {b}: err vs expm {err:.3e}, attempts {len(log.steps)}, f_evals {log.f_evals}")
        assert lo < err < hi
        assert log.steps[-1][0] + log.steps[-1][1] > 1.0        # the interpolant is exercised


def test_rejections_and_gradients_of_the_restatement():
    """A stiffer system rejects steps; autograd through the restatement sees the step sizes as constants."""
    x, a1, w, bias = R.input_law(16, gain=8.0)
    y, log = R.fcode((x + a1).double(), w, bias, "relu", 1e-3)
    assert sum(not a for a in log.accepted) == 3 and len(log.steps) == 11 and log.f_evals == 2 + 6 * 11
    x, a1, w, bias = R.input_law(4)
    xr = (x + a1).double().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    y, log = R.fcode(xr, wr, bias, "tanh", 1e-3)
    y.sum().backward()
    assert xr.grad is not None and wr.grad is not None and all(isinstance(s[1], float) for s in log.steps)


def test_dopri5_option_host_side():
    """What the dopri5 option decides without a GPU: FCODE accepts it and reads tol / the step cap, the vector program and
    the any-width path refuse it by name, every other method name is still refused."""
    from agplace_amd import _lib
    from agplace_amd.network_mm.ffns import FCODE
    from agplace_amd.options import Options, from_reference_opt
    from agplace_amd.vecprog import VecProgram, VecProgramUnfit
    m = FCODE(256, "relu", opt=Options(odeint_method="dopri5", tol=1e-4, odeint_max_steps=32))
    assert m.adaptive and m.tol == 1e-4 and m.max_steps == 32 and m.dts is None
    e = FCODE(256, "relu", opt=Options())
    assert not e.adaptive and len(e.dts) == 10
    with pytest.raises(RuntimeError):
        m.solver_stats()                                          # nothing has run yet
    with pytest.raises(VecProgramUnfit, match="adaptive solver"):
        VecProgram.fcode(None, 0, m, 0)
    narrow = FCODE(128, "relu", opt=Options(odeint_method="dopri5"))
    with pytest.raises(NotImplementedError, match="dopri5"):
        narrow(torch.zeros(2, 128))
    for bad in ("dopri8", "bosh3", "adaptive_heun"):
        with pytest.raises(NotImplementedError):
            FCODE(256, "relu", opt=Options(odeint_method=bad))
    with pytest.raises(ValueError):
        Options(odeint_max_steps=0)
    with pytest.raises(ValueError):
        FCODE(256, "relu", opt=Options(odeint_method="dopri5", tol=0.0))
    o = from_reference_opt(types.SimpleNamespace(odeint_method="dopri5", tol=1e-4))
    assert o.odeint_method == "dopri5" and o.tol == 1e-4 and o.odeint_max_steps == 64
    assert "dopri5" in _lib.ODE_ADAPTIVE and "dopri5" not in _lib.ODE
    L = _lib.load()
    assert L.agp_fcode_adaptive_ctrl_bytes(64) == 32 + 3 * 8 * 64
    assert L.agp_fcode_adaptive_ring_floats(5, 64, 0) == 2 * 8 * 5 * 256
    assert L.agp_fcode_adaptive_ring_floats(5, 64, 1) == 65 * 8 * 5 * 256
    assert L.agp_fcode_adaptive_bwd_workspace_bytes(5, 64) == 2 * (6 * 64 + 1) * 16 * 256 * 4
