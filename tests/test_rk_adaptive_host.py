"""The fp64 restatement over a Butcher table (tests/rk_adaptive_ref.py) and what the bosh3 option decides without a GPU."""
import types

import pytest
import torch

import dopri5_ref as R
import rk_adaptive_ref as K


@pytest.mark.parametrize("act,gain,tol,b", [("relu", 1.0, 1e-3, 16), ("relu", 4.0, 1e-4, 16), ("tanh", 1.0, 1e-4, 37),
                                            ("id", 4.0, 1e-4, 3), ("sigmoid", 1.0, 1e-3, 64), ("relu", 8.0, 1e-3, 16)])
def test_the_dopri5_table_reproduces_dopri5_ref(act, gain, tol, b):
    """The general restatement with the Dormand-Prince table IS dopri5_ref: the same y, steps and f-evaluations, exactly."""
    x, a1, w, bias = R.input_law(b, gain)
    yr, lr = R.fcode((x + a1).double(), w, bias, act, tol)
    yk, lk = K.fcode((x + a1).double(), w, bias, act, tol, "dopri5")
    assert torch.equal(yr, yk) and lr.steps == lk.steps and lr.f_evals == lk.f_evals and lr.first_dt == lk.first_dt
    for x_ in (0.0, 0.3, 1.0):
        assert K.beta(x_, K.TABLES["dopri5"]) == R.beta(x_)


def test_bosh3_table():
    tb = K.TABLES["bosh3"]
    assert (tb.S, tb.ORDER) == (4, 3)
    assert abs(sum(tb.CE)) < 1e-16
    assert K.beta(1.0, tb) == pytest.approx(tb.CS, abs=1e-15) and K.beta(0.0, tb) == [0.0] * 4
    # the rows of A sum to the stage times 1/2, 3/4, 1; the solution weights to 1
    assert [sum(r) for r in tb.A[1:]] == pytest.approx([0.5, 0.75, 1.0], abs=1e-15) and sum(tb.CS) == pytest.approx(1.0, abs=1e-15)
    # the interpolant is the quartic through y, y + dt k2 / 2 and y1: at x = 1/2 its weights are MID
    assert K.beta(0.5, tb) == pytest.approx(tb.MID, abs=1e-15)
    # the controller's exponent is 1/3
    assert K.step_factor(0.5, tb) == pytest.approx(0.9 / 0.5 ** (1 / 3)) and K.step_factor(0.9, tb) == 1.0
    assert K.step_factor(0.0, tb) == 10 and K.step_factor(1e9, tb) == 0.2 and K.step_factor(2.0, tb) == pytest.approx(0.9 / 2 ** (1 / 3))


def test_bosh3_is_of_order_three():
    """Halving h shrinks the one-step local error on y' = -y by 2^4 = 16 (14 .. 18 asserted)."""
    tb = K.TABLES["bosh3"]
    y0 = torch.tensor([1.0, -2.0, 0.5], dtype=torch.float64)

    def local_error(h):
        y1, _ = K.one_step(lambda v: -v, y0, h, tb)
        return float((y1 - y0 * torch.exp(torch.tensor(-h, dtype=torch.float64))).abs().max())
    for h in (0.2, 0.1, 0.05):
        q = local_error(h) / local_error(h / 2)
        print(f"BOSH3 REF local error ratio at h = {h}: {q:.2f}")
        assert 14.0 < q < 18.0


def test_bosh3_first_step_and_f_evals():
    x, a1, w, bias = R.input_law(16)
    y, log = K.fcode((x + a1).double(), w, bias, "relu", 1e-3, "bosh3")
    assert log.f_evals == 2 + 3 * len(log.steps) and log.steps[0][1] == log.first_dt
    assert log.accepted[-1] and log.steps[-1][0] + log.steps[-1][1] > 1.0


def test_bosh3_linear_system_against_the_matrix_exponential():
    """act = id: the restatement's own error against expm, the yardstick of the GPU tests.  The interpolant's mid-point is
    the midpoint rule's value, so the end error does not follow tol down: it stays near 1e-4."""
    for tol in (1e-3, 1e-6):
        for b in (3, 16, 37, 64):
            x, a1, w, bias = R.input_law(b)
            y, log = K.fcode((x + a1).double(), w, bias, "id", tol, "bosh3")
            ex = R.linear_exact(x + a1, w, bias)
            err = float((y - ex).norm() / ex.norm())
            print(f"BOSH3 REF id tol {tol} b {b}: err vs expm {err:.3e}, attempts {len(log.steps)}, f_evals {log.f_evals}")
            assert 1e-5 < err < 2e-3


def test_bosh3_gradients_of_the_restatement():
    x, a1, w, bias = R.input_law(4)
    xr = (x + a1).double().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    y, log = K.fcode(xr, wr, bias, "tanh", 1e-3, "bosh3")
    y.sum().backward()
    assert xr.grad is not None and wr.grad is not None and all(isinstance(s[1], float) for s in log.steps)


def test_bosh3_option_host_side():
    """FCODE takes 'bosh3' only behind Options.odeint_adaptive_family; the vector program and the other widths refuse it by
    name; the method number is the header's."""
    from agplace_amd import _lib
    from agplace_amd.network_mm.ffns import FCODE
    from agplace_amd.options import Options, from_reference_opt
    from agplace_amd.vecprog import VecProgram, VecProgramUnfit
    assert _lib.ODE_ADAPTIVE["bosh3"] == 4 and _lib.ODE_ADAPTIVE["dopri5"] == 3 and "bosh3" not in _lib.ODE
    opt = Options(odeint_adaptive_family=True, odeint_method="bosh3", tol=1e-4, odeint_max_steps=32)
    m = FCODE(256, "relu", opt=opt)
    assert m.adaptive and m.method == "bosh3" and m.tol == 1e-4 and m.max_steps == 32 and m.dts is None
    with pytest.raises(RuntimeError):
        m.solver_stats()                                          # nothing has run yet
    with pytest.raises(VecProgramUnfit, match="adaptive solver"):
        VecProgram.fcode(None, 0, m, 0)
    with pytest.raises(NotImplementedError, match="bosh3"):
        FCODE(256, "relu", opt=Options(odeint_method="bosh3"))
    # the switch opens the family this build serves, nothing else; dopri5 and the fixed grids do not need it
    for bad in ("dopri8", "adaptive_heun", "fehlberg2"):
        with pytest.raises(NotImplementedError):
            FCODE(256, "relu", opt=Options(odeint_adaptive_family=True, odeint_method=bad))
    assert FCODE(256, "relu", opt=Options(odeint_adaptive_family=True, odeint_method="dopri5")).adaptive
    assert not FCODE(256, "relu", opt=Options(odeint_adaptive_family=True)).adaptive
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="odeint_adaptive_family"):
            Options(odeint_adaptive_family=bad)
    with pytest.raises(ValueError):
        FCODE(256, "relu", opt=Options(odeint_adaptive_family=True, odeint_method="bosh3", tol=0.0))
    o = from_reference_opt(types.SimpleNamespace(odeint_method="bosh3", tol=1e-4, odeint_adaptive_family=True))
    assert o.odeint_method == "bosh3" and o.odeint_adaptive_family is False
    assert Options().odeint_adaptive_family is False and o.copy(odeint_adaptive_family=True).odeint_adaptive_family is True
    narrow = FCODE(128, "relu", opt=opt)
    with pytest.raises(NotImplementedError, match="bosh3"):
        narrow(torch.zeros(2, 128))
    wide = FCODE(384, "relu", opt=opt)                            # 384 columns need Options.fcode_wide as well
    assert not wide.wide_routes
    with pytest.raises(NotImplementedError, match="bosh3"):
        wide(torch.zeros(2, 384))
    assert FCODE(384, "relu", opt=opt.copy(fcode_wide=True)).wide_routes
