"""Options.fcode_wide and the size helpers of the fixed-grid training entries at 384 columns (include/agplace_hip.h
agp_fcode_wide_traj_floats / agp_fcode_wide_bwd_workspace_bytes): no GPU needed."""
from types import SimpleNamespace

import pytest

from agplace_amd import _lib
from agplace_amd.options import Options, from_reference_opt

NEW = ("agp_fcode_wide_traj_floats", "agp_fcode_wide_fwd_traj", "agp_fcode_wide_bwd_workspace_bytes", "agp_fcode_wide_bwd")
STAGES = {"euler": 1, "midpoint": 2, "rk4": 4}


def test_the_switch_is_a_bool_and_defaults_to_off():
    assert Options().fcode_wide is False
    assert Options(fcode_wide=True).fcode_wide is True
    assert Options().copy(fcode_wide=True).fcode_wide is True
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="fcode_wide"):
            Options(fcode_wide=bad)


def test_a_reference_namespace_cannot_carry_the_switch():
    o = from_reference_opt(SimpleNamespace(fcode_wide=True, odeint_method="rk4"))
    assert o.fcode_wide is False and o.odeint_method == "rk4"
    assert o.copy(fcode_wide=True).fcode_wide is True


def test_symbols_are_exported_and_bound():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None


@pytest.mark.parametrize("method", sorted(STAGES))
@pytest.mark.parametrize("b", [1, 15, 16, 17, 35])
@pytest.mark.parametrize("nsteps", [1, 4, 64])
def test_size_helpers_follow_their_formulas(method, b, nsteps):
    lib, m, st = _lib.load(), _lib.ODE[method], STAGES[method]
    bp = (b + 15) // 16 * 16
    assert lib.agp_fcode_wide_traj_floats(b, 384, m, nsteps) == nsteps * (1 + st) * b * 384
    assert lib.agp_fcode_wide_bwd_workspace_bytes(b, 384, m, nsteps) == 2 * nsteps * st * bp * 384 * 4


@pytest.mark.parametrize("b,d,method,nsteps", [(4, 256, 0, 4), (0, 384, 0, 4), (-3, 384, 0, 4), (4, 384, 0, 65), (4, 384, 0, 0),
                                               (4, 384, 3, 4), (4, 384, -1, 4), (4, 128, 2, 4)])
def test_size_helpers_return_zero_for_what_the_entries_refuse(b, d, method, nsteps):
    lib = _lib.load()
    assert lib.agp_fcode_wide_traj_floats(b, d, method, nsteps) == 0
    assert lib.agp_fcode_wide_bwd_workspace_bytes(b, d, method, nsteps) == 0
