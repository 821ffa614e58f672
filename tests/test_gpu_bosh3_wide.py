"""-m gpu tests of the adaptive bosh3 solver at 384 columns (agp_fcode_adaptive_wide_fwd / _bwd with AGP_ODE_BOSH3, the Tableau
Bosh3 of csrc/fusion_adaptive.hip over the Streamed384 engine) against the fp64 restatement in tests/rk_adaptive_ref.py, on the
input law of tests/test_gpu_dopri5_wide.py and through FCODE(384) with Options(fcode_wide=True, odeint_adaptive_family=True).

Bounds: those tests/test_gpu_bosh3.py holds the same arithmetic to at 256 columns.  Output: rel_l2 < 1e-4.  Gradients:
rel_l2 < 1e-3 against fp64 autograd through the restatement.  Decisions: the accept / reject sequence equals the restatement's;
every parity case asserts ON THE REFERENCE RUN that no attempted step's ratio lies within 0.05 of 1, that the last accepted
step overshoots t = 1 and that the solve attempts at most 64 steps.  Step sizes: every attempted dt within DT_BOUND[tol] relative
of the restatement's, twice the worst difference measured on an MI355X over the forward cases of this file, rounded up to one
significant digit.
MEASURED (MI355X, the 31 forward cases below): the accept / reject sequence equals the restatement's in every case; worst dt
difference 4.49e-5 at tol = 1e-3 and 1.05e-4 at tol = 1e-4 (both relu, gain 1, b = 3), so the bounds are 9e-5 and 3e-4; worst
output difference 5.0e-6.  Gradients: worst 1.1e-4 (gw, relu, gain 2, 14 steps), through the module within 1.7e-6.  Against the matrix exponential the device's error equals the restatement's own to three digits (1.447e-3 .. 1.810e-3)."""
import ctypes
import functools
import math

import pytest
import torch

import dopri5_ref as R
import rk_adaptive_ref as K
from gpu_util import rel_l2

pytestmark = pytest.mark.gpu
METHOD = "bosh3"
D = 384
# worst relative dt difference over the forward cases of this file on an MI355X, per tol, and the bound: twice that, rounded up
DT_MEASURED = {1e-3: 4.49e-5, 1e-4: 1.05e-4}
DT_BOUND = {1e-3: 9e-5, 1e-4: 3e-4}
# (act, gain, tol, b, seed, attempts, rejected) of the restatement: stiffer weights, rejected steps, up to 27 attempts
LONG = [("relu", 4.0, 1e-3, 16, 14, 13, 1), ("relu", 4.0, 1e-3, 16, 11, 13, 1), ("relu", 4.0, 1e-4, 16, 15, 27, 1),
        ("relu", 2.0, 1e-4, 37, 12, 14, 0), ("tanh", 16.0, 1e-4, 16, 11, 22, 0)]


@functools.lru_cache(maxsize=None)
def input_law(b, gain=1.0, seed=11):
    """The law of tests/test_gpu_dopri5_wide.py: x, add1, w = randn / sqrt(384) * gain, bias: CPU tensors, shared and never
    modified."""
    g = torch.Generator().manual_seed(seed)
    x, a1 = torch.randn(b, D, generator=g), torch.randn(b, D, generator=g) * 0.5
    w = torch.randn(D, D, generator=g) / math.sqrt(D) * gain
    bias = torch.randn(D, generator=g) * 0.1
    return x, a1, w, bias


def _options(**kw):
    from agplace_amd.options import Options
    return Options(odeint_method=METHOD, fcode_wide=True, odeint_adaptive_family=True, **kw)


@functools.lru_cache(maxsize=None)
def _restated(act, gain, tol, b, seed):
    """(y, log) of the fp64 restatement, once per case."""
    x, a1, w, bias = input_law(b, gain, seed)
    with torch.no_grad():
        return K.fcode((x + a1).double(), w, bias, act, tol, METHOD)


def _precondition(log, tag):
    margin = min(abs(r - 1) for r in log.ratios)
    assert margin > 0.05, ("precondition: a reference ratio within 0.05 of 1", tag, log.ratios)
    assert log.accepted[-1] and log.steps[-1][0] + log.steps[-1][1] > 1.0, tag                 # the interpolant is exercised
    assert len(log.steps) <= 64, tag
    return margin


def _solve_and_compare(dev, act, gain, tol, b, seed=11):
    from agplace_amd import ops
    x, a1, w, bias = input_law(b, gain, seed)
    lw = ops.LinearWeights(w.to(dev), bias.to(dev))
    y, ctrl = ops.fcode_adaptive(x.to(dev), lw, act, METHOD, tol, 64, add1=a1.to(dev))
    st = ops.ode_stats(ctrl)
    yr, log = _restated(act, gain, tol, b, seed)
    tag = (act, gain, tol, b, seed)
    margin = _precondition(log, tag)
    assert st["status"] == 0, (tag, st)
    assert [a[2] for a in st["attempts"]] == log.accepted, (tag, st["attempts"], log.steps)
    assert st["f_evals"] == log.f_evals == 2 + 3 * len(log.steps)
    assert st["accepted"] == sum(log.accepted) and st["rejected"] == len(log.steps) - sum(log.accepted)
    dtrel = max(abs(a[0] - s[1]) / s[1] for a, s in zip(st["attempts"], log.steps))
    err = rel_l2(y, yr)
    print(f"BOSH3-384 {act} gain {gain} tol {tol} b {b} seed {seed}: attempts {len(log.steps)} rejected {st['rejected']} "
          f"margin {margin:.3f} dt rel {dtrel:.2e} out rel_l2 {err:.2e} t1 {st['t1']:.4f}")
    assert [d for d, a in zip([a[0] for a in st["attempts"]], log.accepted) if a] == st["dts"]
    assert abs(st["t1"] - (log.steps[-1][0] + log.steps[-1][1])) < DT_BOUND[tol] * 2
    assert dtrel < DT_BOUND[tol], (tag, dtrel)
    assert err < 1e-4, (tag, err)
    return st, log


@pytest.mark.parametrize("tol", [1e-3, 1e-4])
@pytest.mark.parametrize("act", ["relu", "tanh", "sigmoid"])
def test_forward_matches_the_restatement(dev, act, tol):
    """One row tile with dead rows, one full tile, three tiles with a partial last one, four full tiles."""
    for b in (3, 16, 37, 64):
        _solve_and_compare(dev, act, 1.0, tol, b)


def test_forward_matches_the_restatement_identity(dev):
    """act = id at tol = 1e-3, b = 37 and 64 (at b = 3 and 16 the restatement's own ratios come within 0.047 and 0.051 of 1;
    at tol = 1e-4 within 0.02 at every b)."""
    for b in (37, 64):
        _solve_and_compare(dev, "id", 1.0, 1e-3, b)


@pytest.mark.parametrize("act,gain,tol,b,seed,attempts,rejected", LONG)
def test_forward_with_rejections_and_long_sequences(dev, act, gain, tol, b, seed, attempts, rejected):
    st, log = _solve_and_compare(dev, act, gain, tol, b, seed)
    assert (len(log.steps), st["rejected"]) == (attempts, rejected)


def test_identity_against_the_matrix_exponential(dev):
    """act = id has an exact answer: the device's error against it is at most 1.5 x the fp64 restatement's own, as at 256."""
    from agplace_amd import ops
    for b in (3, 16, 37, 64):
        x, a1, w, bias = input_law(b)
        lw = ops.LinearWeights(w.to(dev), bias.to(dev))
        y, _ = ops.fcode_adaptive(x.to(dev), lw, "id", METHOD, 1e-3, 64, add1=a1.to(dev))
        yr, _ = _restated("id", 1.0, 1e-3, b, 11)
        ex = R.linear_exact(x + a1, w, bias)
        e_dev, e_ref = rel_l2(y, ex), rel_l2(yr, ex)
        print(f"BOSH3-384 id vs expm tol 1e-3 b {b}: device {e_dev:.3e} restatement {e_ref:.3e}")
        assert e_dev <= 1.5 * e_ref, (b, e_dev, e_ref)


@pytest.mark.parametrize("act,gain,tol,b,seed,accepted,rejected", [("relu", 4.0, 1e-3, 16, 14, 12, 1), ("relu", 2.0, 1e-4, 37, 12, 14, 0),
                                                                     ("tanh", 16.0, 1e-4, 16, 11, 22, 0)])
def test_backward_through_long_sequences(dev, act, gain, tol, b, seed, accepted, rejected):
    """Op level: twelve or more accepted steps (the FSAL adjoint flows into the step before), a rejected step (it contributes
    nothing), a partial row tile."""
    from agplace_amd import ops
    x, a1, w, bias = input_law(b, gain, seed)
    G = torch.randn(b, D, generator=torch.Generator().manual_seed(5))
    lw = ops.LinearWeights(w.to(dev), bias.to(dev), with_transpose=True)
    y, ctrl, traj = ops.fcode_adaptive(x.to(dev), lw, act, METHOD, tol, 64, add1=a1.to(dev), want_traj=True)
    gx, gw, gb = ops.fcode_adaptive_bwd(traj, ctrl, G.to(dev), lw, act, METHOD, 64)
    st = ops.ode_stats(ctrl)
    W, B = w.double().requires_grad_(True), bias.double().requires_grad_(True)
    xr = (x + a1).double().requires_grad_(True)
    yr, log = K.fcode(xr, W, B, act, tol, METHOD)
    (yr * G.double()).sum().backward()
    _precondition(log, (act, gain, tol, b, seed))
    assert [a[2] for a in st["attempts"]] == log.accepted and (st["accepted"], st["rejected"]) == (accepted, rejected), (st, log.steps)
    errs = (rel_l2(y, yr), rel_l2(gx, xr.grad), rel_l2(gw, W.grad), rel_l2(gb, B.grad))
    print(f"BOSH3-384 BWD {act} gain {gain} tol {tol} b {b}: attempts {len(log.steps)} rejected {st['rejected']} "
          f"y {errs[0]:.2e} gx {errs[1]:.2e} gw {errs[2]:.2e} gb {errs[3]:.2e}")
    assert errs[0] < 1e-4 and max(errs[1:]) < 1e-3, errs


@pytest.mark.parametrize("act", ["relu", "tanh", "sigmoid", "id"])
def test_autograd_backward_matches_autograd_through_the_restatement(dev, act):
    """An FCODE(384) block with bosh3 and default initialisation, called as a module: x, add1, weight and bias gradients.
    relu: the derivative at a pre-activation within the device's resolution of 0 is the device's own choice
    (rk_adaptive_ref.relu_kinks); at b = 35 the fp64 run has z = 3.79e-6 at (stage 4 of step 1, row 2, feature 219), the
    device's k there is 0, and that one element is worth 8.7e-4 (gx), 2.4e-3 (gw, gb) of the gradients' norms -- measured on
    the device against the plain reference and reproduced in fp64 by flipping that one derivative."""
    from agplace_amd import ops
    from agplace_amd.network_mm.ffns import FCODE
    g = torch.Generator().manual_seed(21)
    torch.manual_seed(1)
    for b in (5, 16, 35):
        m = FCODE(D, act, opt=_options()).to(dev)
        x = torch.randn(b, D, generator=g)
        a1 = torch.randn(b, D, generator=g) * 0.3
        G = torch.randn(b, D, generator=g)
        xd, a1d = x.to(dev).requires_grad_(True), a1.to(dev).requires_grad_(True)
        y = m(xd, add1=a1d)
        (y * G.to(dev)).sum().backward()
        st = m.solver_stats()
        W = m.func.func.fc.weight.detach().cpu().double().requires_grad_(True)
        B = m.func.func.fc.bias.detach().cpu().double().requires_grad_(True)
        xr = x.double().requires_grad_(True)
        slopes, kinks = None, (0, 0)
        if act == "relu":      # pre-activations the device cannot tell from 0 (rk_adaptive_ref.relu_kinks): its own choice there
            with torch.no_grad():
                _, log0 = K.fcode(x.double() + a1.double(), W, B, act, 1e-3, METHOD)
                _, _, traj = ops.fcode_adaptive(x.to(dev), m._prep.get(with_transpose=True), act, METHOD, 1e-3, 64,
                                                add1=a1.to(dev), want_traj=True)
            slopes, kinks = K.relu_kinks(log0, W, traj.view(-1, 8, b, D).cpu(), METHOD)
        yr, log = K.fcode(xr + a1.double(), W, B, act, 1e-3, METHOD, relu_slope=slopes)
        (yr * G.double()).sum().backward()
        _precondition(log, (act, b))
        assert [a[2] for a in st["attempts"]] == log.accepted and st["accepted"] >= 2
        assert kinks[0] <= 1e-3 * 13 * b * D, kinks      # the band is a sliver of the evaluated elements
        errs = (rel_l2(y, yr), rel_l2(xd.grad, xr.grad), rel_l2(a1d.grad, xr.grad), rel_l2(m.func.func.fc.weight.grad, W.grad),
                rel_l2(m.func.func.fc.bias.grad, B.grad))
        print(f"BOSH3-384 AUTOGRAD BWD {act} b {b}: steps {st['accepted']} y {errs[0]:.2e} gx {errs[1]:.2e} ga1 {errs[2]:.2e} "
              f"gw {errs[3]:.2e} gb {errs[4]:.2e} relu kinks in band {kinks[0]}, taken the device's way {kinks[1]}")
        assert errs[0] < 1e-4
        assert errs[1] < 1e-3 and errs[2] < 1e-3 and errs[3] < 1e-3 and errs[4] < 1e-3, (act, b, errs)


def test_repeatable_bits_and_independence_of_trailing_memory(dev):
    from agplace_amd import ops
    x, a1, w, bias = input_law(37, 4.0)       # no reference here: how close a ratio comes to 1 does not matter
    lw = ops.LinearWeights(w.to(dev), bias.to(dev), with_transpose=True)
    G = torch.randn(37, D, generator=torch.Generator().manual_seed(3)).to(dev)

    def run(xin, ain):
        y, ctrl, traj = ops.fcode_adaptive(xin, lw, "relu", METHOD, 1e-4, 64, add1=ain, want_traj=True)
        return (y,) + ops.fcode_adaptive_bwd(traj, ctrl, G, lw, "relu", METHOD, 64) + (ctrl,)
    first = run(x.to(dev), a1.to(dev))
    assert ops.ode_stats(first[4])["status"] == 0 and all(bool(torch.isfinite(t).all()) for t in first[:4])
    for _ in range(3):
        again = run(x.to(dev), a1.to(dev))
        assert all(torch.equal(p, q) for p, q in zip(first, again))
    # the same 37 rows at the head of larger buffers: what follows them must not matter (the last tile is padded to 48 rows)
    for fill in (float("nan"), 1e30):
        big_x = torch.full((64, D), fill, device=dev)
        big_a = torch.full((64, D), fill, device=dev)
        big_x[:37], big_a[:37] = x.to(dev), a1.to(dev)
        y, ctrl = ops.fcode_adaptive(big_x[:37], lw, "relu", METHOD, 1e-4, 64, add1=big_a[:37])
        assert torch.equal(y, first[0]) and torch.equal(ctrl, first[4])


def test_solve_inside_a_captured_graph(dev):
    """One launch, no host round trip: the solve replays from a captured graph, with a data-dependent step count."""
    from agplace_amd import ops
    x, a1, w, bias = input_law(16, 4.0)
    lw = ops.LinearWeights(w.to(dev), bias.to(dev))
    inputs = [(x * s).to(dev) for s in (1.0, 0.05, 6.0)]
    eager = [ops.fcode_adaptive(xi, lw, "relu", METHOD, 1e-4, 64, add1=a1.to(dev)) for xi in inputs]
    counts = [ops.ode_stats(c)["attempted"] for _, c in eager]
    print(f"BOSH3-384 captured: attempted steps {counts}")
    assert all(ops.ode_stats(c)["status"] == 0 for _, c in eager) and len(set(counts)) > 1, counts
    xs, a1s = inputs[0].clone(), a1.to(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.fcode_adaptive(xs, lw, "relu", METHOD, 1e-4, 64, add1=a1s)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ys, ctrls = ops.fcode_adaptive(xs, lw, "relu", METHOD, 1e-4, 64, add1=a1s)
    for xi, (ye, ce) in zip(inputs, eager):
        xs.copy_(xi)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(ys, ye) and torch.equal(ctrls, ce)


def test_step_cap_gives_nan_and_a_status(dev):
    """odeint_max_steps = 2 on a solve that needs four steps: a clean return, NaN output, solver_stats() raises."""
    from agplace_amd import ops
    from agplace_amd.network_mm.ffns import FCODE
    x, a1, w, bias = input_law(16)
    assert len(_restated("relu", 1.0, 1e-3, 16, 11)[1].steps) == 4
    ok = FCODE(D, "relu", opt=_options(tol=1e-3)).to(dev)
    capped = FCODE(D, "relu", opt=_options(tol=1e-3, odeint_max_steps=2)).to(dev)
    ok.load_state_dict({"func.func.fc.weight": w, "func.func.fc.bias": bias})
    capped.load_state_dict(ok.state_dict())
    with torch.no_grad():
        y = ok(x.to(dev), add1=a1.to(dev))
        assert bool(torch.isfinite(y).all()) and ok.solver_stats()["attempted"] == 4
        yc = capped(x.to(dev), add1=a1.to(dev))
    assert bool(torch.isnan(yc).all())
    with pytest.raises(RuntimeError, match="odeint_max_steps"):
        capped.solver_stats()
    assert ops.ode_stats(capped._ctrl)["status"] == 1 and ops.ode_stats(capped._ctrl)["attempted"] == 2
    # training through a failed solve: NaN gradients, no fault
    xd = x.to(dev).requires_grad_(True)
    capped(xd, add1=a1.to(dev)).sum().backward()
    assert bool(torch.isnan(xd.grad).all()) and bool(torch.isnan(capped.func.func.fc.weight.grad).all())
    assert bool(torch.isnan(capped.func.func.fc.bias.grad).all())
    torch.cuda.synchronize()


def test_refusals(dev):
    from agplace_amd import _lib
    from agplace_amd.network_mm.ffns import FCODE
    from agplace_amd.options import Options
    # without Options.fcode_wide FCODE(384) keeps refusing an adaptive method, by name
    m = FCODE(D, "relu", opt=Options(odeint_method=METHOD, odeint_adaptive_family=True)).to(dev)
    with pytest.raises(NotImplementedError, match=METHOD):
        m(torch.zeros(4, D, device=dev))
    # the C entry points: every refusal returns before any launch (the outputs keep their poison)
    L = _lib.load()
    b, cap = 16, 8
    x = torch.zeros(b, D, device=dev)
    planes = torch.zeros(2, D * D, dtype=torch.bfloat16, device=dev)
    y = torch.full((b, D), -3.0, device=dev)
    ring = torch.empty(2 * 8 * b * D, device=dev)
    ctrl = torch.full((L.agp_fcode_adaptive_ctrl_bytes(cap),), 7, dtype=torch.uint8, device=dev)
    bosh3 = _lib.ODE_ADAPTIVE[METHOD]

    def fwd(bb=b, d=D, tol=1e-3, max_steps=cap, method=bosh3):
        return L.agp_fcode_adaptive_wide_fwd(x.data_ptr(), None, None, planes[0].data_ptr(), planes[1].data_ptr(), None, bb, d,
                                             _lib.ACT["relu"], method, ctypes.c_double(tol), ctypes.c_double(tol), max_steps,
                                             y.data_ptr(), ring.data_ptr(), 0, ctrl.data_ptr(), _lib.stream())
    assert fwd(d=256) == _lib.E_UNSUPPORTED
    assert fwd(bb=0) == 1 and fwd(max_steps=0) == 1 and fwd(tol=0.0) == 1 and fwd(method=5) == 1 and fwd(method=2) == 1
    ws = torch.empty(L.agp_fcode_adaptive_wide_bwd_workspace_bytes(b, D, cap), dtype=torch.uint8, device=dev)
    gx = torch.full((b, D), -3.0, device=dev)

    def bwd(bb=b, d=D, max_steps=cap, nbytes=ws.numel(), method=bosh3):
        return L.agp_fcode_adaptive_wide_bwd(ring.data_ptr(), ctrl.data_ptr(), x.data_ptr(), planes[0].data_ptr(),
                                             planes[1].data_ptr(), bb, d, _lib.ACT["relu"], method, max_steps,
                                             gx.data_ptr(), None, None, ws.data_ptr(), nbytes, _lib.stream())
    assert bwd(d=256) == _lib.E_UNSUPPORTED
    assert bwd(bb=0) == 1 and bwd(max_steps=0) == 1 and bwd(nbytes=ws.numel() - 1) == 1 and bwd(method=5) == 1
    torch.cuda.synchronize()
    assert bool((y == -3.0).all()) and bool((gx == -3.0).all()) and bool((ctrl == 7).all())
