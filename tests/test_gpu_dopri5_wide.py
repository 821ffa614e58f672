"""-m gpu tests of the adaptive dopri5 solver at 384 columns (agp_fcode_adaptive_wide_fwd / _bwd, csrc/fusion_adaptive.hip)
against the fp64 restatement in tests/dopri5_ref.py, and of the 256-column route against a dump of the build before it.

Bounds: those tests/test_gpu_dopri5.py holds the same arithmetic to at 256 columns.  Output: rel_l2 < 1e-4.  Step sizes: every
attempted dt within 1e-3 relative of the restatement's at tol = 1e-3 and within 0.15 at tol = 1e-4.  Decisions: the accept /
reject sequence equals the restatement's; every parity case asserts ON THE REFERENCE RUN that no attempted step's ratio lies
within 0.05 of 1 (a decision that close may flip in fp32) and that the last accepted step overshoots t = 1.  Gradients:
rel_l2 < 1e-3 against fp64 autograd through the restatement.  Each case prints its figures.
MEASURED (MI355X, the 38 forward cases below): the accept / reject sequence equals the restatement's in every case; worst dt
difference 4.6e-5 at tol = 1e-3 (relu, gain 8, seed 14) and 6.8e-2 at tol = 1e-4 (id, gain 1, b = 16, the second step: the first
step's ratio is 5e-6, an error estimate at fp32 rounding noise, and its factor 0.9 ratio^(-1/5) = 10.2 stands at the growth limit of
10 -- 6.3e-2 .. 6.8e-2 at all four b; the other activations and the long sequences stay within 3.1e-4); worst output difference 1.15e-5 (the same
id case; 5.1e-6 elsewhere).  Against the matrix exponential the device's error is 1.887e-4 .. 1.964e-4 at tol = 1e-3 (the
restatement's own 1.886e-4 .. 1.964e-4) and 3.91e-5 .. 4.17e-5 at 1e-4 (4.11e-5 .. 4.35e-5).  Gradients: worst 9.2e-5 (gb, tanh,
gain 16, seven steps), otherwise within 5.7e-6 at the op level and within 5.4e-6 through autograd_ops.FCODEFn."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest
import torch

import dopri5_ref as R
from gpu_util import rel_l2

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
D = 384
DT_BOUND = {1e-3: 1e-3, 1e-4: 0.15}
# (act, gain, tol, b, seed, attempts, rejected) of the restatement: stiffer weights, rejected steps, up to 12 attempts
LONG = [("relu", 4.0, 1e-4, 16, 11, 9, 1), ("id", 4.0, 1e-4, 16, 11, 8, 1), ("id", 4.0, 1e-4, 37, 12, 8, 1),
        ("relu", 8.0, 1e-3, 16, 12, 11, 3), ("relu", 8.0, 1e-3, 16, 14, 12, 3), ("tanh", 16.0, 1e-4, 16, 11, 7, 0)]


@functools.lru_cache(maxsize=None)
def input_law(b, gain=1.0, seed=11):
    """x, add1, w = randn / sqrt(384) * gain, bias: CPU tensors, shared and never modified."""
    g = torch.Generator().manual_seed(seed)
    x, a1 = torch.randn(b, D, generator=g), torch.randn(b, D, generator=g) * 0.5
    w = torch.randn(D, D, generator=g) / math.sqrt(D) * gain
    bias = torch.randn(D, generator=g) * 0.1
    return x, a1, w, bias


@functools.lru_cache(maxsize=None)
def _restated(act, gain, tol, b, seed):
    """(y, log) of the fp64 restatement, once per case."""
    x, a1, w, bias = input_law(b, gain, seed)
    with torch.no_grad():
        return R.fcode((x + a1).double(), w, bias, act, tol)


def _precondition(log, tag):
    margin = min(abs(r - 1) for r in log.ratios)
    assert margin > 0.05, ("precondition: a reference ratio within 0.05 of 1", tag, log.ratios)
    assert log.accepted[-1] and log.steps[-1][0] + log.steps[-1][1] > 1.0, tag                 # the interpolant is exercised
    return margin


def _solve_and_compare(dev, act, gain, tol, b, seed=11):
    from agplace_amd import ops
    x, a1, w, bias = input_law(b, gain, seed)
    lw = ops.LinearWeights(w.to(dev), bias.to(dev))
    y, ctrl = ops.fcode_adaptive(x.to(dev), lw, act, "dopri5", tol, 64, add1=a1.to(dev))
    st = ops.ode_stats(ctrl)
    yr, log = _restated(act, gain, tol, b, seed)
    tag = (act, gain, tol, b, seed)
    margin = _precondition(log, tag)
    assert st["status"] == 0, (tag, st)
    assert [a[2] for a in st["attempts"]] == log.accepted, (tag, st["attempts"], log.steps)
    assert st["f_evals"] == log.f_evals and st["accepted"] == sum(log.accepted) and st["rejected"] == len(log.steps) - sum(log.accepted)
    dtrel = max(abs(a[0] - s[1]) / s[1] for a, s in zip(st["attempts"], log.steps))
    err = rel_l2(y, yr)
    print(f"DOPRI5-384 {act} gain {gain} tol {tol} b {b} seed {seed}: attempts {len(log.steps)} rejected {st['rejected']} "
          f"margin {margin:.3f} dt rel {dtrel:.2e} out rel_l2 {err:.2e} t1 {st['t1']:.4f}")
    assert [d for d, a in zip([a[0] for a in st["attempts"]], log.accepted) if a] == st["dts"]
    assert abs(st["t1"] - (log.steps[-1][0] + log.steps[-1][1])) < DT_BOUND[tol] * 2
    assert dtrel < DT_BOUND[tol], (tag, dtrel)
    assert err < 1e-4, (tag, err)
    return st, log


@pytest.mark.parametrize("tol", [1e-3, 1e-4])
@pytest.mark.parametrize("act", ["relu", "tanh", "sigmoid", "id"])
def test_forward_matches_the_restatement(dev, act, tol):
    """One row tile with dead rows, one full tile, three tiles with a partial last one, four full tiles."""
    for b in (3, 16, 37, 64):
        _solve_and_compare(dev, act, 1.0, tol, b)


@pytest.mark.parametrize("act,gain,tol,b,seed,attempts,rejected", LONG)
def test_forward_with_rejections_and_long_sequences(dev, act, gain, tol, b, seed, attempts, rejected):
    st, log = _solve_and_compare(dev, act, gain, tol, b, seed)
    assert (len(log.steps), st["rejected"]) == (attempts, rejected)


@pytest.mark.parametrize("tol", [1e-3, 1e-4])
def test_identity_against_the_matrix_exponential(dev, tol):
    """act = id has an exact answer: the device's error against it is at most 1.5 x the fp64 restatement's own, as at 256."""
    from agplace_amd import ops
    for b in (3, 16, 37, 64):
        x, a1, w, bias = input_law(b)
        lw = ops.LinearWeights(w.to(dev), bias.to(dev))
        y, _ = ops.fcode_adaptive(x.to(dev), lw, "id", "dopri5", tol, 64, add1=a1.to(dev))
        yr, _ = _restated("id", 1.0, tol, b, 11)
        ex = R.linear_exact(x + a1, w, bias)
        e_dev, e_ref = rel_l2(y, ex), rel_l2(yr, ex)
        print(f"DOPRI5-384 id vs expm tol {tol} b {b}: device {e_dev:.3e} restatement {e_ref:.3e}")
        assert e_dev <= 1.5 * e_ref, (tol, b, e_dev, e_ref)


@pytest.mark.parametrize("act,gain,b,seed,accepted,rejected", [("relu", 4.0, 16, 11, 8, 1), ("id", 4.0, 37, 12, 7, 1),
                                                                 ("tanh", 16.0, 16, 11, 7, 0)])
def test_backward_through_long_sequences(dev, act, gain, b, seed, accepted, rejected):
    """Op level, tol = 1e-4: seven or more accepted steps (the FSAL adjoint flows into the step before), a rejected step
    (it contributes nothing), a partial row tile."""
    from agplace_amd import ops
    x, a1, w, bias = input_law(b, gain, seed)
    G = torch.randn(b, D, generator=torch.Generator().manual_seed(5))
    lw = ops.LinearWeights(w.to(dev), bias.to(dev), with_transpose=True)
    y, ctrl, traj = ops.fcode_adaptive(x.to(dev), lw, act, "dopri5", 1e-4, 64, add1=a1.to(dev), want_traj=True)
    gx, gw, gb = ops.fcode_adaptive_bwd(traj, ctrl, G.to(dev), lw, act, "dopri5", 64)
    st = ops.ode_stats(ctrl)
    W, B = w.double().requires_grad_(True), bias.double().requires_grad_(True)
    xr = (x + a1).double().requires_grad_(True)
    yr, log = R.fcode(xr, W, B, act, 1e-4)
    (yr * G.double()).sum().backward()
    _precondition(log, (act, gain, b, seed))
    assert [a[2] for a in st["attempts"]] == log.accepted and (st["accepted"], st["rejected"]) == (accepted, rejected), (st, log.steps)
    errs = (rel_l2(y, yr), rel_l2(gx, xr.grad), rel_l2(gw, W.grad), rel_l2(gb, B.grad))
    print(f"DOPRI5-384 BWD {act} gain {gain} b {b}: attempts {len(log.steps)} rejected {st['rejected']} "
          f"y {errs[0]:.2e} gx {errs[1]:.2e} gw {errs[2]:.2e} gb {errs[3]:.2e}")
    assert errs[0] < 1e-4 and max(errs[1:]) < 1e-3, errs


def _solve(m, x, add1=None):
    """The block's solve through the autograd layer.  FCODE.forward itself keeps its refusal of dopri5 at 384 columns
    (tests/test_gpu_fcode_wide.py holds it to that), so the block's parameters, options and control block enter here."""
    from agplace_amd import autograd_ops
    fc = m.func.func.fc
    return autograd_ops.FCODEFn.apply(x, fc.weight, fc.bias, m, add1, None)


@pytest.mark.parametrize("act", ["relu", "tanh", "sigmoid", "id"])
def test_autograd_backward_matches_autograd_through_the_restatement(dev, act):
    """An FCODE(384) block with dopri5 and default initialisation through autograd_ops.FCODEFn: x, add1, weight and bias
    gradients."""
    from agplace_amd.network_mm.ffns import FCODE
    from agplace_amd.options import Options
    g = torch.Generator().manual_seed(21)
    torch.manual_seed(1)
    for b in (5, 16, 35):
        m = FCODE(D, act, opt=Options(odeint_method="dopri5")).to(dev)
        x = torch.randn(b, D, generator=g)
        a1 = torch.randn(b, D, generator=g) * 0.3
        G = torch.randn(b, D, generator=g)
        xd, a1d = x.to(dev).requires_grad_(True), a1.to(dev).requires_grad_(True)
        y = _solve(m, xd, a1d)
        (y * G.to(dev)).sum().backward()
        st = m.solver_stats()
        W = m.func.func.fc.weight.detach().cpu().double().requires_grad_(True)
        B = m.func.func.fc.bias.detach().cpu().double().requires_grad_(True)
        xr = x.double().requires_grad_(True)
        yr, log = R.fcode(xr + a1.double(), W, B, act, 1e-3)
        (yr * G.double()).sum().backward()
        _precondition(log, (act, b))
        assert [a[2] for a in st["attempts"]] == log.accepted and st["accepted"] >= 2
        errs = (rel_l2(y, yr), rel_l2(xd.grad, xr.grad), rel_l2(a1d.grad, xr.grad), rel_l2(m.func.func.fc.weight.grad, W.grad),
                rel_l2(m.func.func.fc.bias.grad, B.grad))
        print(f"DOPRI5-384 AUTOGRAD BWD {act} b {b}: steps {st['accepted']} y {errs[0]:.2e} gx {errs[1]:.2e} ga1 {errs[2]:.2e} "
              f"gw {errs[3]:.2e} gb {errs[4]:.2e}")
        assert errs[0] < 1e-4
        assert errs[1] < 1e-3 and errs[2] < 1e-3 and errs[3] < 1e-3 and errs[4] < 1e-3, (act, b, errs)


def test_repeatable_bits_and_independence_of_trailing_memory(dev):
    from agplace_amd import ops
    x, a1, w, bias = input_law(37, 4.0)       # no reference here: how close a ratio comes to 1 does not matter
    lw = ops.LinearWeights(w.to(dev), bias.to(dev), with_transpose=True)
    G = torch.randn(37, D, generator=torch.Generator().manual_seed(3)).to(dev)

    def run(xin, ain):
        y, ctrl, traj = ops.fcode_adaptive(xin, lw, "relu", "dopri5", 1e-4, 64, add1=ain, want_traj=True)
        return (y,) + ops.fcode_adaptive_bwd(traj, ctrl, G, lw, "relu", "dopri5", 64) + (ctrl,)
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
        y, ctrl = ops.fcode_adaptive(big_x[:37], lw, "relu", "dopri5", 1e-4, 64, add1=big_a[:37])
        assert torch.equal(y, first[0]) and torch.equal(ctrl, first[4])


def test_solve_inside_a_captured_graph(dev):
    """One launch, no host round trip: the solve replays from a captured graph, with a data-dependent step count."""
    from agplace_amd import ops
    x, a1, w, bias = input_law(16, 4.0)
    lw = ops.LinearWeights(w.to(dev), bias.to(dev))
    inputs = [(x * s).to(dev) for s in (1.0, 0.05, 6.0)]
    eager = [ops.fcode_adaptive(xi, lw, "relu", "dopri5", 1e-4, 64, add1=a1.to(dev)) for xi in inputs]
    counts = [ops.ode_stats(c)["attempted"] for _, c in eager]
    print(f"DOPRI5-384 captured: attempted steps {counts}")
    assert len(set(counts)) > 1, counts
    xs, a1s = inputs[0].clone(), a1.to(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.fcode_adaptive(xs, lw, "relu", "dopri5", 1e-4, 64, add1=a1s)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ys, ctrls = ops.fcode_adaptive(xs, lw, "relu", "dopri5", 1e-4, 64, add1=a1s)
    for xi, (ye, ce) in zip(inputs, eager):
        xs.copy_(xi)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(ys, ye) and torch.equal(ctrls, ce)


def test_step_cap_gives_nan_and_a_status(dev):
    """odeint_max_steps = 2 on a solve that needs three steps: a clean return, NaN output, solver_stats() raises (the block
    through the autograd layer, see _solve)."""
    from agplace_amd import ops
    from agplace_amd.network_mm.ffns import FCODE
    from agplace_amd.options import Options
    x, a1, w, bias = input_law(16)
    assert len(_restated("relu", 1.0, 1e-3, 16, 11)[1].steps) == 3
    ok = FCODE(D, "relu", opt=Options(odeint_method="dopri5", tol=1e-3)).to(dev)
    capped = FCODE(D, "relu", opt=Options(odeint_method="dopri5", tol=1e-3, odeint_max_steps=2)).to(dev)
    ok.load_state_dict({"func.func.fc.weight": w, "func.func.fc.bias": bias})
    capped.load_state_dict(ok.state_dict())
    with torch.no_grad():
        y = _solve(ok, x.to(dev), a1.to(dev))
        assert bool(torch.isfinite(y).all()) and ok.solver_stats()["attempted"] == 3
        yc = _solve(capped, x.to(dev), a1.to(dev))
    assert bool(torch.isnan(yc).all())
    with pytest.raises(RuntimeError, match="odeint_max_steps"):
        capped.solver_stats()
    assert ops.ode_stats(capped._ctrl)["status"] == 1 and ops.ode_stats(capped._ctrl)["attempted"] == 2
    # training through a failed solve: NaN gradients, no fault
    xd = x.to(dev).requires_grad_(True)
    _solve(capped, xd, a1.to(dev)).sum().backward()
    assert bool(torch.isnan(xd.grad).all()) and bool(torch.isnan(capped.func.func.fc.weight.grad).all())
    assert bool(torch.isnan(capped.func.func.fc.bias.grad).all())
    torch.cuda.synchronize()


def test_refusals(dev):
    from agplace_amd import _lib, ops
    w = torch.randn(128, 128, generator=torch.Generator().manual_seed(1)) / 12
    lw = ops.LinearWeights(w.to(dev), torch.zeros(128).to(dev), with_transpose=True)
    with pytest.raises(NotImplementedError, match="256.*384"):
        ops.fcode_adaptive(torch.zeros(4, 128, device=dev), lw, "relu", "dopri5", 1e-3, 64)
    with pytest.raises(NotImplementedError, match="256.*384"):
        ops.fcode_adaptive_bwd(torch.zeros(1, device=dev), torch.zeros(64, dtype=torch.uint8, device=dev),
                               torch.zeros(4, 128, device=dev), lw, "relu", "dopri5", 64)
    # the C entry point: every refusal returns before any launch (the output keeps its poison)
    L = _lib.load()
    b, cap = 16, 8
    x = torch.zeros(b, D, device=dev)
    planes = torch.zeros(2, D * D, dtype=torch.bfloat16, device=dev)
    y = torch.full((b, D), -3.0, device=dev)
    ring = torch.empty(2 * 8 * b * D, device=dev)
    ctrl = torch.full((L.agp_fcode_adaptive_ctrl_bytes(cap),), 7, dtype=torch.uint8, device=dev)

    def fwd(bb=b, d=D, tol=1e-3, max_steps=cap, xp=x.data_ptr()):
        return L.agp_fcode_adaptive_wide_fwd(xp, None, None, planes[0].data_ptr(), planes[1].data_ptr(), None, bb, d,
                                             _lib.ACT["relu"], _lib.ODE_ADAPTIVE["dopri5"], ctypes.c_double(tol),
                                             ctypes.c_double(tol), max_steps, y.data_ptr(), ring.data_ptr(), 0, ctrl.data_ptr(),
                                             _lib.stream())
    assert fwd(d=256) == _lib.E_UNSUPPORTED
    assert fwd(bb=0) == 1 and fwd(max_steps=0) == 1 and fwd(tol=0.0) == 1 and fwd(xp=None) == 1
    ws = torch.empty(L.agp_fcode_adaptive_wide_bwd_workspace_bytes(b, D, cap), dtype=torch.uint8, device=dev)
    gx = torch.full((b, D), -3.0, device=dev)

    def bwd(bb=b, d=D, max_steps=cap, nbytes=ws.numel()):
        return L.agp_fcode_adaptive_wide_bwd(ring.data_ptr(), ctrl.data_ptr(), x.data_ptr(), planes[0].data_ptr(),
                                             planes[1].data_ptr(), bb, d, _lib.ACT["relu"], _lib.ODE_ADAPTIVE["dopri5"], max_steps,
                                             gx.data_ptr(), None, None, ws.data_ptr(), nbytes, _lib.stream())
    assert bwd(d=256) == _lib.E_UNSUPPORTED
    assert bwd(bb=0) == 1 and bwd(max_steps=0) == 1 and bwd(nbytes=ws.numel() - 1) == 1
    torch.cuda.synchronize()
    assert bool((y == -3.0).all()) and bool((gx == -3.0).all()) and bool((ctrl == 7).all())


def test_the_256_route_equals_the_parent_build(dev):
    """The 256-column adaptive route is untouched: y, gx, gw, gb and the control block of one solve with trajectory
    (dopri5_ref.input_law(37, 4.0), relu, tol 1e-4, cap 64, cotangent randn seed 3) are bit-equal to those of a build of the
    commit before the 384-column solver (tests/golden/fcode_adaptive_256_parent.npz, dumped on an MI355X)."""
    from agplace_amd import ops
    want = np.load(os.path.join(GOLDEN, "fcode_adaptive_256_parent.npz"))
    x, a1, w, bias = R.input_law(37, 4.0)
    G = torch.randn(37, 256, generator=torch.Generator().manual_seed(3)).to(dev)
    lw = ops.LinearWeights(w.to(dev), bias.to(dev), with_transpose=True)
    y, ctrl, traj = ops.fcode_adaptive(x.to(dev), lw, "relu", "dopri5", 1e-4, 64, add1=a1.to(dev), want_traj=True)
    gx, gw, gb = ops.fcode_adaptive_bwd(traj, ctrl, G, lw, "relu", "dopri5", 64)
    assert ops.ode_stats(ctrl)["accepted"] == 8
    for name, t in (("y", y), ("gx", gx), ("gw", gw), ("gb", gb), ("ctrl", ctrl)):
        got = t.cpu().numpy()
        assert got.dtype == want[name].dtype and np.array_equal(got, want[name]), name
