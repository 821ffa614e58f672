"""-m gpu tests of the adaptive dopri5 solver of FCODE (agp_fcode_adaptive_fwd / _bwd, csrc/fusion_adaptive.hip) against the
fp64 restatement in tests/dopri5_ref.py.

Bounds.  Output: rel_l2 < 1e-4, the bar of test_fcode_matches_oracle.  Step sizes: every attempted dt within 1e-3 relative
of the restatement's at tol = 1e-3 and within 0.15 at tol = 1e-4 (where the ratio is far below 1 the error estimate is a
cancelling sum near fp32 noise, and dt follows ratio^(-1/5)).  Decisions: the accept / reject sequence equals the
restatement's; every case asserts ON THE REFERENCE RUN that no attempted step's ratio lies in [0.95, 1.05], since a decision
that close to 1 may flip in fp32.  Measured on an MI355X (five-product f): worst dt difference 5.2e-5
at tol = 1e-3 and 1.1e-3 at tol = 1e-4 (id, b = 3), worst output difference 4.8e-6."""
import os

import numpy as np
import pytest
import torch

import dopri5_ref as R
from gpu_util import cpu_state, randomize_bn, rel_l2, to_dev
from oracle import nets

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DT_BOUND = {1e-3: 1e-3, 1e-4: 0.15}


def _solve_and_compare(dev, act, gain, tol, b):
    from agplace_amd import ops
    x, a1, w, bias = R.input_law(b, gain)
    lw = ops.LinearWeights(w.to(dev), bias.to(dev))
    y, ctrl = ops.fcode_adaptive(x.to(dev), lw, act, "dopri5", tol, 64, add1=a1.to(dev))
    st = ops.ode_stats(ctrl)
    yr, log = R.fcode((x + a1).double(), w, bias, act, tol)
    tag = (act, gain, tol, b)
    margin = min(abs(r - 1) for r in log.ratios)
    assert margin > 0.05, ("precondition: a reference ratio within 0.05 of 1", tag, log.ratios)
    assert log.steps[-1][0] + log.steps[-1][1] > 1.0, tag                 # the interpolant is exercised
    assert st["status"] == 0, (tag, st)
    assert [a[2] for a in st["attempts"]] == log.accepted, (tag, st["attempts"], log.steps)
    assert st["f_evals"] == log.f_evals and st["accepted"] == sum(log.accepted) and st["rejected"] == len(log.steps) - sum(log.accepted)
    dtrel = max(abs(a[0] - s[1]) / s[1] for a, s in zip(st["attempts"], log.steps))
    err = rel_l2(y, yr)
    print(f"DOPRI5 {act} gain {gain} tol {tol} b {b}: attempts {len(log.steps)} rejected {st['rejected']} margin {margin:.3f} "
          f"dt rel {dtrel:.2e} out rel_l2 {err:.2e} t1 {st['t1']:.4f}")
    assert [d for d, a in zip([a[0] for a in st["attempts"]], log.accepted) if a] == st["dts"]
    assert abs(st["t1"] - (log.steps[-1][0] + log.steps[-1][1])) < DT_BOUND[tol] * 2
    assert dtrel < DT_BOUND[tol], (tag, dtrel)
    assert err < 1e-4, (tag, err)
    return y, yr, st, log


@pytest.mark.parametrize("tol", [1e-3, 1e-4])
@pytest.mark.parametrize("act", ["relu", "tanh", "sigmoid", "id"])
def test_forward_matches_the_restatement(dev, act, tol):
    for b in (3, 16, 37, 64):
        _solve_and_compare(dev, act, 1.0, tol, b)


@pytest.mark.parametrize("act,gain,tol,b,attempts,rejected", [("relu", 4.0, 1e-4, 16, 9, 1), ("id", 4.0, 1e-4, 16, 8, 1),
                                                              ("id", 4.0, 1e-4, 37, 8, 1), ("relu", 8.0, 1e-3, 16, 11, 3),
                                                              ("relu", 8.0, 1e-4, 16, 20, 4)])
def test_forward_with_rejections_and_long_sequences(dev, act, gain, tol, b, attempts, rejected):
    """Stiffer weights (w = randn / 16 * gain): rejected steps, up to 20 attempted steps."""
    _, _, st, log = _solve_and_compare(dev, act, gain, tol, b)
    assert (len(log.steps), st["rejected"]) == (attempts, rejected)


@pytest.mark.parametrize("tol", [1e-3, 1e-4])
def test_identity_against_the_matrix_exponential(dev, tol):
    """act = id has an exact answer: the device's error against it is at most 1.5 x the fp64 restatement's own (1.9e-4 ..
    2.0e-4 at tol = 1e-3, 4.2e-5 at 1e-4: tests/test_dopri5_ref.py); the factor is margin for the split-bf16 f."""
    from agplace_amd import ops
    for b in (3, 16, 37, 64):
        x, a1, w, bias = R.input_law(b)
        lw = ops.LinearWeights(w.to(dev), bias.to(dev))
        y, _ = ops.fcode_adaptive(x.to(dev), lw, "id", "dopri5", tol, 64, add1=a1.to(dev))
        yr, _ = R.fcode((x + a1).double(), w, bias, "id", tol)
        ex = R.linear_exact(x + a1, w, bias)
        e_dev, e_ref = rel_l2(y, ex), rel_l2(yr, ex)
        print(f"DOPRI5 id vs expm tol {tol} b {b}: device {e_dev:.3e} restatement {e_ref:.3e}")
        assert e_dev <= 1.5 * e_ref, (tol, b, e_dev, e_ref)


@pytest.mark.parametrize("act", ["relu", "tanh", "sigmoid", "id"])
def test_backward_matches_autograd_through_the_restatement(dev, act):
    """Discretise-then-optimise through the accepted steps (step control detached), the last step through its interpolant;
    the bars and the seed discipline of test_fcode_backward_matches_autograd_oracle."""
    from agplace_amd.network_mm.ffns import FCODE
    from agplace_amd.options import Options
    g = torch.Generator().manual_seed(21)
    torch.manual_seed(1)
    for b in (5, 16, 35):
        m = FCODE(256, act, opt=Options(odeint_method="dopri5")).to(dev)
        x = torch.randn(b, 256, generator=g)
        a1 = torch.randn(b, 256, generator=g) * 0.3
        G = torch.randn(b, 256, generator=g)
        xd, a1d = x.to(dev).requires_grad_(True), a1.to(dev).requires_grad_(True)
        y = m(xd, add1=a1d)
        (y * G.to(dev)).sum().backward()
        st = m.solver_stats()
        W = m.func.func.fc.weight.detach().cpu().double().requires_grad_(True)
        B = m.func.func.fc.bias.detach().cpu().double().requires_grad_(True)
        xr = x.double().requires_grad_(True)
        yr, log = R.fcode(xr + a1.double(), W, B, act, 1e-3)
        (yr * G.double()).sum().backward()
        assert min(abs(r - 1) for r in log.ratios) > 0.05, ("precondition", act, b, log.ratios)
        assert [a[2] for a in st["attempts"]] == log.accepted and st["accepted"] >= 2
        errs = (rel_l2(y, yr), rel_l2(xd.grad, xr.grad), rel_l2(a1d.grad, xr.grad), rel_l2(m.func.func.fc.weight.grad, W.grad),
                rel_l2(m.func.func.fc.bias.grad, B.grad))
        print(f"DOPRI5 BWD {act} b {b}: steps {st['accepted']} y {errs[0]:.2e} gx {errs[1]:.2e} ga1 {errs[2]:.2e} gw {errs[3]:.2e} gb {errs[4]:.2e}")
        assert errs[0] < 1e-4
        assert errs[1] < 1e-3 and errs[2] < 1e-3 and errs[3] < 1e-3 and errs[4] < 1e-3, (act, b, errs)


@pytest.mark.parametrize("act,gain,steps,rejected", [("id", 4.0, 7, 1), ("tanh", 16.0, 7, 0)])
def test_backward_through_long_sequences(dev, act, gain, steps, rejected):
    """Seven accepted steps: the adjoint of a step's first stage flows into the step before (FSAL); a rejected step (the
    smooth saturating activations reject none on this input law, so that case is the linear one) contributes nothing."""
    from agplace_amd import ops
    x, a1, w, bias = R.input_law(16, gain)
    G = torch.randn(16, 256, generator=torch.Generator().manual_seed(5))
    lw = ops.LinearWeights(w.to(dev), bias.to(dev), with_transpose=True)
    y, ctrl, traj = ops.fcode_adaptive(x.to(dev), lw, act, "dopri5", 1e-4, 64, add1=a1.to(dev), want_traj=True)
    gx, gw, gb = ops.fcode_adaptive_bwd(traj, ctrl, G.to(dev), lw, act, "dopri5", 64)
    st = ops.ode_stats(ctrl)
    W, B = w.double().requires_grad_(True), bias.double().requires_grad_(True)
    xr = (x + a1).double().requires_grad_(True)
    yr, log = R.fcode(xr, W, B, act, 1e-4)
    (yr * G.double()).sum().backward()
    assert min(abs(r - 1) for r in log.ratios) > 0.05, ("precondition", log.ratios)
    assert [a[2] for a in st["attempts"]] == log.accepted and (st["accepted"], st["rejected"]) == (steps, rejected), (st, log.steps)
    errs = (rel_l2(y, yr), rel_l2(gx, xr.grad), rel_l2(gw, W.grad), rel_l2(gb, B.grad))
    print(f"DOPRI5 BWD {act} gain {gain}: attempts {len(log.steps)} rejected {st['rejected']} errs {errs}")
    assert errs[0] < 1e-4 and max(errs[1:]) < 1e-3, errs


def test_repeatable_bits_and_independence_of_trailing_memory(dev):
    from agplace_amd import ops
    x, a1, w, bias = R.input_law(37, 4.0)       # no reference here: how close a ratio comes to 1 does not matter
    lw = ops.LinearWeights(w.to(dev), bias.to(dev), with_transpose=True)
    G = torch.randn(37, 256, generator=torch.Generator().manual_seed(3)).to(dev)

    def run(xin, ain):
        y, ctrl, traj = ops.fcode_adaptive(xin, lw, "relu", "dopri5", 1e-4, 64, add1=ain, want_traj=True)
        return (y,) + ops.fcode_adaptive_bwd(traj, ctrl, G, lw, "relu", "dopri5", 64) + (ctrl,)
    first = run(x.to(dev), a1.to(dev))
    for _ in range(3):
        again = run(x.to(dev), a1.to(dev))
        assert all(torch.equal(p, q) for p, q in zip(first, again))
    # the same 37 rows at the head of larger buffers: what follows them must not matter (the last tile is padded to 48 rows)
    for fill in (float("nan"), 1e30):
        big_x = torch.full((64, 256), fill, device=dev)
        big_a = torch.full((64, 256), fill, device=dev)
        big_x[:37], big_a[:37] = x.to(dev), a1.to(dev)
        y, ctrl = ops.fcode_adaptive(big_x[:37], lw, "relu", "dopri5", 1e-4, 64, add1=big_a[:37])
        assert torch.equal(y, first[0]) and torch.equal(ctrl, first[4])


def test_solve_inside_a_captured_graph(dev):
    """One launch, no host round trip: the solve replays from a captured graph, with a data-dependent step count."""
    from agplace_amd import ops
    x, a1, w, bias = R.input_law(16, 4.0)
    lw = ops.LinearWeights(w.to(dev), bias.to(dev))
    inputs = [(x * s).to(dev) for s in (1.0, 0.05, 6.0)]
    eager = [ops.fcode_adaptive(xi, lw, "relu", "dopri5", 1e-4, 64, add1=a1.to(dev)) for xi in inputs]
    counts = [ops.ode_stats(c)["attempted"] for _, c in eager]
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
    """odeint_max_steps = 2 on a solve that needs three steps: a clean return, NaN output, solver_stats() raises."""
    from agplace_amd import ops
    from agplace_amd.network_mm.ffns import FCODE
    from agplace_amd.options import Options
    torch.manual_seed(1)
    x, a1, _, _ = R.input_law(16)
    ok = FCODE(256, "relu", opt=Options(odeint_method="dopri5")).to(dev)
    capped = FCODE(256, "relu", opt=Options(odeint_method="dopri5", odeint_max_steps=2)).to(dev)
    capped.load_state_dict(ok.state_dict())
    with torch.no_grad():
        y = ok(x.to(dev), add1=a1.to(dev))
        assert bool(torch.isfinite(y).all()) and ok.solver_stats()["attempted"] > 2
        yc = capped(x.to(dev), add1=a1.to(dev))
    assert bool(torch.isnan(yc).all())
    with pytest.raises(RuntimeError, match="odeint_max_steps"):
        capped.solver_stats()
    assert ops.ode_stats(capped._ctrl)["status"] == 1 and ops.ode_stats(capped._ctrl)["attempted"] == 2
    # training through a failed solve: NaN gradients, no fault
    xd = x.to(dev).requires_grad_(True)
    capped(xd, add1=a1.to(dev)).sum().backward()
    assert bool(torch.isnan(xd.grad).all()) and bool(torch.isnan(capped.func.func.fc.weight.grad).all())
    torch.cuda.synchronize()


def _restated_odeint(tol):
    def odeint(f, y0, method, step_size, dt_dtype=torch.float32):
        assert method == "dopri5"
        return R.solve(f, y0, tol, dtype=y0.dtype)[0]
    return odeint


@pytest.mark.parametrize("prec,tol", [(3, 5e-5), (2, 2e-4), (4, 1e-3)])
def test_mm_inference_with_dopri5(dev, prec, tol, monkeypatch):
    """MM with odeint_method = 'dopri5' runs its vector path per op (the fused vector program refuses an adaptive solver) and
    equals the oracle with its fixed-grid integrator replaced by the restatement, at the bars of test_mm_precision_modes."""
    from agplace_amd import vecprog
    from agplace_amd.network_mm.mm import MM
    from agplace_amd.options import Options
    from oracle import ode
    opt = Options(mfma_precision=prec, odeint_method="dopri5")
    torch.manual_seed(3)
    model = randomize_bn(MM(opt=opt)).to(dev).eval()
    data = nets.synth_query(2, 64, 128, opt, seed=6)
    ran = []
    real = vecprog.VecProgram.run
    monkeypatch.setattr(vecprog.VecProgram, "run", lambda self, *a, **k: (ran.append(1), real(self, *a, **k))[1])
    with torch.no_grad():
        out = model(to_dev(data, dev), mode="q")
    assert not ran, "the fused vector program ran an adaptive solve"
    blocks = [m for m in model.modules() if getattr(m, "adaptive", False)]
    assert blocks and all(m.solver_stats()["status"] == 0 for m in blocks)
    monkeypatch.setattr(ode, "odeint_fixed", _restated_odeint(opt.tol))
    ref = nets.mm_forward_q(data, cpu_state(model), opt)
    err = rel_l2(out["embedding"], ref["embedding"])
    print(f"DOPRI5 MM prec {prec} embedding rel_l2 {err:.2e}, {len(blocks)} adaptive blocks")
    assert err < tol


def test_mm_training_step_with_dopri5(dev):
    """One training step fills every gradient the euler run fills."""
    from agplace_amd.network_mm.mm import MM
    from agplace_amd.options import Options
    filled = {}
    for method in ("euler", "dopri5"):
        opt = Options(odeint_method=method)
        torch.manual_seed(23)
        mq = MM(opt=opt).to(dev).train()
        data = to_dev(nets.synth_query(2, 64, 128, opt, seed=6), dev)
        out = mq(data, mode="q")
        (out["embedding"] ** 2).sum().backward()
        filled[method] = {n for n, p in mq.named_parameters() if p.grad is not None}
        assert all(bool(torch.isfinite(p.grad).all()) for p in mq.parameters() if p.grad is not None), method
        if method == "dopri5":
            blocks = [m for m in mq.modules() if getattr(m, "adaptive", False)]
            assert blocks and all(m.solver_stats()["accepted"] >= 1 for m in blocks)
            assert all(float(m.func.func.fc.weight.grad.abs().max()) > 0 for m in blocks)
    assert filled["dopri5"] == filled["euler"] and len(filled["euler"]) > 50


def test_fixed_grid_outputs_equal_the_parent_build(dev):
    """The fixed-grid solver is untouched: euler / 0.1 (relu) and rk4 / 0.25 (tanh) outputs of ops.fcode are bit-equal to those
    of a build of the commit before the adaptive solver (tests/golden/fcode_fixed_grid_parent.npy, dumped on an MI355X)."""
    from agplace_amd import ops
    want = np.load(os.path.join(GOLDEN, "fcode_fixed_grid_parent.npy"))
    g = torch.Generator().manual_seed(77)
    x, a1 = torch.randn(37, 256, generator=g), torch.randn(37, 256, generator=g) * 0.5
    w = torch.randn(256, 256, generator=g) / 16
    bias = torch.randn(256, generator=g) * 0.1
    lw = ops.LinearWeights(w.to(dev), bias.to(dev))
    for i, (method, step, act) in enumerate((("euler", 0.1, "relu"), ("rk4", 0.25, "tanh"))):
        y = ops.fcode(x.to(dev), lw, act, method, ops.ode_grid_dts(step), add1=a1.to(dev)).cpu().numpy()
        assert np.array_equal(y, want[i]), (method, float(np.abs(y - want[i]).max()))
