"""-m gpu tests of the adaptive bosh3 solver of FCODE at 256 columns (agp_fcode_adaptive_fwd / _bwd with AGP_ODE_BOSH3, the
Tableau Bosh3 of csrc/fusion_adaptive.hip) against the fp64 restatement in tests/rk_adaptive_ref.py.  Structure, bars and seed
discipline are those of tests/test_gpu_dopri5.py.

Bounds.  Output: rel_l2 < 1e-4, the bar of test_fcode_matches_oracle.  Gradients: rel_l2 < 1e-3 against fp64 autograd through
the restatement.  Decisions: the accept / reject sequence equals the restatement's; every parity case asserts ON THE REFERENCE
RUN that no attempted step's ratio lies within 0.05 of 1 (a decision that close may flip in fp32), that the last accepted step
overshoots t = 1 and that the solve attempts at most 64 steps.  Step sizes: every attempted dt within DT_BOUND[tol] relative of
the restatement's; the bound is twice the worst difference measured on an MI355X over the forward cases of this file, rounded
up to one significant digit (dt follows ratio^(-1/3) here, not ratio^(-1/5), so dopri5's bound does not carry over).
MEASURED (MI355X, the 33 forward cases below): the accept / reject sequence equals the restatement's in every case; worst dt
difference 3.31e-5 at tol = 1e-3 (relu, gain 8, seed 12, 31 attempts) and 2.26e-4 at tol = 1e-4 (relu, gain 1, b = 3), so the
bounds are 7e-5 and 5e-4; worst output difference 4.2e-6.  Against the matrix exponential the device's error equals the
restatement's own to four digits (1.438e-3 .. 1.553e-3: the interpolant's crude mid-point).  Gradients:
worst 6.8e-5 (gw, tanh, gain 16, ten steps), otherwise within 3.5e-6.  MM (mfma_precision = 3): 3.6e-6."""
import ctypes
import functools

import pytest
import torch

import dopri5_ref as R
import rk_adaptive_ref as K
from gpu_util import cpu_state, randomize_bn, rel_l2, to_dev
from oracle import nets

pytestmark = pytest.mark.gpu
METHOD = "bosh3"
# worst relative dt difference over the forward cases of this file on an MI355X, per tol, and the bound: twice that, rounded up
DT_MEASURED = {1e-3: 3.31e-5, 1e-4: 2.26e-4}
DT_BOUND = {1e-3: 7e-5, 1e-4: 5e-4}
# (act, gain, tol, b, seed, attempts, rejected) of the restatement: stiffer weights, rejected steps, up to 31 attempts
LONG = [("relu", 4.0, 1e-3, 37, 15, 13, 1), ("relu", 8.0, 1e-3, 16, 12, 31, 5), ("relu", 3.0, 1e-4, 16, 17, 21, 1),
        ("id", 2.0, 1e-3, 37, 14, 8, 1), ("tanh", 8.0, 1e-4, 16, 11, 16, 0)]


@functools.lru_cache(maxsize=None)
def _restated(act, gain, tol, b, seed):
    """(y, log) of the fp64 restatement, once per case."""
    x, a1, w, bias = R.input_law(b, gain, seed)
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
    x, a1, w, bias = R.input_law(b, gain, seed)
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
    print(f"BOSH3 {act} gain {gain} tol {tol} b {b} seed {seed}: attempts {len(log.steps)} rejected {st['rejected']} "
          f"margin {margin:.3f} dt rel {dtrel:.2e} out rel_l2 {err:.2e} t1 {st['t1']:.4f}")
    assert [d for d, a in zip([a[0] for a in st["attempts"]], log.accepted) if a] == st["dts"]
    assert abs(st["t1"] - (log.steps[-1][0] + log.steps[-1][1])) < DT_BOUND[tol] * 2
    assert dtrel < DT_BOUND[tol], (tag, dtrel)
    assert err < 1e-4, (tag, err)
    return st, log


@pytest.mark.parametrize("act,tol", [("relu", 1e-3), ("relu", 1e-4), ("tanh", 1e-3), ("tanh", 1e-4), ("sigmoid", 1e-3),
                                     ("sigmoid", 1e-4), ("id", 1e-3)])
def test_forward_matches_the_restatement(dev, act, tol):
    """One row tile with dead rows, one full tile, three tiles with a partial last one, four full tiles.  (id at tol = 1e-4
    is left out: the restatement's own ratios come within 0.004 .. 0.03 of 1 there.)"""
    for b in (3, 16, 37, 64):
        _solve_and_compare(dev, act, 1.0, tol, b)


@pytest.mark.parametrize("act,gain,tol,b,seed,attempts,rejected", LONG)
def test_forward_with_rejections_and_long_sequences(dev, act, gain, tol, b, seed, attempts, rejected):
    st, log = _solve_and_compare(dev, act, gain, tol, b, seed)
    assert (len(log.steps), st["rejected"]) == (attempts, rejected)


def test_identity_against_the_matrix_exponential(dev):
    """act = id has an exact answer: the device's error against it is at most 1.5 x the fp64 restatement's own (dopri5's
    factor: margin for the split-bf16 f)."""
    from agplace_amd import ops
    for b in (3, 16, 37, 64):
        x, a1, w, bias = R.input_law(b)
        lw = ops.LinearWeights(w.to(dev), bias.to(dev))
        y, _ = ops.fcode_adaptive(x.to(dev), lw, "id", METHOD, 1e-3, 64, add1=a1.to(dev))
        yr, _ = _restated("id", 1.0, 1e-3, b, 11)
        ex = R.linear_exact(x + a1, w, bias)
        e_dev, e_ref = rel_l2(y, ex), rel_l2(yr, ex)
        print(f"BOSH3 id vs expm tol 1e-3 b {b}: device {e_dev:.3e} restatement {e_ref:.3e}")
        assert e_dev <= 1.5 * e_ref, (b, e_dev, e_ref)


@pytest.mark.parametrize("act", ["relu", "tanh", "sigmoid", "id"])
def test_backward_matches_autograd_through_the_restatement(dev, act):
    """Discretise-then-optimise through the accepted steps (step control detached), the last step through its interpolant,
    through the FCODE module; the law of tests/test_gpu_dopri5.py's test of the same name."""
    from agplace_amd.network_mm.ffns import FCODE
    from agplace_amd.options import Options
    g = torch.Generator().manual_seed(21)
    torch.manual_seed(1)
    for b in (5, 16, 35):
        m = FCODE(256, act, opt=Options(odeint_method=METHOD, odeint_adaptive_family=True)).to(dev)
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
        yr, log = K.fcode(xr + a1.double(), W, B, act, 1e-3, METHOD)
        (yr * G.double()).sum().backward()
        margin = _precondition(log, (act, b))
        assert [a[2] for a in st["attempts"]] == log.accepted and st["accepted"] >= 2
        errs = (rel_l2(y, yr), rel_l2(xd.grad, xr.grad), rel_l2(a1d.grad, xr.grad), rel_l2(m.func.func.fc.weight.grad, W.grad),
                rel_l2(m.func.func.fc.bias.grad, B.grad))
        print(f"BOSH3 BWD {act} b {b}: steps {st['accepted']} margin {margin:.3f} y {errs[0]:.2e} gx {errs[1]:.2e} "
              f"ga1 {errs[2]:.2e} gw {errs[3]:.2e} gb {errs[4]:.2e}")
        assert errs[0] < 1e-4
        assert errs[1] < 1e-3 and errs[2] < 1e-3 and errs[3] < 1e-3 and errs[4] < 1e-3, (act, b, errs)


@pytest.mark.parametrize("act,gain,b,seed,accepted,rejected", [("tanh", 16.0, 16, 11, 10, 0), ("id", 2.0, 37, 14, 7, 1)])
def test_backward_through_long_sequences(dev, act, gain, b, seed, accepted, rejected):
    """Op level, tol = 1e-3: ten accepted steps (the FSAL adjoint flows into the step before); a rejected step (it
    contributes nothing) and a partial row tile."""
    from agplace_amd import ops
    x, a1, w, bias = R.input_law(b, gain, seed)
    G = torch.randn(b, 256, generator=torch.Generator().manual_seed(5))
    lw = ops.LinearWeights(w.to(dev), bias.to(dev), with_transpose=True)
    y, ctrl, traj = ops.fcode_adaptive(x.to(dev), lw, act, METHOD, 1e-3, 64, add1=a1.to(dev), want_traj=True)
    gx, gw, gb = ops.fcode_adaptive_bwd(traj, ctrl, G.to(dev), lw, act, METHOD, 64)
    st = ops.ode_stats(ctrl)
    W, B = w.double().requires_grad_(True), bias.double().requires_grad_(True)
    xr = (x + a1).double().requires_grad_(True)
    yr, log = K.fcode(xr, W, B, act, 1e-3, METHOD)
    (yr * G.double()).sum().backward()
    _precondition(log, (act, gain, b, seed))
    assert [a[2] for a in st["attempts"]] == log.accepted and (st["accepted"], st["rejected"]) == (accepted, rejected), (st, log.steps)
    errs = (rel_l2(y, yr), rel_l2(gx, xr.grad), rel_l2(gw, W.grad), rel_l2(gb, B.grad))
    print(f"BOSH3 BWD {act} gain {gain} b {b}: attempts {len(log.steps)} rejected {st['rejected']} "
          f"y {errs[0]:.2e} gx {errs[1]:.2e} gw {errs[2]:.2e} gb {errs[3]:.2e}")
    assert errs[0] < 1e-4 and max(errs[1:]) < 1e-3, errs


def test_repeatable_bits_and_independence_of_trailing_memory(dev):
    from agplace_amd import ops
    x, a1, w, bias = R.input_law(37, 4.0)       # no reference here: how close a ratio comes to 1 does not matter
    lw = ops.LinearWeights(w.to(dev), bias.to(dev), with_transpose=True)
    G = torch.randn(37, 256, generator=torch.Generator().manual_seed(3)).to(dev)

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
        big_x = torch.full((64, 256), fill, device=dev)
        big_a = torch.full((64, 256), fill, device=dev)
        big_x[:37], big_a[:37] = x.to(dev), a1.to(dev)
        y, ctrl = ops.fcode_adaptive(big_x[:37], lw, "relu", METHOD, 1e-4, 64, add1=big_a[:37])
        assert torch.equal(y, first[0]) and torch.equal(ctrl, first[4])
    # another table on the same inputs is another solve
    yd, _ = ops.fcode_adaptive(x.to(dev), lw, "relu", "dopri5", 1e-4, 64, add1=a1.to(dev))
    assert not torch.equal(yd, first[0])


def test_solve_inside_a_captured_graph(dev):
    """One launch, no host round trip: the solve replays from a captured graph, with a data-dependent step count."""
    from agplace_amd import ops
    x, a1, w, bias = R.input_law(16, 4.0)
    lw = ops.LinearWeights(w.to(dev), bias.to(dev))
    inputs = [(x * s).to(dev) for s in (1.0, 0.05, 6.0)]
    eager = [ops.fcode_adaptive(xi, lw, "relu", METHOD, 1e-4, 64, add1=a1.to(dev)) for xi in inputs]
    counts = [ops.ode_stats(c)["attempted"] for _, c in eager]
    print(f"BOSH3 captured: attempted steps {counts}")
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
    """odeint_max_steps = 2 on a solve that needs more: a clean return, NaN output, solver_stats() raises, NaN gradients."""
    from agplace_amd import ops
    from agplace_amd.network_mm.ffns import FCODE
    from agplace_amd.options import Options
    torch.manual_seed(1)
    x, a1, _, _ = R.input_law(16)
    ok = FCODE(256, "relu", opt=Options(odeint_method=METHOD, odeint_adaptive_family=True)).to(dev)
    capped = FCODE(256, "relu", opt=Options(odeint_method=METHOD, odeint_adaptive_family=True, odeint_max_steps=2)).to(dev)
    capped.load_state_dict(ok.state_dict())
    with torch.no_grad():
        y = ok(x.to(dev), add1=a1.to(dev))
        st = ok.solver_stats()
        assert bool(torch.isfinite(y).all()) and st["attempted"] > 2 and st["f_evals"] == 2 + 3 * st["attempted"]
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


def test_abi_refusals(dev):
    """The C entry points take AGP_ODE_DOPRI5 and AGP_ODE_BOSH3 and nothing else: method 5 (and a fixed grid's number) is
    AGP_E_BADARG before any launch (the outputs keep their poison)."""
    from agplace_amd import _lib
    L = _lib.load()
    b, cap, D = 16, 8, 256
    x = torch.zeros(b, D, device=dev)
    planes = torch.zeros(2, D * D, dtype=torch.bfloat16, device=dev)
    y = torch.full((b, D), -3.0, device=dev)
    ring = torch.empty(L.agp_fcode_adaptive_ring_floats(b, cap, 1), device=dev)
    ctrl = torch.full((L.agp_fcode_adaptive_ctrl_bytes(cap),), 7, dtype=torch.uint8, device=dev)
    ws = torch.empty(L.agp_fcode_adaptive_bwd_workspace_bytes(b, cap), dtype=torch.uint8, device=dev)
    gx = torch.full((b, D), -3.0, device=dev)

    def fwd(method, max_steps=cap):
        return L.agp_fcode_adaptive_fwd(x.data_ptr(), None, None, planes[0].data_ptr(), planes[1].data_ptr(), None, b,
                                        _lib.ACT["relu"], method, ctypes.c_double(1e-3), ctypes.c_double(1e-3), max_steps,
                                        y.data_ptr(), ring.data_ptr(), 1, ctrl.data_ptr(), _lib.stream())

    def bwd(method, nbytes=ws.numel()):
        return L.agp_fcode_adaptive_bwd(ring.data_ptr(), ctrl.data_ptr(), x.data_ptr(), planes[0].data_ptr(), planes[1].data_ptr(),
                                        b, _lib.ACT["relu"], method, cap, gx.data_ptr(), None, None, ws.data_ptr(), nbytes,
                                        _lib.stream())
    for method in (5, 2, -1):
        assert fwd(method) == 1 and bwd(method) == 1, method
    assert fwd(_lib.ODE_ADAPTIVE[METHOD], max_steps=0) == 1 and bwd(_lib.ODE_ADAPTIVE[METHOD], nbytes=ws.numel() - 1) == 1
    torch.cuda.synchronize()
    assert bool((y == -3.0).all()) and bool((gx == -3.0).all()) and bool((ctrl == 7).all())
    # and the method's own number is taken: y' = relu(0 y + 0) = 0 from y = 0 stays at 0 (seven steps, each ten times the last)
    assert fwd(_lib.ODE_ADAPTIVE[METHOD]) == 0 and bwd(_lib.ODE_ADAPTIVE[METHOD]) == 0
    torch.cuda.synchronize()
    assert bool((y == 0.0).all()) and bool((gx == 0.0).all())


def _restated_odeint(tol):
    def odeint(f, y0, method, step_size, dt_dtype=torch.float32):
        assert method == METHOD
        return K.solve(f, y0, tol, K.TABLES[METHOD], dtype=y0.dtype)[0]
    return odeint


def test_mm_inference_with_bosh3(dev, monkeypatch):
    """MM with odeint_method = 'bosh3' runs its vector path per op (the fused vector program refuses an adaptive solver) and
    equals the oracle with its fixed-grid integrator replaced by the restatement, at the bar test_mm_inference_with_dopri5
    holds mfma_precision = 3 to (5e-5)."""
    from agplace_amd import vecprog
    from agplace_amd.network_mm.mm import MM
    from agplace_amd.options import Options
    from oracle import ode
    opt = Options(mfma_precision=3, odeint_method=METHOD, odeint_adaptive_family=True)
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
    assert blocks and all(m.method == METHOD and m.solver_stats()["status"] == 0 for m in blocks)
    assert all(m.solver_stats()["f_evals"] == 2 + 3 * m.solver_stats()["attempted"] for m in blocks)
    monkeypatch.setattr(ode, "odeint_fixed", _restated_odeint(opt.tol))
    ref = nets.mm_forward_q(data, cpu_state(model), opt)
    err = rel_l2(out["embedding"], ref["embedding"])
    print(f"BOSH3 MM prec 3 embedding rel_l2 {err:.2e}, {len(blocks)} adaptive blocks")
    assert err < 5e-5


def test_mm_training_step_with_bosh3(dev):
    """One training step fills every gradient the euler run fills."""
    from agplace_amd.network_mm.mm import MM
    from agplace_amd.options import Options
    filled = {}
    for method in ("euler", METHOD):
        opt = Options(odeint_method=method, odeint_adaptive_family=True)
        torch.manual_seed(23)
        mq = MM(opt=opt).to(dev).train()
        data = to_dev(nets.synth_query(2, 64, 128, opt, seed=6), dev)
        out = mq(data, mode="q")
        (out["embedding"] ** 2).sum().backward()
        filled[method] = {n for n, p in mq.named_parameters() if p.grad is not None}
        assert all(bool(torch.isfinite(p.grad).all()) for p in mq.parameters() if p.grad is not None), method
        if method == METHOD:
            blocks = [m for m in mq.modules() if getattr(m, "adaptive", False)]
            assert blocks and all(m.solver_stats()["accepted"] >= 1 for m in blocks)
            assert all(float(m.func.func.fc.weight.grad.abs().max()) > 0 for m in blocks)
    assert filled[METHOD] == filled["euler"] and len(filled["euler"]) > 50
