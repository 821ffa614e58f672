"""-m gpu tests of the one-launch fixed-grid solver at 384 columns (csrc/fusion_wide.hip, ops.fcode_wide) and of its dispatch in
FCODE.forward.

Parity bound.  The kernel's arithmetic is that of the 256-column kernel (split-bf16, three products, fp32 state), whose forward
tests ask rel_l2 < 1e-4 of it.  The figures below were MEASURED with this file's cases on an MI355X (every act x method x b x add
combination, against fp64 oracle.ode.fcode; each case prints its own figure before it asserts):
    worst rel_l2 = 8.929e-07 (id, midpoint/0.3)   worst rel_max = 1.402e-06 (relu, midpoint/0.3)
and the asserted bounds are 4x those (differences between machines; the convention of tests/test_gpu_convnext.py), never looser
than 1e-4.  A dropped product (hi*lo or lo*hi) shows at about 1e-3.
"""
import ctypes

import pytest
import torch

from oracle import ode
from gpu_util import rel_l2, rel_max

pytestmark = pytest.mark.gpu

D = 384
MEASURED_REL_L2, MEASURED_REL_MAX = 8.929e-07, 1.402e-06
BOUND_L2, BOUND_MAX = min(4 * MEASURED_REL_L2, 1e-4), min(4 * MEASURED_REL_MAX, 1e-4)
GRIDS = [("euler", 0.1), ("midpoint", 0.3), ("rk4", 0.25)]        # step 0.3: an uneven last step
ACTS = ["id", "relu", "tanh", "sigmoid"]


def _block(dev, act, method, step, seed=0):
    from agplace_amd.network_mm.ffns import FCODE
    from agplace_amd.options import Options
    torch.manual_seed(seed)
    m = FCODE(D, act, opt=Options(odeint_method=method, odeint_size=step)).to(dev)
    with torch.no_grad():
        m.func.func.fc.weight.mul_(0.5)        # as in the any-width test (tests/test_gpu_kernels.py)
    return m


def _ref(m, x, adds, act, method, step):
    fc = m.func.func.fc
    y0 = x.double().cpu()
    for a in adds:
        y0 = y0 + a.double().cpu()
    return ode.fcode(y0, fc.weight.detach().double().cpu(), fc.bias.detach().double().cpu(), act, method, step)


def _batches():
    from agplace_amd import ops
    r = ops.FCODE_WIDE_ROWS
    return [1, r - 1, r, r + 1, 35]


@pytest.mark.parametrize("method,step", GRIDS)
@pytest.mark.parametrize("act", ACTS)
def test_fcode_wide_matches_fp64_oracle(dev, act, method, step):
    from agplace_amd import ops
    m = _block(dev, act, method, step, seed=len(act) + len(method))
    lw = m._prep.get()
    g = torch.Generator().manual_seed(17)
    worst = [0.0, 0.0]
    for b in _batches():
        x = torch.randn(b, D, generator=g).to(dev)
        a1, a2 = (0.5 * torch.randn(b, D, generator=g)).to(dev), (0.25 * torch.randn(b, D, generator=g)).to(dev)
        for adds in ((), (a1,), (a1, a2)):
            y = ops.fcode_wide(x, lw, act, method, m.dts, *adds)
            ref = _ref(m, x, adds, act, method, step)
            e2, em = rel_l2(y, ref), rel_max(y, ref)
            print(f"fcode_wide {act} {method}/{step} b={b} adds={len(adds)}: rel_l2 {e2:.3e} rel_max {em:.3e}")
            worst = [max(worst[0], e2), max(worst[1], em)]
            assert y.shape == (b, D) and y.dtype == torch.float32
            assert e2 < BOUND_L2 and em < BOUND_MAX, (act, method, b, len(adds), e2, em)
    print(f"fcode_wide {act} {method}/{step} WORST rel_l2 {worst[0]:.3e} rel_max {worst[1]:.3e}")


def test_fcode_wide_known_answer_euler_identity(dev):
    """act = id, Euler: y_N = (I + hW)^N y0 + sum_k (I + hW)^k h b, in fp64 with h = 0.1 exactly -- the kernel's
    fp32 step sizes differ from it by < 1e-7 relative."""
    from agplace_amd import ops
    m = _block(dev, "id", "euler", 0.1, seed=3)
    fc = m.func.func.fc
    x = torch.randn(19, D, generator=torch.Generator().manual_seed(4)).to(dev)
    y = ops.fcode_wide(x, m._prep.get(), "id", "euler", m.dts)
    ref = ode.euler_linear_closed_form(x.double().cpu(), fc.weight.detach().double().cpu(), fc.bias.detach().double().cpu(), 0.1, 10)
    assert len(m.dts) == 10
    assert rel_l2(y, ref) < BOUND_L2 and rel_max(y, ref) < BOUND_MAX


@pytest.mark.parametrize("method,step", GRIDS)
def test_fcode_wide_repeats_and_replays_bit_for_bit(dev, method, step):
    m = _block(dev, "tanh", method, step, seed=5).eval()
    g = torch.Generator().manual_seed(6)
    x, a1 = torch.randn(35, D, generator=g).to(dev), torch.randn(35, D, generator=g).to(dev)
    with torch.no_grad():
        y1 = m(x, add1=a1)              # (also the warm-up: the weight planes are prepared here, outside the capture)
        y2 = m(x, add1=a1)
        assert torch.equal(y1, y2)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            yg = m(x, add1=a1)
        yg.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(yg, y1)


def test_fcode_wide_refuses_unprepared_planes_inside_a_capture(dev, monkeypatch):
    """The fragment planes are built once per parameter version and never inside a capture (the capture state is faked: the
    refusal comes before any launch)."""
    from agplace_amd import ops
    m = _block(dev, "relu", "euler", 0.1, seed=7)
    lw = ops.LinearWeights(m.func.func.fc.weight, m.func.func.fc.bias)
    x = torch.randn(4, D, device=dev)
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="before capturing"):
            ops.fcode_wide(x, lw, "relu", "euler", m.dts)
    planes = ops.fcode_wide_planes(lw)
    assert ops.fcode_wide_planes(lw) is planes and planes[0].shape == (8, 12, 3, 4, 16, 8)


def _raw(x, lw, act, method, dts, y, d=D):
    from agplace_amd import _lib, ops
    f_hi, f_lo = ops.fcode_wide_planes(lw)
    arr = (ctypes.c_float * len(dts))(*dts)
    return _lib.load().agp_fcode_wide_fwd(x.data_ptr(), None, None, f_hi.data_ptr(), f_lo.data_ptr(), lw.bias.data_ptr(), x.shape[0], d,
                                          _lib.ACT[act], _lib.ODE[method], arr, len(dts), y.data_ptr(), _lib.stream())


@pytest.mark.parametrize("b", [1, 17, 32])
def test_fcode_wide_leaves_rows_beyond_b_alone(dev, b):
    """The last workgroup's dead rows compute but never store: the rows around y[0:b] inside a larger allocation keep their poison."""
    from agplace_amd import ops
    m = _block(dev, "relu", "rk4", 0.25, seed=8)
    lw = m._prep.get()
    x = torch.randn(b, D, generator=torch.Generator().manual_seed(b)).to(dev)
    buf = torch.full((b + 40, D), -777.0, device=dev)
    assert _raw(x, lw, "relu", "rk4", m.dts, buf[3:3 + b]) == 0
    torch.cuda.synchronize()
    assert torch.equal(buf[3:3 + b], ops.fcode_wide(x, lw, "relu", "rk4", m.dts))
    assert bool((buf[:3] == -777.0).all()) and bool((buf[3 + b:] == -777.0).all())


@pytest.mark.parametrize("d", [256, 512])
def test_fcode_wide_entry_refuses_other_widths(dev, d):
    from agplace_amd import _lib
    m = _block(dev, "relu", "euler", 0.1, seed=9)
    x = torch.zeros(2, 512, device=dev)
    y = torch.full((2, 512), 5.0, device=dev)
    assert _raw(x, m._prep.get(), "relu", "euler", m.dts, y, d=d) == _lib.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((y == 5.0).all())


def _spies(monkeypatch):
    from agplace_amd import autograd_ops, ops
    calls = {"wide": 0, "linear": 0}
    wide, lin = ops.fcode_wide, autograd_ops.linear

    def spy_wide(*a, **k):
        calls["wide"] += 1
        return wide(*a, **k)

    def spy_lin(*a, **k):
        calls["linear"] += 1
        return lin(*a, **k)
    monkeypatch.setattr(ops, "fcode_wide", spy_wide)
    monkeypatch.setattr(autograd_ops, "linear", spy_lin)
    return calls


def test_fcode_384_dispatch_inference_takes_the_one_launch_kernel(dev, monkeypatch):
    m = _block(dev, "relu", "euler", 0.1, seed=10)
    calls = _spies(monkeypatch)
    x = torch.randn(5, D, device=dev)
    with torch.no_grad():
        y = m(x)
    assert calls == {"wide": 1, "linear": 0}
    assert rel_l2(y, _ref(m, x, (), "relu", "euler", 0.1)) < BOUND_L2
    # gradients enabled but nobody wants one: still the inference kernel
    for p in m.parameters():
        p.requires_grad_(False)
    m(x)
    assert calls == {"wide": 2, "linear": 0}


@pytest.mark.parametrize("method,step,act", [("euler", 0.1, "relu"), ("rk4", 0.25, "sigmoid")])
def test_fcode_384_dispatch_with_a_gradient_wanted_takes_the_any_width_route(dev, monkeypatch, method, step, act):
    """... and its gradients match fp64 autograd through the oracle's solver (the bound of the any-width test, 2e-4)."""
    m = _block(dev, act, method, step, seed=11)
    fc = m.func.func.fc
    calls = _spies(monkeypatch)
    b = 9
    x = torch.randn(b, D, device=dev, requires_grad=True)
    a1 = (0.5 * torch.randn(b, D, device=dev)).requires_grad_(True)
    y = m(x, add1=a1)
    assert calls["wide"] == 0 and calls["linear"] == ode.n_feval(method, step)
    xr, ar = x.detach().double().cpu().requires_grad_(True), a1.detach().double().cpu().requires_grad_(True)
    wr, br = fc.weight.detach().double().cpu().requires_grad_(True), fc.bias.detach().double().cpu().requires_grad_(True)
    ref = ode.fcode(xr + ar, wr, br, act, method, step)
    assert rel_l2(y, ref) < 1e-4
    gy = torch.randn(b, D, generator=torch.Generator().manual_seed(b))
    y.backward(gy.to(dev))
    ref.backward(gy.double())
    assert rel_l2(x.grad, xr.grad) < 2e-4 and rel_l2(a1.grad, ar.grad) < 2e-4
    assert rel_l2(fc.weight.grad, wr.grad) < 2e-4 and rel_l2(fc.bias.grad, br.grad) < 2e-4
    # only an input wants a gradient (frozen weights): the any-width route as well
    for p in m.parameters():
        p.requires_grad_(False)
    m(x)
    assert calls["wide"] == 0


@pytest.mark.parametrize("dim", [256, 128])
def test_other_widths_never_reach_the_wide_op(dev, monkeypatch, dim):
    from agplace_amd.network_mm.ffns import FCODE
    from agplace_amd.options import Options
    m = FCODE(dim, "relu", opt=Options()).to(dev)
    calls = _spies(monkeypatch)
    with torch.no_grad():
        y = m(torch.randn(3, dim, device=dev))
    assert calls["wide"] == 0 and y.shape == (3, dim)


def test_dopri5_at_384_keeps_its_refusal(dev):
    from agplace_amd.network_mm.ffns import FCODE
    from agplace_amd.options import Options
    m = FCODE(D, "relu", opt=Options(odeint_method="dopri5")).to(dev)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="dim=256"):
        m(torch.randn(3, D, device=dev))
