"""-m gpu tests of Options.fcode_wide: the fixed-grid training kernels at 384 columns (csrc/fusion_wide.hip:
agp_fcode_wide_fwd_traj, agp_fcode_wide_bwd), their routing in FCODE.forward with the routing of dopri5, and MM on the
ConvNeXt-tiny trunk with the switch on.

Kernel cases: b = 1, 15, 16, 17, 35 (one row, a ragged tile, an exact tile, one row into a second workgroup, three workgroups with
a ragged last) x euler/0.1, midpoint/0.3 (a short last step), rk4/0.25, euler/1.0 (one step), euler/0.015625 (64 steps: the limit)
x the four activations; the forward also x {no add, add1, add1 + add2}.  Operands: w = randn(384, 384) / sqrt(384),
bias = 0.3 randn, seeded.
Bars: tests/head_ref.py's fcode_fwd_bars / fcode_bwd_bars -- the fp64 closed form against its three-product and float32 forms,
min(4 x floor, ceiling), the yardstick of the 256-column kernels (tests/test_gpu_head_kernels.py); the helpers take the width from
w.  Every comparison prints its worst row beside that row's bar before it asserts.  The references are computed once per case
(_reference) and shared by the forward and the backward test.
Module and model tests use the bounds of the files whose routes they replace: tests/test_gpu_fcode_wide.py (1e-4 output, 2e-4
gradients against fp64 autograd through oracle.ode.fcode) and tests/test_gpu_mm_convnext_train.py (_end_to_end's own bars).
"""
import functools

import pytest
import torch

import head_ref as H
import mm_convnext_ref
import test_gpu_fcode_wide as W
import test_gpu_head_kernels as K
from gpu_util import rel_l2, to_dev
from oracle import nets, ode

pytestmark = pytest.mark.gpu

D = 384
BATCHES = (1, 15, 16, 17, 35)
GRIDS = (("euler", 0.1), ("midpoint", 0.3), ("rk4", 0.25), ("euler", 1.0), ("euler", 0.015625))
BADARG, UNSUPPORTED = K._header_code("AGP_E_BADARG"), K._header_code("AGP_E_UNSUPPORTED")


def _draw(b, seed=0):
    """x, add1, add2 [b, 384], w [384, 384] (unit-variance pre-activations), bias, gy"""
    g = torch.Generator().manual_seed(1000 * seed + b)
    x, a1, a2, gy = (torch.randn((b, D), generator=g) for _ in range(4))
    w = torch.randn((D, D), generator=g) / D ** 0.5
    return x, 0.5 * a1, 0.25 * a2, w, 0.3 * torch.randn(D, generator=g), gy


@functools.lru_cache(maxsize=None)
def _reference(b, method, step, act):
    """The operands of a case and, with both adds, the fp64 forward with its bars: shared by the tests below, never modified."""
    ops_ = _draw(b)
    dts = H.grid_dts(step)
    return ops_, dts, H.fcode_fwd_bars(*ops_[:5], act, method, dts)


def _planes(lw, transpose=False):
    from agplace_amd import ops
    return ops.fcode_wide_planes_t(lw) if transpose else ops.fcode_wide_planes(lw)


def _fwd_traj(dev, lw, x, a1, a2, act, method, dts, y, traj, d=D, nsteps=None, method_code=None):
    f_hi, f_lo = _planes(lw)
    return K._L().agp_fcode_wide_fwd_traj(K._ptr(x), K._ptr(a1), K._ptr(a2), f_hi.data_ptr(), f_lo.data_ptr(), K._ptr(lw.bias),
                                          x.shape[0], d, K._act(act), K._ode(method) if method_code is None else method_code,
                                          K._dt_array(dts), len(dts) if nsteps is None else nsteps, y, traj, K._stream())


def _bwd(dev, lw, traj, gy, act, method, dts, gx, gw, gb, ws, nbytes, d=D, nsteps=None, method_code=None):
    t_hi, t_lo = _planes(lw, transpose=True)
    return K._L().agp_fcode_wide_bwd(traj, K._ptr(gy), t_hi.data_ptr(), t_lo.data_ptr(), gy.shape[0], d, K._act(act),
                                     K._ode(method) if method_code is None else method_code, K._dt_array(dts),
                                     len(dts) if nsteps is None else nsteps, gx, gw, gb, ws, nbytes, K._stream())


# ------------------------------------------------------------------------------------------------------- 1. forward with traj
@pytest.mark.parametrize("method,step", GRIDS)
@pytest.mark.parametrize("act", H.ACTS)
def test_forward_with_trajectory(dev, act, method, step):
    from agplace_amd import ops
    L = K._L()
    nslot = 1 + H.stages(method)
    for b in BATCHES:
        (x, a1, a2, w, bias, _), dts, full = _reference(b, method, step, act)
        lw = K._weights(w, bias, dev)
        xd, a1d, a2d = K._d(x, dev), K._d(a1, dev), K._d(a2, dev)
        n = len(dts)
        assert int(L.agp_fcode_wide_traj_floats(b, D, K._ode(method), n)) == n * nslot * b * D
        for adds in (0, 1, 2):
            u1, u2 = (a1 if adds >= 1 else None), (a2 if adds == 2 else None)
            y64, traj64, by, bt = full if adds == 2 else H.fcode_fwd_bars(x, u1, u2, w, bias, act, method, dts)
            y, traj = K.Out(b, D, dev), K.Out(n * nslot * b, D, dev)
            K._ok(_fwd_traj(dev, lw, xd, a1d if adds >= 1 else None, a2d if adds == 2 else None, act, method, dts, y.ptr(),
                            traj.ptr()), "agp_fcode_wide_fwd_traj")
            what = "fcode_wide_fwd_traj b %d %s %g %s adds %d" % (b, method, step, act, adds)
            vy = y.value(what + " y")                                  # (the canaries round y and traj are checked here)
            K._rows_ok(vy, y64, by, what + " y")
            K._rows_ok(traj.value(what + " traj"), traj64.reshape(-1, D), bt.reshape(-1), what + " traj (every slot)")
            plain = ops.fcode_wide(xd, lw, act, method, dts, add1=a1d if adds >= 1 else None, add2=a2d if adds == 2 else None)
            assert torch.equal(plain.cpu(), vy), what + ": y differs from agp_fcode_wide_fwd's bits"


# -------------------------------------------------------------------------------------- 2. backward from the reference trajectory
@pytest.mark.parametrize("method,step", GRIDS)
@pytest.mark.parametrize("act", H.ACTS)
def test_backward_from_the_reference_trajectory(dev, act, method, step):
    """The backward kernel alone: its input is head_ref.fcode_traj's fp64 trajectory rounded to fp32.  The workspace starts as
    NaN: the GZ / S rows of a tile's dead batch rows are summed into gw / gb, so they must have been written as zeros."""
    L = K._L()
    for b in BATCHES:
        (x, a1, a2, w, bias, gy), dts, (_, traj64, _, _) = _reference(b, method, step, act)
        t32 = traj64.float()
        (rx, rw, rb), bx, bw, bb = H.fcode_bwd_bars(t32, gy, w, act, method, dts)
        lw = K._weights(w, bias, dev)
        _planes(lw, transpose=True)      # (prepared before the workspaces below exist: nothing is allocated between them and a launch)
        need = int(L.agp_fcode_wide_bwd_workspace_bytes(b, D, K._ode(method), len(dts)))
        assert need == 2 * len(dts) * H.stages(method) * ((b + 15) // 16 * 16) * D * 4
        td, gyd = K._d(t32, dev), K._d(gy, dev)
        what = "fcode_wide_bwd b %d %s %g %s" % (b, method, step, act)
        gx, gw, gb = K.Out(b, D, dev), K.Out(D, D, dev, spare=4), K.Out(1, D, dev, spare=1)
        ws, ws2 = K._nan(need, dev), K._nan(need, dev)               # (held until the results have been read)
        K._ok(_bwd(dev, lw, K._ptr(td), gyd, act, method, dts, gx.ptr(), gw.ptr(), gb.ptr(), K._ptr(ws), need), "agp_fcode_wide_bwd")
        vx, vw, vb = gx.value(what + " gx"), gw.value(what + " gw"), gb.value(what + " gb")
        assert bool(torch.isfinite(vw).all()) and bool(torch.isfinite(vb).all()), what + ": gw / gb took in rows nobody wrote"
        K._rows_ok(vx, rx, bx, what + " gx per batch row")
        K._rows_ok(vw, rw, bw, what + " gw per output row")
        K._rows_ok(vb, rb[None], bb, what + " gb")
        gx2, gw2, gb2 = K.Out(b, D, dev), K.Out(D, D, dev, spare=4), K.Out(1, D, dev, spare=1)
        K._ok(_bwd(dev, lw, K._ptr(td), gyd, act, method, dts, gx2.ptr(), None, None, K._ptr(ws2), need), "agp_fcode_wide_bwd")
        assert torch.equal(gx2.value(what + " gx"), vx) and gw2.untouched() and gb2.untouched(), what + ": gw / gb NULL"


# ------------------------------------------------------------------------------------------------------------------ 3. refusals
def test_refusals_write_nothing(dev):
    L = K._L()
    b = 4
    x, _, _, w, bias, gy = _draw(b, seed=3)
    lw = K._weights(w, bias, dev)
    xd, gyd = K._d(x, dev), K._d(gy, dev)
    dts65 = [0.5] * 65
    y, traj = K.Out(b, 512, dev), K.Out(2 * 2 * b, 512, dev)

    def fwd(d=D, nsteps=2, method=0, traj_ptr=traj.ptr()):
        return _fwd_traj(dev, lw, xd, None, None, "relu", None, dts65, y.ptr(), traj_ptr, d=d, nsteps=nsteps, method_code=method)
    assert fwd(d=256) == UNSUPPORTED and fwd(d=128) == UNSUPPORTED, "another width"
    assert fwd(nsteps=0) == BADARG and fwd(nsteps=65) == BADARG, "nsteps 0 and 65"
    assert fwd(method=3) == BADARG, "a bad method"
    assert fwd(traj_ptr=None) == BADARG, "a null traj"
    assert y.untouched() and traj.untouched()
    for args in ((b, 256, 0, 2), (b, 128, 0, 2), (b, D, 0, 0), (b, D, 0, 65), (b, D, 3, 2), (0, D, 0, 2)):
        assert int(L.agp_fcode_wide_traj_floats(*args)) == 0 and int(L.agp_fcode_wide_bwd_workspace_bytes(*args)) == 0, args

    need = int(L.agp_fcode_wide_bwd_workspace_bytes(b, D, 0, 2))
    assert need == 2 * 2 * 16 * D * 4
    ws = torch.full((need // 4 + 64,), K.POISON, dtype=torch.int32, device=dev)
    td = torch.zeros((2 * 2 * b, 512), dtype=torch.float32, device=dev)
    gx, gw, gb = K.Out(b, 512, dev), K.Out(512, 512, dev, spare=4), K.Out(1, 512, dev, spare=1)

    def bwd(d=D, nsteps=2, method=0, nbytes=1 << 40, traj_ptr=td.data_ptr()):
        return _bwd(dev, lw, traj_ptr, gyd, "relu", None, dts65, gx.ptr(), gw.ptr(), gb.ptr(), K._ptr(ws), nbytes, d=d,
                    nsteps=nsteps, method_code=method)
    assert bwd(d=256) == UNSUPPORTED and bwd(d=128) == UNSUPPORTED, "another width"
    assert bwd(nsteps=0) == BADARG and bwd(nsteps=65) == BADARG, "nsteps 0 and 65"
    assert bwd(method=3) == BADARG, "a bad method"
    assert bwd(nbytes=need - 1) == BADARG, "a workspace one byte short"
    assert bwd(traj_ptr=None) == BADARG, "a null traj"
    assert gx.untouched() and gw.untouched() and gb.untouched() and bool((ws == K.POISON).all())


# ------------------------------------------------------------------------------------------------------------- 4. repeatability
@pytest.mark.parametrize("method,step", GRIDS[:3])
def test_forward_and_backward_repeat_and_replay_bit_for_bit(dev, method, step):
    from agplace_amd import ops
    b = 35
    x, a1, _, w, bias, gy = _draw(b, seed=4)
    x2, a12, _, _, _, gy2 = _draw(b, seed=5)
    lw = K._weights(w, bias, dev)
    dts = H.grid_dts(step)

    def step_(xs, as_, gs):
        y, traj = ops.fcode_wide(xs, lw, "tanh", method, dts, add1=as_, want_traj=True)
        return (y,) + ops.fcode_wide_bwd(traj, gs, lw, "tanh", method, dts)
    ins = [tuple(K._d(t, dev) for t in c) for c in ((x, a1, gy), (x2, a12, gy2))]
    eager = [step_(*c) for c in ins]                 # (also the warm-up: both sets of planes are prepared here, outside the capture)
    again = step_(*ins[0])
    assert all(torch.equal(p, q) for p, q in zip(eager[0], again)), "two eager runs differ"
    static = [torch.empty_like(t) for t in ins[0]]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step_(*static)
    for c, want in zip(ins, eager):
        for s, t in zip(static, c):
            s.copy_(t)
        for o in outs:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(p, q) for p, q in zip(outs, want)), "a replay differs from the eager run"


# ------------------------------------------------------------------------------------------------------ 5. module, fixed grid
def _block(dev, act, method, step=0.1, seed=0, switch=True):
    from agplace_amd.network_mm.ffns import FCODE
    from agplace_amd.options import Options
    torch.manual_seed(seed)
    m = FCODE(D, act, opt=Options(fcode_wide=switch, odeint_method=method, odeint_size=step)).to(dev)
    with torch.no_grad():
        m.func.func.fc.weight.mul_(0.5)        # as tests/test_gpu_fcode_wide.py's block
    return m


@pytest.mark.parametrize("method,step,act", [("euler", 0.1, "relu"), ("rk4", 0.25, "sigmoid")])
def test_module_trains_on_the_one_launch_kernels(dev, monkeypatch, method, step, act):
    m = _block(dev, act, method, step, seed=11)
    fc = m.func.func.fc
    calls = W._spies(monkeypatch)
    b = 9
    x = torch.randn(b, D, device=dev, requires_grad=True)
    a1 = (0.5 * torch.randn(b, D, device=dev)).requires_grad_(True)
    y = m(x, add1=a1)
    assert calls == {"wide": 1, "linear": 0}
    xr, ar = x.detach().double().cpu().requires_grad_(True), a1.detach().double().cpu().requires_grad_(True)
    wr, br = fc.weight.detach().double().cpu().requires_grad_(True), fc.bias.detach().double().cpu().requires_grad_(True)
    ref = ode.fcode(xr + ar, wr, br, act, method, step)
    print(f"FCODE(384) fcode_wide {act} {method}/{step}: y rel_l2 {rel_l2(y, ref):.3e}")
    assert rel_l2(y, ref) < 1e-4
    gy = torch.randn(b, D, generator=torch.Generator().manual_seed(b))
    y.backward(gy.to(dev))
    ref.backward(gy.double())
    errs = {"x": rel_l2(x.grad, xr.grad), "add1": rel_l2(a1.grad, ar.grad), "weight": rel_l2(fc.weight.grad, wr.grad),
            "bias": rel_l2(fc.bias.grad, br.grad)}
    print(f"FCODE(384) fcode_wide {act} {method}/{step}: gradients rel_l2 " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert all(v < 2e-4 for v in errs.values()), errs
    assert calls["linear"] == 0
    # frozen weights, only x wants a gradient: the same route, no weight gradient
    for p in m.parameters():
        p.requires_grad_(False)
        p.grad = None
    x2 = x.detach().clone().requires_grad_(True)
    m(x2, add1=a1.detach()).backward(gy.to(dev))
    assert calls == {"wide": 2, "linear": 0}
    assert torch.equal(x2.grad, x.grad) and fc.weight.grad is None and fc.bias.grad is None
    # no gradient wanted: the inference launch, the bits of the model without the switch
    off = _block(dev, act, method, step, seed=11, switch=False)
    with torch.no_grad():
        y_on, y_off = m(x, add1=a1), off(x, add1=a1)
    assert calls == {"wide": 4, "linear": 0}
    assert torch.equal(y_on, y_off) and torch.equal(y_on, y.detach())


def test_module_without_the_switch_routes_as_before(dev, monkeypatch):
    m = _block(dev, "relu", "euler", 0.1, seed=12, switch=False)
    calls = W._spies(monkeypatch)
    m(torch.randn(5, D, device=dev, requires_grad=True))
    assert calls == {"wide": 0, "linear": ode.n_feval("euler", 0.1)}


# ---------------------------------------------------------------------------------------------------------- 6. module, dopri5
def test_module_routes_dopri5_to_the_adaptive_kernels(dev):
    from agplace_amd import autograd_ops, ops
    m = _block(dev, "relu", "dopri5", seed=13)
    fc = m.func.func.fc
    g = torch.Generator().manual_seed(14)
    x, a1 = torch.randn(9, D, generator=g).to(dev), (0.5 * torch.randn(9, D, generator=g)).to(dev)
    with torch.no_grad():
        y = m(x, add1=a1)
    assert m.solver_stats()["status"] == 0
    assert torch.equal(y, ops.fcode_adaptive(x, m._prep.get(), "relu", "dopri5", m.tol, m.max_steps, add1=a1)[0])
    gy = torch.randn(9, D, generator=g).to(dev)
    grads = []
    for call in (lambda xx: m(xx, add1=a1), lambda xx: autograd_ops.FCODEFn.apply(xx, fc.weight, fc.bias, m, a1, None)):
        fc.weight.grad = fc.bias.grad = None
        xx = x.clone().requires_grad_(True)
        out = call(xx)
        assert torch.equal(out.detach(), y)
        out.backward(gy)
        grads.append((xx.grad, fc.weight.grad, fc.bias.grad))
    assert m.solver_stats()["status"] == 0
    assert all(p is not None and torch.equal(p, q) for p, q in zip(*grads))


# -------------------------------------------------------------------------------------------------------------------- 7. model
@pytest.mark.parametrize("kw", [{}, {"odeint_method": "rk4", "odeint_size": 0.25}], ids=["euler", "rk4"])
def test_model_trains_with_the_switch_on(dev, monkeypatch, kw):
    import test_gpu_mm_convnext_train as T
    calls = W._spies(monkeypatch)
    assert "fuseblocktoshallow.blocks.0.blocks.0.func.func.fc.weight" in T.MUST
    T._end_to_end(dev, True, False, fcode_wide=True, **kw)
    assert calls["wide"] == 3, calls             # the three FCODE(384) blocks, each on the recording launch


def test_model_takes_dopri5_with_the_switch_on(dev):
    from agplace_amd import ops
    from agplace_amd.network_mm.ffns import FCODE
    from agplace_amd.network_mm.mm import MM
    import test_gpu_mm_convnext_train as T
    opt = mm_convnext_ref.options("1_1_1", fcode_wide=True, odeint_method="dopri5")
    torch.manual_seed(0)
    model = MM(opt=opt)
    model.load_state_dict(T._state(), strict=True)
    model = model.to(dev).eval()
    blocks = [m for m in model.modules() if isinstance(m, FCODE)]
    assert len(blocks) == 3 and all(m.func.func.fc.in_features == D for m in blocks)
    seen = {}
    hooks = [m.register_forward_hook(lambda mod, args, out: seen.__setitem__(mod, (args, out))) for m in blocks]
    data = nets.synth_query(T.B, T.H, T.W, mm_convnext_ref.options(), seed=9)
    with torch.no_grad():
        out = model(to_dev(data, dev), mode="q")
    for h in hooks:
        h.remove()
    assert len(seen) == 3
    for m in blocks:
        args, y = seen[m]
        x, a1, a2 = (tuple(args) + (None, None))[:3]
        want = ops.fcode_adaptive(x, m._prep.get(), m.act_name, "dopri5", m.tol, m.max_steps, add1=a1, add2=a2)[0]
        assert torch.equal(y, want) and m.solver_stats()["status"] == 0
    assert len(T.KEYS) == 7
    for k in T.KEYS:
        assert bool(torch.isfinite(out[k]).all()), k
