"""FC / ODEFunc / FCODE, drop-ins for reference network_mm/ffns.py:14-21,51-76,78-87.

FCODE.forward(x[b,D]) = odeint(f, x, t=[0,1], method=opt.odeint_method,
options={'step_size': opt.odeint_size})[-1] with f(t, y) = act(Linear(y)).  torchdiffeq is not
used: the whole fixed-grid solve (all steps, all stages) is ONE persistent HIP kernel
(agp_fcode_fwd) that keeps W's MFMA fragments in registers.  dim = 384 in inference (no gradient wanted) is one launch as well
(agp_fcode_wide_fwd: W's `hi` plane in registers, the `lo` plane streamed from L2); every other width, and
384 with a gradient wanted, runs the same steps as a sequence of differentiable launches (_forward_any_width) -- unless
Options.fcode_wide opted in: FCODE(384) then trains on the one-launch kernel recording its trajectory and its one-launch backward
(agp_fcode_wide_fwd_traj / agp_fcode_wide_bwd) and takes the adaptive methods (agp_fcode_adaptive_wide_fwd / _bwd).
The time grid follows torchdiffeq's constructor exactly (niters = ceil(1/step + 1), arange * step, last point forced
to 1) and is kept in fp32 (the reference builds t with .float().type_as(x)).
'rk4' is torchdiffeq's 3/8-rule variant.  rtol/atol (opt.tol) are ignored by fixed-grid solvers.
odeint_method = 'dopri5' (torchdiffeq's default, adaptive) reads them: rtol = atol = opt.tol, one launch per solve as well
(agp_fcode_adaptive_fwd), at most opt.odeint_max_steps attempted steps; odeint_size is ignored.
odeint_method = 'bosh3' (Bogacki-Shampine 3(2), four stages) is the same controller and the same kernels over another table;
it is taken only with Options.odeint_adaptive_family set and refused otherwise.
state_dict keys: func.func.fc.{weight,bias} (via ODEFunc -> FC -> nn.Linear).
"""
import torch
import torch.nn as nn

from .. import _lib, autograd_ops, ops
from ..options import get_options

_ACTS = (None, 'id', 'relu', 'tanh', 'sigmoid')


def select_act(act):
    """Same contract as the reference: returns the activation NAME's module (for introspection);
    unknown names raise NotImplementedError (ffns.py:62-63)."""
    if act is None or act == 'id':
        return nn.Identity()
    if act == 'relu':
        return nn.ReLU()
    if act == 'tanh':
        return nn.Tanh()
    if act == 'sigmoid':
        return nn.Sigmoid()
    raise NotImplementedError


class _PreparedLinear:
    """Caches the split-bf16 planes of an nn.Linear until its parameters change."""

    def __init__(self, linear, with_transpose=False):
        self.linear, self.with_transpose = linear, with_transpose
        self._key, self._lw = None, None

    def get(self, with_transpose=False, exp=0):
        """Split planes of W (and of W^T when a backward pass needs gz W).  exp (inference only): W and b times 2^exp -- the
        projection of a vector that is added into a map stored with an exponent (agplace_amd/map_exponents.py); exact, the
        split planes scale with it."""
        w, b = self.linear.weight, self.linear.bias
        wt = self.with_transpose or with_transpose
        key = (w.data_ptr(), w._version, None if b is None else (b.data_ptr(), b._version), exp)
        if key != self._key or (wt and self._lw.wt_hi is None):
            if exp:
                e = torch.tensor(exp, device=w.device)
                self._lw = ops.LinearWeights(torch.ldexp(w.detach().float(), e), None if b is None else torch.ldexp(b.detach().float(), e),
                                             with_transpose=wt)
            else:
                self._lw = ops.LinearWeights(w, b, with_transpose=wt)
            self._key = key
        return self._lw


class FC(nn.Module):
    def __init__(self, indim, outdim, act=None):
        super().__init__()
        if act not in _ACTS:
            raise NotImplementedError
        self.fc = nn.Linear(indim, outdim)
        self.act = select_act(act)
        self.act_name = act
        self._prep = _PreparedLinear(self.fc)

    def forward(self, x):
        return autograd_ops.linear(x, self.fc, self._prep, act=self.act_name)


class ODEFunc(nn.Module):
    def __init__(self, func):
        super().__init__()
        self.func = func

    def forward(self, t, x):
        return self.func(x)


class FCODE(nn.Module):
    def __init__(self, dim, act=None, opt=None):
        super().__init__()
        opt = opt or get_options()
        self.func = ODEFunc(FC(dim, dim, act))
        self.act_name = act
        self.method = opt.odeint_method
        self.step_size = opt.odeint_size
        family = tuple(_lib.ODE_ADAPTIVE) if opt.odeint_adaptive_family else ('dopri5',)
        if self.method not in ('euler', 'midpoint', 'rk4') + family:
            raise NotImplementedError(self.method)
        self.adaptive = self.method in _lib.ODE_ADAPTIVE
        self.tol = float(opt.tol)
        self.max_steps = int(opt.odeint_max_steps)
        if self.adaptive and not self.tol > 0.0:
            raise ValueError(f"tol {opt.tol!r}: {self.method} needs rtol = atol > 0")
        self.dts = None if self.adaptive else ops.ode_grid_dts(self.step_size)
        self._ctrl = None                 # device control block of the last adaptive solve (solver_stats)
        self.wide_routes = bool(opt.fcode_wide) and dim == ops.FCODE_WIDE_DIM       # Options.fcode_wide, at its one width
        self._prep = _PreparedLinear(self.func.func.fc)

    def forward(self, x, add1=None, add2=None):
        fc = self.func.func.fc
        if fc.in_features == 256:
            return autograd_ops.FCODEFn.apply(x, fc.weight, fc.bias, self, add1, add2)
        if self.wide_routes and (self.adaptive or (torch.is_grad_enabled() and any(
                t is not None and t.requires_grad for t in (x, add1, add2, fc.weight, fc.bias)))):
            # opted in at 384 columns: a fixed grid with a gradient wanted records its trajectory in the one-launch kernel, an
            # adaptive method runs on the adaptive kernels; a fixed grid without a gradient is the inference launch below either way
            return autograd_ops.FCODEFn.apply(x, fc.weight, fc.bias, self, add1, add2)
        if fc.in_features == ops.FCODE_WIDE_DIM and not self.adaptive and not (torch.is_grad_enabled() and any(
                t is not None and t.requires_grad for t in (x, add1, add2, fc.weight, fc.bias))):
            # inference at 384 columns: the whole solve in one launch (csrc/fusion_wide.hip); with a gradient wanted the
            # any-width route below, whose launches are differentiable
            return ops.fcode_wide(x, self._prep.get(), self.act_name, self.method, self.dts, add1=add1, add2=add2)
        return self._forward_any_width(x, add1, add2)

    def solver_stats(self):
        """The record of this block's last adaptive solve (synchronises): status, accepted, rejected, attempted, f_evals,
        t0, t1, dts.  Raises RuntimeError when that solve failed (its output is NaN)."""
        if self._ctrl is None:
            raise RuntimeError("solver_stats: no adaptive solve has run on this block")
        st = ops.ode_stats(self._ctrl)
        if st["status"] != 0:
            raise RuntimeError(f"FCODE {self.method}: {_lib.ODE_STATUS.get(st['status'], st['status'])} after "
                               f"{st['attempted']} attempted steps (t = {st['t0']:.6g}); the output is NaN")
        return st

    def _forward_any_width(self, x, add1, add2):
        """FCODE(dim) for dim != 256 (the reference's class takes any width, ffns.py:78-87; `--mm_stg2fuse_dim`,
        tools/options.py:113): the persistent one-launch solver keeps W as 64 VGPRs of MFMA fragments per wave, which is a
        256 x 256 matrix; other widths run the same fixed-grid steps as a sequence of launches -- act(Linear(y)) on
        agp_linear_fwd and the stage combinations on agp_wsum_fwd (both differentiable through autograd_ops) -- with the
        time grid of torchdiffeq's constructor.  Latency-bound like the fused kernel, ~3 launches per stage instead of one
        per solve."""
        fc, dev = self.func.func.fc, x.device
        if self.adaptive:
            raise NotImplementedError(f"FCODE {self.method}: the adaptive solver is built for dim=256, got {fc.in_features}")
        if fc.in_features % 32:
            raise NotImplementedError("FCODE: dim must be a multiple of 32")
        key = str(dev)
        if getattr(self, "_consts_dev", None) != key:
            def c(v):
                return torch.tensor([v], dtype=torch.float32, device=dev)
            self._consts = [{"dt": c(dt), "hdt": c(0.5 * dt), "dt3": c(dt / 3.0), "mdt3": c(-dt / 3.0), "mdt": c(-dt),
                             "dt8": c(dt * 0.125), "3dt8": c(dt * 0.375)} for dt in self.dts]
            self._consts_dev = key

        def f(y):
            return autograd_ops.linear(y, fc, self._prep, act=self.act_name)
        ws = autograd_ops.wsum
        y = x if add1 is None and add2 is None else ws([t for t in (x, add1, add2) if t is not None])
        for k in self._consts:
            if self.method == 'euler':
                y = ws([y, f(y)], [None, k["dt"]])
            elif self.method == 'midpoint':
                k1 = f(y)
                y = ws([y, f(ws([y, k1], [None, k["hdt"]]))], [None, k["dt"]])
            else:       # torchdiffeq's 'rk4' = the 3/8 rule (rk4_alt_step_func)
                k1 = f(y)
                k2 = f(ws([y, k1], [None, k["dt3"]]))
                k3 = f(ws([y, k2, k1], [None, k["dt"], k["mdt3"]]))
                k4 = f(ws([y, k1, k2, k3], [None, k["dt"], k["mdt"], k["dt"]]))
                y = ws([y, k1, k2, k3, k4], [None, k["dt8"], k["3dt8"], k["3dt8"], k["dt8"]])
        return y
