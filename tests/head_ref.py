"""fp64 closed forms of the row-wise descriptor head (csrc/fusion.hip, csrc/fusion_bwd.hip, csrc/vecprog.hip): Linear(+act),
LayerNorm, L2-normalise, the weighted sum, the dot product and the fixed-grid Neural-ODE block FCODE, forward and backward.
Plain torch on the CPU, no autograd: tests/test_head_ref.py pins every form to fp64 autograd (F.layer_norm, F.normalize,
oracle/ode.py) and evaluates the floors and bars that tests/test_gpu_head_kernels.py holds the kernels to.

Every form takes `dtype` (float64: the reference; float32: the same closed form in the kernels' arithmetic, the floor of the
row-wise ops) and the matrix forms take `product`, the function that forms x W^T: `exact` (a plain matmul in `dtype`) or
`three_product`, the MFMA path's arithmetic (operands as bf16 pairs, hi*hi + hi*lo + lo*hi, fp64 accumulate) -- the arithmetic
floor of every Linear / FCODE comparison.

Bars (the rule of the whole file, evaluated from the reference alone):
    bar = min(4 x floor, ceiling),  floor never below 2^-24 (one rounding of the fp32 output)
  * matrix products: floor = per-row error of the three-product form (for the products the kernels form in plain fp32 -- the
    weight gradients -- of the float32 form) against exact fp64; ceilings 2e-5 Linear forward, 1e-4 FCODE forward and every data
    gradient, 1e-3 FCODE parameter gradients; tanh / sigmoid go through device fast-math the floor cannot model: bar = ceiling;
  * row-wise fp32 ops: floor = the float32 form's worst row; ceilings 1e-5 forward, 1e-4 backward;
  * column sums (gb, ggamma, gbeta): SUM_BAR of the sum of the absolute terms.
"""
import torch

ACTS = ("id", "relu", "tanh", "sigmoid")
CEIL_LINEAR_FWD, CEIL_DATA, CEIL_PARAM = 2e-5, 1e-4, 1e-3
CEIL_ROW_FWD, CEIL_ROW_BWD = 1e-5, 1e-4
SUM_BAR = 1e-5                   # |got - ref| <= SUM_BAR * sum |terms|: fp32 chains of a few dozen terms are ~2^-24 per term
MARGIN = 4.0                     # the factor tests/test_gpu_bn_bwd_kernels.py and tests/test_gpu_convnext_bwd.py give such a floor
ONE_ROUNDING = 2.0 ** -24
L2_CLAMP = 1e-12

# Butcher tableaus (A rows below the diagonal, b): torchdiffeq's euler, midpoint and rk4 (= the 3/8 rule, rk4_alt_step_func).
# "rk4_classic" is NOT what the kernels implement: the deliberately wrong variant of the discrimination tests.
TABLEAUS = {
    "euler": ([[]], [1.0]),
    "midpoint": ([[], [0.5]], [0.0, 1.0]),
    "rk4": ([[], [1.0 / 3.0], [-1.0 / 3.0, 1.0], [1.0, -1.0, 1.0]], [0.125, 0.375, 0.375, 0.125]),
    "rk4_classic": ([[], [0.5], [0.0, 0.5], [0.0, 0.0, 1.0]], [1.0 / 6.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 6.0]),
}


def stages(method):
    return len(TABLEAUS[method][1])


# ------------------------------------------------------------------------------------------------------------------ pieces
def _c(t, dtype):
    return None if t is None else t.to(dtype)


def act_fn(v, act):
    if act in (None, "id"):
        return v
    if act == "relu":
        return v.clamp_min(0)
    if act == "tanh":
        return torch.tanh(v)
    if act == "sigmoid":
        return 1.0 / (1.0 + torch.exp(-v))
    raise NotImplementedError(act)


def dact_from_output(y, act):
    """act' written in terms of the OUTPUT y = act(z), as the kernels take it (fusion_bwd.hip: dact_from_output)."""
    if act in (None, "id"):
        return torch.ones_like(y)
    if act == "relu":
        return (y > 0).to(y.dtype)
    if act == "tanh":
        return 1.0 - y * y
    if act == "sigmoid":
        return y * (1.0 - y)
    raise NotImplementedError(act)


def exact(x, w):
    """x [b, K], w [N, K] -> x w^T in the operands' dtype"""
    return x @ w.t()


def bf16_pair(v):
    """fp32 values -> (hi, lo) as fp64: hi = rn_bf16(v), lo = rn_bf16(v - hi)"""
    f = v.float()
    hi = f.bfloat16()
    lo = (f - hi.float()).bfloat16()
    return hi.double(), lo.double()


def three_product(x, w):
    """x w^T as the MFMA path forms it: both operands rounded to fp32 and split into bf16 pairs, hi*hi + hi*lo + lo*hi (the
    lo*lo term and the pairs' own rounding are what is dropped), accumulated in fp64."""
    xh, xl = bf16_pair(x)
    wh, wl = bf16_pair(w)
    return xh @ wh.t() + xh @ wl.t() + xl @ wh.t()


def per_row_rel(got, ref):
    """rel_l2 of every row (last dimension) -> 1-d fp64; a row whose reference is all zero must be zero: inf otherwise"""
    g, r = got.double().reshape(-1, got.shape[-1]), ref.double().reshape(-1, ref.shape[-1])
    num, den = (g - r).norm(dim=1), r.norm(dim=1)
    rel = num / den.clamp_min(1e-300)
    return torch.where(den > 0, rel, torch.where(num > 0, torch.full_like(num, float("inf")), torch.zeros_like(num)))


def worst_row(got, ref):
    rel = per_row_rel(got, ref)
    return float(rel.max()) if rel.numel() else 0.0


def bar_of(floor, ceiling, fast_math=False):
    """min(4 x floor, ceiling) with the floor never below one fp32 rounding; the ceiling itself behind device fast-math"""
    if fast_math:
        return ceiling
    return min(MARGIN * max(float(floor), ONE_ROUNDING), ceiling)


def sum_check(got, terms, magnitudes=None):
    """A column sum against fp64: (worst |got - sum| / sum |terms| over the columns, ok); terms [rows, columns]; magnitudes:
    the terms' sizes where a term is itself a difference (default |terms|)"""
    ref, mag = terms.double().sum(0), (terms if magnitudes is None else magnitudes).double().abs().sum(0)
    err = (got.double() - ref).abs()
    ok = bool((err <= SUM_BAR * mag).all())
    return float((err / mag.clamp_min(1e-300)).max()) if err.numel() else 0.0, ok


# ------------------------------------------------------------------------------------------------------------------ Linear
def linear(x, add1, add2, w, bias, act, dtype=torch.float64, product=exact):
    """act((x + add1 + add2) w^T + bias); x [b, K], w [N, K]"""
    v = x.to(dtype)
    if add1 is not None:
        v = v + add1.to(dtype)
    if add2 is not None:
        v = v + add2.to(dtype)
    z = product(v, w.to(dtype)).to(dtype)
    if bias is not None:
        z = z + bias.to(dtype)
    return act_fn(z, act)


def linear_gz(y, gy, act, dtype=torch.float64):
    gy = gy.to(dtype)
    return gy if act in (None, "id") else gy * dact_from_output(y.to(dtype), act)


def linear_bwd(x, y, gy, w, act, dtype=torch.float64, product=exact, drop_row=None):
    """-> gx [b, K], gw [N, K], gb [N] of y = act(x w^T + bias), act' from the output y.  drop_row: the wrong variant whose
    parameter gradients miss that batch row."""
    gz = linear_gz(y, gy, act, dtype)
    gx = product(gz, w.to(dtype).t().contiguous()).to(dtype)
    gzp, xp = gz, x.to(dtype)
    if drop_row is not None:
        keep = [i for i in range(gz.shape[0]) if i != drop_row]
        gzp, xp = gz[keep], xp[keep]
    return gx, gzp.t() @ xp, gzp.sum(0)


# --------------------------------------------------------------------------------------------------------------- LayerNorm
def _ln_stats(x, eps):
    mean = x.mean(1, keepdim=True)
    d = x - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(1, keepdim=True) + eps)
    return d * rstd, rstd


def layernorm(x, gamma, beta, eps, relu, res, dtype=torch.float64):
    """relu?(LN(x) gamma + beta + res) over the last dimension, biased variance"""
    xh, _ = _ln_stats(x.to(dtype), eps)
    y = xh
    if gamma is not None:
        y = y * gamma.to(dtype)
    if beta is not None:
        y = y + beta.to(dtype)
    if res is not None:
        y = y + res.to(dtype)
    return y.clamp_min(0) if relu else y


def layernorm_bwd(x, gamma, y, gy, eps, relu, dtype=torch.float64, drop_s2=False, mask_params=True):
    """-> gx, gres, ggamma, gbeta, the ReLU mask taken from the output y:
         g = gy [y > 0],  gxh = g gamma,  gx = rstd (gxh - mean(gxh) - xhat mean(gxh xhat)),  gres = g,
         ggamma = sum_rows g xhat,  gbeta = sum_rows g.
    Wrong variants: drop_s2 leaves the `xhat mean(gxh xhat)` term out, mask_params=False sums ggamma / gbeta without the mask."""
    x, gy = x.to(dtype), gy.to(dtype)
    g = gy * (y.to(dtype) > 0).to(dtype) if relu else gy
    xh, rstd = _ln_stats(x, eps)
    gxh = g if gamma is None else g * gamma.to(dtype)
    s1 = gxh.mean(1, keepdim=True)
    s2 = (gxh * xh).mean(1, keepdim=True)
    gx = rstd * (gxh - s1 - (0 if drop_s2 else xh * s2))
    gpar = g if mask_params else gy
    return gx, g, (gpar * xh).sum(0), gpar.sum(0)


def layernorm_param_terms(x, y, gy, eps, relu):
    """the terms of ggamma and gbeta, [b, d] each (fp64), and the sizes of ggamma's: a term g (x - mean) rstd is a difference --
    where x is close to the row's mean its float32 error is 2^-24 of |g| (|x| + |mean|) rstd, not of the term -- so that is what
    sum_check measures the error of ggamma against.  This DEPARTS from "1e-5 of the sum of the absolute terms" |g xhat|, to the
    looser side (1x to 5x): the float32 closed form itself misses that bound where a row has few terms (b = 1 .. 5)."""
    x, gy = x.double(), gy.double()
    g = gy * (y.double() > 0).double() if relu else gy
    xh, rstd = _ln_stats(x, eps)
    return g * xh, g, g.abs() * (x.abs() + x.mean(1, keepdim=True).abs()) * rstd


# ------------------------------------------------------------------------------------------------------------ L2-normalise
def l2normalize(x, dtype=torch.float64):
    """x / max(|x|, 1e-12): a row with |x| <= 1e-12 gives 0 (it is all but zero already)"""
    x = x.to(dtype)
    nrm = torch.sqrt((x * x).sum(1, keepdim=True))
    return x / nrm.clamp_min(L2_CLAMP)


def l2normalize_bwd(x, gy, dtype=torch.float64):
    """gx = (gy - y (y . gy)) / |x|, y = x / |x|; a clamped row (|x| <= 1e-12) has the constant divisor: gx = gy / 1e-12"""
    x, gy = x.to(dtype), gy.to(dtype)
    nrm = torch.sqrt((x * x).sum(1, keepdim=True))
    live = nrm > L2_CLAMP
    safe = torch.where(live, nrm, torch.ones_like(nrm))
    dot = (x * gy).sum(1, keepdim=True)
    return torch.where(live, (gy - x * (dot / (safe * safe))) / safe, gy / L2_CLAMP)


# ---------------------------------------------------------------------------------------------------------------- wsum, dot
def wsum(xs, ws=None, dtype=torch.float64):
    """sum_t ws[t] xs[t]; a weight that is None counts 1"""
    ws = [None] * len(xs) if ws is None else ws
    s = torch.zeros_like(xs[0], dtype=dtype)
    for x, w in zip(xs, ws):
        s = s + x.to(dtype) * (1.0 if w is None else w.to(dtype).reshape(()))
    return s


def dot(a, b, dtype=torch.float64):
    return (a.to(dtype).reshape(-1) * b.to(dtype).reshape(-1)).sum()


# ------------------------------------------------------------------------------------------------------------------- FCODE
def fcode_traj(x, w, bias, act, method, dts, add1=None, add2=None, dtype=torch.float64, product=exact):
    """The fixed-grid solve of y' = act(y w^T + bias), y(0) = x (+ adds) over the steps dts -> (y, traj); traj in the kernels'
    layout [step][slot][b][256], slot 0 = the step's state, slots 1.. = k_i.  Stage inputs as fusion.hip's comments give them:
        euler     k1 = f(y);                                   y' = y + dt k1
        midpoint  k1 = f(y), k2 = f(y + k1 dt / 2);            y' = y + dt k2
        rk4 (3/8) k1 = f(y), k2 = f(y + dt k1 / 3), k3 = f(y + dt (k2 - k1 / 3)), k4 = f(y + dt (k1 - k2 + k3));
                  y' = y + (k1 + 3 (k2 + k3) + k4) dt / 8"""
    A, bw = TABLEAUS[method]
    wd, bd = w.to(dtype), _c(bias, dtype)
    y = x.to(dtype)
    for a in (add1, add2):
        if a is not None:
            y = y + a.to(dtype)
    traj = []
    for dt in dts:
        dt = float(dt)
        ks = []
        for i in range(len(bw)):
            s = y
            for j, aij in enumerate(A[i]):
                if aij:
                    s = s + (dt * aij) * ks[j]
            z = product(s, wd).to(dtype)
            ks.append(act_fn(z if bd is None else z + bd, act))
        traj.append(torch.stack([y] + ks))
        for bi, k in zip(bw, ks):
            if bi:
                y = y + (dt * bi) * k
    return y, torch.stack(traj)


def fcode_bwd(traj, gy, w, act, method, dts, dtype=torch.float64, product=exact, drop_row=None):
    """-> gx, gw, gb by the recurrences at the top of fusion_bwd.hip, one step at a time from the last (a = dL/dy'):
         for i = last .. first:  u_i = dt b_i a + dt sum_{j > i} A_ji gs_j,  gz_i = u_i act'(k_i),  gs_i = gz_i W
         dL/dy = a + sum_i gs_i;  dW += gz_i^T s_i;  db += sum_batch gz_i        (s_i = y + dt sum_j A_ij k_j, k_i recorded)"""
    A, bw = TABLEAUS[method]
    nst = len(bw)
    wd = w.to(dtype)
    wt = wd.t().contiguous()
    a = gy.to(dtype)
    tr = traj.to(dtype)
    gw = torch.zeros_like(wd)
    gb = torch.zeros(wd.shape[0], dtype=dtype)
    keep = None if drop_row is None else [i for i in range(a.shape[0]) if i != drop_row]
    for s in range(len(dts) - 1, -1, -1):
        dt = float(dts[s])
        y, ks = tr[s, 0], [tr[s, 1 + i] for i in range(nst)]
        gs = [None] * nst
        total = a
        for i in range(nst - 1, -1, -1):
            u = (dt * bw[i]) * a
            for j in range(i + 1, nst):
                if A[j][i]:
                    u = u + (dt * A[j][i]) * gs[j]
            gz = u * dact_from_output(ks[i], act)
            sin = y
            for j, aij in enumerate(A[i]):
                if aij:
                    sin = sin + (dt * aij) * ks[j]
            gs[i] = product(gz, wt).to(dtype)
            total = total + gs[i]
            gzp, sp = (gz, sin) if keep is None else (gz[keep], sin[keep])
            gw = gw + gzp.t() @ sp
            gb = gb + gzp.sum(0)
        a = total
    return a, gw, gb


# ------------------------------------------------------------------------------------------- the cases of the GPU tests
# Shared by tests/test_head_ref.py (floors, bars, discrimination: on the CPU) and tests/test_gpu_head_kernels.py.
LINEAR_B = (1, 16, 17, 33)                       # one row, a full 16-row block, one row into the next, three blocks
LINEAR_K = (32, 96, 256, 288, 320, 1024)         # nks = 1, 3, 8 (one whole fetch chunk), 9 and 10 (a ragged second chunk), 32 (MAXK)


def linear_fwd_cases():
    """[(b, k, n, act, adds, bias)]: every (b, K) once; N, the activation, the number of add operands and bias == NULL cycle with
    periods 2, 4, 3 and 5 (shifted per b), so each value meets every K"""
    out = []
    for i, (b, k) in enumerate((b, k) for b in LINEAR_B for k in LINEAR_K):
        j = i + i // len(LINEAR_K)
        out.append((b, k, (256, 512)[j % 2], ACTS[j % 4], i % 3, i % 5 != 4))
    return out


LINEAR_BWD_SHAPES = ((1, 32, 256), (17, 96, 100), (33, 256, 128), (16, 320, 40), (70, 96, 256))
LN_D = (32, 64, 100, 256, 4096)
LN_B = (1, 3, 4, 5, 9)
# name -> (gamma and beta given, relu, residual / gres, ggamma and gbeta wanted)
LN_VARIANTS = {"affine_relu_res": (True, True, True, True), "plain": (False, False, False, False),
               "affine": (True, False, False, True), "noaffine_relu_res_params": (False, True, True, True)}
LN_EPS = 1e-5
FCODE_SOLVERS = (("euler", 1.0), ("euler", 0.1), ("midpoint", 0.3), ("rk4", 0.25))
FCODE_ACTS = ("relu", "tanh", "sigmoid", "id")


def fcode_cases():
    """[(b, method, step, act)]: every solver meets every activation once; b runs through a Latin square, so every b meets
    every solver and every activation once (four times in all)"""
    return [(LINEAR_B[(i + j) % 4], m, s, a) for i, (m, s) in enumerate(FCODE_SOLVERS) for j, a in enumerate(FCODE_ACTS)]


def grid_dts(step):
    """the per-step dt of torchdiffeq's fixed grid on [0, 1], in fp32 as the solver builds it -> list of floats"""
    from oracle import ode
    return [float(v) for v in ode.grid_dts(step)]


def _gen(*key):
    seed = 0
    for v in key:
        seed = (seed * 1000003 + int(v)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def draw_linear(b, k, n, seed=0):
    """fp32 operands of a Linear: x, add1, add2 [b, k], w [n, k] (unit-variance outputs), bias [n], gy [b, n]"""
    g = _gen(b, k, n, seed)
    x, a1, a2 = (torch.randn((b, k), generator=g) for _ in range(3))
    w = torch.randn((n, k), generator=g) / k ** 0.5
    return x, 0.5 * a1, 0.25 * a2, w, 0.3 * torch.randn(n, generator=g), torch.randn((b, n), generator=g)


def draw_rows(b, d, seed=0, zero_row=None):
    """fp32 operands of the row-wise ops: x (rows of different scale and offset), res, gy [b, d], gamma, beta [d]"""
    g = _gen(b, d, seed, 7)
    x = torch.randn((b, d), generator=g) * (0.5 + 2 * torch.rand((b, 1), generator=g)) + torch.randn((b, 1), generator=g)
    res, gy = torch.randn((b, d), generator=g), torch.randn((b, d), generator=g)
    gamma = (0.5 + torch.rand(d, generator=g)) * torch.where(torch.rand(d, generator=g) < 0.25, -1.0, 1.0)
    beta = 0.3 * torch.randn(d, generator=g)
    if zero_row is not None:
        x[zero_row] = 0
    return x, res, gy, gamma, beta


def draw_fcode(b, seed=0):
    """x, add1, add2 [b, 256], w [256, 256] (spectral radius about 1: the solve neither dies nor blows up), bias, gy"""
    g = _gen(b, seed, 11)
    x, a1, a2, gy = (torch.randn((b, 256), generator=g) for _ in range(4))
    w = torch.randn((256, 256), generator=g) / 16.0
    return x, 0.5 * a1, 0.25 * a2, w, 0.3 * torch.randn(256, generator=g), gy


# ------------------------------------------------------------------------------------------------------ bars of the cases
def row_bars(floor_rows, ceiling, fast_math=False):
    """per-row bars from per-row floors"""
    if fast_math:
        return torch.full_like(floor_rows, ceiling)
    return (MARGIN * floor_rows.clamp_min(ONE_ROUNDING)).clamp_max(ceiling)


def fast_math(act):
    return act in ("tanh", "sigmoid")


def linear_fwd_bars(x, add1, add2, w, bias, act):
    """-> (y64, per-row bars, per-row floors) of agp_linear_fwd on these operands"""
    ref = linear(x, add1, add2, w, bias, act)
    floor = per_row_rel(linear(x, add1, add2, w, bias, act, product=three_product), ref)
    return ref, row_bars(floor, CEIL_LINEAR_FWD, fast_math(act)), floor


def linear_bwd_bars(x, y, gy, w, act):
    """-> ((gx, gw, gb) fp64, gx bars per batch row, gw bars per output row, gz fp64: the terms of gb).  gx is a three-product
    of the MFMA path, gw a plain fp32 GEMM: the floor of each is its own arithmetic."""
    ref = linear_bwd(x, y, gy, w, act)
    gx3 = linear_bwd(x, y, gy, w, act, product=three_product)[0]
    gw32 = linear_bwd(x, y, gy, w, act, dtype=torch.float32)[1]
    return (ref, row_bars(per_row_rel(gx3, ref[0]), CEIL_DATA), row_bars(per_row_rel(gw32, ref[1]), CEIL_DATA),
            linear_gz(y, gy, act))


def rowwise_bar(form32, form64, ceiling):
    """(bar, floor) of a row-wise fp32 op: floor = the worst row of the float32 form"""
    floor = worst_row(form32, form64)
    return bar_of(floor, ceiling), floor


def fcode_fwd_bars(x, add1, add2, w, bias, act, method, dts):
    """-> (y64, traj64, bars [b] of y, bars [step, slot, b] of traj)"""
    y, traj = fcode_traj(x, w, bias, act, method, dts, add1, add2)
    y3, traj3 = fcode_traj(x, w, bias, act, method, dts, add1, add2, product=three_product)
    fy = per_row_rel(y3, y)
    ft = per_row_rel(traj3, traj).reshape(traj.shape[:3])
    return y, traj, row_bars(fy, CEIL_DATA, fast_math(act)), row_bars(ft, CEIL_DATA, fast_math(act))


def fcode_bwd_bars(traj, gy, w, act, method, dts):
    """-> ((gx, gw, gb) fp64, gx bars per batch row, gw bars per output row (one value: see below), the gb bar): the floor is the
    larger of the three-product form's error (the gz W products feed every later gz) and the float32 form's (gw / gb are plain
    fp32 sums)"""
    ref = fcode_bwd(traj, gy, w, act, method, dts)
    e3 = fcode_bwd(traj, gy, w, act, method, dts, product=three_product)
    e32 = fcode_bwd(traj, gy, w, act, method, dts, dtype=torch.float32)
    fx = torch.maximum(per_row_rel(e3[0], ref[0]), per_row_rel(e32[0], ref[0]))
    # A row n of gw is sum_r gz[r][n] s[r][:]: its relative error is that of the few SCALARS gz[r][n] (one per stage and step at
    # b = 1), and a scalar of a three-product row is off by 3e-6 of the row's norm, not of itself -- a heavy-tailed figure of which
    # one row's floor is a single sample, the kernel's (another association of the same sums) a second one.  The yardstick is the
    # scale of that distribution: the worst row of the case, for every row.
    fw = torch.maximum(per_row_rel(e3[1], ref[1]), per_row_rel(e32[1], ref[1]))
    fw = torch.full_like(fw, float(fw.max()))
    fb = max(worst_row(e3[2][None], ref[2][None]), worst_row(e32[2][None], ref[2][None]))
    return ref, row_bars(fx, CEIL_DATA), row_bars(fw, CEIL_PARAM), bar_of(fb, CEIL_PARAM)
