"""References and problem builders of the sparse-kernel tests (tests/test_sparse_kernel_ref.py pins them to oracle/sparse.py on
the CPU, tests/test_gpu_sparse_kernels.py holds the HIP kernels against them): gather tables without coordinates, plain fp64
forms of the gather-GEMM, its weight gradient and the segment operations of csrc/sparse.hip, the storage-format emulation of
the convolution, and the per-granule error.  Every function works on the device of its arguments (torch's own ops only)."""
import numpy as np
import torch

from conv_sched_util import _bf16_pair, _f16


# ------------------------------------------------------------------------------------------------------------------ tables
def gather_table(ntaps, n_out, n_in, density, seed, centre=None, lacking=None, single=None, absent_rows=0):
    """int32 [ntaps, n_out] gather table with entries in [0, n_in]; n_in is the zero row ("no neighbour").  A (tap, row) pair
    has a neighbour with probability `density`, a uniformly drawn input row.  Switches, applied in this order:
      centre       tap index that becomes the identity (row i reads input row i, the zero row beyond n_in)
      lacking      {granule: taps}: the 128-row granule [128 g, 128 g + 128) has no neighbour through these taps
      single       (granule, tap): every row of the granule keeps that one tap (made present) and loses all others
      absent_rows  this many rows (drawn without replacement, the last row always among them) lose every tap"""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, max(n_in, 1), size=(ntaps, n_out), dtype=np.int64)
    tab = np.where(rng.random((ntaps, n_out)) < density, idx, n_in).astype(np.int32)
    if centre is not None:
        rows = np.arange(n_out)
        tab[centre] = np.where(rows < n_in, rows, n_in)
    for g, taps in (lacking or {}).items():
        tab[list(taps), g * 128:(g + 1) * 128] = n_in
    if single is not None:
        g, tap = single
        sl = slice(g * 128, min((g + 1) * 128, n_out))
        keep = np.where(tab[tap, sl] == n_in, rng.integers(0, max(n_in, 1), size=sl.stop - sl.start), tab[tap, sl])
        tab[:, sl] = n_in
        tab[tap, sl] = keep
    if absent_rows:
        rows = rng.choice(n_out, size=min(absent_rows, n_out), replace=False)
        rows[0] = n_out - 1
        tab[:, rows] = n_in
    return tab


def one_hot_table(n_out, n_in, seed, ntaps=8):
    """The table SparseTensor.up_map makes for a transposed convolution: every output row has ONE parent, through one tap."""
    rng = np.random.default_rng(seed)
    tab = np.full((ntaps, n_out), n_in, dtype=np.int32)
    tab[rng.integers(0, ntaps, n_out), np.arange(n_out)] = rng.integers(0, max(n_in, 1), n_out)
    return tab


def granule_masks(table, zero_row, perm=None, n_valid=None, ngran=None):
    """What agp_sparse_tile_taps must write: per 128 GEMM rows (row m computes output row perm[m], or m) the OR of
    (1 << tap) over the taps for which at least one of the granule's VALID rows (m < n_valid) has a neighbour."""
    ntaps, n_out = table.shape
    n_valid = n_out if n_valid is None else min(n_valid, n_out)
    ngran = (n_out + 127) // 128 if ngran is None else ngran
    rows = np.arange(n_out) if perm is None else np.asarray(perm)
    out = np.zeros(ngran, dtype=np.uint64)
    for g in range(ngran):
        r = rows[g * 128:min((g + 1) * 128, n_valid)]
        for t in range(ntaps):
            if r.size and bool((table[t, r] != zero_row).any()):
                out[g] |= np.uint64(1 << t)
    return out


# ------------------------------------------------------------------------------------------------------- gather-GEMM, fp64
def _idx(table, dev):
    return torch.as_tensor(table, device=dev).long()


def conv_ref64(x, table, w, scale=None, shift=None, res=None, relu=False):
    """out[i] = relu?( scale * sum_t x[table[t][i]] @ w[t] + shift + res[i] ) in fp64.  x [n_in + 1, cin] (the last row zero),
    table [ntaps, n_out], w [ntaps, cin, cout], scale / shift [cout], res [n_out, cout]."""
    x, w = x.double(), w.double()
    tab = _idx(table, x.device)
    y = torch.zeros((tab.shape[1], w.shape[2]), dtype=torch.float64, device=x.device)
    for t in range(tab.shape[0]):
        y += x.index_select(0, tab[t]) @ w[t]
    if scale is not None:
        y = y * scale.double()
    if shift is not None:
        y = y + shift.double()
    if res is not None:
        y = y + res.double()
    return torch.relu(y) if relu else y


def store_round(prec):
    """The rounding of a precision's FEATURE storage format (4 and 2: one fp16 plane; 3: a bf16 pair)."""
    return _bf16_pair if prec == 3 else _f16


def weight_round(prec):
    """The rounding of a precision's WEIGHT planes (4: fp16; 2: an fp16 pair; 3: a bf16 pair)."""
    if prec == 4:
        return _f16
    if prec == 3:
        return _bf16_pair

    def f16_pair(t):
        t = t.float()
        hi = t.half()
        return hi.double() + (t - hi.float()).half().double()
    return f16_pair


def emulate(prec, x, table, w, scale=None, shift=None, res=None, relu=False):
    """conv_sched_util.emulate for the gather-GEMM: operands and residual rounded to the mode's storage formats, fp64
    arithmetic, the result rounded to the stored format."""
    rnd = store_round(prec)
    return rnd(conv_ref64(rnd(x), table, weight_round(prec)(w), scale, shift, None if res is None else rnd(res), relu))


def wgrad_ref64(x, table, g):
    """gw[t][ci][co] = sum_i x[table[t][i]][ci] * g[i][co] in fp64 -> [ntaps, cin, cout]."""
    x, g = x.double(), g.double()
    tab = _idx(table, x.device)
    return torch.stack([x.index_select(0, tab[t]).t() @ g for t in range(tab.shape[0])])


def wgrad_f32(x, table, g):
    """The same sum in plain fp32 (index_select + matmul): the yardstick of the weight-gradient bar."""
    x, g = x.float(), g.float()
    tab = _idx(table, x.device)
    return torch.stack([x.index_select(0, tab[t]).t() @ g for t in range(tab.shape[0])])


# ------------------------------------------------------------------------------------------------------ segment ops, fp64
def seg_bidx(seg_off):
    """int64 [n]: the segment of every row (empty segments own no row)."""
    cnt = seg_off[1:] - seg_off[:-1]
    return torch.repeat_interleave(torch.arange(cnt.numel(), device=seg_off.device), cnt)


def _seg_sum(v, seg_off):
    """[B, C]: the sum of every segment's rows (plain slices: a handful of segments, however long)"""
    o = seg_off.tolist()
    return torch.stack([v[a:b].sum(0) for a, b in zip(o[:-1], o[1:])])


def _cnt(seg_off, dtype=torch.float64):
    return (seg_off[1:] - seg_off[:-1]).to(dtype).unsqueeze(1)


def seg_mean64(x, seg_off):
    """[B, C]: the mean of every segment's rows; 0 for an empty segment."""
    cnt = _cnt(seg_off)
    return torch.where(cnt > 0, _seg_sum(x.double(), seg_off) / cnt.clamp_min(1), torch.zeros_like(cnt))


def seg_gem64(x, seg_off, p, eps=1e-6):
    """[B, C]: ( mean_i max(x_i, eps)^p )^(1/p) per segment; 0 for an empty segment.  p may be a tensor that requires grad."""
    cnt = _cnt(seg_off)
    m = _seg_sum(x.double().clamp(min=eps).pow(p), seg_off) / cnt.clamp_min(1)
    return torch.where(cnt > 0, torch.where(cnt > 0, m, torch.ones_like(m)).pow(1.0 / p), torch.zeros_like(m))


def seg_affine64(y, bidx, scale=None, add=None, res=None, relu=False):
    """relu?( y[i] * scale[b(i)] + add[b(i)] + res[i] )"""
    v = y.double()
    b = bidx.long()
    if scale is not None:
        v = v * scale.double()[b]
    if add is not None:
        v = v + add.double()[b]
    if res is not None:
        v = v + res.double()
    return torch.relu(v) if relu else v


def seg_dot64(a, b, seg_off):
    """[B, C]: sum over a segment's rows of a * b (b None: of a)."""
    return _seg_sum(a.double() if b is None else a.double() * b.double(), seg_off)


def _gem_dp_parts(x, seg_off, ggem, gem_y, p, eps):
    """dL/dp of the segment GeM as two [B, C] terms, dp = sum(a - b):
         a = ggem y mean_i(xc^p ln xc) / (p mean_i xc^p),   b = ggem y ln(mean_i xc^p) / p^2,   xc = max(x, eps)"""
    xc = x.double().clamp(min=eps)
    y = gem_y.double()
    cnt = _cnt(seg_off)
    live = cnt > 0
    m = torch.where(live, _seg_sum(xc.pow(p), seg_off) / cnt.clamp_min(1), torch.ones_like(y))
    ml = _seg_sum(xc.pow(p) * xc.log(), seg_off) / cnt.clamp_min(1)
    gy = ggem.double() * y * live
    return gy * ml / (p * m), gy * m.log() / (p * p)


def gem_dp_magnitude64(x, seg_off, ggem, gem_y, p, eps=1e-6):
    """sum |a| + |b| of the terms of dL/dp: what an error of dL/dp is relative to (the terms cancel)."""
    a, b = _gem_dp_parts(x, seg_off, ggem, gem_y, float(p), eps)
    return float(a.abs().sum() + b.abs().sum())


def seg_pool_bwd64(x, seg_off, gmean=None, ggem=None, gem_y=None, p=None, eps=1e-6, base=None):
    """Backward of the segment mean / GeM into the rows, and dL/dp (closed forms of the kernel's header comment):
         out[i] = base[i] + gmean[b] / n_b + ggem[b] y[b]^(1-p) max(x_i, eps)^(p-1) [x_i >= eps] / n_b
         dp     = sum_{b,c} ggem y ( mean_i(xc^p ln xc) / (p mean_i xc^p) - ln(mean_i xc^p) / p^2 ),  xc = max(x, eps)
    -> (out [n, C], dp scalar or None)."""
    b = seg_bidx(seg_off)
    inv = (1.0 / _cnt(seg_off).clamp_min(1))[b]
    n = int(seg_off[-1])
    c = (gmean if gmean is not None else ggem).shape[1]
    out = base.double().clone() if base is not None else torch.zeros((n, c), dtype=torch.float64, device=seg_off.device)
    dp = None
    if gmean is not None:
        out = out + gmean.double()[b] * inv
    if ggem is not None:
        p = float(p)
        xd = x.double()
        xc = xd.clamp(min=eps)
        live = _cnt(seg_off) > 0
        ysafe = torch.where(live, gem_y.double(), torch.ones_like(gem_y.double()))
        out = out + (ggem.double() * ysafe.pow(1 - p))[b] * xc.pow(p - 1) * (xd >= eps) * inv
        pa, pb = _gem_dp_parts(xd, seg_off, ggem, gem_y, p, eps)
        dp = (pa - pb).sum()
    return out, dp


def _chan_conv(v, w, flip=False):
    """zero-padded correlation over the channel axis: out[b][c] = sum_j w[j] v[b][c + j - k/2] (flip: c - (j - k/2))"""
    k = w.numel()
    vp = torch.nn.functional.pad(v, (k // 2, k // 2))
    c = v.shape[1]
    out = torch.zeros_like(v)
    for j in range(k):
        jj = k - 1 - j if flip else j
        out = out + w[j] * vp[:, jj:jj + c]
    return out


def eca64(mean, w):
    """ECALayer: sigmoid( sum_j w[j] mean[b][c + j - k/2] ), zero padding at both ends of the channel axis."""
    return torch.sigmoid(_chan_conv(mean.double(), w.double().view(-1)))


def eca_bwd64(mean, s, gs, seg_off, w):
    """ECALayer backward on the [B, C] vectors: g_pre = gs s (1 - s);
         add[b][c] = (1 / n_b) sum_j w[j] g_pre[b][c - (j - k/2)]   (0 for an empty segment)
         gw[j]     = sum_{b,c} g_pre[b][c] mean[b][c + j - k/2]
    -> (add [B, C], gw [k])."""
    mean, s, gs, w = mean.double(), s.double(), gs.double(), w.double().view(-1)
    k, c = w.numel(), mean.shape[1]
    gpre = gs * s * (1 - s)
    cnt = _cnt(seg_off)
    add = torch.where(cnt > 0, _chan_conv(gpre, w, flip=True) / cnt.clamp_min(1), torch.zeros_like(gpre))
    mp = torch.nn.functional.pad(mean, (k // 2, k // 2))
    gw = torch.stack([(gpre * mp[:, j:j + c]).sum() for j in range(k)])
    return add, gw


# --------------------------------------------------------------------------------------------------------------- the error
def granule_rel(got, ref, rows=128, cols=64):
    """The rms error of every (rows x cols) block of a [n, c] output divided by the rms of the WHOLE reference (a block of
    all-zero rows divides by nothing small) -> (the largest, "rows a..b columns c..d", the [blocks, c / cols] matrix)."""
    got, ref = got.double(), ref.double()
    n, c = ref.shape
    rms = float(ref.pow(2).mean().sqrt())
    rms = rms if rms > 0 else 1.0
    d2 = (got - ref).pow(2)
    nb, ncb = (n + rows - 1) // rows, (c + cols - 1) // cols
    pad = torch.zeros((nb * rows, ncb * cols), dtype=torch.float64, device=ref.device)
    pad[:n, :c] = d2
    s = pad.view(nb, rows, ncb, cols).sum((1, 3))
    cnt_r = torch.full((nb,), float(rows), dtype=torch.float64, device=ref.device)
    cnt_r[-1] = n - (nb - 1) * rows
    cnt_c = torch.full((ncb,), float(cols), dtype=torch.float64, device=ref.device)
    cnt_c[-1] = c - (ncb - 1) * cols
    rel = (s / (cnt_r[:, None] * cnt_c[None, :])).sqrt() / rms
    i = int(torch.nan_to_num(rel, nan=float("inf")).argmax())
    b, cb = divmod(i, ncb)
    where = "rows %d..%d columns %d..%d" % (b * rows, min(n, (b + 1) * rows) - 1, cb * cols, min(c, (cb + 1) * cols) - 1)
    return float(torch.nan_to_num(rel, nan=float("inf")).max()), where, rel
