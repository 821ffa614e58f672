"""Helpers of the conv tile-schedule tests (tests/test_conv_schedules_host.py, tests/test_gpu_conv_schedules.py): geometry-only
descriptors for the host-side plan query, deterministic problems, fp64 references, CPU emulations of the storage formats, and
the per-block error along the kernels' own raster."""
import torch
import torch.nn.functional as F

# the project's existing whole-map bars per MFMA precision (tests/test_gpu_kernels.py test_conv2d_matches_oracle)
BARS = {4: 6e-4, 2: 4e-4, 3: 2e-5}


def desc3x3(cin, cout, h, w, n, prec=4, pool=False, stat=False, hi_only=False):
    """A 3x3 / stride-1 / pad-1 agp_conv_desc on 1-pixel-halo maps for agp_conv2d_tile_plan: geometry, plus pointer fields set
    to 1 where the launch would look at them as NULL / non-NULL (the query dereferences nothing)."""
    from agplace_amd import _lib
    d = _lib.ConvDesc()
    d.in_hi = d.w_hi = d.out_hi = 1
    if prec == 3:
        d.in_lo = d.w_lo = d.out_lo = 1
    if prec == 2:
        d.w_lo = 1
    d.n, d.hin, d.win, d.pin = n, h, w, 1
    d.cin = d.in_w_step = cin
    d.hout, d.wout, d.cout, d.pout = h, w, cout, 1
    d.kh = d.kw = 3
    d.stride = d.pad = 1
    d.prec = prec
    d.pool_partial = 1 if pool else None
    d.stat_partial = 1 if stat else None
    d.hi_only = 1 if hi_only else 0
    return d


def plan3x3(*a, **k):
    from agplace_amd import ops
    return ops.tile_plan(desc3x3(*a, **k))


def plan_group(shapes, cin, cout, prec=4):
    """Plan of agp_conv2d_fwd_grouped over [(n, h, w), ...] of one channel shape."""
    from agplace_amd import _lib, ops
    arr = (_lib.ConvDesc * len(shapes))(*[desc3x3(cin, cout, h, w, n, prec) for (n, h, w) in shapes])
    return ops.tile_plan(arr)


def regime(p):
    """The schedule a plan describes: every row tile as half tiles, 256-row tiles only, or both."""
    if p["half_tiles"] == 0:
        return "full-only"
    return "all-half" if p["MT_full"] == 0 else "mixed"


def raster_rows(n, h, w):
    """GEMM rows of the 3x3 stride-1 kernels' padded-width raster (img, y, x' in [0, w + 2))."""
    return n * h * (w + 2)


# ---------------------------------------------------------------------------------------------------------------- problems
def images(c, h, w, n, seed, first=0):
    """Images [first, first + n) of a stream in which image i depends on (seed, c, h, w, i) only: a batch cut differently holds the
    same images."""
    out = torch.empty(n, c, h, w)
    for i in range(n):
        out[i] = torch.randn(c, h, w, generator=torch.Generator().manual_seed((seed * 1000003 + first + i) * 7 + c))
    return out


def weights(cin, cout, seed=0):
    g = torch.Generator().manual_seed(seed * 131 + cin + 3 * cout)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    scale = 0.5 + torch.rand(cout, generator=g)
    shift = 0.3 * torch.randn(cout, generator=g)
    return wt, scale, shift


def ref64(x, wt, scale, shift, res, relu):
    y = F.conv2d(x.double(), wt.double(), None, 1, 1)
    if scale is not None:
        y = y * scale.double().view(1, -1, 1, 1)
    if shift is not None:
        y = y + shift.double().view(1, -1, 1, 1)
    if res is not None:
        y = y + res.double()
    return torch.relu(y) if relu else y


def _f16(t):
    return t.float().half().double()


def _bf16_pair(t):
    t = t.float()
    hi = t.bfloat16()
    return hi.double() + (t - hi.float()).bfloat16().double()


def emulate(prec, x, wt, scale, shift, res, relu, hi_only=False):
    """What the kernels compute, with their STORAGE roundings and exact arithmetic in between: operands and the residual rounded to
    the mode's formats (4: fp16 x, w; 2: fp16 x, fp16-pair w; 3: bf16 pairs; hi_only: the bf16 hi planes, as that mode defines),
    an fp64 conv, the result rounded to the stored format."""
    if prec == 4:
        xe, we, re, rnd = _f16(x), _f16(wt), None if res is None else _f16(res), _f16
    elif prec == 2:
        w32 = wt.float()
        wh = w32.half()
        xe, we, re, rnd = _f16(x), wh.double() + (w32 - wh.float()).half().double(), None if res is None else _f16(res), _f16
    else:
        xe, we = (x.float().bfloat16().double(), wt.float().bfloat16().double()) if hi_only else (_bf16_pair(x), _bf16_pair(wt))
        re, rnd = None if res is None else _bf16_pair(res), _bf16_pair
    return rnd(ref64(xe, we, scale, shift, re, relu))


# ------------------------------------------------------------------------------------------------------------- block errors
def block_rel_l2(got, ref, rows=64, cols=128):
    """rel_l2 of every (rows x cols) block of the kernels' raster: got / ref [n, c, h, w] -> [blocks, c / cols] over each block's
    interior pixels (the raster's two halo columns per row hold nothing); nan for a block without an interior pixel."""
    n, c, h, w = ref.shape
    d = (got.double() - ref.double()).permute(0, 2, 3, 1).reshape(n, h, w, c // cols, cols)
    r = ref.double().permute(0, 2, 3, 1).reshape(n, h, w, c // cols, cols)

    def per_block(t):
        e = F.pad((t * t).sum(-1), (0, 0, 1, 1))                  # [n, h, w + 2, ct]: the raster's rows
        e = e.reshape(n * h * (w + 2), c // cols)
        e = F.pad(e, (0, 0, 0, (-e.shape[0]) % rows))
        return e.reshape(-1, rows, c // cols).sum(1)
    num, den = per_block(d), per_block(r)
    return torch.where(den > 0, (num / den.clamp_min(1e-300)).sqrt(), torch.full_like(den, float("nan")))


def worst_block(got, ref, bm=256, rows=64, cols=128, mt_end=None):
    """(largest block rel_l2, "problem P row tile T half H block B column tile C") of a launch's output; mt_end: the row tiles
    before this problem in a grouped launch (named only)."""
    rel = torch.nan_to_num(block_rel_l2(got, ref, rows, cols), nan=0.0)
    i = int(rel.argmax())
    b, ct = divmod(i, rel.shape[1])
    row = b * rows
    where = "problem %s row tile %d half %d block %d (raster rows %d..%d) column tile %d" % (
        "-" if mt_end is None else mt_end, row // bm, (row % bm) // (bm // 2), b, row, row + rows - 1, ct)
    return float(rel.max()), where


# ------------------------------------------------------------------------------------------------------------- guarded maps
GUARD = 4096                    # elements before and after the plane
GUARD_BITS, FILL_BITS = 0x7EAD, 0x7EEF      # fp16 NaNs / bf16 values near 1e38: nothing a conv of these problems stores


def guarded_map(n, h, w, c, prec, dev):
    """A SplitMap whose planes lie in the middle of larger buffers: guard regions and interior pre-filled with two patterns, the
    halo zero as SplitMap.alloc leaves it.  Returns (map, [whole buffers])."""
    from agplace_amd import ops
    numel = n * (h + 2) * (w + 2) * c
    planes, bufs = [], []
    for _ in range(2 if prec == 3 else 1):
        buf = torch.full((GUARD + numel + GUARD,), GUARD_BITS, dtype=torch.int16, device=dev)
        m = buf[GUARD:GUARD + numel].view(n, h + 2, w + 2, c)
        m.fill_(FILL_BITS)
        m[:, 0] = 0
        m[:, -1] = 0
        m[:, :, 0] = 0
        m[:, :, -1] = 0
        planes.append(m.view(torch.bfloat16 if prec == 3 else torch.float16))
        bufs.append(buf)
    return ops.SplitMap(planes[0], planes[1] if prec == 3 else None, n, h, w, c, 1), bufs


def assert_only_the_interior_was_written(m, bufs):
    for plane, buf in zip([m.hi] + ([m.lo] if m.lo is not None else []), bufs):
        bits = plane.view(torch.int16)
        assert bool((buf[:GUARD] == GUARD_BITS).all()) and bool((buf[-GUARD:] == GUARD_BITS).all()), "guard region written"
        assert not bool(bits[:, 0].any()) and not bool(bits[:, -1].any()), "halo rows written"
        assert not bool(bits[:, :, 0].any()) and not bool(bits[:, :, -1].any()), "halo columns written"
        miss = bits[:, 1:-1, 1:-1] == FILL_BITS
        left = int(miss.sum())
        if left:
            img, y, x, ch = (int(v) for v in miss.nonzero()[0])
            row = (img * m.h + y) * (m.w + 2) + x + 1
            raise AssertionError("%d interior elements were not written; the first: image %d y %d x %d channel %d = raster row %d "
                                 "(row tile %d of 256 rows, half %d, column tile %d)" % (left, img, y, x, ch, row, row // 256,
                                                                                        row % 256 // 128, ch // 128))


# ------------------------------------------------------------------------------------------------------------------ shapes
# name -> ((cin, cout, h, w, n), the regime the plan query must report).  Picked with the query; both test files assert the
# regime through it, so a heuristic that moves fails here instead of silently losing the coverage.
WIDE_CASES = {
    "all_half_control": ((128, 128, 28, 170, 5), "all-half"),
    "mixed_stage2": ((128, 128, 28, 170, 32), "mixed"),                      # the bench's stage-2 shape: 512 + 90 row tiles
    "mixed_nt2": ((256, 256, 14, 86, 64), "mixed"),
    "mixed_last_tile_has_one_half": ((128, 128, 28, 170, 31), "mixed"),      # M % 256 = 48: the second half tile returns early
    "mixed_last_half_tile_partial": ((128, 128, 28, 170, 29), "mixed"),      # M % 256 = 144: rows past M in the second half tile
    "full_only": ((128, 128, 28, 170, 16), "full-only"),
    "full_only_nt2": ((256, 256, 14, 86, 34), "full-only"),
    "full_only_last_tile_partial": ((128, 128, 28, 170, 15), "full-only"),   # M % 256 = 48, MT = 283: ragged last XCD chunk
    "full_only_nt3": ((128, 384, 14, 30, 40), "full-only"),
    "nt3_refuses_to_mix": ((128, 384, 14, 30, 100), "full-only"),            # T = 525 > 512, tail = 13, 13 % 3 != 0
}
# the other kernels of the family: name -> ((cin, cout, h, w, n), prec, flags, (kernel, BM, BN))
FAMILY_CASES = {
    "kxr2_cout64": ((64, 64, 56, 338, 12), 4, {}, ("kxr2", 256, 64)),
    "kxr_mode2_128": ((128, 128, 28, 60, 16), 2, {}, ("kxr", 256, 64)),
    "kxr_mode2_256": ((128, 256, 28, 60, 16), 2, {}, ("kxr", 256, 64)),
    "kxr_mode3_128": ((128, 128, 28, 60, 16), 3, {}, ("kxr", 128, 128)),
    "kxr_mode3_256": ((128, 256, 28, 60, 16), 3, {}, ("kxr", 128, 128)),         # the <128, 128, 2, 2, 3, 3> instantiation
    "kxr_hi_only_128": ((128, 128, 28, 60, 16), 3, {"hi_only": True}, ("kxr", 256, 128)),
    "kxr_hi_only_256": ((128, 256, 28, 60, 16), 3, {"hi_only": True}, ("kxr", 256, 128)),
    "kxr_mode3_stat_128": ((128, 128, 28, 60, 16), 3, {"stat": True}, ("kxr", 128, 128)),
    "kxr_mode3_stat_256": ((128, 256, 28, 60, 16), 3, {"stat": True}, ("kxr", 128, 128)),
}

# [(n, h, w), ...] of 128 -> 128 problems; where the problem boundaries (mt_end) fall is asserted from the plans below
GROUPS = {
    "boundary_inside_the_full_region": [(16, 28, 170), (15, 28, 170), (1, 28, 170)],
    "boundary_exactly_at_MT_full": [(32, 32, 126), (5, 28, 170)],
    "small_last_problem_inside_the_half_region": [(31, 28, 170), (2, 9, 9), (1, 14, 30)],
}
