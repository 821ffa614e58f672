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


def desc_conv(cin, cout, h, w, n, k=3, stride=1, prec=4, stat=False, res=False, relu=False, stem=False):
    """desc3x3's general sibling: a k x k conv (k 1 or 3, pad k // 2, stride 1 or 2) on 1-pixel-halo maps, or (stem) the packed
    7x7 / stride-2 / pad-3 stem on a 4-channel image with a 3-pixel halo, as ops.ConvWeights(stem=True) describes it."""
    d = desc3x3(cin, cout, h, w, n, prec=prec, stat=stat)
    if stem:
        k, stride, pad = 7, 2, 3
        d.cin, d.in_w_step, d.pin = 32, 4, 3
        d.kh, d.kw = 7, 1
    else:
        pad = k // 2
        d.kh = d.kw = k
    d.stride, d.pad = stride, pad
    d.hout, d.wout = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    d.res_hi = 1 if res else None
    if res and prec == 3:
        d.res_lo = 1
    d.relu = 1 if relu else 0
    return d


def plan_conv(*a, **k):
    from agplace_amd import ops
    return ops.tile_plan(desc_conv(*a, **k))


def descs_s2(shapes, cin, cout):
    """[3x3/s2 conv of every trunk ..., its 1x1/s2 downsample of every trunk ...] over [(n, h, w), ...]: the stage entry as
    resnet.forward_maps_multi issues it (a trunk's two convs read the same input: equal in_hi)."""
    from agplace_amd import _lib
    ds = [desc_conv(cin, cout, h, w, n, k=3, stride=2, relu=True) for (n, h, w) in shapes] + \
         [desc_conv(cin, cout, h, w, n, k=1, stride=2) for (n, h, w) in shapes]
    return (_lib.ConvDesc * len(ds))(*ds)


def plan_s2(shapes, cin, cout):
    from agplace_amd import ops
    return ops.tile_plan(descs_s2(shapes, cin, cout))


def smallest_batch(plan_of, rows_of, most=4096):
    """The smallest batch n whose plan has MT >= 100, MT % 8 != 0 (a ragged last XCD chunk) and rows_of(n) % BM != 0 (a partial
    last tile)."""
    for n in range(1, most):
        p = plan_of(n)
        if p["MT"] >= 100 and p["MT"] % 8 != 0 and rows_of(n) % p["BM"] != 0:
            return n
    raise AssertionError("no batch below %d qualifies" % most)


def out_size(h, w, k, stride):
    return (h + 2 * (k // 2) - k) // stride + 1, (w + 2 * (k // 2) - k) // stride + 1


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


def weights(cin, cout, seed=0, k=3):
    g = torch.Generator().manual_seed(seed * 131 + cin + 3 * cout)
    wt = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    scale = 0.5 + torch.rand(cout, generator=g)
    shift = 0.3 * torch.randn(cout, generator=g)
    return wt, scale, shift


def ref64(x, wt, scale, shift, res, relu, k=3, stride=1, pad=1):
    assert tuple(wt.shape[-2:]) == (k, k)
    y = F.conv2d(x.double(), wt.double(), None, stride, pad)
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


def ref64_by_image(x, wt, scale, shift, res, relu, k=3, stride=1, pad=1, chunk=4):
    """ref64 in chunks of a few images: the fp64 copies of a large batch never exist at once."""
    return torch.cat([ref64(x[a:a + chunk], wt, scale, shift, None if res is None else res[a:a + chunk], relu, k, stride, pad)
                      for a in range(0, x.shape[0], chunk)])


def emulate(prec, x, wt, scale, shift, res, relu, hi_only=False, k=3, stride=1, pad=1):
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
    return rnd(ref64(xe, we, scale, shift, re, relu, k, stride, pad))


# ------------------------------------------------------------------------------------------------------------- block errors
def block_rel_l2(got, ref, rows=64, cols=128, raster="padded"):
    """rel_l2 of every (rows x cols) block of the kernels' raster: got / ref [n, c, h, w] -> [blocks, c / cols] over each block's
    interior pixels; nan for a block without an interior pixel.  raster "padded": the padded-width raster (img, y, x' in
    [0, w + 2)) of the OUTPUT map, whose two halo columns per row hold nothing (the 3x3 stride-1 family; igemm_s2); "plain": the
    [n][h][w] raster of the output (the generic kernel, igemm_d16)."""
    assert raster in ("padded", "plain")
    halo = 1 if raster == "padded" else 0
    n, c, h, w = ref.shape
    d = (got.double() - ref.double()).permute(0, 2, 3, 1).reshape(n, h, w, c // cols, cols)
    r = ref.double().permute(0, 2, 3, 1).reshape(n, h, w, c // cols, cols)

    def per_block(t):
        e = F.pad((t * t).sum(-1), (0, 0, halo, halo))            # [n, h, w + 2 * halo, ct]: the raster's rows
        e = e.reshape(n * h * (w + 2 * halo), c // cols)
        e = F.pad(e, (0, 0, 0, (-e.shape[0]) % rows))
        return e.reshape(-1, rows, c // cols).sum(1)
    num, den = per_block(d), per_block(r)
    return torch.where(den > 0, (num / den.clamp_min(1e-300)).sqrt(), torch.full_like(den, float("nan")))


def worst_block(got, ref, bm=256, rows=64, cols=128, mt_end=None, raster="padded"):
    """(largest block rel_l2, "problem P row tile T half H block B column tile C") of a launch's output; bm: the rows of the
    kernel's tile, raster: its raster (block_rel_l2); mt_end: the row tiles before this problem in a grouped launch (named
    only)."""
    rel = torch.nan_to_num(block_rel_l2(got, ref, rows, cols, raster), nan=0.0)
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

# ------------------------------------------------------------------------------ the stage-entry, generic and stem kernels
# (tests/test_gpu_conv_entry_schedules.py).  Every batch below is smallest_batch() of its plan: MT >= 100 (several grid rounds of
# the XCD-chunked map), MT % 8 != 0 (ragged last chunk), rows % BM != 0 (partial last tile); the host tests assert that.
# igemm_s2 (AGP_PREC_F16): name -> ((cin, cout, h, w, n), (BN, NT)); BN 128 = the TN 4 instantiation, 64 = TN 2
S2_CASES = {
    "tn4_nt1_bench_stage2": ((64, 128, 56, 336, 4), (128, 1)),          # the bench's stage-2 geometry: 56 x 336 -> 28 x 168
    "tn4_nt2_odd": ((128, 256, 29, 85, 19), (128, 2)),
    "tn4_nt4_odd": ((256, 512, 15, 43, 67), (128, 4)),
    "tn2_nt1_odd": ((64, 64, 57, 85, 10), (64, 1)),
    "tn2_nt3_odd": ((64, 192, 57, 85, 10), (64, 3)),
}
# query + db trunk of 64 -> 128 in one launch: [(n, h, w), ...]; where mt_end[0] falls is asserted from the plans
S2_GROUPS = {
    "boundary_inside_a_chunk": [(2, 56, 336), (5, 56, 56)],             # mt_end[0] = 75 of 108, chunks of 14
    "boundary_on_a_chunk_boundary": [(3, 56, 336), (2, 56, 56)],        # mt_end[0] = 112 of 126, chunks of 16
}
# the generic LDS-staged kernel: name -> ((cin, cout, k, stride, h, w, n), prec, flags, (BM, BN))
GENERIC_CASES = {
    "m4_1x1_64_256": ((64, 256, 1, 1, 29, 43, 11), 4, {}, (128, 128)),
    "m4_1x1_256_64_res_relu": ((256, 64, 1, 1, 29, 43, 21), 4, {"res": True}, (256, 64)),
    "m2_3x3s2_128_256": ((128, 256, 3, 2, 57, 85, 11), 2, {"res": True}, (128, 128)),
    "m2_1x1s2_64_128": ((64, 128, 1, 2, 57, 85, 11), 2, {}, (128, 128)),
    "m2_1x1_256_64_res_relu": ((256, 64, 1, 1, 29, 43, 21), 2, {"res": True}, (256, 64)),
    "m3_3x3s2_64_128_stat": ((64, 128, 3, 2, 57, 85, 11), 3, {"stat": True}, (128, 128)),      # the training stage entry
    "m3_1x1s2_64_128_stat": ((64, 128, 1, 2, 57, 85, 11), 3, {"stat": True}, (128, 128)),
    "m3_1x1_256_64_stat": ((256, 64, 1, 1, 29, 43, 21), 3, {"stat": True}, (256, 64)),
    "m3_1x1_256_64_res_relu": ((256, 64, 1, 1, 29, 43, 21), 3, {"res": True}, (256, 64)),
}
# launch_group_f16: two trunks' 1x1 pairs (64 -> 128 with ReLU and 64 -> 256 on the same input): [(n, h, w), ...] of the trunks
GENERIC_GROUP = [(11, 29, 43), (9, 28, 30)]
# igemm_d16: the packed 7x7 / stride-2 stem (3 -> 64) in mode 3 with stat_partial: (h, w, n)
STEM_CASE = (97, 271, 4)
