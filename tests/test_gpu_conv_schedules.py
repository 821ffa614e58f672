"""-m gpu: the 3x3 stride-1 conv kernels against fp64 in EVERY tile-schedule regime of their launchers -- igemm_kxrw's all-half,
full-only and mixed grids (and the cout = 384 launch that refuses to mix), partial last tiles in the XCD-chunked and in the
half-tile region, grouped launches with problem boundaries in each region, conv-epilogue pooling and the range-guard twin outside
the all-half regime, and one multi-round shape for each other kernel of the family (igemm_kxr2, igemm_kxr modes 2 / 3 / hi_only /
stat_partial).  Every test asserts through agp_conv2d_tile_plan (the launch path itself) that it ran in the regime it names.

Bars: the project's existing ones (conv_sched_util.BARS: mode 4 6e-4, mode 2 4e-4, mode 3 2e-5), applied to the whole map AND to the
worst 64-row x 128-column block of the kernels' raster.  tests/test_conv_schedules_host.py shows that the storage roundings alone
stay under them per block."""
import pytest
import torch

from conv_sched_util import BARS, FAMILY_CASES, GROUPS, WIDE_CASES, assert_only_the_interior_was_written, emulate, guarded_map, images, \
    raster_rows, ref64, regime, weights, worst_block
from gpu_util import rel_l2, rel_max

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


_PROBLEMS = {}


def _problem(cin, cout, h, w, n):
    """(x, res, wt, scale, shift, fp64 reference with residual + ReLU) of the first n images of a channel / map shape's stream;
    the reference is computed once per shape, for the largest batch WIDE_CASES asks of it."""
    key = (cin, cout, h, w)
    if key not in _PROBLEMS:
        nmax = max(c[4] for c, _ in WIDE_CASES.values() if c[:4] == key)
        x, res = images(cin, h, w, nmax, 1), images(cout, h, w, nmax, 2)
        wt, scale, shift = weights(cin, cout)
        _PROBLEMS[key] = (x, res, wt, scale, shift, ref64(x, wt, scale, shift, res, True))
    x, res, wt, scale, shift, ref = _PROBLEMS[key]
    return x[:n], res[:n], wt, scale, shift, ref[:n]


def _pack(t, prec, dev):
    from agplace_amd import ops
    return ops.pack_f32(t.to(dev), t.shape[1], 1, prec)


def _check_parity(out, ref, prec, bm, what, tol=None):
    """Checks 1 and 2: whole-map rel_l2 and the worst raster block under the same bar; the message names the block."""
    tol = BARS[prec] if tol is None else tol
    got = out.to_f32().cpu()
    whole = rel_l2(got, ref)
    worst, where = worst_block(got, ref, bm=bm, cols=min(128, ref.shape[1]))      # (cout = 64: the whole width)
    print("%s: whole map %.3g worst block %.3g (bar %.3g) at %s" % (what, whole, worst, tol, where))
    assert whole < tol, (what, whole)
    assert worst < tol, (what, worst, where)
    return got


def _chunk_size(plan_of, n, want):
    """The largest batch <= n / 2 whose launch the query reports in regime `want`."""
    for k in range(n // 2, 0, -1):
        if regime(plan_of(k)) == want:
            return k
    raise AssertionError("no batch of <= %d images runs %s" % (n // 2, want))


def _run_in_chunks(xm, cw, rm, out, k, relu, plan_want):
    """The same images as launches of k images each (the last one overlaps: it recomputes images it shares)."""
    from agplace_amd import ops
    n = xm.n
    for a in list(range(0, n - k, k)) + [n - k]:
        job = (ops.slice_map(xm, a, a + k), cw, ops.slice_map(out, a, a + k), None if rm is None else ops.slice_map(rm, a, a + k), relu)
        assert regime(ops.conv_tile_plan([job], 4)) == plan_want
        ops.conv2d(job[0], cw, job[2], residual=job[3], relu=relu, prec=4)


@pytest.mark.parametrize("name", list(WIDE_CASES))
def test_wide_f16_conv_in_every_tile_schedule(dev, name):
    """igemm_kxrw (AGP_PREC_F16, cout % 128 == 0), residual + scale / shift + ReLU: fp64 parity over EVERY image, whole map and
    worst 64 x 128 block; nothing but the interior written (guard regions, halo, rows past M of a partial last tile); and the
    stored bits do not depend on the schedule -- the same images as all-half launches and as full-only launches give torch.equal
    maps (each output element is one lane's accumulator over the same K sequence in 256-row and 128-row tiles).
    Worst block (bar 6e-4): CPU emulation of mode 4's storage roundings 3.40e-4; kernel, measured on an MI355X, 3.33e-4 .. 3.65e-4
    over these shapes (whole map 3.21e-4 .. 3.48e-4).  Every run prints its figures."""
    from agplace_amd import ops
    (cin, cout, h, w, n), want = WIDE_CASES[name]
    x, res, wt, scale, shift, ref = _problem(cin, cout, h, w, n)
    xm, rm = _pack(x, 4, dev), _pack(res, 4, dev)
    cw = ops.ConvWeights(wt.to(dev), scale.to(dev), shift.to(dev), 1, 1)
    out, bufs = guarded_map(n, h, w, cout, 4, dev)
    p = ops.conv_tile_plan([(xm, cw, out, rm, True)], 4)
    assert p["kernel"] == "kxrw" and regime(p) == want, p
    ops.conv2d(xm, cw, out, residual=rm, relu=True, prec=4)
    torch.cuda.synchronize()
    assert_only_the_interior_was_written(out, bufs)
    _check_parity(out, ref, 4, p["BM"], name)
    # schedule independence, bit for bit (5 images cannot form a full-only launch: mixed_stage2 holds the control's images, same
    # weights, and is compared with both)
    for other in ("all-half", "full-only"):
        if other == want or (name == "all_half_control" and other == "full-only"):
            continue
        k = _chunk_size(lambda k: ops.conv_tile_plan([(ops.slice_map(xm, 0, k), cw, ops.slice_map(out, 0, k), None, True)], 4), n, other)
        o2 = ops.SplitMap.alloc(n, h, w, cout, 1, 4, dev)
        _run_in_chunks(xm, cw, rm, o2, k, True, other)
        assert torch.equal(o2.hi, out.hi), (name, "differs from the same images run as %s launches of %d" % (other, k))


def _group_problem(dev, cin, cout, n, h, w, seed, use_res, relu):
    from agplace_amd import ops
    x = images(cin, h, w, n, seed)
    res = images(cout, h, w, n, seed + 50) if use_res else None
    wt, scale, shift = weights(cin, cout, seed)
    cw = ops.ConvWeights(wt.to(dev), scale.to(dev), shift.to(dev), 1, 1)
    return dict(x=x, res=res, wt=wt, scale=scale, shift=shift, relu=relu, cw=cw, xm=_pack(x, 4, dev),
                rm=None if res is None else _pack(res, 4, dev), shape=(n, h, w))


@pytest.mark.parametrize("name", list(GROUPS))
def test_grouped_launch_with_problem_boundaries_in_each_region(dev, name):
    """ops.conv2d_grouped on igemm_kxrw's mixed grid: the block -> (problem, row tile) lookup through mt_end[] in the XCD-chunked
    part, at its end, and in the half-tile part (a small last problem that lies wholly in it, with partial last tiles).  Each
    output bit-identical to its separate launch, and under the whole-map and per-block bars against fp64."""
    from agplace_amd import ops
    from conv_sched_util import plan3x3
    shapes = GROUPS[name]
    probs = [_group_problem(dev, 128, 128, n, h, w, 3 + i, use_res=(i != 1), relu=(i != len(shapes) - 1))
             for i, (n, h, w) in enumerate(shapes)]
    outs = [guarded_map(n, h, w, 128, 4, dev) for (n, h, w) in shapes]
    jobs = [(q["xm"], q["cw"], o[0], q["rm"], q["relu"]) for q, o in zip(probs, outs)]
    p = ops.conv_tile_plan(jobs, 4)
    assert p["kernel"] == "kxrw" and regime(p) == "mixed", p
    ends, mt = [], 0
    for (n, h, w) in shapes:                       # row tiles per problem, from the query of each problem alone
        mt += plan3x3(128, 128, h, w, n)["MT"]
        ends.append(mt)
    assert ends[-1] == p["MT"]
    if name == "boundary_inside_the_full_region":
        assert 0 < ends[0] < p["MT_full"] and ends[0] % 8 != 0
    elif name == "boundary_exactly_at_MT_full":
        assert ends[0] == p["MT_full"]
    else:
        assert p["MT_full"] < ends[0] < ends[1] < p["MT"]
    ops.conv2d_grouped(jobs, 4)
    torch.cuda.synchronize()
    for i, (q, (o, bufs)) in enumerate(zip(probs, outs)):
        assert_only_the_interior_was_written(o, bufs)
        n, h, w = q["shape"]
        sep = ops.SplitMap.alloc(n, h, w, 128, 1, 4, dev)
        ops.conv2d(q["xm"], q["cw"], sep, residual=q["rm"], relu=q["relu"], prec=4)
        assert torch.equal(o.hi, sep.hi), (name, i)
        _check_parity(o, ref64(q["x"], q["wt"], q["scale"], q["shift"], q["res"], q["relu"]), 4, 256, "%s problem %d" % (name, i))


@pytest.mark.parametrize("name", ["mixed_stage2", "full_only"])
def test_conv_epilogue_pooling_outside_the_all_half_regime(dev, name):
    """PoolReq (mean + GeM, p = 3 and p = 2.5) and SqStatReq on a mixed and a full-only launch: the stored map bit-identical to the
    conv without the request; the pooled values against fp64 on the stored map (1e-6) and against ops.pool_map; bit-identical under
    an image permutation and when the batch is cut so that every launch is all-half (in a half tile the odd wave hands its sums
    to the even wave of its pair; in a full tile a wave is a block).
    This test found the GeM sums of a 64-row block added in a different order by the two tile shapes (a full tile's wave: one chain
    over 64 rows; a half tile: rows 0..31 + rows 32..63), so an image's GeM vector moved in its last bits with its position in a
    mixed launch; igemm_kxrw now sums (rows 0..31) + (rows 32..63) in both."""
    from agplace_amd import ops
    (cin, cout, h, w, n), want = WIDE_CASES[name]
    x, res, wt, scale, shift, _ = _problem(cin, cout, h, w, n)
    xm, rm = _pack(x, 4, dev), _pack(res, 4, dev)
    cw = ops.ConvWeights(wt.to(dev), scale.to(dev), shift.to(dev), 1, 1)
    o0 = ops.SplitMap.alloc(n, h, w, cout, 1, 4, dev)
    ops.conv2d(xm, cw, o0, residual=rm, relu=True, prec=4)
    dense = o0.to_f32().double()
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1))
    xp, rp = _pack(x[perm], 4, dev), _pack(res[perm], 4, dev)
    permd = perm.to(dev)
    k = None
    for pw in (3.0, 2.5):
        pt = torch.tensor([pw], device=dev)
        req = ops.PoolReq(pt, want_mean=True, want_gem=True)
        o1, bufs = guarded_map(n, h, w, cout, 4, dev)
        p = ops.conv_tile_plan([(xm, cw, o1, rm, True, req)], 4)
        assert p["kernel"] == "kxrw" and regime(p) == want and p["MT"] == (n * ((h * (w + 2) + 63) // 64 * 64) + 255) // 256, p
        ops.conv2d(xm, cw, o1, residual=rm, relu=True, prec=4, pool=req)
        assert req.fused and torch.equal(o1.hi, o0.hi)
        assert_only_the_interior_was_written(o1, bufs)
        assert rel_l2(req.mean, dense.mean((2, 3))) < 1e-6
        assert rel_l2(req.gem, dense.clamp(min=1e-6).pow(pw).mean((2, 3)).pow(1 / pw)) < 1e-6
        mean_ref, gem_ref = ops.pool_map(o0, pt)
        assert rel_max(req.mean, mean_ref) < 1e-5 and rel_max(req.gem, gem_ref) < 1e-5
        # image permutation
        reqp = ops.PoolReq(pt, want_mean=True, want_gem=True)
        ops.conv2d(xp, cw, ops.SplitMap.alloc(n, h, w, cout, 1, 4, dev), residual=rp, relu=True, prec=4, pool=reqp)
        assert torch.equal(reqp.mean, req.mean[permd]) and torch.equal(reqp.gem, req.gem[permd])
        # the batch cut into all-half launches
        if k is None:
            k = _chunk_size(lambda k: ops.conv_tile_plan([(ops.slice_map(xm, 0, k), cw, ops.slice_map(o0, 0, k), None, True,
                                                           ops.PoolReq(pt, want_mean=True, want_gem=True))], 4), n, "all-half")
        for a in list(range(0, n - k, k)) + [n - k]:
            reqc = ops.PoolReq(pt, want_mean=True, want_gem=True)
            oc = ops.SplitMap.alloc(k, h, w, cout, 1, 4, dev)
            job = (ops.slice_map(xm, a, a + k), cw, oc, ops.slice_map(rm, a, a + k), True, reqc)
            assert regime(ops.conv_tile_plan([job], 4)) == "all-half"
            ops.conv2d(job[0], cw, oc, residual=job[3], relu=True, prec=4, pool=reqc)
            assert reqc.fused and torch.equal(oc.hi, o0.hi[a:a + k])
            assert torch.equal(reqc.mean, req.mean[a:a + k]) and torch.equal(reqc.gem, req.gem[a:a + k]), (pw, a)
    # sum and sum of squares (the BatchNorm statistics' first stage): [64-row block][2][cout], image-aligned blocks
    sq = ops.SqStatReq()
    o2 = ops.SplitMap.alloc(n, h, w, cout, 1, 4, dev)
    assert regime(ops.conv_tile_plan([(xm, cw, o2, rm, True, sq)], 4)) == want
    ops.conv2d(xm, cw, o2, residual=rm, relu=True, prec=4, pool=sq)
    assert sq.fused and torch.equal(o2.hi, o0.hi)
    part = sq.partial.view(-1, 2, cout)[:sq.blocks]
    assert rel_l2(part[:, 0].double().sum(0), dense.sum((0, 2, 3))) < 1e-6
    assert rel_l2(part[:, 1].double().sum(0), (dense * dense).sum((0, 2, 3))) < 1e-6
    bpi = sq.blocks // n                           # blocks per image
    per_image = part.view(n, bpi, 2, cout).double().sum(1)
    assert rel_l2(per_image[:, 0], dense.sum((2, 3))) < 1e-6 and rel_l2(per_image[:, 1], (dense * dense).sum((2, 3))) < 1e-6
    for a in list(range(0, n - k, k)) + [n - k]:
        sqc = ops.SqStatReq()
        oc = ops.SplitMap.alloc(k, h, w, cout, 1, 4, dev)
        job = (ops.slice_map(xm, a, a + k), cw, oc, ops.slice_map(rm, a, a + k), True, sqc)
        assert regime(ops.conv_tile_plan([job], 4)) == "all-half"
        ops.conv2d(job[0], cw, oc, residual=job[3], relu=True, prec=4, pool=sqc)
        assert sqc.fused and torch.equal(sqc.partial.view(-1, 2, cout)[:sqc.blocks], part[a * bpi:(a + k) * bpi]), a


def _guarded(dev, fn):
    """fn() with a fresh range-guard word bound on this thread -> the word after the work (tests/test_gpu_range_guard.py)."""
    from agplace_amd import _lib
    lib = _lib.load()
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    prev = lib.agp_range_flag_set(word.data_ptr())
    try:
        fn()
    finally:
        lib.agp_range_flag_set(prev)
    torch.cuda.synchronize()
    return int(word.item())


@pytest.mark.parametrize("name", ["mixed_stage2", "full_only"])
def test_range_guard_twin_outside_the_all_half_regime(dev, name):
    """With a guard word bound the mixed and full-only launches (the RG = true instantiations) store the same bits and leave the
    word 0 on in-range data; one out-of-range value planted in a row that a FULL tile owns, and (mixed) in one that a HALF tile
    owns, sets the word and is stored as +-65504."""
    from agplace_amd import ops
    (cin, cout, h, w, n), want = WIDE_CASES[name]
    x, res, wt, scale, _, _ = _problem(cin, cout, h, w, n)
    ch = 77
    shift = torch.zeros(cout)
    xm = _pack(x, 4, dev)
    o0 = ops.SplitMap.alloc(n, h, w, cout, 1, 4, dev)
    rm = _pack(res, 4, dev)
    cw = ops.ConvWeights(wt.to(dev), scale.to(dev), shift.to(dev), 1, 1)
    p = ops.conv_tile_plan([(xm, cw, o0, rm, True)], 4)
    assert p["kernel"] == "kxrw" and regime(p) == want, p
    ops.conv2d(xm, cw, o0, residual=rm, relu=True, prec=4)
    o1 = ops.SplitMap.alloc(n, h, w, cout, 1, 4, dev)
    assert _guarded(dev, lambda: ops.conv2d(xm, cw, o1, residual=rm, relu=True, prec=4)) == 0
    assert torch.equal(o1.hi, o0.hi)
    # raster row -> (image, y, x): a row in the first full tile region, and one in the last row tile (a half tile when mixed)
    wp = w + 2
    rows = [(p["MT_full"] // 2) * 256 + 100]
    if want == "mixed":
        assert p["MT"] - p["MT_full"] >= 2
        rows.append((p["MT"] - 2) * 256 + 128 + 17)          # the second half tile of a row tile past MT_full
    for row, sign, relu in zip(rows, (1.0, -1.0), (True, False)):
        img, rem = divmod(row, h * wp)
        y, xq = divmod(rem, wp)
        xq = min(max(xq, 1), w)                               # an interior column of that raster row
        assert (row >= p["MT_full"] * 256) == (sign < 0)
        r2 = res.clone()
        r2[img, ch, y, xq - 1] = sign * 65000.0
        r2m = _pack(r2, 4, dev)
        cw2 = ops.ConvWeights(wt.to(dev), scale.to(dev), (shift + sign * 2000.0 * torch.nn.functional.one_hot(torch.tensor(ch), cout)).to(dev), 1, 1)
        plain = ops.SplitMap.alloc(n, h, w, cout, 1, 4, dev)
        ops.conv2d(xm, cw2, plain, residual=r2m, relu=relu, prec=4)
        o2 = ops.SplitMap.alloc(n, h, w, cout, 1, 4, dev)
        assert _guarded(dev, lambda: ops.conv2d(xm, cw2, o2, residual=r2m, relu=relu, prec=4)) == 1, (name, row)
        assert torch.equal(o2.hi, plain.hi)
        assert float(o2.hi[img, y + 1, xq, ch]) == sign * 65504.0
        # ... and only that value left the range
        assert int((o2.hi.float().abs() >= 65504).sum()) == 1


@pytest.mark.parametrize("name", list(FAMILY_CASES))
def test_other_3x3_kernels_at_a_multi_round_shape(dev, name):
    """igemm_kxr2 (cout = 64) and igemm_kxr (modes 2 and 3, the one-product hi_only form, the stat_partial training form; cout 128
    and 256) share the XCD-chunked block -> tile map: one shape each with MT >= 100 and a ragged last chunk, fp64 parity over every
    image (whole map and worst 64 x 128 block), nothing but the interior written.  hi_only is compared with the fp64 conv of the
    bf16 hi planes (what the mode defines) at mode 3's bar, as its existing test does.
    Worst block, CPU emulation of the storage roundings / kernel measured on an MI355X: mode 4 (igemm_kxr2) 3.40e-4 / 3.50e-4 (bar
    6e-4), mode 2 3.00e-4 / 3.04e-4 (bar 4e-4), mode 3 4.03e-6 / 4.56e-6 (bar 2e-5), hi_only 3.14e-6 / 3.18e-6 (bar 2e-5).  The
    fp16 statistics form (AGP_PREC_F16 with stat_partial) does not exist: the launch refuses it, and so does the plan query
    (tests/test_conv_schedules_host.py)."""
    from agplace_amd import ops
    (cin, cout, h, w, n), prec, flags, (kernel, bm, bn) = FAMILY_CASES[name]
    hi_only, stat = bool(flags.get("hi_only")), bool(flags.get("stat"))
    x, res = images(cin, h, w, n, 1), images(cout, h, w, n, 2)
    wt, scale, shift = weights(cin, cout)
    relu = not stat
    xm, rm = _pack(x, prec, dev), _pack(res, prec, dev)
    cw = ops.ConvWeights(wt.to(dev), scale.to(dev), shift.to(dev), 1, 1)
    out, bufs = guarded_map(n, h, w, cout, prec, dev)
    p = ops.conv_tile_plan([(xm, cw, out, rm, relu)], prec, stat_partial=stat, hi_only=hi_only)
    assert (p["kernel"], p["BM"], p["BN"]) == (kernel, bm, bn) and p["MT"] >= 100 and p["MT"] % 8 != 0, p
    part = None
    if stat:
        tiles = ops.conv_stat_tiles(xm, cw, out, prec, hi_only=hi_only)
        assert tiles == p["MT"]
        part = torch.zeros((tiles, 2, cout), dtype=torch.float32, device=dev)
    ops.conv2d(xm, cw, out, residual=rm, relu=relu, prec=prec, stat_partial=part, hi_only=hi_only)
    torch.cuda.synchronize()
    assert_only_the_interior_was_written(out, bufs)
    if hi_only:
        ref = ref64(x.bfloat16().double(), wt.bfloat16().double(), scale, shift, res, relu)
    else:
        ref = ref64(x, wt, scale, shift, res, relu)
    _check_parity(out, ref, prec, bm, name)
    if stat:
        sums = part.double().sum(0).cpu()
        assert rel_l2(sums[0], ref.sum((0, 2, 3))) < 1e-4 and rel_l2(sums[1], (ref * ref).sum((0, 2, 3))) < 1e-4
