"""-m gpu: the conv kernels outside the 3x3 stride-1 family against fp64 at multi-round size, by the method of
tests/test_gpu_conv_schedules.py -- igemm_s2 (the fused stage entry: both tile widths, every NT, the bench's stage-2 geometry, odd
inputs, two-trunk launches with the problem boundary inside an XCD chunk and on a chunk boundary, the range-guard twins, the
chunk-major weight plane), every instantiation of the generic LDS-staged kernel the default dispatch picks (modes 4 / 2 / 3,
128 x 128 and 256 x 64 tiles, stat_partial, launch_group_f16) and the packed stem on igemm_d16 with stat_partial.

Every case asserts through agp_conv2d_tile_plan (the launch path itself) the kernel and tile shape it ran, with MT >= 100,
a ragged last XCD chunk (MT % 8 != 0) and a partial last tile; compares EVERY image with fp64 on the whole map and on the worst
64-row x 64-column block of the kernel's own raster under the project's existing bars (conv_sched_util.BARS: mode 4 6e-4, mode 2
4e-4, mode 3 2e-5); checks that nothing but the interior was written; and prints its plan and figures.
tests/test_conv_schedules_host.py shows that the storage roundings alone stay under the bars per block."""
import pytest
import torch

from conv_sched_util import BARS, GENERIC_CASES, GENERIC_GROUP, S2_CASES, S2_GROUPS, STEM_CASE, assert_only_the_interior_was_written, \
    guarded_map, images, out_size, ref64_by_image, weights, worst_block
from gpu_util import rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


def _pack(t, prec, dev):
    from agplace_amd import ops
    return ops.pack_f32(t.to(dev), t.shape[1], 1, prec)


def _check_parity(out, ref, prec, bm, raster, what):
    """Whole-map rel_l2 and the worst 64 x 64 block of the kernel's raster under the same bar; the message names the block."""
    tol = BARS[prec]
    got = out.to_f32().cpu()
    whole = rel_l2(got, ref)
    worst, where = worst_block(got, ref, bm=bm, rows=64, cols=64, raster=raster)
    print("%s: whole map %.3g worst block %.3g (bar %.3g) at %s" % (what, whole, worst, tol, where))
    assert whole < tol, (what, whole)
    assert worst < tol, (what, worst, where)


def _multi_round(p, kernel, bm, bn, nt, rows):
    """The plan is the kernel, tile shape and regime the case names (no case passes vacuously on another kernel or a small grid)."""
    assert (p["kernel"], p["BM"], p["BN"], p["NT"]) == (kernel, bm, bn, nt), p
    assert p["MT"] == (rows + bm - 1) // bm and p["MT"] >= 100 and p["MT"] % 8 != 0 and rows % bm != 0, p
    assert p["grid"] == (p["MT"] + 7) // 8 * 8 * p["NT"] and p["half_tiles"] == 0, p


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


# ------------------------------------------------------------------------------------------------ the stage entry (igemm_s2)
def _trunk(dev, cin, cout, n, h, w, seed=0):
    """One trunk's stage entry: the 3x3/s2 conv (+ ReLU) and the 1x1/s2 downsample of the same input."""
    from agplace_amd import ops
    x = images(cin, h, w, n, 1 + seed)
    w3, s3, t3 = weights(cin, cout, seed, k=3)
    w1, s1, t1 = weights(cin, cout, seed + 7, k=1)
    ho, wo = out_size(h, w, 3, 2)
    assert (ho, wo) == out_size(h, w, 1, 2)
    return dict(x=x, xm=_pack(x, 4, dev), w3=(w3, s3, t3), w1=(w1, s1, t1), n=n, ho=ho, wo=wo, cout=cout,
                c3=ops.ConvWeights(w3.to(dev), s3.to(dev), t3.to(dev), 2, 1), c1=ops.ConvWeights(w1.to(dev), s1.to(dev), t1.to(dev), 2, 0))


def _entry_jobs(dev, trunks, guard_maps=False, c3=None, c1=None, xm=None):
    """[3x3/s2 of every trunk ..., 1x1/s2 of every trunk ...] (the order resnet.forward_maps_multi issues) -> (jobs, [guard bufs])"""
    from agplace_amd import ops
    outs = []
    for _ in range(2):
        for t in trunks:
            outs.append(guarded_map(t["n"], t["ho"], t["wo"], t["cout"], 4, dev) if guard_maps
                        else (ops.SplitMap.alloc(t["n"], t["ho"], t["wo"], t["cout"], 1, 4, dev), None))
    k = len(trunks)
    pick = lambda given, own: own if given is None else given
    jobs = [(pick(xm, t["xm"]), pick(c3, t["c3"]), outs[i][0], None, True) for i, t in enumerate(trunks)] + \
           [(pick(xm, t["xm"]), pick(c1, t["c1"]), outs[k + i][0], None, False) for i, t in enumerate(trunks)]
    return jobs, [o[1] for o in outs]


def _entry_refs(t):
    w3, s3, t3 = t["w3"]
    w1, s1, t1 = t["w1"]
    return ref64_by_image(t["x"], w3, s3, t3, None, True, 3, 2, 1), ref64_by_image(t["x"], w1, s1, t1, None, False, 1, 2, 0)


@pytest.mark.parametrize("name", list(S2_CASES))
def test_stage_entry_kernel_at_multi_round_size(dev, name):
    """igemm_s2, one trunk: both outputs (3x3/s2 + ReLU, 1x1/s2 downsample) of EVERY image against fp64, whole map and worst 64 x 64
    block of the padded-width output raster; nothing but the interior written in either map (guard regions, halo, the raster's
    halo columns, rows past M of the partial last tile, the tiles of the ragged last XCD chunk that return early).  TN 4 (128 x 128
    tiles) at NT 1 / 2 / 4 and TN 2 (128 x 64 tiles, cout % 128 != 0: reached by no other test) at NT 1 / 3; the bench's stage-2
    geometry and odd input sizes.
    Worst block (bar 6e-4): CPU emulation of mode 4's storage roundings at these very shapes 3.7e-4 .. 3.8e-4 (3x3) and 3.7e-4
    (downsample); the kernel's figures on an MI355X have not been measured yet: every run prints them."""
    from agplace_amd import ops
    (cin, cout, h, w, n), (bn, nt) = S2_CASES[name]
    t = _trunk(dev, cin, cout, n, h, w)
    jobs, bufs = _entry_jobs(dev, [t], guard_maps=True)
    p = ops.conv_tile_plan(jobs, 4)
    print(name, p)
    _multi_round(p, "s2", 128, bn, nt, n * t["ho"] * (t["wo"] + 2))
    ops.conv2d_grouped(jobs, 4)
    torch.cuda.synchronize()
    r3, r1 = _entry_refs(t)
    for job, buf, ref, what in zip(jobs, bufs, (r3, r1), ("3x3/s2", "1x1/s2 downsample")):
        assert_only_the_interior_was_written(job[2], buf)
        _check_parity(job[2], ref, 4, 128, "padded", "%s %s" % (name, what))


@pytest.mark.parametrize("name", list(S2_GROUPS))
def test_stage_entry_of_two_trunks_with_the_problem_boundary_in_and_on_a_chunk(dev, name):
    """Query + db trunk in ONE igemm_s2 launch (the bench's form: 56 x 336 and 56 x 56 inputs): the block -> (problem, row tile)
    lookup through mt_end[0] with the boundary strictly inside an XCD chunk, and exactly on a chunk boundary (both asserted from
    the plans).  Each trunk's two outputs bit-identical to its launch alone, under the bars against fp64, nothing but the interior
    written.  Worst block, CPU emulation: 3.7e-4 .. 4.0e-4 (bar 6e-4)."""
    from agplace_amd import ops
    shapes = S2_GROUPS[name]
    trunks = [_trunk(dev, 64, 128, n, h, w, seed=i) for i, (n, h, w) in enumerate(shapes)]
    jobs, bufs = _entry_jobs(dev, trunks, guard_maps=True)
    p = ops.conv_tile_plan(jobs, 4)
    singles = [ops.conv_tile_plan(_entry_jobs(dev, [t])[0], 4) for t in trunks]
    print(name, p, [q["MT"] for q in singles])
    assert (p["kernel"], p["BM"], p["BN"], p["NT"]) == ("s2", 128, 128, 1) and all(q["kernel"] == "s2" for q in singles)
    assert p["MT"] == sum(q["MT"] for q in singles) and p["MT"] >= 100 and p["MT"] % 8 != 0
    mt_chunk, e0 = (p["MT"] + 7) // 8, singles[0]["MT"]
    assert p["grid"] == mt_chunk * 8
    if name == "boundary_inside_a_chunk":
        assert e0 % mt_chunk != 0
    else:
        assert e0 % mt_chunk == 0 and 0 < e0 < p["MT"]
    ops.conv2d_grouped(jobs, 4)
    torch.cuda.synchronize()
    for i, t in enumerate(trunks):
        alone, _ = _entry_jobs(dev, [t])
        ops.conv2d_grouped(alone, 4)
        r3, r1 = _entry_refs(t)
        for j, a, ref, what in ((i, 0, r3, "3x3/s2"), (len(trunks) + i, 1, r1, "1x1/s2 downsample")):
            assert torch.equal(jobs[j][2].hi, alone[a][2].hi), (name, i, what)
            assert_only_the_interior_was_written(jobs[j][2], bufs[j])
            _check_parity(jobs[j][2], ref, 4, 128, "padded", "%s trunk %d %s" % (name, i, what))


@pytest.mark.parametrize("name", ["tn4_nt1_bench_stage2", "tn2_nt3_odd"])
def test_stage_entry_range_guard_twin(dev, name):
    """The guarded instantiations igemm_s2_kernel<4, true, uint32_t*> and <2, true, uint32_t*> (a guard word bound on the thread):
    the same stored bits as the unguarded launch and the word 0 on in-range data; one out-of-range value planted in the 3x3
    output (a middle row tile), and one in the downsample output in a late row tile, each sets the word and is stored as
    +-65504 while nothing else saturates.  (The value is planted through one input element at an even pixel, which only the
    centre tap of one output pixel reads, times one enlarged weight of one output channel.)"""
    from agplace_amd import ops
    (cin, cout, h, w, n), (bn, nt) = S2_CASES[name]
    t = _trunk(dev, cin, cout, n, h, w)
    plain, _ = _entry_jobs(dev, [t])
    p = ops.conv_tile_plan(plain, 4)
    print(name, p)
    _multi_round(p, "s2", 128, bn, nt, n * t["ho"] * (t["wo"] + 2))
    ops.conv2d_grouped(plain, 4)
    twin, _ = _entry_jobs(dev, [t])
    plans = []

    def guarded_launch(jobs):
        plans.append(ops.conv_tile_plan(jobs, 4))
        ops.conv2d_grouped(jobs, 4)
    assert _guarded(dev, lambda: guarded_launch(twin)) == 0
    assert plans[-1] == p                                  # the guarded twin has the unguarded launch's tiles
    assert torch.equal(twin[0][2].hi, plain[0][2].hi) and torch.equal(twin[1][2].hi, plain[1][2].hi)
    ch, c0, wpo = cout - 19, 5, t["wo"] + 2
    for which, row, sign in ((0, (p["MT"] // 2) * 128 + 100, 1.0), (1, (p["MT"] - 2) * 128 + 17, -1.0)):
        img, rem = divmod(row, t["ho"] * wpo)
        oy, xq = divmod(rem, wpo)
        ox = min(max(xq, 1), t["wo"]) - 1                  # an interior column of that raster row
        x2 = t["x"].clone()
        x2[img, c0, 2 * oy, 2 * ox] = 40000.0
        w3, w1 = t["w3"][0].clone(), t["w1"][0].clone()
        if which == 0:
            w3[ch, c0, 1, 1] = 8.0                         # 320000 x scale (>= 0.5): far out of range, ReLU keeps the sign
        else:
            w1[ch, c0, 0, 0] = -8.0
        c3 = ops.ConvWeights(w3.to(dev), t["w3"][1].to(dev), t["w3"][2].to(dev), 2, 1)
        c1 = ops.ConvWeights(w1.to(dev), t["w1"][1].to(dev), t["w1"][2].to(dev), 2, 0)
        x2m = _pack(x2, 4, dev)
        a, _ = _entry_jobs(dev, [t], c3=c3, c1=c1, xm=x2m)
        ops.conv2d_grouped(a, 4)
        b, _ = _entry_jobs(dev, [t], c3=c3, c1=c1, xm=x2m)
        assert _guarded(dev, lambda: guarded_launch(b)) == 1, (name, which, row)
        assert plans[-1] == p
        assert torch.equal(a[0][2].hi, b[0][2].hi) and torch.equal(a[1][2].hi, b[1][2].hi)
        assert float(b[which][2].hi[img, oy + 1, ox + 1, ch]) == sign * 65504.0
        assert int((b[0][2].hi.float().abs() >= 65504).sum()) + int((b[1][2].hi.float().abs() >= 65504).sum()) == 1


@pytest.mark.parametrize("name", ["tn4_nt2_odd", "tn2_nt1_odd"])
def test_stage_entry_chunk_major_weight_plane_is_bitwise_neutral_at_multi_round_size(dev, name, monkeypatch):
    """agp_conv_desc::w_cm on and off (ops.USE_W_CM) for the 3x3 weights and the downsample's, one multi-round shape per TN: the
    same bits in both outputs."""
    from agplace_amd import ops
    (cin, cout, h, w, n), (bn, nt) = S2_CASES[name]
    t = _trunk(dev, cin, cout, n, h, w)
    assert t["c3"].cm() is not None and t["c1"].cm() is not None
    outs = []
    for use in (True, False):
        monkeypatch.setattr(ops, "USE_W_CM", use)
        jobs, _ = _entry_jobs(dev, [t])
        _multi_round(ops.conv_tile_plan(jobs, 4), "s2", 128, bn, nt, n * t["ho"] * (t["wo"] + 2))
        ops.conv2d_grouped(jobs, 4)
        torch.cuda.synchronize()
        outs.append((jobs[0][2].hi, jobs[1][2].hi))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert float(outs[0][0].float().abs().max()) > 0 and float(outs[0][1].float().abs().max()) > 0


# ------------------------------------------------------------------------------------------ the generic kernel and the stem
def _stat_buffer(tiles, cout, dev):
    """stat_partial with four rows more than the kernel's tiles, all NaN: the kernel must write rows [0, tiles) and no other."""
    return torch.full((tiles + 4, 2, cout), float("nan"), dtype=torch.float32, device=dev)


def _check_stats(part, tiles, ref):
    """Every tile's row written, nothing behind them; channel sums and sums of squares against fp64 at 1e-4."""
    assert not bool(part[:tiles].isnan().any()), "a row tile wrote no statistics"
    assert bool(part[tiles:].isnan().all()), "statistics written past the plan's MT rows"
    sums = part[:tiles].double().sum(0).cpu()
    assert rel_l2(sums[0], ref.sum((0, 2, 3))) < 1e-4 and rel_l2(sums[1], (ref * ref).sum((0, 2, 3))) < 1e-4


@pytest.mark.parametrize("name", list(GENERIC_CASES))
def test_generic_kernel_at_multi_round_size(dev, name):
    """igemm_kernel (every 1x1 conv; every stride-2 conv of modes 2 and 3; the training stage entry with stat_partial): one shape
    with MT >= 100, a ragged last XCD chunk and a partial last tile for each instantiation the default dispatch picks -- modes 4,
    2 and 3 on 128 x 128 tiles (cout % 128 == 0) and on 256 x 64 tiles.  fp64 parity over every image (whole map and worst 64 x 64
    block of the plain [n][hout][wout] raster), nothing but the interior written; with stat_partial the buffer's rows are the
    plan's MT (agp_conv2d_stat_tiles mirrors the kernel), each written, none behind them, and the statistics match fp64 at 1e-4.
    Worst block, CPU emulation of the storage roundings at these very shapes: mode 4 3.4e-4 .. 3.7e-4 (bar 6e-4), mode 2
    3.0e-4 .. 3.1e-4 (bar 4e-4), mode 3 4.1e-6 .. 4.5e-6 (bar 2e-5); the kernel's figures on an MI355X have not been measured
    yet: every run prints them."""
    from agplace_amd import ops
    (cin, cout, k, stride, h, w, n), prec, flags, (bm, bn) = GENERIC_CASES[name]
    stat, use_res = bool(flags.get("stat")), bool(flags.get("res"))
    ho, wo = out_size(h, w, k, stride)
    x = images(cin, h, w, n, 1)
    res = images(cout, ho, wo, n, 2) if use_res else None
    wt, scale, shift = weights(cin, cout, k=k)
    xm, rm = _pack(x, prec, dev), None if res is None else _pack(res, prec, dev)
    cw = ops.ConvWeights(wt.to(dev), scale.to(dev), shift.to(dev), stride, k // 2)
    out, bufs = guarded_map(n, ho, wo, cout, prec, dev)
    p = ops.conv_tile_plan([(xm, cw, out, rm, use_res)], prec, stat_partial=stat)
    print(name, p)
    _multi_round(p, "generic", bm, bn, cout // bn, n * ho * wo)
    part = None
    if stat:
        assert ops.conv_stat_tiles(xm, cw, out, prec) == p["MT"]
        part = _stat_buffer(p["MT"], cout, dev)
    ops.conv2d(xm, cw, out, residual=rm, relu=use_res, prec=prec, stat_partial=part)
    torch.cuda.synchronize()
    assert_only_the_interior_was_written(out, bufs)
    ref = ref64_by_image(x, wt, scale, shift, res, use_res, k, stride, k // 2)
    _check_parity(out, ref, prec, bm, "plain", name)
    if stat:
        _check_stats(part, p["MT"], ref)


def test_generic_grouped_launch_at_multi_round_size(dev):
    """launch_group_f16: the 1x1 pairs (64 -> 128 + ReLU, 64 -> 256; problems of one and of two column tiles) of two trunks as ONE
    grid of 336 row tiles in which every problem has a ragged last XCD chunk.  Each output bit-identical to its separate launch,
    under the bars against fp64, nothing but the interior written."""
    from agplace_amd import ops
    jobs, bufs, probs = [], [], []
    for i, (n, h, w) in enumerate(GENERIC_GROUP):
        x = images(64, h, w, n, 11 + i)
        xm = _pack(x, 4, dev)
        for cout, relu in ((128, True), (256, False)):
            wt, scale, shift = weights(64, cout, seed=i, k=1)
            cw = ops.ConvWeights(wt.to(dev), scale.to(dev), shift.to(dev), 1, 0)
            out, buf = guarded_map(n, h, w, cout, 4, dev)
            jobs.append((xm, cw, out, None, relu))
            bufs.append(buf)
            probs.append((x, wt, scale, shift, relu))
    p = ops.conv_tile_plan(jobs, 4)
    singles = [ops.conv_tile_plan([j], 4) for j in jobs]
    print("generic group", p, [(q["MT"], q["NT"]) for q in singles])
    assert (p["kernel"], p["BM"], p["BN"]) == ("generic", 128, 128)
    assert p["MT"] == sum(q["MT"] for q in singles) and p["grid"] == sum(q["grid"] for q in singles)
    assert all((q["kernel"], q["BM"], q["BN"]) == ("generic", 128, 128) and q["MT"] % 8 != 0 for q in singles) and singles[0]["MT"] >= 100
    ops.conv2d_grouped(jobs, 4)
    torch.cuda.synchronize()
    for i, (job, buf, (x, wt, scale, shift, relu)) in enumerate(zip(jobs, bufs, probs)):
        assert_only_the_interior_was_written(job[2], buf)
        sep = ops.SplitMap.alloc(job[2].n, job[2].h, job[2].w, job[2].c, 1, 4, dev)
        ops.conv2d(job[0], job[1], sep, relu=relu, prec=4)
        assert torch.equal(job[2].hi, sep.hi), i
        _check_parity(job[2], ref64_by_image(x, wt, scale, shift, None, relu, 1, 1, 0), 4, 128, "plain", "generic group problem %d" % i)


def test_packed_stem_with_statistics_at_multi_round_size(dev):
    """igemm_d16: the packed 7x7 / stride-2 stem (3 -> 64, + ReLU) in mode 3 with stat_partial, as the training path's first
    BatchNorm reads it, on 4 images of 97 x 271 (105 row tiles of 256 rows; the existing test stops at 2 x 32 x 48 inputs, 2 row
    tiles).  The checks of test_generic_kernel_at_multi_round_size, statistics and tile count included.
    Worst block (bar 2e-5): CPU emulation at this shape 4.5e-6; the kernel's figure on an MI355X has not been measured yet: the
    run prints it."""
    from agplace_amd import ops
    h, w, n = STEM_CASE
    ho, wo = ops.conv_out_size(h, 7, 2, 3), ops.conv_out_size(w, 7, 2, 3)
    x = images(3, h, w, n, 1)
    wt, scale, shift = weights(3, 64, k=7)
    xm = ops.pack_f32(x.to(dev), 4, 3, 3)
    cw = ops.ConvWeights(wt.to(dev), scale.to(dev), shift.to(dev), 2, 3, stem=True)
    out, bufs = guarded_map(n, ho, wo, 64, 3, dev)
    p = ops.conv_tile_plan([(xm, cw, out, None, True)], 3, stat_partial=True)
    print("stem", p)
    _multi_round(p, "direct-x", 256, 64, 1, n * ho * wo)
    assert ops.conv_stat_tiles(xm, cw, out, 3) == p["MT"]
    part = _stat_buffer(p["MT"], 64, dev)
    ops.conv2d(xm, cw, out, relu=True, prec=3, stat_partial=part)
    torch.cuda.synchronize()
    assert_only_the_interior_was_written(out, bufs)
    ref = ref64_by_image(x, wt, scale, shift, None, True, 7, 2, 3)
    _check_parity(out, ref, 3, 256, "plain", "stem")
    _check_stats(part, p["MT"], ref)
