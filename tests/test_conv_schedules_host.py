"""Host-side checks of the conv tile-plan query (agp_conv2d_tile_plan: the launch path stopped before the launch) and of the
per-block error bars that tests/test_gpu_conv_schedules.py applies on the GPU.  No GPU needed."""
import pytest
import torch

from conv_sched_util import BARS, FAMILY_CASES, GENERIC_CASES, GENERIC_GROUP, GROUPS, S2_CASES, S2_GROUPS, STEM_CASE, WIDE_CASES, \
    block_rel_l2, desc3x3, desc_conv, descs_s2, emulate, images, out_size, plan3x3, plan_conv, plan_group, plan_s2, raster_rows, ref64, \
    regime, smallest_batch, weights


def _consistent(p):
    """The identities between a plan's fields that hold for every kernel of the 3x3 stride-1 family."""
    assert p["MT_full"] + p["half_tiles"] // (2 * p["NT"]) == p["MT"] and p["half_tiles"] % (2 * p["NT"]) == 0
    mt_chunk = (p["MT_full"] + 7) // 8
    assert p["grid"] == mt_chunk * 8 * p["NT"] + p["half_tiles"]


@pytest.mark.parametrize("name", list(WIDE_CASES))
def test_tile_plan_of_the_wide_fp16_kernel_reports_the_intended_regime(name):
    (cin, cout, h, w, n), want = WIDE_CASES[name]
    for pool in (False, True):
        p = plan3x3(cin, cout, h, w, n, pool=pool)
        assert (p["kernel"], p["BM"], p["BN"], p["NT"]) == ("kxrw", 256, 128, cout // 128)
        rows = n * ((h * (w + 2) + 63) // 64 * 64) if pool else raster_rows(n, h, w)     # pooling: 64-row aligned images
        assert p["MT"] == (rows + 255) // 256
        _consistent(p)
        if not pool:
            assert regime(p) == want, (name, p)
    p = plan3x3(cin, cout, h, w, n)
    T, r = p["MT"] * p["NT"], raster_rows(n, h, w) % 256
    if want == "all-half":
        assert T <= 128 and p["MT_full"] == 0 and p["grid"] == 2 * T
    if want == "mixed":
        assert T > 512 and 0 < p["half_tiles"] <= 256 and p["MT_full"] * p["NT"] % 512 == 0
    if name == "mixed_last_tile_has_one_half":
        assert 0 < r <= 128
    if name == "mixed_last_half_tile_partial":
        assert r > 128
    if name == "full_only_last_tile_partial":
        assert r != 0 and p["MT"] % 8 != 0
    if name == "nt3_refuses_to_mix":
        tail = T - (T - 1) // 512 * 512
        assert T > 512 and tail <= 128 and tail % 3 != 0       # small enough a tail to mix, but not whole row tiles


@pytest.mark.parametrize("name", list(FAMILY_CASES))
def test_tile_plan_of_the_other_3x3_kernels(name):
    (cin, cout, h, w, n), prec, flags, (kernel, bm, bn) = FAMILY_CASES[name]
    p = plan3x3(cin, cout, h, w, n, prec=prec, **flags)
    assert (p["kernel"], p["BM"], p["BN"]) == (kernel, bm, bn)
    assert p["MT"] == (raster_rows(n, h, w) + bm - 1) // bm and p["NT"] == cout // bn
    assert p["half_tiles"] == 0 and p["MT_full"] == p["MT"]
    _consistent(p)
    # multi-round shapes with a ragged last XCD chunk
    assert p["MT"] >= 100 and p["MT"] % 8 != 0 and p["grid"] > p["MT"] * p["NT"]
    if kernel == "kxr2":
        assert p["MT"] * p["NT"] > 768           # more than one residency round of three workgroups per CU


def test_f16_conv_past_the_32_bit_output_offsets_plans_on_igemm_kxr():
    """igemm_kxr2 / igemm_kxrw address the output plane with 32-bit element offsets: with 2^31 or more elements in the padded output
    map an AGP_PREC_F16 conv leaves them for igemm_kxr's one-product fp16 form (<256, 64, 4, 1, 4, 3>, 256 x 64 tiles) -- the only
    way to that instantiation; one image fewer and it stays.  (32 -> 128 channels, 993 images of 128 x 128: 1.07e9 input bytes,
    under the kernels' 2^31.)"""
    pad = 130 * 130
    assert 993 * pad * 32 * 2 < 2 ** 31 <= 993 * pad * 128 and 992 * pad * 128 < 2 ** 31
    p = plan3x3(32, 128, 128, 128, 993, prec=4)
    assert (p["kernel"], p["BM"], p["BN"], p["NT"]) == ("kxr", 256, 64, 2) and p["MT"] == (993 * 128 * 130 + 255) // 256
    _consistent(p)
    assert plan3x3(32, 128, 128, 128, 992, prec=4)["kernel"] == "kxrw"
    assert plan3x3(32, 64, 128, 128, 993, prec=4)["kernel"] == "kxr2"          # (cout 64: the output is half as large)


@pytest.mark.parametrize("name", list(GROUPS))
def test_tile_plan_of_the_grouped_launches_is_mixed(name):
    p = plan_group(GROUPS[name], 128, 128)
    assert p["kernel"] == "kxrw" and regime(p) == "mixed"
    assert p["MT"] == sum(plan3x3(128, 128, h, w, n)["MT"] for (n, h, w) in GROUPS[name])
    _consistent(p)


def test_tile_plan_follows_the_dispatch():
    from agplace_amd import _lib, ops
    # grouped launches: the row tiles of all problems form one sequence
    shapes = [(16, 28, 170), (16, 28, 170)]
    p = plan_group(shapes, 128, 128)
    assert (p["kernel"], p["MT"], p["MT_full"], p["half_tiles"]) == ("kxrw", 602, 512, 180) and regime(p) == "mixed"
    assert regime(plan3x3(128, 128, 28, 170, 16)) == "full-only"       # (each of them alone is not)
    p64 = plan_group([(3, 56, 100), (2, 40, 60)], 64, 64)
    assert p64["kernel"] == "kxr2" and p64["MT"] == (3 * 56 * 102 + 255) // 256 + (2 * 40 * 62 + 255) // 256
    # a group the one-launch kernels do not take runs as separate launches: no single plan
    arr = (_lib.ConvDesc * 2)(desc3x3(128, 128, 9, 9, 2), desc3x3(128, 256, 9, 9, 2))
    with pytest.raises(RuntimeError, match="AGP_E_UNSUPPORTED"):
        ops.tile_plan(arr)
    # the statistics epilogue exists on split-bf16 maps only: the launch refuses the fp16 form, and so does the query
    with pytest.raises(RuntimeError, match="AGP_E_BADARG"):
        plan3x3(128, 128, 28, 60, 16, prec=4, stat=True)
    # the other kernels answer with their id and, from their own grid arithmetic, their tiles
    d = desc3x3(64, 128, 12, 20, 2)
    d.kh = d.kw = 1
    d.pad = 0
    assert ops.tile_plan(d)["kernel"] == "generic"
    assert ops.tile_plan(d) == dict(kernel="generic", BM=128, BN=128, MT=4, NT=1, MT_full=4, half_tiles=0, grid=8)
    d = desc3x3(64, 128, 12, 20, 2)
    d.stride, d.hout, d.wout = 2, 6, 10
    assert ops.tile_plan(d)["kernel"] == "generic"
    assert ops.tile_plan(d) == dict(kernel="generic", BM=128, BN=128, MT=1, NT=1, MT_full=1, half_tiles=0, grid=8)
    # invalid descriptors fail as the launch would
    d = desc3x3(48, 128, 12, 20, 2)
    with pytest.raises(RuntimeError, match="AGP_E_BADARG"):
        ops.tile_plan(d)


@pytest.mark.parametrize("prec,hi_only", [(4, False), (2, False), (3, False), (3, True)])
def test_storage_rounding_alone_stays_under_the_bar_in_every_64_row_block(prec, hi_only):
    """The per-block form of the parity bars: an emulation of each mode's STORAGE roundings around an exact conv (conv_sched_util.
    emulate), against fp64, must keep every 64-row x 128-column block of the raster under the whole-map bar with room -- otherwise
    the GPU test's per-block assertion would be a guess.  Measured (3 images of 128 -> 256 at 28 x 60, residual + scale/shift +
    ReLU; worst block / whole map): mode 4 3.40e-4 / 3.25e-4 (bar 6e-4), mode 2 3.00e-4 / 2.91e-4 (bar 4e-4), mode 3 4.03e-6 / 3.84e-6
    (bar 2e-5), hi_only (against the fp64 conv of the hi planes) 3.14e-6 / 2.97e-6.  The worst block lies within 5 % of the whole
    map in every mode, so a larger block would buy nothing: the room is the bar's own (mode 2: the fp16 rounding of x, residual
    and output is 0.73 of its bar before any kernel runs)."""
    cin, cout, h, w, n = 128, 256, 28, 60, 3
    x, res = images(cin, h, w, n, 1), images(cout, h, w, n, 2)
    wt, scale, shift = weights(cin, cout)
    emu = emulate(prec, x, wt, scale, shift, res, True, hi_only=hi_only)
    if hi_only:
        ref = ref64(x.bfloat16().double(), wt.bfloat16().double(), scale, shift, res, True)
    else:
        ref = ref64(x, wt, scale, shift, res, True)
    rel = block_rel_l2(emu, ref)
    worst = float(torch.nan_to_num(rel, nan=0.0).max())
    whole = float((emu - ref).norm() / ref.norm())
    print("prec %d hi_only %d: worst block %.3g whole map %.3g" % (prec, hi_only, worst, whole))
    assert 0 < worst < 0.8 * BARS[prec] and worst < 1.1 * whole


# ------------------------------------------------------------------------- the stage-entry, generic and stem kernels' plans
def _xcd_chunked(p, kernel, bm, bn, nt, rows):
    """What every case of tests/test_gpu_conv_entry_schedules.py needs of its plan: the kernel and tile shape it names, the tile
    counts of `rows` GEMM rows, one XCD-chunked grid of several rounds with a ragged last chunk and a partial last tile."""
    assert (p["kernel"], p["BM"], p["BN"], p["NT"]) == (kernel, bm, bn, nt), p
    assert p["MT"] == (rows + bm - 1) // bm and p["MT_full"] == p["MT"] and p["half_tiles"] == 0
    _consistent(p)
    assert p["MT"] >= 100 and p["MT"] % 8 != 0 and rows % bm != 0 and p["grid"] > p["MT"] * p["NT"], p


@pytest.mark.parametrize("name", list(S2_CASES))
def test_tile_plan_of_the_stage_entry_kernel(name):
    (cin, cout, h, w, n), (bn, nt) = S2_CASES[name]
    ho, wo = out_size(h, w, 3, 2)
    rows = lambda k: k * ho * (wo + 2)                    # the padded-width raster of the OUTPUT map
    _xcd_chunked(plan_s2([(n, h, w)], cin, cout), "s2", 128, bn, nt, rows(n))
    assert nt == (cout // 128 if cout % 128 == 0 else cout // 64)
    assert n == smallest_batch(lambda k: plan_s2([(k, h, w)], cin, cout), rows)
    if name == "tn4_nt1_bench_stage2":
        assert (h, w, ho, wo) == (56, 336, 28, 168)
    else:
        assert h % 2 == 1 and w % 2 == 1


@pytest.mark.parametrize("name", list(S2_GROUPS))
def test_tile_plan_of_the_two_trunk_stage_entry(name):
    shapes = S2_GROUPS[name]
    p = plan_s2(shapes, 64, 128)
    singles = [plan_s2([sh], 64, 128)["MT"] for sh in shapes]
    assert (p["kernel"], p["BM"], p["BN"], p["NT"]) == ("s2", 128, 128, 1) and p["MT"] == sum(singles)
    _consistent(p)
    assert p["MT"] >= 100 and p["MT"] % 8 != 0
    mt_chunk, e0 = (p["MT"] + 7) // 8, singles[0]
    if name == "boundary_inside_a_chunk":
        assert e0 % mt_chunk != 0
    else:
        assert e0 % mt_chunk == 0 and 0 < e0 < p["MT"]


@pytest.mark.parametrize("name", list(GENERIC_CASES))
def test_tile_plan_of_the_generic_kernel(name):
    from agplace_amd import _lib
    import ctypes as C
    (cin, cout, k, stride, h, w, n), prec, flags, (bm, bn) = GENERIC_CASES[name]
    ho, wo = out_size(h, w, k, stride)
    kw = dict(k=k, stride=stride, prec=prec, stat=bool(flags.get("stat")), res=bool(flags.get("res")), relu=bool(flags.get("res")))
    p = plan_conv(cin, cout, h, w, n, **kw)
    _xcd_chunked(p, "generic", bm, bn, cout // bn, n * ho * wo)
    assert n == smallest_batch(lambda q: plan_conv(cin, cout, h, w, q, **kw), lambda q: q * ho * wo)
    tiles = int(_lib.load().agp_conv2d_stat_tiles(C.byref(desc_conv(cin, cout, h, w, n, **kw))))
    if flags.get("stat"):
        assert tiles == p["MT"]                           # the statistics buffer's rows mirror the kernel's own tile count
    elif prec == 3:
        assert tiles == p["MT"]                           # (asked without the pointer: the same answer)
    else:
        assert tiles == 0


def test_tile_plan_of_the_generic_grouped_launch():
    from agplace_amd import _lib, ops
    ds, singles = [], []
    for (n, h, w) in GENERIC_GROUP:
        for cout, relu in ((128, True), (256, False)):
            ds.append(desc_conv(64, cout, h, w, n, k=1, relu=relu))
            singles.append(plan_conv(64, cout, h, w, n, k=1, relu=relu))
    p = ops.tile_plan((_lib.ConvDesc * len(ds))(*ds))
    assert (p["kernel"], p["BM"], p["BN"], p["NT"]) == ("generic", 128, 128, 0)         # (problems of 1 and 2 column tiles)
    assert p["MT"] == sum(q["MT"] for q in singles) and p["grid"] == sum(q["grid"] for q in singles)
    assert p["MT_full"] == p["MT"] and p["half_tiles"] == 0
    assert all(q["MT"] % 8 != 0 and (q["kernel"], q["BM"], q["BN"]) == ("generic", 128, 128) for q in singles) and singles[0]["MT"] >= 100
    # one width: NT is that of every problem
    same = (_lib.ConvDesc * 2)(*[desc_conv(64, 256, h, w, n, k=1) for (n, h, w) in GENERIC_GROUP])
    assert ops.tile_plan(same)["NT"] == 2


def test_tile_plan_of_the_packed_stem():
    from agplace_amd import _lib
    import ctypes as C
    h, w, n = STEM_CASE
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    kw = dict(prec=3, stat=True, stem=True)
    p = plan_conv(3, 64, h, w, n, **kw)
    _xcd_chunked(p, "direct-x", 256, 64, 1, n * ho * wo)
    assert n == smallest_batch(lambda q: plan_conv(3, 64, h, w, q, **kw), lambda q: q * ho * wo)
    assert int(_lib.load().agp_conv2d_stat_tiles(C.byref(desc_conv(3, 64, h, w, n, **kw)))) == p["MT"]
    assert plan_conv(3, 128, h, w, n, prec=4, stem=True)["BN"] == 128


def test_stage_entry_dispatch_refuses_what_the_fused_kernel_cannot_run():
    """A [3x3/s2, 1x1/s2] pair that igemm_s2 must not take -- a residual on either conv, ReLU on the downsample, geometries that
    differ, a map over the kernel's 2^31-byte addressing -- comes back from the query as the generic grouped launch, or, where
    that cannot take it either (cout % 128 != 0), as AGP_E_UNSUPPORTED (separate launches): never as "s2"."""
    from agplace_amd import ops
    shape = (3, 20, 36)

    def pair(cin=64, cout=128, n=3, h=20, w=36):
        return descs_s2([(n, h, w)], cin, cout)
    assert ops.tile_plan(pair())["kernel"] == "s2" and ops.tile_plan(pair(cout=64))["kernel"] == "s2"      # the controls
    bad = {}
    for cout in (128, 64):
        a = pair(cout=cout); a[0].res_hi = 1
        b = pair(cout=cout); b[1].res_hi = 1
        c = pair(cout=cout); c[1].relu = 1
        d = pair(cout=cout); d[1].hin, d[1].hout = 22, 11                 # another map height
        e = pair(cout=cout); e[1].n = 2                                   # another batch
        f = pair(cout=cout); f[1].in_hi = 2                               # another input map
        g = pair(cout=cout); g[1].cin = g[1].in_w_step = 128              # other input channels
        # 58 x 338 x 64 fp16 = 2.5 MB per padded image: 900 images are over 2^31 bytes and under the generic kernel's 2^32
        big = pair(cout=cout, n=900, h=56, w=336)
        assert 2 ** 31 <= 900 * 58 * 338 * 64 * 2 < 2 ** 32
        bad[cout] = dict(conv_residual=a, downsample_residual=b, downsample_relu=c, other_height=d, other_batch=e, other_input=f,
                         other_cin=g, over_the_map_limit=big)
    for what, arr in bad[128].items():
        assert ops.tile_plan(arr)["kernel"] == "generic", what
    for what, arr in bad[64].items():
        with pytest.raises(RuntimeError, match="AGP_E_UNSUPPORTED"):
            ops.tile_plan(arr)
    # ... the output map's limit as well: 30 x 170 x 512 fp16 = 5.2 MB per padded output image
    out_big = descs_s2([(420, 56, 336)], 64, 512)
    assert 420 * 58 * 338 * 64 * 2 < 2 ** 31 <= 420 * 30 * 170 * 512 * 2
    assert ops.tile_plan(out_big)["kernel"] == "generic"
    assert ops.tile_plan(descs_s2([(400, 56, 336)], 64, 512))["kernel"] == "s2"


# name -> (cin, cout, k, stride, residual + ReLU, raster of the kernel that runs it in mode 4 / in modes 2 and 3)
_EMU_SHAPES = {
    "3x3s2_64_128": (64, 128, 3, 2, False, "padded", "plain"),
    "1x1s2_64_128": (64, 128, 1, 2, False, "padded", "plain"),          # mode 4: the downsample output of igemm_s2
    "3x3s2_64_64": (64, 64, 3, 2, False, "padded", "plain"),
    "1x1_256_64_res_relu": (256, 64, 1, 1, True, "plain", "plain"),
    "1x1_64_256": (64, 256, 1, 1, False, "plain", "plain"),
}


@pytest.mark.parametrize("name,prec", [(name, prec) for name in _EMU_SHAPES for prec in (4, 2, 3)] + [("stem", 3)])
def test_storage_rounding_of_the_entry_and_generic_kernels_stays_under_the_bar_per_block(name, prec):
    """test_storage_rounding_alone_stays_under_the_bar_in_every_64_row_block for the stride-2, 1x1 and stem convs, on the raster
    of the kernel that runs each (igemm_s2: padded-width output raster; generic kernel, igemm_d16: plain raster), per 64-row x
    64-column block.  Measured (3 images of 29 x 43 / 57 x 85 inputs; worst block): mode 4 3.4e-4 .. 3.8e-4 (bar 6e-4), mode 2
    3.0e-4 .. 3.1e-4 (bar 4e-4), mode 3 4.0e-6 .. 4.4e-6 (bar 2e-5); the stem (3 -> 64, 7x7/s2 + ReLU) in mode 3 4.3e-6."""
    if name == "stem":
        h, w, n = 33, 47, 3
        x = images(3, h, w, n, 1)
        wt, scale, shift = weights(3, 64, k=7)
        geo, res, relu, raster = dict(k=7, stride=2, pad=3), None, True, "plain"
    else:
        cin, cout, k, stride, rr, r4, r23 = _EMU_SHAPES[name]
        h, w, n = (57, 85, 3) if stride == 2 else (29, 43, 3)
        ho, wo = out_size(h, w, k, stride)
        x = images(cin, h, w, n, 1)
        res = images(cout, ho, wo, n, 2) if rr else None
        wt, scale, shift = weights(cin, cout, k=k)
        geo, relu, raster = dict(k=k, stride=stride, pad=k // 2), rr, (r4 if prec == 4 else r23)
    emu = emulate(prec, x, wt, scale, shift, res, relu, **geo)
    ref = ref64(x, wt, scale, shift, res, relu, **geo)
    worst = float(torch.nan_to_num(block_rel_l2(emu, ref, rows=64, cols=64, raster=raster), nan=0.0).max())
    whole = float((emu - ref).norm() / ref.norm())
    print("%s prec %d: worst 64 x 64 block %.3g whole map %.3g" % (name, prec, worst, whole))
    assert 0 < whole < worst < BARS[prec]
