"""Host-side checks of the conv tile-plan query (agp_conv2d_tile_plan: the launch path stopped before the launch) and of the
per-block error bars that tests/test_gpu_conv_schedules.py applies on the GPU.  No GPU needed."""
import pytest
import torch

from conv_sched_util import BARS, FAMILY_CASES, GROUPS, WIDE_CASES, block_rel_l2, desc3x3, emulate, images, plan3x3, plan_group, \
    raster_rows, ref64, regime, weights


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
    # other kernels answer with their id
    d = desc3x3(64, 128, 12, 20, 2)
    d.kh = d.kw = 1
    d.pad = 0
    assert ops.tile_plan(d)["kernel"] == "generic"
    d = desc3x3(64, 128, 12, 20, 2)
    d.stride, d.hout, d.wout = 2, 6, 10
    assert ops.tile_plan(d)["kernel"] == "generic"
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
