"""Writes tests/golden/conv_dispatch_table.npz: what the host-side conv dispatch of ONE build of the library answers for a fixed
sweep of descriptors -- return code and plan[8] of agp_conv2d_tile_plan, and for single descriptors agp_conv2d_stat_tiles and
agp_conv2d_pool_blocks, asked once with the fake pointers of conv_sched_util.desc_conv and once with none (as ops.conv_desc
asks).  Nothing is launched or dereferenced: no GPU needed.  tests/test_conv_dispatch_table.py replays sweep() against the
library it is given and compares every row, so a change to the dispatch that moves a route, a return code, a plan or a size
shows up as a row.

Recorded from the build of the commit BEFORE the dispatch moved into csrc/conv_dispatch.hip.  To record again (after a change
that is meant to move rows), build the library of the commit to record from and run, from the repository root:
    AGP_HIP_LIB=/path/to/that/libagplace_hip.so python tests/golden/make_conv_dispatch_table.py <that commit's hash>"""
import ctypes as C
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))) if p not in sys.path]
from conv_sched_util import GENERIC_GROUP, desc3x3, desc_conv, descs_s2  # noqa: E402

OUT = os.path.join(HERE, "conv_dispatch_table.npz")
OK, BADARG, UNSUPPORTED = 0, 1, 3
GENERIC, DIRECT_X, KXR, KXR2, KXRW, S2 = 1, 2, 3, 4, 5, 6
# columns of the table; the size queries are -1 for groups
COLS = ("n", "prec", "rc", "kernel", "BM", "BN", "MT", "NT", "MT_full", "half_tiles", "grid",
        "stat_tiles", "pool_blocks", "stat_tiles_noptr", "pool_blocks_noptr")
COL = {c: i for i, c in enumerate(COLS)}
_POINTERS = None


def _pointers():
    from agplace_amd import _lib
    global _POINTERS
    if _POINTERS is None:
        _POINTERS = [name for name, t in _lib.ConvDesc._fields_ if t is C.c_void_p]
    return _POINTERS


def _copy(d):
    from agplace_amd import _lib
    c = _lib.ConvDesc()
    C.memmove(C.byref(c), C.byref(d), C.sizeof(d))
    return c


# ---------------------------------------------------------------------------------------------------------------- the sweep
def _res(d):
    d.res_hi = 1
    if d.prec == 3:
        d.res_lo = 1


def _bstat(d, stat=True, mean=True):
    d.stat_partial = 1 if stat else None
    d.bstat_z_hi = d.bstat_rstd = 1
    d.bstat_mean = 1 if mean else None


# name -> edit of a descriptor whose pointers are desc_conv's (w_hi = 1)
FLAGS = {
    "plain": lambda d: None,
    "stat": lambda d: setattr(d, "stat_partial", 1),
    "hi_only": lambda d: setattr(d, "hi_only", 1),
    "pool": lambda d: setattr(d, "pool_partial", 1),
    "res": _res,
    "pin0": lambda d: setattr(d, "pin", 0),
    "w_cm": lambda d: setattr(d, "w_cm", 5),
    "w_cm_is_w_hi": lambda d: setattr(d, "w_cm", 1),
    "w_cm_lo": lambda d: (setattr(d, "w_cm", 5), setattr(d, "w_cm_lo", 6)),
    "w_q8": lambda d: setattr(d, "w_q8", 7),
    "bstat_stat": _bstat,
    "bstat_nostat": lambda d: _bstat(d, stat=False),
    # ... and the combinations the training step makes of them
    "bstat_no_mean": lambda d: _bstat(d, mean=False),
    "hi_only_stat": lambda d: (setattr(d, "hi_only", 1), setattr(d, "stat_partial", 1)),
    "hi_only_w_cm_is_w_hi": lambda d: (setattr(d, "hi_only", 1), setattr(d, "w_cm", 1)),
    "hi_only_bstat": lambda d: (setattr(d, "hi_only", 1), _bstat(d)),
    "stat_w_cm_pair_is_w": lambda d: (setattr(d, "stat_partial", 1), setattr(d, "w_cm", 1), setattr(d, "w_cm_lo", 6)),
    "pool_res": lambda d: (setattr(d, "pool_partial", 1), _res(d)),
    "pool_stat1": lambda d: (setattr(d, "pool_partial", 1), setattr(d, "pool_stat", 1)),
    "pool_stat2": lambda d: (setattr(d, "pool_partial", 1), setattr(d, "pool_stat", 2)),
}
CONVS = {"3x3s1": dict(k=3, stride=1), "3x3s2": dict(k=3, stride=2), "1x1s1": dict(k=1, stride=1), "1x1s2": dict(k=1, stride=2),
         "stem": dict(stem=True)}
MAPS = [(12, 20), (9, 13)]


def singles():
    rows = []
    for prec in (2, 3, 4):
        for conv, kw in CONVS.items():
            for cin in (32, 48, 64, 128):
                for cout in (64, 96, 128, 256, 512):
                    for (h, w) in MAPS:
                        for flag, edit in FLAGS.items():
                            d = desc_conv(cin, cout, h, w, 2, prec=prec, **kw)
                            if conv == "stem":
                                d.cin = cin                 # (desc_conv packs 32 channels: the other widths are refusals)
                            edit(d)
                            rows.append(("%s prec %d %d->%d %dx%d %s" % (conv, prec, cin, cout, h, w, flag), [d]))
    # ---- the size cliffs, a row on each side
    for prec in (3, 2):             # igemm_kxr's 2^31-byte input plane: 1985 / 1986 images of 130 x 130 x 32 (x 2 bytes)
        for n in (1985, 1986):
            for flag in ("plain", "stat", "hi_only"):
                d = desc3x3(32, 64, 128, 128, n, prec=prec)
                FLAGS[flag](d)
                rows.append(("cliff kxr input bytes prec %d n %d %s" % (prec, n, flag), [d]))
    for n in (992, 993):            # igemm_kxr2 / igemm_kxrw: 2^31 elements of the padded output plane
        for cout in (64, 128):
            for pool in (False, True):
                rows.append(("cliff kxr2 output elements n %d cout %d pool %d" % (n, cout, pool),
                             [desc3x3(32, cout, 128, 128, n, prec=4, pool=pool)]))
    for prec in (4, 3):             # conv_fill_params: 2^32 bytes of the input plane (128 x 128 x 32 x 2 bytes = 2^20 per image)
        for n in (4095, 4096):
            rows.append(("cliff input 2^32 bytes prec %d n %d" % (prec, n), [desc_conv(32, 64, 126, 126, n, k=1, prec=prec)]))
        for cout in (32704, 32768):  # ... and 2^31 bytes of weights
            rows.append(("cliff weights 2^31 bytes prec %d cout %d" % (prec, cout), [desc_conv(32768, cout, 9, 13, 1, k=1, prec=prec)]))
    for n in (0, -1):
        for prec in (3, 4):
            rows.append(("no images prec %d n %d" % (prec, n), [desc3x3(64, 64, 12, 20, n, prec=prec)]))
    return rows


def _s2_perturbations(shapes, cout):
    """Every single-field edit of test_stage_entry_dispatch_refuses_what_the_fused_kernel_cannot_run on the first trunk of a stage
    entry, and the fields that only agp_conv2d_s2_fwd looks at (w_lo, res_lo, hi_only on the 3x3 conv)."""
    h = len(shapes)

    def make(edit):
        a = [_copy(d) for d in descs_s2(shapes, 64, cout)]
        edit(a)
        return a

    def other_height(a):
        a[h].hin, a[h].hout = a[h].hin + 2, a[h].hout + 1

    def other_cin(a):
        a[h].cin = a[h].in_w_step = 128
    edits = {
        "control": lambda a: None,
        "conv_residual": lambda a: setattr(a[0], "res_hi", 1),
        "downsample_residual": lambda a: setattr(a[h], "res_hi", 1),
        "downsample_relu": lambda a: setattr(a[h], "relu", 1),
        "other_height": other_height,
        "other_batch": lambda a: setattr(a[h], "n", a[h].n + 1),
        "other_input": lambda a: setattr(a[h], "in_hi", 2),
        "other_cin": other_cin,
        "conv_w_lo": lambda a: setattr(a[0], "w_lo", 1),
        "conv_res_lo": lambda a: setattr(a[0], "res_lo", 1),
        "conv_hi_only": lambda a: setattr(a[0], "hi_only", 1),
        "downsample_w_lo": lambda a: setattr(a[h], "w_lo", 1),
        "downsample_hi_only": lambda a: setattr(a[h], "hi_only", 1),
        "conv_stat": lambda a: setattr(a[0], "stat_partial", 1),
        "downsample_pool": lambda a: setattr(a[h], "pool_partial", 1),
        "conv_prec2": lambda a: (setattr(a[0], "prec", 2), setattr(a[0], "w_lo", 1)),
        "conv_w_cm": lambda a: (setattr(a[0], "w_cm", 5), setattr(a[h], "w_cm", 6)),
        "conv_pin0": lambda a: setattr(a[0], "pin", 0),
        "no_images": lambda a: (setattr(a[0], "n", 0), setattr(a[h], "n", 0)),
        "swapped": lambda a: a.__setitem__(slice(0, 2 * h), a[h:] + a[:h]),
    }
    return [("s2 %d trunks cout %d %s" % (h, cout, what), make(edit)) for what, edit in edits.items()]


def groups():
    rows = []
    sizes = [(3, 12, 20), (2, 9, 13), (4, 28, 60), (1, 14, 30), (2, 12, 20)]
    for cout in (64, 128):
        for n in (2, 3, 4, 5):      # (five: more than one launch takes)
            rows.append(("3x3 group of %d cout %d" % (n, cout), [desc3x3(64, cout, h, w, b) for (b, h, w) in sizes[:n]]))
        base = lambda: [desc3x3(64, cout, h, w, b) for (b, h, w) in sizes[:3]]
        for what, edit in {
            "other_cout": lambda g: g.__setitem__(1, desc3x3(64, 2 * cout, 9, 13, 2)),
            "other_cin": lambda g: g.__setitem__(2, desc3x3(128, cout, 28, 60, 4)),
            "prec2_member": lambda g: g.__setitem__(1, desc3x3(64, cout, 9, 13, 2, prec=2)),
            "all_prec3": lambda g: g.__setitem__(slice(0, 3), [desc3x3(64, cout, h, w, b, prec=3) for (b, h, w) in sizes[:3]]),
            "pool_member": lambda g: setattr(g[1], "pool_partial", 1),
            "stat_member": lambda g: setattr(g[1], "stat_partial", 1),
            "res_member": lambda g: setattr(g[2], "res_hi", 1),
            "res_lo_member": lambda g: setattr(g[2], "res_lo", 1),
            "in_lo_member": lambda g: setattr(g[0], "in_lo", 1),
            "w_lo_member": lambda g: setattr(g[0], "w_lo", 1),
            "hi_only_member": lambda g: setattr(g[0], "hi_only", 1),
            "w_cm_members": lambda g: [setattr(d, "w_cm", 5) for d in g],
            "no_images_member": lambda g: setattr(g[1], "n", 0),
            "stride2_member": lambda g: g.__setitem__(1, desc_conv(64, cout, 9, 13, 2, k=3, stride=2)),
            "1x1_member": lambda g: g.__setitem__(1, desc_conv(64, cout, 9, 13, 2, k=1)),
        }.items():
            g = base()
            edit(g)
            rows.append(("3x3 group cout %d %s" % (cout, what), g))
        # a member past igemm_kxr2's 2^31 output elements (cout 128) / past the family's 2^31 input bytes (cout 64), and one below
        for n in (993 * 128 // cout, 992 * 128 // cout - (cout == 64)):
            rows.append(("3x3 group cout %d large member n %d" % (cout, n), [desc3x3(32, cout, 128, 128, n), desc3x3(32, cout, 9, 13, 2)]))
    # ---- the stage entry: [3x3/s2 ..., 1x1/s2 ...] of one and of two trunks
    for cout in (128, 64):
        rows += _s2_perturbations([(3, 20, 36)], cout)
        rows += _s2_perturbations([(3, 20, 36), (2, 57, 85)], cout)
        # 58 x 338 x 64 fp16 per padded image: 856 images are over the kernel's 2^31 input bytes (and under the generic kernel's 2^32)
        for n in (855, 856, 900):
            rows.append(("s2 input bytes cout %d n %d" % (cout, n), list(descs_s2([(n, 56, 336)], 64, cout))))
    for n in (400, 420):            # ... the output map's limit: 30 x 170 x 512 fp16 per padded output image
        rows.append(("s2 output bytes n %d" % n, list(descs_s2([(n, 56, 336)], 64, 512))))
    # ---- fp16 groups of the generic kernel: 1x1 convs of one and of two widths
    pairs = [desc_conv(64, cout, h, w, n, k=1, relu=relu) for (n, h, w) in GENERIC_GROUP for cout, relu in ((128, True), (256, False))]
    same = lambda: [desc_conv(64, 256, h, w, n, k=1) for (n, h, w) in GENERIC_GROUP]
    rows.append(("1x1 group of two widths", pairs))
    rows.append(("1x1 group of one width", same()))
    rows.append(("1x1 group of three", pairs[:3]))
    rows.append(("1x1 group of five", pairs + same()[:1]))
    for what, edit in {
        "cout64_member": lambda g: g.__setitem__(1, desc_conv(64, 64, 28, 30, 9, k=1)),
        "cin32_member": lambda g: g.__setitem__(1, desc_conv(32, 256, 28, 30, 9, k=1)),
        "prec2_member": lambda g: g.__setitem__(1, desc_conv(64, 256, 28, 30, 9, k=1, prec=2)),
        "3x3s1_member": lambda g: g.__setitem__(1, desc3x3(64, 256, 28, 30, 9)),
        "stem_member": lambda g: g.__setitem__(1, desc_conv(3, 256, 28, 30, 9, stem=True)),
        "res_member": lambda g: setattr(g[1], "res_hi", 1),
        "res_lo_member": lambda g: setattr(g[1], "res_lo", 1),
        "stat_member": lambda g: setattr(g[1], "stat_partial", 1),
        "pool_member": lambda g: setattr(g[1], "pool_partial", 1),
        "input_past_2^32_bytes_member": lambda g: g.__setitem__(1, desc_conv(64, 256, 126, 126, 2048, k=1)),
    }.items():
        g = same()
        edit(g)
        rows.append(("1x1 group %s" % what, g))
    return rows


def sweep():
    """[(name, [ConvDesc, ...]), ...] in the table's row order."""
    return singles() + groups()


# ------------------------------------------------------------------------------------------------------------- the answers
def evaluate(lib, rows):
    """(table [len(rows)][len(COLS)] of `lib`'s answers, crc32 of every row's descriptor bytes)."""
    from agplace_amd import _lib
    table = np.full((len(rows), len(COLS)), -1, dtype=np.int32)
    crc = np.zeros(len(rows), dtype=np.uint32)
    plan = (C.c_int32 * 8)()
    for r, (name, ds) in enumerate(rows):
        arr = (_lib.ConvDesc * len(ds))(*ds)
        crc[r] = zlib.crc32(bytes(arr))
        table[r, COL["n"]], table[r, COL["prec"]] = len(ds), ds[0].prec
        for i in range(8):
            plan[i] = 0
        rc = int(lib.agp_conv2d_tile_plan(arr, len(ds), plan))
        table[r, COL["rc"]] = rc
        table[r, COL["kernel"]:COL["kernel"] + 8] = [int(v) for v in plan] if rc == OK else 0
        if len(ds) == 1:
            bare = _copy(ds[0])
            for f in _pointers():
                setattr(bare, f, None)
            table[r, COL["stat_tiles"]] = lib.agp_conv2d_stat_tiles(C.byref(arr[0]))
            table[r, COL["pool_blocks"]] = lib.agp_conv2d_pool_blocks(C.byref(arr[0]))
            table[r, COL["stat_tiles_noptr"]] = lib.agp_conv2d_stat_tiles(C.byref(bare))
            table[r, COL["pool_blocks_noptr"]] = lib.agp_conv2d_pool_blocks(C.byref(bare))
    return table, crc


def check_coverage(table, names):
    """What the recorded table must contain for the replay to mean something."""
    t = {c: table[:, i] for c, i in COL.items()}
    ok, single = t["rc"] == OK, t["n"] == 1
    assert set(range(1, 7)) <= set(t["kernel"][ok].tolist()), "every kernel id 1..6 occurs"
    assert {OK, BADARG, UNSUPPORTED} <= set(t["rc"].tolist()), "every return code occurs"
    for col in ("stat_tiles", "stat_tiles_noptr"):
        st = ok & single & (t[col] > 0)
        for kernel in (GENERIC, DIRECT_X, KXR):
            assert (st & (t["kernel"] == kernel)).any(), (col, "with plan kernel", kernel)
        for bm in (128, 256):
            assert (st & (t["kernel"] == KXR) & (t["BM"] == bm)).any(), (col, "igemm_kxr tile height", bm)
        is3x3s1 = np.array([n.startswith("3x3s1 ") or n.startswith("cliff kxr input") for n in names])
        assert (ok & single & is3x3s1 & (t["prec"] == 3) & (t["kernel"] == GENERIC) & (t[col] == 0)).any(), \
            (col, "0 for a BF16X3 3x3/s1 conv that plans as generic")
        # the statistics buffer has one row per tile of the kernel that runs the conv
        sized = st & np.isin(t["kernel"], (GENERIC, DIRECT_X, KXR))
        bad = np.nonzero(sized & (t[col] != t["MT"]))[0]
        assert bad.size == 0, (col, "!= plan MT", [names[i] for i in bad[:5]])
    for col in ("pool_blocks", "pool_blocks_noptr"):
        assert (single & (t[col] > 0)).any(), (col, "> 0")
        is3x3s1 = np.array([n.startswith("3x3s1 ") or n.startswith("cliff kxr2") for n in names])
        assert (single & is3x3s1 & (t["prec"] == 4) & (t[col] == 0)).any(), (col, "0 for an F16 3x3/s1 conv")


def main():
    from agplace_amd import _lib
    if len(sys.argv) != 2 or not os.environ.get("AGP_HIP_LIB"):
        raise SystemExit(__doc__)
    rows = sweep()
    names = [name for name, _ in rows]
    assert len(set(names)) == len(names)
    table, crc = evaluate(_lib.load(), rows)
    check_coverage(table, names)
    np.savez_compressed(OUT, table=table, crc=crc, cols=np.array(COLS), commit=np.array(sys.argv[1]))
    print("%d rows from %s -> %s (%d bytes)" % (len(rows), _lib.LIB_PATH, OUT, os.path.getsize(OUT)))
    for rc in (OK, BADARG, UNSUPPORTED):
        print("  rc %d: %d rows" % (rc, int((table[:, COL["rc"]] == rc).sum())))
    for k in range(1, 7):
        print("  kernel %d: %d rows" % (k, int(((table[:, COL["rc"]] == OK) & (table[:, COL["kernel"]] == k)).sum())))


if __name__ == "__main__":
    main()
