#!/usr/bin/env python3
"""ConvNeXt-tiny trunk at the database tile size: time per kernel and of the whole trunk, with the ResNet18 trunk in mode 3 on
the same batch for context; then one training forward + backward of '2_2_2' (the opt-in training path, .eval() with gradients:
no stochastic depth) and each backward entry alone.

python tools/convnext_bench.py [--batch 64] [--size 256] [--reps 10] [--windows 5] [--json out.json] [--train-only]
                               [--precision {3,4}] [--infer-only] [--range-guard] [--pair]
--pair measures nothing of the above: it times a ConvNeXt query / database pair (Options.convnext_pair) as two separate forwards,
as pair.embed_pair with the trunks in lock-step, and as two pair.CapturedPair in flight, at 16 + 64 and at 2 + 8 (pair_leg).
--precision 4 times the inference legs in the opt-in one-product fp16 mode (Options.convnext_precision = 4); the training leg runs
in mode 3 whatever the precision and is skipped then.  --range-guard (with --precision 4 only) turns Options.convnext_range_guard on
for the measured trunks -- each eager forward then binds the module's fp16 range guard and publishes behind it -- and binds a guard's
word around the per-kernel legs, which then run the guarded twins.
Events on the launch stream around `reps` back-to-back calls, the median of `windows` such windows after a warm-up.  GMAC are
algorithmic (one multiply-accumulate per weight use, whatever the three bf16 products cost); the fraction of peak is
2 * MAC / time over the 2.5 PFLOP/s dense bf16 peak.  Weights are seeded random values (zeros would flatter the clock)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench_inputs  # noqa: E402
from agplace_amd import convnext as cnx, range_guard  # noqa: E402
from agplace_amd.options import Options  # noqa: E402
from agplace_amd.network.image_fe import ImageFE  # noqa: E402

PEAK = 2.5e15


def convnext_macs(layers, h, w):
    """Algorithmic MACs of the truncated trunk on one h x w image, and per kernel kind and stage."""
    sizes = cnx.ConvNeXt.map_sizes(h, w)
    per = {"stem": sizes[0][0] * sizes[0][1] * 96 * 48}
    for s, (hh, ww) in enumerate(sizes):
        c, px = cnx.DIMS[s], hh * ww
        per[("dwconv", c)] = px * c * 49
        per[("mlp", c)] = px * 8 * c * c
        if s > 0:
            per[("down", cnx.DIMS[s - 1])] = px * c * 4 * cnx.DIMS[s - 1]
    total = per["stem"] + sum(per[("down", cnx.DIMS[s])] for s in range(2))
    total += sum(min(layers[s], cnx.DEPTHS[s]) * (per[("dwconv", cnx.DIMS[s])] + per[("mlp", cnx.DIMS[s])]) for s in range(3))
    return total, per


def timed(fn, reps, windows):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    return statistics.median(ms), min(ms), max(ms)


def randomize(fe, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in fe.named_parameters():
            if name.endswith("layer_scale"):
                p.copy_(torch.rand(p.shape, generator=g) * 0.9 + 0.3)
            elif p.dim() > 1:
                p.copy_(torch.randn(p.shape, generator=g) / (p[0].numel() ** 0.5))
            elif name.endswith("bias"):
                p.copy_(0.2 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.5 + torch.rand(p.shape, generator=g))
    return fe


def train_leg(a, dev, x, report, rows):
    """'2_2_2' with the training switch on: the forward that keeps its tape, its backward (gradients fed into all three maps), and
    every backward entry alone at the map sizes of this input.  MACs: the backward of a GEMM costs two of them (data and weight
    gradient), the recomputed operand and hidden map are not counted."""
    n, hw = x.shape[0], x.shape[2]
    sizes = cnx.ConvNeXt.map_sizes(hw, hw)
    macs, per = convnext_macs([2, 2, 2], hw, hw)
    torch.set_grad_enabled(True)
    fe = randomize(ImageFE("convnext_tiny", "2_2_2"), 0).to(dev).eval()
    fe.fe.enable_training()
    reps = max(2, a.reps // 2)
    t_f = timed(lambda: fe(x), reps, a.windows)
    report("train fwd 2_2_2 (tape kept)", n * macs, t_f)
    maps = fe(x)[1]
    gs = [torch.randn(m.shape, device=dev).contiguous(memory_format=torch.channels_last) for m in maps]
    t_b = timed(lambda: torch.autograd.backward(maps, grad_tensors=gs, retain_graph=True), reps, a.windows)
    report("train bwd 2_2_2", 2 * n * macs, t_b)
    rows.append({"name": "train bwd / fwd", "ratio": t_b[0] / t_f[0]})
    print(f"backward / forward = {t_b[0] / t_f[0]:.2f}")
    del maps, gs
    torch.set_grad_enabled(False)
    prep, pb = fe.fe._prepared(), fe.fe._prepared_bwd()
    feats = fe.fe.features
    for s, (h, w) in enumerate(sizes):
        c = cnx.DIMS[s]
        cur, g = torch.randn(n, h, w, c, device=dev), torch.randn(n, h, w, c, device=dev)
        ws = torch.empty(cnx.workspace_bytes(n, h, w, c), dtype=torch.uint8, device=dev)
        bws = torch.empty(cnx.bwd_workspace_bytes(n, h, w, c), dtype=torch.uint8, device=dev)
        blk, p = feats[1 + 2 * s][0], prep[("blocks", s)][0]
        zeros = lambda *ps: [torch.zeros(q.shape, device=dev) for q in ps]
        cnx.dwconv_ln_fwd(cur, p, ws)
        gm = zeros(blk.block[3].weight, blk.block[3].bias, blk.block[5].weight, blk.block[5].bias, blk.layer_scale)
        report(f"mlp bwd C={c} {h}x{w}", 2 * n * per[("mlp", c)],
               timed(lambda: cnx.mlp_bwd(ws, p, pb[("blocks", s)][0], g, None, gm, bws), a.reps, a.windows))
        gd = zeros(blk.block[0].weight, blk.block[0].bias, blk.block[2].weight, blk.block[2].bias)
        report(f"ln+dwconv bwd C={c} {h}x{w}", 2 * n * per[("dwconv", c)],
               timed(lambda: cnx.dwconv_ln_bwd(cur, g, g, p, gd, bws), a.reps, a.windows))
        if s < 2:
            ln, conv = feats[2 + 2 * s]
            go = torch.randn(n, h // 2, w // 2, 2 * c, device=dev)
            gw = zeros(ln.weight, ln.bias, conv.weight, conv.bias)
            report(f"ln+downsample bwd C={c} {h}x{w}", 2 * n * per[("down", c)],
                   timed(lambda: cnx.downsample_bwd(cur, go, prep[("down", s)], pb[("down", s)], gw, bws), a.reps, a.windows))
        if s == 0:
            gst = zeros(feats[0][0].weight, feats[0][0].bias, feats[0][1].weight, feats[0][1].bias)
            report("stem bwd", n * per["stem"], timed(lambda: cnx.stem_bwd(x, g, prep["stem"], gst, bws), a.reps, a.windows))
        del cur, g, ws, bws


def timed_alternating(fns, reps, windows):
    """timed() for several legs in ONE run, their windows alternating (leg 0, leg 1, ..., leg 0, ...), so that a drift of the clock
    or of the neighbours on the host reaches every leg alike.  Returns [(median, min, max) ms per call]."""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(windows):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / reps)
    return [(statistics.median(m), min(m), max(m)) for m in ms]


def pair_leg(a, dev, rows):
    """--pair: MM and DBVanilla2D on '2_2_2' ConvNeXt trunks with Options.convnext_pair, dense voxel stand-ins, at the serving shape
    (16 panoramas 224 x 1344 + 64 tiles 256 x 256) and at batch 2 + 8, where the launches are smallest.  Per shape, windows
    alternating in one run: (a) the two separate forwards back to back on one stream (the only route without the switch), (b)
    pair.embed_pair eager (the trunks in lock-step, grouped launches), (c) two pair.CapturedPair on two streams replayed
    alternately, both in flight (time per pair); and the trunks alone, per trunk and in lock-step."""
    from agplace_amd import pair
    from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
    from agplace_amd.network_mm.mm import MM
    from oracle import nets
    prec = a.precision
    qopt = Options(mm_imgfe="convnext_tiny", mm_imgfe_layers="2_2_2", mm_imgfe_planes="96_192_384", mm_imgfe_dim=384,
                   mm_stg2fuse_dim=384, mm_voxfe_planes="64_128_384", mm_voxfe_dim=384, convnext_pair=True, convnext_precision=prec)
    dopt = Options(dbimage_fe="convnext_tiny", dbimage_fe_layers="2_2_2", features_dim=384, convnext_pair=True, convnext_precision=prec)
    torch.manual_seed(0)
    mq, mdb = MM(opt=qopt), DBVanilla2D("db", 384, opt=dopt)
    randomize(mq.image_fe.fe, 0)
    for i, e in enumerate(mdb.dbimage_fes):
        randomize(e.fe, 1 + i)
    mq, mdb = mq.to(dev).eval(), mdb.to(dev).eval()
    for bq, bd in ((16, 64), (2, 8)):
        def inputs(seed):
            qd = {k: ([t.to(dev) for t in v] if isinstance(v, list) else v.to(dev))
                  for k, v in nets.synth_query(bq, 224, 1344, qopt, seed=seed).items()}
            return qd, {"db_map": torch.randn(bd, 1, 3, 256, 256, generator=torch.Generator().manual_seed(seed + 1)).to(dev)}
        qd, dd = inputs(1)
        assert pair.can_pair(mq, mdb, qd, dd)
        want = mq(qd, mode="q"), mdb(dd, mode="db")
        got = pair.embed_pair(mq, mdb, qd, dd)
        torch.cuda.synchronize()
        same = all(torch.equal(got[0][k], want[0][k]) for k in want[0]) and torch.equal(got[1]["embedding"], want[1]["embedding"])
        if not same:
            raise SystemExit("pair.embed_pair differs from the separate forwards")
        cps = [pair.CapturedPair(mq, mdb, *inputs(10 + i), stream=torch.cuda.Stream(device=dev)) for i in range(2)]
        turn = [0]

        def captured():
            cps[turn[0] & 1].replay()
            turn[0] += 1

        def captured_window():        # (the replays run on the captures' own streams: join them before the window's end event)
            captured()
            captured()
            cur = torch.cuda.current_stream(dev)
            for cp in cps:
                cur.wait_stream(cp.stream)
        fq, fdb, x, tiles = mq.image_fe.fe, mdb.dbimage_fes[0].fe, qd["query_image"], dd["db_map"][:, 0]
        legs = [("(a) separate forwards, one stream", lambda: (mq(qd, mode="q"), mdb(dd, mode="db"))),
                ("(b) embed_pair eager, lock-step", lambda: pair.embed_pair(mq, mdb, qd, dd)),
                ("(c) two CapturedPair in flight, per pair", captured_window),
                ("trunks alone, one after the other", lambda: (fq.forward_maps(x), fdb.forward_maps(tiles))),
                ("trunks alone, lock-step", lambda: cnx.ConvNeXt.forward_maps_multi([fq, fdb], [x, tiles]))]
        res = timed_alternating([fn for _, fn in legs], max(2, a.reps // 2), a.windows)
        for cp in cps:
            cp.finish()
        for (name, _), (med, lo, hi) in zip(legs, res):
            div = 2.0 if name.startswith("(c)") else 1.0
            med, lo, hi = med / div, lo / div, hi / div
            rows.append({"name": f"pair {bq}+{bd} prec {prec}: {name}", "ms": med, "ms_min": lo, "ms_max": hi})
            print(f"pair {bq:2d} x [3,224,1344] + {bd:2d} x [3,256,256], prec {prec}: {name:42s} {med:9.3f} ms (min {lo:.3f} max {hi:.3f})")
        del cps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--train-only", action="store_true", help="skip the inference legs")
    ap.add_argument("--infer-only", action="store_true", help="skip the training leg")
    ap.add_argument("--precision", type=int, choices=(3, 4), default=3, help="ConvNeXt inference precision (Options.convnext_precision)")
    ap.add_argument("--range-guard", action="store_true", help="Options.convnext_range_guard on the measured model (--precision 4 only)")
    ap.add_argument("--pair", action="store_true", help="only the lock-step pair measurement (Options.convnext_pair): see pair_leg")
    a = ap.parse_args()
    if a.pair:
        if a.range_guard:
            ap.error("--pair with --range-guard: a guarded pair is not run in lock-step")
        torch.set_grad_enabled(False)
        rows = []
        pair_leg(a, torch.device("cuda:0"), rows)
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as f:
                json.dump({"pair": True, "reps": max(2, a.reps // 2), "windows": a.windows, "precision": a.precision, "rows": rows}, f, indent=1)
        return
    prec = a.precision
    if a.range_guard and prec != 4:
        ap.error("--range-guard needs --precision 4 (the guard covers the fp16 operands of that mode only)")
    tag = "" if prec == 3 else ", prec 4" + (", range guard" if a.range_guard else "")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    n, hw = a.batch, a.size
    x = torch.randn(n, 3, hw, hw, generator=torch.Generator().manual_seed(1)).to(dev)
    rows = []

    def report(name, macs, t):
        med, lo, hi = t
        rows.append({"name": name, "gmac": macs / 1e9, "ms": med, "ms_min": lo, "ms_max": hi, "frac_peak": 2 * macs / (med * 1e-3) / PEAK})
        print(f"{name:34s} {macs / 1e9:9.2f} GMAC {med:9.3f} ms (min {lo:.3f} max {hi:.3f})  {2 * macs / med / 1e9:8.1f} TFLOP/s "
              f"algorithmic = {100 * rows[-1]['frac_peak']:5.2f} % of peak")

    if not a.train_only:
        # ---- per kernel, at the map sizes of this input
        fe = randomize(ImageFE("convnext_tiny", "3_3_9"), 0).to(dev).eval()
        sizes = cnx.ConvNeXt.map_sizes(hw, hw)
        _, per = convnext_macs([3, 3, 9], hw, hw)
        prep = fe.fe._prepared(prec)
        if a.range_guard:       # the guarded twins: a word bound for the whole per-kernel section
            bound = range_guard.Guard("convnext_bench").bind(dev)
            bound.__enter__()
        report("stem", n * per["stem"], timed(lambda: cnx.stem_fwd(x, prep["stem"]), a.reps, a.windows))
        for s, (h, w) in enumerate(sizes):
            c = cnx.DIMS[s]
            cur = torch.randn(n, h, w, c, device=dev)
            ws = torch.empty(cnx.workspace_bytes(n, h, w, c), dtype=torch.uint8, device=dev)
            p = prep[("blocks", s)][0]
            out = torch.empty_like(cur)
            report(f"dwconv+ln C={c} {h}x{w}", n * per[("dwconv", c)], timed(lambda: cnx.dwconv_ln_fwd(cur, p, ws, prec), a.reps, a.windows))
            report(f"fused mlp C={c} {h}x{w}", n * per[("mlp", c)], timed(lambda: cnx.mlp_fwd(ws, p, cur, out, prec), a.reps, a.windows))
            if s < 2:
                d = prep[("down", s)]
                report(f"ln+downsample C={c} {h}x{w}", n * per[("down", c)], timed(lambda: cnx.downsample_fwd(cur, d, prec), a.reps, a.windows))
            del cur, ws, out
        if a.range_guard:
            bound.__exit__(None, None, None)
        # ---- whole trunks
        for layers in ("2_2_2", "3_3_9"):
            fe = randomize(ImageFE("convnext_tiny", layers, opt=Options(convnext_precision=prec, convnext_range_guard=a.range_guard)),
                           0).to(dev).eval()
            macs, _ = convnext_macs([int(v) for v in layers.split("_")], hw, hw)
            report(f"convnext_tiny {layers} trunk{tag}", n * macs, timed(lambda: fe(x), max(2, a.reps // 2), a.windows))
            del fe
        r18 = ImageFE("resnet18", "2_2_2").to(dev).eval()
        report("resnet18 2_2_2 trunk, mode 3", n * bench_inputs.resnet_gmacs("resnet18", 3, hw, hw),
               timed(lambda: r18(x, prec=3), max(2, a.reps // 2), a.windows))
    if not a.infer_only and (prec == 3 or a.train_only):
        train_leg(a, dev, x, report, rows)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump({"batch": n, "size": hw, "reps": a.reps, "windows": a.windows, **({} if prec == 3 else {"precision": prec}),
                       **({"range_guard": True} if a.range_guard else {}), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
