"""Cost of the fp32 <-> split-bf16 bridge of MM's ConvNeXt training: python tools/mm_convnext_train_cost.py [--steps 50]
[--windows 5] [--mm-steps 3] [--no-mm].

At the bench's last-map shape [16, 14, 84, 384] (HIP events, a warm-up, the median of `windows` windows with minimum and maximum):
  1. ops.bcast_add_f32 (agp_bcast_add_f32_fwd) against ops.pack_f32 + ops.bcast_add, the sequence it replaces in training;
  2. ops.pool_f32_bwd with all three terms (agp_pool_f32_bwd) against SplitMap.to_f32 + ops.gem_f32_bwd + the two adds.
The comparison sequences are existing ops of this tree.  Beside each time: the bytes the route must move, computed from the shape
(reads + writes of every pass), and the rate that gives.
  3. one whole training step (forward, loss, backward) of MM(mm_imgfe='convnext_tiny', layers 2_2_2, convnext_train=True) in
     .train() on 16 x [3, 224, 1344] with the dense voxel stand-ins, with Options.fcode_wide off (its three FCODE(384) blocks on
     the any-width route) and on (on agp_fcode_wide_fwd_traj / agp_fcode_wide_bwd); the same seed, so the same weights.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from agplace_amd import ops  # noqa: E402
from agplace_amd.options import Options  # noqa: E402

SHAPE = (16, 14, 84, 384)


def window_us(fn, steps, windows):
    out = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1000.0 / steps)
    return statistics.median(out), min(out), max(out)


def timed(fn, steps, windows, nbytes=None):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    med, lo, hi = window_us(fn, steps, windows)
    row = {"us": round(med, 2), "min_us": round(lo, 2), "max_us": round(hi, 2)}
    if nbytes is not None:
        row.update(bytes=nbytes, gb_per_s=round(nbytes / med / 1e3, 1))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--mm-steps", type=int, default=3)
    ap.add_argument("--no-mm", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, h, w, c = SHAPE
    el = n * h * w * c
    res = {"tool": "mm_convnext_train_cost", "device": torch.cuda.get_device_name(0), "map": list(SHAPE)}
    torch.manual_seed(0)
    x = torch.randn(n, h, w, c, device=dev) * 0.7 + 0.3
    xl = x.permute(0, 3, 1, 2)                       # the trunk's exported [n,C,h,w] view
    vec = torch.randn(n, c, device=dev)
    with torch.no_grad():
        # ---- 1. forward bridge
        out = ops.SplitMap.alloc(n, h, w, c, 1, 3, dev)
        mid = ops.SplitMap.alloc(n, h, w, c, 1, 3, dev)
        one = timed(lambda: ops.bcast_add_f32(x, vec, out), args.steps, args.windows, el * (4 + 4))
        got = out.to_f32().clone()

        def pack_then_add():
            ops.pack_f32(xl, c, 1, 3, out=mid)
            ops.bcast_add(mid, vec, out)
        seq = timed(pack_then_add, args.steps, args.windows, el * (4 + 4) + el * (4 + 4))
        want = out.to_f32()
        res["bcast_add_f32"] = {"one_pass": one, "pack_f32+bcast_add": seq,
                                "outputs_rel_l2": float((got.double() - want.double()).norm() / want.double().norm())}
        # ---- 2. backward bridge
        p = torch.tensor([3.0], device=dev)
        mean, y = ops.pool_f32(xl, p, want_mean=True, want_gem=True)
        gmean, ggem = torch.randn(n, c, device=dev), torch.randn(n, c, device=dev)
        base = ops.SplitMap.alloc(n, h, w, c, 1, 3, dev)
        ops.bcast_add_f32(torch.randn(n, h, w, c, device=dev), torch.zeros(n, c, device=dev), base)
        gp = ops.new_gp(dev)
        one = timed(lambda: ops.pool_f32_bwd(x, gmean=gmean, ggem=ggem, gem_y=y, p=p, base=base, gp=gp), args.steps, args.windows,
                    el * (4 + 4 + 4))
        got = ops.pool_f32_bwd(x, gmean=gmean, ggem=ggem, gem_y=y, p=p, base=base, gp=gp)
        inv = 1.0 / (h * w)

        def per_op():
            b32 = base.to_f32()                                  # split planes -> fp32
            gx, _ = ops.gem_f32_bwd(xl, p, y, ggem)              # x -> dGeM/dx (and dL/dp)
            return (b32 + gx) + (gmean * inv)[:, :, None, None]  # the two adds
        seq = timed(per_op, args.steps, args.windows, el * ((4 + 4) + (4 + 4) + (4 + 4 + 4) + (4 + 4)))
        want = per_op().permute(0, 2, 3, 1)
        res["pool_f32_bwd"] = {"one_pass": one, "to_f32+gem_f32_bwd+adds": seq,
                               "outputs_rel_l2": float((got.double() - want.double()).norm() / want.double().norm())}
    # ---- 3. a whole training step
    if not args.no_mm:
        from agplace_amd.network_mm.mm import MM
        from bench_inputs import synth_query
        data, G = None, torch.randn(16, 384, device=dev)
        res["mm_train_step"] = {"layers": "2_2_2", "image": [16, 3, 224, 1344], "voxel": "dense stand-ins"}
        for name, switch in (("fcode_wide_off", False), ("fcode_wide_on", True)):
            opt = Options(mm_imgfe="convnext_tiny", mm_imgfe_layers="2_2_2", mm_imgfe_planes="96_192_384", mm_imgfe_dim=384,
                          mm_stg2fuse_dim=384, mm_voxfe_planes="64_128_384", mm_voxfe_dim=384, convnext_train=True, fcode_wide=switch)
            torch.manual_seed(2)
            model = MM(opt=opt).to(dev).train()
            if data is None:
                data = {k: ([t.to(dev) for t in v] if isinstance(v, list) else v.to(dev))
                        for k, v in synth_query(16, 224, 1344, opt, seed=1).items()}

            def step():
                for q in model.parameters():
                    q.grad = None
                (model(data, mode="q")["embedding"] * G).sum().backward()
            row = timed(step, args.mm_steps, args.windows)
            res["mm_train_step"][name] = {"ms": round(row["us"] / 1e3, 2), "min_ms": round(row["min_us"] / 1e3, 2),
                                          "max_ms": round(row["max_us"] / 1e3, 2)}
            del model
    print(json.dumps(res))


if __name__ == "__main__":
    main()
