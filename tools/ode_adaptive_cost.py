"""Cost of one FCODE solve by method: python tools/ode_adaptive_cost.py [--steps 50] [--windows 5] [--tol 1e-3]
[--methods euler/0.1,rk4/0.25,dopri5,bosh3] [--dims 256,384].

The adaptive dopri5 and bosh3 solves (ONE persistent workgroup for the whole batch: torchdiffeq's step control couples all rows,
see csrc/fusion_adaptive.hip) beside the fixed-grid euler / 0.1 and rk4 / 0.25 solves (one workgroup per 16 rows), relu,
default-init weights, b = 16 and 64, at 256 columns ("rows") and at 384 columns with Options.fcode_wide ("rows_384").
--methods restricts the rows, so that the same tool runs against a library built before a method existed (AGP_HIP_LIB).  Each solve is captured into a hipGraph (inference form: no trajectory) and replayed
`steps` times between two HIP events; the median of `windows` windows.  With the attempted steps and f-evaluations per solve,
so that the cost per f-evaluation of the one-workgroup design shows next to the 16-rows-per-workgroup kernel's.  Also the
training pair (forward with trajectory + backward) of every method, timed eagerly (it allocates).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from agplace_amd import ops  # noqa: E402
from agplace_amd.network_mm.ffns import FCODE  # noqa: E402
from agplace_amd.options import Options  # noqa: E402


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


def captured(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = fn()
    return graph, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--tol", type=float, default=1e-3)
    ap.add_argument("--methods", default="euler/0.1,rk4/0.25,dopri5,bosh3")
    ap.add_argument("--dims", default="256,384")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"tool": "ode_adaptive_cost", "device": torch.cuda.get_device_name(0), "tol": args.tol, "act": "relu"}
    for dim in (int(v) for v in args.dims.split(",")):
        res["rows" if dim == 256 else f"rows_{dim}"] = {f"b{b}": rows(args, dev, dim, b) for b in (16, 64)}
    print(json.dumps(res))


def rows(args, dev, dim, b):
    """The rows of one width and batch size."""
    torch.manual_seed(0)
    x = torch.randn(b, dim, device=dev)
    G = torch.randn(b, dim, device=dev)
    row = {}
    wide = dim == ops.FCODE_WIDE_DIM      # the one-launch kernels of 384 columns are behind Options.fcode_wide
    for name, opt in (("euler/0.1", Options(odeint_method="euler", odeint_size=0.1, fcode_wide=wide)),
                      ("rk4/0.25", Options(odeint_method="rk4", odeint_size=0.25, fcode_wide=wide)),
                      ("dopri5", Options(odeint_method="dopri5", tol=args.tol, fcode_wide=wide)),
                      ("bosh3", Options(odeint_method="bosh3", tol=args.tol, fcode_wide=wide, odeint_adaptive_family=True))):
        if name not in args.methods.split(","):
            continue
        torch.manual_seed(1)
        m = FCODE(dim, "relu", opt=opt).to(dev)
        lw = m._prep.get()
        if m.adaptive:
            def solve():
                return ops.fcode_adaptive(x, lw, "relu", m.method, m.tol, m.max_steps)
        elif wide:
            def solve():
                return ops.fcode_wide(x, lw, "relu", m.method, m.dts)
        else:
            def solve():
                return ops.fcode(x, lw, "relu", m.method, m.dts)
        with torch.no_grad():
            graph, keep = captured(solve)
            for _ in range(5):
                graph.replay()
            torch.cuda.synchronize()
            med, lo, hi = window_us(graph.replay, args.steps, args.windows)
        if m.adaptive:
            st = ops.ode_stats(keep[1])
            fe, att = st["f_evals"], st["attempted"]
        else:
            fe = len(m.dts) * {"euler": 1, "rk4": 4}[m.method]
            att = len(m.dts)
        xg = x.clone().requires_grad_(True)

        def train():
            for p in m.parameters():
                p.grad = None
            (m(xg) * G).sum().backward()
        for _ in range(3):
            train()
        torch.cuda.synchronize()
        tmed, _, _ = window_us(train, max(5, args.steps // 5), args.windows)
        row[name] = {"solve_us": round(med, 2), "min_us": round(lo, 2), "max_us": round(hi, 2), "attempted_steps": att,
                     "f_evals": fe, "us_per_f_eval": round(med / fe, 3), "train_fwd_bwd_us_eager": round(tmed, 1)}
    return row


if __name__ == "__main__":
    main()
