"""Cost of FCODE(384) by route: python tools/fcode_width_cost.py [--steps 50] [--windows 5] [--mm-steps 10] [--no-mm] [--dopri5] [--train].

First timing: one FCODE(384) solve (relu, default-init weights, inference) for b = 16 and 64 and euler / 0.1, rk4 / 0.25, through
the one-launch kernel (ops.fcode_wide, csrc/fusion_wide.hip) and through FCODE._forward_any_width -- called directly: it is
the route every width other than 256 took before the kernel existed, a sequence of agp_linear_fwd / agp_wsum_fwd launches.
Each route is captured into a hipGraph and replayed `steps` times between two HIP events; the median of `windows` windows with
their minimum and maximum, and the number of kernel launches the route records (`counted_launches`: the calls of agp_fcode_wide_fwd,
agp_linear_fwd and agp_wsum_fwd at the C ABI during the capture -- all of an FCODE route, the vector path's share of an MM forward).

Second timing: the whole MM forward on the ConvNeXt-tiny trunk (layers 2_2_2, image [16, 3, 224, 1344], dense voxel stand-ins),
captured and replayed, with FCODE(384) on the one-launch kernel and -- the same model -- on the any-width route.

--dopri5 adds a third timing: one adaptive solve (odeint_method = 'dopri5', relu, tol = 1e-3, default-init weights, inference) for
b = 16 and 64 at 256 columns (agp_fcode_adaptive_fwd) and at 384 (agp_fcode_adaptive_wide_fwd), captured and replayed, the median of
its windows, with the attempted-step and f-evaluation counts of the solve beside the time: the kernel is latency-bound, its time
is the step count times the cost of an attempted step.

--train adds a fourth timing: forward + backward of one FCODE(384) block (relu, default-init weights) with the gradients of x,
weight and bias wanted, for b = 16 and 64 and euler / 0.1, rk4 / 0.25, captured and replayed like the others: with
Options.fcode_wide (agp_fcode_wide_fwd_traj, then agp_fcode_wide_bwd: the state kernel, the weight gradient's GEMM and the column
sum) and without it (the any-width route: agp_linear_fwd / agp_wsum_fwd forward, autograd's agp_linear_bwd and weighted sums
behind them).  Both blocks hold the same weights; `entry_calls` counts calls at the C ABI, and an entry of a backward is more than
one kernel.  `new_not_slower` is the condition the switch was built under, per cell.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from agplace_amd import _lib, autograd_ops, ops  # noqa: E402
from agplace_amd.network_mm.ffns import FCODE  # noqa: E402
from agplace_amd.options import Options  # noqa: E402

COUNTED = ("agp_fcode_wide_fwd", "agp_linear_fwd", "agp_wsum_fwd", "agp_fcode_adaptive_fwd", "agp_fcode_adaptive_wide_fwd",
           "agp_fcode_wide_fwd_traj", "agp_fcode_wide_bwd", "agp_linear_bwd")


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


class LaunchCount:
    """Counts the calls of the vector-path entries at the C ABI (one kernel launch each) while active."""

    def __enter__(self):
        self.lib, self.n, self.saved = _lib.load(), {k: 0 for k in COUNTED}, {}
        for name in COUNTED:
            fn = getattr(self.lib, name)
            self.saved[name] = fn

            def counted(*a, _fn=fn, _name=name):
                self.n[_name] += 1
                return _fn(*a)
            setattr(self.lib, name, counted)
        return self

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(self.lib, name, fn)


def captured(fn):
    """(graph, launches recorded): one eager warm-up on a side stream, then the capture."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with LaunchCount() as lc:
        with torch.cuda.graph(graph):
            keep = fn()
    return graph, keep, dict(lc.n)


def timed(fn, steps, windows):
    graph, keep, launches = captured(fn)
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    med, lo, hi = window_us(graph.replay, steps, windows)
    return {"us": round(med, 2), "min_us": round(lo, 2), "max_us": round(hi, 2), "counted_launches": sum(launches.values()),
            "launches_by_entry": {k: v for k, v in launches.items() if v}}, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--mm-steps", type=int, default=10)
    ap.add_argument("--no-mm", action="store_true")
    ap.add_argument("--dopri5", action="store_true")
    ap.add_argument("--train", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    d = ops.FCODE_WIDE_DIM
    res = {"tool": "fcode_width_cost", "device": torch.cuda.get_device_name(0), "dim": d, "act": "relu", "fcode": {}}
    with torch.no_grad():
        for b in (16, 64):
            torch.manual_seed(0)
            x = torch.randn(b, d, device=dev)
            row = {}
            for name, opt in (("euler/0.1", Options(odeint_method="euler", odeint_size=0.1)),
                              ("rk4/0.25", Options(odeint_method="rk4", odeint_size=0.25))):
                torch.manual_seed(1)
                m = FCODE(d, "relu", opt=opt).to(dev)
                wide, yw = timed(lambda: m(x), args.steps, args.windows)
                anyw, ya = timed(lambda: m._forward_any_width(x, None, None), args.steps, args.windows)
                assert wide["launches_by_entry"] == {"agp_fcode_wide_fwd": 1}, wide
                row[name] = {"one_launch": wide, "any_width": anyw,
                             "outputs_rel_l2": float((yw.double() - ya.double()).norm() / ya.double().norm())}
            res["fcode"][f"b{b}"] = row
        if args.dopri5:
            res["dopri5"] = {"act": "relu", "tol": 1e-3}
            for width in (256, d):
                for b in (16, 64):
                    torch.manual_seed(0)
                    x = torch.randn(b, width, device=dev)
                    torch.manual_seed(1)
                    m = FCODE(width, "relu", opt=Options(odeint_method="dopri5", tol=1e-3)).to(dev)
                    fc = m.func.func.fc      # (through the autograd layer: FCODE.forward refuses dopri5 at 384 columns)
                    t, _ = timed(lambda: autograd_ops.FCODEFn.apply(x, fc.weight, fc.bias, m, None, None), args.steps, args.windows)
                    st = m.solver_stats()
                    t.update(attempted=st["attempted"], rejected=st["rejected"], f_evals=st["f_evals"])
                    res["dopri5"][f"d{width}_b{b}"] = t
        if not args.no_mm:
            from agplace_amd.network_mm.mm import MM
            from bench_inputs import synth_query
            opt = Options(mm_imgfe="convnext_tiny", mm_imgfe_layers="2_2_2", mm_imgfe_planes="96_192_384", mm_imgfe_dim=384,
                          mm_stg2fuse_dim=384, mm_voxfe_planes="64_128_384", mm_voxfe_dim=384)
            torch.manual_seed(2)
            model = MM(opt=opt).to(dev).eval()
            data = {k: ([t.to(dev) for t in v] if isinstance(v, list) else v.to(dev)) for k, v in synth_query(16, 224, 1344, opt, seed=1).items()}
            one, _ = timed(lambda: model(data, mode="q"), args.mm_steps, args.windows)
            plain = FCODE.forward
            FCODE.forward = lambda self, x, add1=None, add2=None: self._forward_any_width(x, add1, add2)
            try:
                anyw, _ = timed(lambda: model(data, mode="q"), args.mm_steps, args.windows)
            finally:
                FCODE.forward = plain
            res["mm_forward"] = {"layers": "2_2_2", "image": [16, 3, 224, 1344], "voxel": "dense stand-ins",
                                 "fcode_one_launch": one, "fcode_any_width": anyw}
    if args.train:
        res["train"] = {"act": "relu", "gradients": ["x", "weight", "bias"]}
        for b in (16, 64):
            torch.manual_seed(0)
            x = torch.randn(b, d, device=dev, requires_grad=True)
            gy = torch.randn(b, d, device=dev)
            row = {}
            for name, kw in (("euler/0.1", dict(odeint_method="euler", odeint_size=0.1)),
                             ("rk4/0.25", dict(odeint_method="rk4", odeint_size=0.25))):
                cell, grads = {}, {}
                for route, switch in (("fcode_wide", True), ("any_width", False)):
                    torch.manual_seed(1)
                    m = FCODE(d, "relu", opt=Options(fcode_wide=switch, **kw)).to(dev)
                    fc = m.func.func.fc
                    t, grads[route] = timed(lambda: torch.autograd.grad(m(x), (x, fc.weight, fc.bias), gy), args.steps, args.windows)
                    t["entry_calls"] = t.pop("counted_launches")
                    t["calls_by_entry"] = t.pop("launches_by_entry")
                    cell[route] = t
                assert set(cell["fcode_wide"]["calls_by_entry"]) == {"agp_fcode_wide_fwd_traj", "agp_fcode_wide_bwd"}, cell
                cell["gradients_rel_l2"] = [float((p.double() - q.double()).norm() / q.double().norm())
                                            for p, q in zip(grads["fcode_wide"], grads["any_width"])]
                cell["new_not_slower"] = cell["fcode_wide"]["us"] <= cell["any_width"]["us"]
                row[name] = cell
            res["train"][f"b{b}"] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()
