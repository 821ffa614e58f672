"""Cost of the fp16 range guard (Options.fp16_range_guard) on the bench step: python tools/range_guard_cost.py [--batch 64]
[--steps 10] [--windows 5].

The step of bench.py's headline (query MM + database DBVanilla2D at the default precision, bench_inputs shapes, trunks in lock-step
through agplace_amd.pair) captured into a hipGraph on a stream of its own, once with the guard off and once with it on (the same
models: the switch is read at capture time); each replayed back to back, `steps` replays per window, the median of `windows`
windows.  Also times agplace_amd.pair.CapturedPair.replay() with the guard on (its poll of the pinned mirrors every
`poll_every` replays included).  Prints one JSON line.  (One step in flight: bench.py's own figure keeps two.)"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench_inputs  # noqa: E402
from agplace_amd import pair  # noqa: E402
from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D  # noqa: E402
from agplace_amd.network_mm.mm import MM  # noqa: E402
from agplace_amd.options import Options  # noqa: E402


def windows(fn, steps, n, stream):
    """ms per call of fn, timed by events on `stream` (the stream fn's work runs on)."""
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(stream)
        for _ in range(steps):
            fn()
        e1.record(stream)
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / steps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    torch.manual_seed(0)
    opt = Options()
    modelq = MM(opt=opt).to(dev).eval()
    modeldb = DBVanilla2D("db", opt.features_dim, opt=opt).to(dev).eval()
    b = args.batch
    data = bench_inputs.synth_query(b, 224, 1344, opt, seed=100)
    data = {k: ([t.to(dev) for t in v] if isinstance(v, list) else v.to(dev)) for k, v in data.items()}
    tiles = {"db_map": torch.randn(b, 1, 3, 224, 224, generator=torch.Generator().manual_seed(200)).to(dev)}

    res = {}
    for guard in (False, True):
        opt.fp16_range_guard = guard
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                pair.embed_pair(modelq, modeldb, data, tiles)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
            pair.embed_pair(modelq, modeldb, data, tiles)
        torch.cuda.synchronize()

        def step():
            with torch.cuda.stream(s):
                g.replay()
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        w = windows(step, args.steps, args.windows, s)
        res["on" if guard else "off"] = {"ms_per_step": round(statistics.median(w), 4), "windows": [round(x, 4) for x in w]}
        del g
    opt.fp16_range_guard = True
    cp = pair.CapturedPair(modelq, modeldb, data, tiles)
    for _ in range(3):
        cp.replay()
    torch.cuda.synchronize()
    w = windows(cp.replay, args.steps, args.windows, cp.stream)
    cp.finish()
    assert modelq.fp16_range_ok() and modeldb.fp16_range_ok(), "the bench inputs must report clean"
    off, on = res["off"]["ms_per_step"], res["on"]["ms_per_step"]
    print(json.dumps({"metric": "range_guard_cost", "batch": b, "guard_off": res["off"], "guard_on": res["on"],
                      "overhead_pct": round((on / off - 1) * 100, 2), "target_pct": 3.0,
                      "captured_pair_ms_per_replay_guard_on": round(statistics.median(w), 4)}))


if __name__ == "__main__":
    main()
