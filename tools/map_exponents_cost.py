"""Cost of installed map exponents (agplace_amd/map_exponents.py) on the bench step: python tools/map_exponents_cost.py
[--batch 64] [--steps 10] [--windows 5] [--exp 3].

The step of bench.py's headline (query MM + database DBVanilla2D at the default precision, bench_inputs shapes, trunks in lock-step
through agplace_amd.pair) captured into a hipGraph on a stream of its own, once with no exponents and once with exponent `--exp`
forced on every group and block-internal map of both models (the same models: the exponents are folded at capture time); each
replayed back to back, `steps` replays per window, the median of `windows` windows.  The two graphs hold the same kernels, so the
figures are expected to agree within the machine spread.  Also times one map_exponents.calibrate() call of each model on the
batch (mode-3 forward + one abs-max pass per map + one read-back; wall clock).  Prints one JSON line.  (One step in flight:
bench.py's own figure keeps two.)"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench_inputs  # noqa: E402
from agplace_amd import map_exponents, pair  # noqa: E402
from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D  # noqa: E402
from agplace_amd.network_mm.mm import MM  # noqa: E402
from agplace_amd.options import Options  # noqa: E402
from range_guard_cost import windows  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--exp", type=int, default=3)
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
    for forced in (False, True):
        for m in (modelq, modeldb):
            map_exponents.set_exponents(m, {k: args.exp if forced else 0 for k in map_exponents.get_exponents(m)})
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
        res["forced" if forced else "none"] = {"ms_per_step": round(statistics.median(w), 4), "windows": [round(x, 4) for x in w]}
        del g
    cal = {}
    for name, m, batch in (("query", modelq, data), ("db", modeldb, tiles)):
        map_exponents.clear_exponents(m)
        map_exponents.calibrate(m, [batch])            # (workspaces of the mode-3 forward exist after this one)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e = map_exponents.calibrate(m, [batch])
        cal[name + "_s"] = round(time.perf_counter() - t0, 4)
        cal[name + "_nonzero"] = sum(1 for v in e.values() if v)
    none, forced = res["none"]["ms_per_step"], res["forced"]["ms_per_step"]
    print(json.dumps({"metric": "map_exponents_cost", "batch": b, "exp": args.exp, "no_exponents": res["none"], "forced": res["forced"],
                      "delta_pct": round((forced / none - 1) * 100, 2), "calibrate_wall": cal}))


if __name__ == "__main__":
    main()
