#!/usr/bin/env python3
"""The layer-1 fused block inside a traced bench step: per-step sum of the `fblock64_kernel` launches.

rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python3 bench.py --gpus 1 --steps 40 --warmup 5
python tools/fblock_step_trace.py DIR [--per-step 2] [--skip 8] [--stats OUT.csv]
Prints the number of steps and the median / min / max of the per-step sum (us); --stats writes the per-kernel totals of the
whole trace in the layout of profiles/r06_bench_kernel_stats.csv."""
import argparse
import csv
import glob
import os
import statistics


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--per-step", type=int, default=2, help="fblock64 launches of one step")
    ap.add_argument("--skip", type=int, default=8, help="leading steps left out (eager warm-up, capture)")
    ap.add_argument("--stats", default=None)
    a = ap.parse_args()
    files = sorted(glob.glob(os.path.join(a.dir, "**", "*kernel_trace.csv"), recursive=True))
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            rows += [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(fh)]
    fb = sorted((s, e - s) for name, s, e in rows if "fblock64_kernel" in name)
    steps = [sum(d for _, d in fb[i:i + a.per_step]) / 1e3 for i in range(0, len(fb) - a.per_step + 1, a.per_step)][a.skip:]
    print("fblock64 launches %d, steps counted %d: per-step sum median %.1f us, min %.1f, max %.1f" %
          (len(fb), len(steps), statistics.median(steps), min(steps), max(steps)))
    if a.stats:
        by = {}
        for name, s, e in rows:
            by.setdefault(name, []).append(e - s)
        total = sum(sum(v) for v in by.values())
        with open(a.stats, "w", newline="") as fh:
            w = csv.writer(fh, quoting=csv.QUOTE_NONNUMERIC)
            w.writerow(["Name", "Calls", "TotalDurationNs", "AverageNs", "Percentage", "MinNs", "MaxNs", "StdDev"])
            for name, v in sorted(by.items(), key=lambda kv: -sum(kv[1])):
                w.writerow([name, len(v), sum(v), round(sum(v) / len(v), 3), round(100.0 * sum(v) / total, 2), min(v), max(v),
                            round(statistics.pstdev(v), 3)])


if __name__ == "__main__":
    main()
