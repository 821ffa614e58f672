"""Cost of the lidar front end (agp_sparse_build_points): python tools/lidar_front_cost.py [--batch 64]
[--points 35000 120000] [--steps 20] [--windows 5] [--level-capacity [ROWS]].

For `batch` synthetic scans of `points` points each (a ring-shaped cloud around the sensor, +-60 m, 6 m high: a few thousand voxels
per scan at quant_size 2) it times, per batch:
  front_ms   level 0 from the RAW points on the device: SparseTensor.from_points_capacity with a per-sample rotation
  parent_ms  agp_sparse_build (SparseTensor.from_coords_capacity) on the same clouds ALREADY quantised, deduplicated and rotated on
             the host -- what the library could do before the front end existed
  stream_ms  one streaming read of the points buffer on the device (a max-reduction): the floor of any pass over the points
  host_ms    the host chain that made the parent's input: numpy floor(p / quant_size), np.unique(axis=0) per scan, coords @ R
             (wall clock, one thread, once)
Device figures: HIP events around `steps` back-to-back calls, the median of `windows` windows, after a warm-up of every shape.
Prints one JSON line per scan size; ratio = front_ms / (parent_ms + stream_ms), the expectation to report against is <= 1.
For the sizes of `--forward-points` it also times the WHOLE eager `MM.forward_q` (bench shapes: 224 x 1344 panoramas) from the raw
points and from the host-made coords: from points every level has the capacity of the raw point count (feature maps, kernel
maps and their padding), which the level-0 figures do not show.
With `--level-capacity` (a row count, or no value = the next power of two above the measured voxel count) the same run also reports
  front_cap_ms          the front end with that level capacity (agp_sparse_build_points_cap), ratio_cap against the same yardstick
  overflow_ms           ONE build at capacity 64 (flag bit 2, empty result): the error path, timed once after one untimed call
  forward_points_cap_ms the whole forward_q with Options(voxel_capacity=...), and the peak device memory of each points route
                        (each route on a model of its own, the allocator's peak reset before it)."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from agplace_amd import ops  # noqa: E402
from agplace_amd.input_pipeline import z_rotation  # noqa: E402
from agplace_amd.sparse import SparseTensor  # noqa: E402


def windows(fn, steps, n):
    out = []
    s = torch.cuda.current_stream()
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(s)
        for _ in range(steps):
            fn()
        e1.record(s)
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / steps)
    return out


def synth_scans(b, p, seed):
    g = np.random.default_rng(seed)
    r = np.minimum(g.gamma(2.0, 9.0, (b, p)), 60.0)
    a = g.random((b, p)) * 2 * math.pi
    z = g.random((b, p)) * 6.0 - 2.0
    return np.stack([r * np.cos(a), r * np.sin(a), z], -1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--points", type=int, nargs="+", default=[35000, 120000])
    ap.add_argument("--quant", type=float, default=2.0)
    ap.add_argument("--forward-points", type=int, nargs="*", default=[35000])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--level-capacity", type=int, nargs="?", const=0, default=None,
                    help="rows of every level on the capped route; without a value: the next power of two above the voxel count")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    b = args.batch
    rots = torch.stack([z_rotation(math.radians(5.0 * (2.0 * i / max(b - 1, 1) - 1.0))) for i in range(b)])
    for p in args.points:
        scans = synth_scans(b, p, seed=p)
        # ---- the host chain (reference: sparse_quantize per scan, batched_coordinates, coords @ R)
        t0 = time.perf_counter()
        rows = []
        for i in range(b):
            q = np.unique(np.floor(scans[i] / args.quant), axis=0)
            rows.append(np.concatenate([np.full((len(q), 1), i, dtype=np.float32), q @ rots[i].numpy()], 1))
        host = np.concatenate(rows, 0)
        host_ms = (time.perf_counter() - t0) * 1e3
        pts = torch.from_numpy(scans.reshape(-1, 3)).to(dev)
        off = (torch.arange(b + 1, dtype=torch.int64) * p).to(dev)
        rdev = rots.to(dev)
        coords = torch.from_numpy(host).to(dev)
        feats = torch.ones((coords.shape[0], 1), device=dev)
        ws_f, ws_p = ops.Workspace(), ops.Workspace()
        sink = torch.empty((), device=dev)

        def front():
            return SparseTensor.from_points_capacity(pts, off, b, args.quant, ws_f, rdev)

        def parent():
            return SparseTensor.from_coords_capacity(feats, coords, b, ws_p)

        def stream():
            torch.amax(pts, out=sink)
        for fn in (front, parent, stream):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        sp, sc = front(), parent()
        nf, nc = int(sp.n_dev.item()), int(sc.n_dev.item())
        assert int(sp.range_flag.item()) == 0 and int(sc.range_flag.item()) == 0
        fns = [("front", front), ("parent", parent), ("stream", stream)]
        lcap, extra = None, {}
        if args.level_capacity is not None:
            lcap = args.level_capacity if args.level_capacity > 0 else 1 << int(nf).bit_length()
            ws_c, ws_o = ops.Workspace(), ops.Workspace()

            def front_cap():
                return SparseTensor.from_points_capacity(pts, off, b, args.quant, ws_c, rdev, level_capacity=lcap)

            def overflow():
                return SparseTensor.from_points_capacity(pts, off, b, args.quant, ws_o, rdev, level_capacity=64)
            for _ in range(3):
                front_cap()
            sq = front_cap()
            assert int(sq.n_dev.item()) == nf and int(sq.range_flag.item()) == 0, "the level capacity is too small for these scans"
            assert torch.equal(sq.keys[:nf], sp.keys[:nf])
            so = overflow()
            assert int(so.range_flag.item()) & 4 and int(so.n_dev.item()) == 0
            extra["overflow_ms"] = round(windows(overflow, 1, 1)[0], 4)
            fns.insert(1, ("front_cap", front_cap))
        res = {name: windows(fn, args.steps, args.windows) for name, fn in fns}
        med = {k: statistics.median(v) for k, v in res.items()}
        if lcap is not None:
            extra.update({"level_capacity": lcap, "front_cap_ms": round(med["front_cap"], 4),
                          "ratio_cap": round(med["front_cap"] / (med["parent"] + med["stream"]), 3)})
        print(json.dumps({"metric": "lidar_front_cost", "batch": b, "points_per_scan": p, "quant_size": args.quant,
                          "voxels_front": nf, "voxels_parent": nc, "host_rows": int(coords.shape[0]),
                          "front_ms": round(med["front"], 4), "parent_ms": round(med["parent"], 4), "stream_ms": round(med["stream"], 4),
                          "host_ms": round(host_ms, 1), "ratio": round(med["front"] / (med["parent"] + med["stream"]), 3), **extra,
                          "windows": {k: [round(x, 4) for x in v] for k, v in res.items()}}), flush=True)
        if lcap is not None:
            del ws_c, ws_o, sq, so
        del sp, sc                                # (the front ends' buffers go before the forwards' peaks are measured)
        ws_f.bufs.clear()
        ws_p.bufs.clear()
        if p in args.forward_points:
            import bench_inputs
            from agplace_amd.network_mm.mm import MM
            from agplace_amd.options import Options
            opt = Options(quant_size=args.quant)
            data = bench_inputs.synth_query(b, 224, 1344, opt, seed=100)
            data = {k: v.to(dev) for k, v in data.items() if k not in ("vox_levels", "voxfeatvec", "stg2voxvec", "voxvec_fuse")}
            d_pts = dict(data, points=pts, point_offsets=off, pc_rotation=rdev)
            d_crd = dict(data, coords=coords, features=feats)
            routes = [("forward_points", d_pts, opt), ("forward_coords", d_crd, opt)]
            if lcap is not None:
                routes.insert(0, ("forward_points_cap", d_pts, opt.copy(voxel_capacity=lcap)))
            fw, peak, refused = {}, {}, {}
            for name, d, o in routes:
                # a model (and so a capacity workspace) per route: the allocator's peak then belongs to that route alone
                torch.manual_seed(0)
                model = MM(opt=o).to(dev).eval()
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                try:
                    for _ in range(3):
                        model(d, mode="q")
                except RuntimeError as err:
                    # a refusal before any launch (a feature matrix of 2 GiB or more: the uncapped route at 64 x 120 k points)
                    refused[name] = str(err)
                    del model
                    continue
                torch.cuda.synchronize()
                fw[name] = windows(lambda: model(d, mode="q"), max(args.steps // 4, 1), args.windows)
                assert model.voxel_coords_in_range()
                peak[name] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
                del model
            print(json.dumps({"metric": "lidar_forward_q", "batch": b, "points_per_scan": p, "capacity_points": int(pts.shape[0]),
                              "capacity_coords": int(coords.shape[0]), "level_capacity": lcap,
                              **{k + "_ms": round(statistics.median(v), 3) for k, v in fw.items()},
                              "gpu_mem_peak_gb": peak, "refused": refused,
                              "windows": {k: [round(x, 3) for x in v] for k, v in fw.items()}}), flush=True)
            del data, d_pts, d_crd
        del ws_f, ws_p, pts, coords, feats


if __name__ == "__main__":
    main()
