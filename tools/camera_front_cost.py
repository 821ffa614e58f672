"""Cost of the camera front end (csrc/camera.hip): python tools/camera_front_cost.py [--batch 64] [--ncam 6]
[--frame 256 455] [--size 192] [--steps 200] [--windows 5] [--timeout 240].

For `batch` x `ncam` synthetic decoded frames (uint8 HWC, random pixels: the kernels' time does not depend on the values) it
measures four things, each in a child process of its own under its own time limit (a measurement that hangs or fails costs that
figure, not the others):
  fused     ops.pack_cameras_resized_u8: frames -> resize -> normalise -> the stem's NHWC4 map, one launch
  two_pass  ops.resize_cameras_u8 followed by ops.pack_cameras_u8 on its output
  pack      ops.pack_cameras_u8 alone on tiles that are already resized: the pass the library had before the front end
  host      Pillow's Image.resize(BILINEAR) of the same frames on the host (if Pillow imports): wall clock of one pass over all
            frames on a thread pool of `--host-threads` threads (Pillow releases the GIL while it resamples)
Opt-in legs of the KITTI-360 chain (nobody has measured them yet; figures go to profiles/README.md when someone does):
  --crop C    crop_fused  ops.pack_cameras_resized_u8(..., crop=C): CenterCrop(C) + Resize(size) + normalise + pack, one launch
  --jitter J  jitter_pack ops.pack_cameras_jittered_u8 on the resized tiles with ColorJitter(J, J, J, hue=min(0.5, J)) records
              (zero + statistics + apply launches); jitter_bcs: the same without the hue op (its HSV round trip is the fp64 part)
Device figures: HIP events around `steps` back-to-back calls, the median of `windows` windows, after a warm-up; the map is the
fp16 plane of precision mode 4.  Prints one JSON line per measurement and a summary line with the fused kernel's byte floor
(frames in + packed map out) / --hbm-tbs."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def windows(fn, steps, n):
    import torch
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


def measure_device(which, args):
    import torch
    from agplace_amd import ops
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    H0, W0 = args.frame
    h, w = ops.resized_size(H0, W0, args.size)
    g = torch.Generator().manual_seed(0)
    frames = torch.randint(0, 256, (args.batch, args.ncam, H0, W0, 3), generator=g, dtype=torch.uint8).to(dev)
    out = ops.SplitMap.alloc(args.batch, h, args.ncam * w, 4, 3, 4, dev)
    ops.prepare_resize(H0, W0, h, w, dev)
    tiles = ops.resize_cameras_u8(frames, (h, w))
    if which == "crop_fused":
        ch, cw = ops.resized_size(args.crop, args.crop, args.size)
        cout = ops.SplitMap.alloc(args.batch, ch, args.ncam * cw, 4, 3, 4, dev)
        ops.prepare_resize(args.crop, args.crop, ch, cw, dev)
        h, w = ch, cw
    if which in ("jitter_pack", "jitter_bcs"):
        from agplace_amd import input_pipeline
        j = args.jitter
        recs = input_pipeline.color_jitter(args.batch * args.ncam, j, j, j, min(0.5, j) if which == "jitter_pack" else 0.0,
                                           generator=torch.Generator().manual_seed(1)).to(dev)
    fns = {"fused": lambda: ops.pack_cameras_resized_u8(frames, (h, w), 4, out=out),
           "crop_fused": lambda: ops.pack_cameras_resized_u8(frames, args.size, 4, out=cout, crop=args.crop),
           "jitter_pack": lambda: ops.pack_cameras_jittered_u8(tiles, recs, 4, out=out),
           "jitter_bcs": lambda: ops.pack_cameras_jittered_u8(tiles, recs, 4, out=out),
           "two_pass": lambda: ops.pack_cameras_u8(ops.resize_cameras_u8(frames, (h, w)), 4, out=out),
           "pack": lambda: ops.pack_cameras_u8(tiles, 4, out=out)}
    fn = fns[which]
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    res = windows(fn, args.steps, args.windows)
    return {"ms": round(statistics.median(res), 4), "windows": [round(x, 4) for x in res], "out_hw": [h, args.ncam * w]}


def measure_host(args):
    try:
        from PIL import Image
    except ImportError:
        return {"ms": None, "note": "Pillow is not installed here"}
    from concurrent.futures import ThreadPoolExecutor
    import numpy as np
    from agplace_amd import ops
    H0, W0 = args.frame
    h, w = ops.resized_size(H0, W0, args.size)
    rng = np.random.default_rng(0)
    imgs = [Image.fromarray(rng.integers(0, 256, (H0, W0, 3), dtype=np.uint8)) for _ in range(args.batch * args.ncam)]

    def one(im):
        return im.resize((w, h), Image.BILINEAR)
    res = []
    with ThreadPoolExecutor(args.host_threads) as pool:
        list(pool.map(one, imgs))                     # warm-up
        for _ in range(args.windows):
            t0 = time.perf_counter()
            list(pool.map(one, imgs))
            res.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    for im in imgs[:32]:
        one(im)
    per_frame_1t = (time.perf_counter() - t0) * 1e3 / 32
    return {"ms": round(statistics.median(res), 3), "windows": [round(x, 3) for x in res], "threads": args.host_threads,
            "frames": len(imgs), "ms_per_frame_one_thread": round(per_frame_1t, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--ncam", type=int, default=6)
    ap.add_argument("--frame", type=int, nargs=2, default=[256, 455])
    ap.add_argument("--size", type=int, default=192)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--timeout", type=float, default=240.0, help="seconds per measurement")
    ap.add_argument("--hbm-tbs", type=float, default=6.3, help="achievable HBM rate the byte floor is quoted at")
    ap.add_argument("--crop", type=int, default=None, help="also time CenterCrop(C) in front of the resize")
    ap.add_argument("--jitter", type=float, default=None, help="also time ColorJitter(J, J, J, min(0.5, J)) on the resized tiles")
    ap.add_argument("--only", choices=["fused", "two_pass", "pack", "host", "crop_fused", "jitter_pack", "jitter_bcs"], help="(internal) run ONE measurement in this process")
    args = ap.parse_args()
    if args.only:
        res = measure_host(args) if args.only == "host" else measure_device(args.only, args)
        print(json.dumps(dict({"metric": "camera_front_cost", "what": args.only}, **res)), flush=True)
        return 0
    got = {}
    extra = (["crop_fused"] if args.crop else []) + (["jitter_pack", "jitter_bcs"] if args.jitter else [])
    for what in ["fused", "two_pass", "pack", "host"] + extra:
        cmd = [sys.executable, os.path.abspath(__file__), "--only", what] + [a for a in sys.argv[1:]]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print(json.dumps({"metric": "camera_front_cost", "what": what, "error": f"time limit of {args.timeout} s"}), flush=True)
            return 1                                   # nothing more is started behind a measurement that hung
        line = next((ln for ln in p.stdout.splitlines() if ln.startswith("{")), None)
        if p.returncode != 0 or line is None:
            print(json.dumps({"metric": "camera_front_cost", "what": what, "error": f"exit {p.returncode}",
                              "stderr": p.stderr[-400:]}), flush=True)
            return 1
        print(line, flush=True)
        got[what] = json.loads(line)
    H0, W0 = args.frame
    h, wt = got["fused"]["out_hw"]
    bytes_in = args.batch * args.ncam * H0 * W0 * 3
    bytes_out = args.batch * h * wt * 4 * 2
    floor_ms = (bytes_in + bytes_out) / (args.hbm_tbs * 1e12) * 1e3
    print(json.dumps({"metric": "camera_front_summary", "batch": args.batch, "ncam": args.ncam, "frame": [H0, W0], "out_hw": [h, wt],
                      "fused_ms": got["fused"]["ms"], "two_pass_ms": got["two_pass"]["ms"], "pack_ms": got["pack"]["ms"],
                      "host_ms": got["host"]["ms"], "bytes_in": bytes_in, "bytes_out": bytes_out, "hbm_tbs": args.hbm_tbs,
                      "byte_floor_ms": round(floor_ms, 4), "fused_over_floor": round(got["fused"]["ms"] / floor_ms, 2),
                      "fused_over_two_pass": round(got["fused"]["ms"] / got["two_pass"]["ms"], 3),
                      **{w + "_ms": got[w]["ms"] for w in extra}}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
