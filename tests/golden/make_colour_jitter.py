"""Writes tests/golden/colour_jitter.npz: Pillow's own output for the centre crop and the colour jitter ops of small synthetic
frames, so that tests/test_colour_ref.py can hold tests/colour_ref.py to Pillow where Pillow is not installed.  The ops are
torchvision's PIL path restated with Pillow alone: ImageEnhance.Brightness / Contrast / Color, and for the hue
convert("HSV") -> H + shift (uint8 wrap) -> convert("RGB").  Needs Pillow and numpy only.  Run from the repository root:
python tests/golden/make_colour_jitter.py"""
import itertools
import os

import numpy as np
from PIL import Image, ImageEnhance

H, W = 19, 23
ALPHAS = [0.0, 0.25, 1.0, 1.0000001192092896, 1.5, 2.0]
CROPS = [(45, 72, 37), (70, 70, 37), (72, 72, 37), (38, 41, 37), (37, 37, 37), (9, 12, 4)]      # (H0, W0, c)


def frames(seed):
    """random, a ramp with a checkerboard, dark, bright, a flat grey (hue has nothing to turn), saturated primaries"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    pat = np.stack([((yy + xx) % 2) * 255, (xx * 255) // (W - 1), (yy * 255) // (H - 1)], -1).astype(np.uint8)
    prim = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255], [0, 0, 0], [255, 255, 255]],
                    dtype=np.uint8)[(yy + 3 * xx) % 8]
    return np.stack([rng.integers(0, 256, (H, W, 3), dtype=np.uint8), pat, rng.integers(0, 40, (H, W, 3), dtype=np.uint8),
                     rng.integers(215, 256, (H, W, 3), dtype=np.uint8), np.full((H, W, 3), 131, np.uint8), prim])


def records():
    """All 24 orders of the four ops, each with its own factors and hue shift; then records with ops left out."""
    rng = np.random.default_rng(7)
    shifts = [0, 1, 128, 243, 17, 200]
    recs = []
    for i, order in enumerate(itertools.permutations([1, 2, 3, 4])):
        f = rng.uniform(0.2, 1.9, 3) if i % 3 else rng.uniform(1.5, 3.0, 3) * (rng.integers(0, 2, 3) * 0.9 + 0.1)
        recs.append(list(order) + [float(np.float32(v)) for v in f] + [shifts[i % len(shifts)]])
    recs += [[0, 0, 0, 0, 1.0, 1.0, 1.0, 0], [0, 2, 0, 0, 1.0, 0.5, 1.0, 0], [4, 0, 1, 0, 1.25, 1.0, 1.0, 77],
             [3, 0, 0, 2, 1.0, 1.75, 0.0, 0], [1, 3, 4, 0, 0.0, 1.0, 2.5, 255]]
    return np.array(recs, dtype=np.float32)


def pil_jitter(frame, rec):
    im = Image.fromarray(frame, "RGB")
    for op in rec[:4].astype(int):
        if op == 1:
            im = ImageEnhance.Brightness(im).enhance(float(rec[4]))
        elif op == 2:
            im = ImageEnhance.Contrast(im).enhance(float(rec[5]))
        elif op == 3:
            im = ImageEnhance.Color(im).enhance(float(rec[6]))
        elif op == 4:
            h, s, v = im.convert("HSV").split()
            np_h = np.array(h, dtype=np.uint8)
            with np.errstate(over="ignore"):
                np_h += np.uint8(int(rec[7]))
            im = Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")
    return np.asarray(im)


def main():
    src, recs = frames(200), records()
    out = {"frames": src, "records": recs, "alphas": np.array(ALPHAS, dtype=np.float32), "crops": np.array(CROPS, dtype=np.int32)}
    # every record on frame (index mod 6)
    out["jittered"] = np.stack([pil_jitter(src[i % len(src)], r) for i, r in enumerate(recs)])
    # the conversions on a sample of colours: 4096 random ones and the 4096 corners-and-edges grid of 16 levels per channel
    rng = np.random.default_rng(201)
    lv = np.array([0, 1, 2, 17, 63, 64, 85, 127, 128, 129, 170, 191, 200, 253, 254, 255], dtype=np.uint8)
    grid = np.stack(np.meshgrid(lv, lv, lv, indexing="ij"), -1).reshape(64, 64, 3)
    cols = np.concatenate([rng.integers(0, 256, (64, 64, 3), dtype=np.uint8), grid])
    out["colours"] = cols
    out["hsv"] = np.asarray(Image.fromarray(cols, "RGB").convert("HSV"))
    out["rgb"] = np.asarray(Image.fromarray(cols, "HSV").convert("RGB"))
    out["luma"] = np.asarray(Image.fromarray(cols, "RGB").convert("L"))
    d, x = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    out["blend"] = np.stack([np.asarray(Image.blend(Image.fromarray(d, "L"), Image.fromarray(x, "L"), float(np.float32(a))))
                             for a in ALPHAS])
    for i, (h0, w0, c) in enumerate(CROPS):
        f = np.random.default_rng(300 + i).integers(0, 256, (h0, w0, 3), dtype=np.uint8)
        top, left = int(round((h0 - c) / 2.0)), int(round((w0 - c) / 2.0))
        out[f"crop_in{i}"] = f
        out[f"crop_out{i}"] = np.asarray(Image.fromarray(f, "RGB").crop((left, top, left + c, top + c)))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "colour_jitter.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
