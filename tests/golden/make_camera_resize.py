"""Writes tests/golden/camera_resize.npz: Pillow's own output (Image.resize(..., BILINEAR), what torchvision's Resize does to a
PIL image) for small synthetic frames, so that tests/test_camera_ref.py can hold tests/camera_ref.py to Pillow where Pillow is
not installed.  Needs Pillow and numpy only.  Run from the repository root:  python tests/golden/make_camera_resize.py"""
import os

import numpy as np
from PIL import Image

# (H0, W0, h, w): the small geometries of tests/test_camera_ref.py (the 256x455 and 300x300 frames stay out: size)
GEOMETRIES = [(37, 53, 16, 22), (20, 31, 20, 17), (9, 9, 9, 9), (16, 24, 32, 48), (5, 64, 3, 38), (64, 64, 16, 16), (8, 8, 32, 32),
              (70, 130, 33, 67)]


def frames(h0, w0, seed):
    """random, patterned (a 1-pixel checkerboard over a ramp: the worst case for a resampler's rounding), all 0, all 255"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h0, 0:w0]
    pat = np.stack([((yy + xx) % 2) * 255, (xx * 255) // max(w0 - 1, 1), (yy * 255) // max(h0 - 1, 1)], -1).astype(np.uint8)
    return np.stack([rng.integers(0, 256, (h0, w0, 3), dtype=np.uint8), pat, np.zeros((h0, w0, 3), np.uint8),
                     np.full((h0, w0, 3), 255, np.uint8)])


def main():
    out = {"geometries": np.array(GEOMETRIES, dtype=np.int32)}
    for i, (h0, w0, h, w) in enumerate(GEOMETRIES):
        src = frames(h0, w0, 100 + i)
        out[f"in{i}"] = src
        out[f"out{i}"] = np.stack([np.asarray(Image.fromarray(f).resize((w, h), Image.BILINEAR)) for f in src])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "camera_resize.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
