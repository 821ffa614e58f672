"""numpy restatement of the camera front end's resize (TEST INFRASTRUCTURE; the specification is DESIGN.md section 1d): Pillow's
ImagingResample for 8-bit channels with the bilinear filter, which is what torchvision's Resize does to a PIL image, and
torchvision's size rule for Resize(int).

Per axis, input size `n_in`, output size `n_out` (all in float64, as Pillow's C doubles):
  scale = n_in / n_out;  fs = max(scale, 1);  support = 1.0 * fs;  ksize = ceil(support) * 2 + 1;  ss = 1 / fs
  center = (xx + 0.5) * scale
  first = max(int(center - support + 0.5), 0);  count = min(int(center + support + 0.5), n_in) - first
  w[x] = max(0, 1 - |(x + first - center + 0.5) * ss|), divided by their sum when that is not zero
  k[x] = int(0.5 + w[x] * 2^22)
  out[xx] = min(255, (2^21 + sum_x k[x] * in[first + x]) >> 22)
The horizontal pass runs first and its result is uint8; the vertical pass reads that.  An axis whose size does not change has
identity coefficients (k = [2^22, 0]) and is not special-cased here."""
import math

import numpy as np

PRECISION_BITS = 22


def resized_size(h, w, size):
    """torchvision Resize(int) on an (h, w) image: the shorter edge becomes `size`, the longer int(size * long / short)."""
    short, long_ = (w, h) if w <= h else (h, w)
    new_short, new_long = size, int(size * long_ / short)
    return (new_long, new_short) if w <= h else (new_short, new_long)


def ksize(n_in, n_out):
    return int(math.ceil(max(n_in / n_out, 1.0))) * 2 + 1


def coeffs(n_in, n_out):
    """(k int32 [n_out, ksize], bounds int32 [n_out, 2] = (first tap, tap count))"""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ks = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    k = np.zeros((n_out, ks), dtype=np.int32)
    bounds = np.zeros((n_out, 2), dtype=np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        first = max(int(center - support + 0.5), 0)
        count = min(int(center + support + 0.5), n_in) - first
        w = []
        for x in range(count):
            a = abs((x + first - center + 0.5) * ss)
            w.append(1.0 - a if a < 1.0 else 0.0)
        ww = 0.0
        for v in w:
            ww += v
        for x in range(count):
            v = w[x] / ww if ww != 0.0 else w[x]
            k[xx, x] = int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (first, count)
    return k, bounds


def _pass(img, k, bounds, axis):
    """One pass along `axis` (0 = rows, 1 = columns) of a uint8 [H, W, C] image."""
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((k.shape[0],) + src.shape[1:], dtype=np.uint8)
    for xx in range(k.shape[0]):
        first, count = int(bounds[xx, 0]), int(bounds[xx, 1])
        acc = np.full(src.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int64)
        for x in range(count):
            acc += int(k[xx, x]) * src[first + x]
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize(img, h, w):
    """uint8 [H0, W0, 3] -> uint8 [h, w, 3]: PIL.Image.fromarray(img).resize((w, h), BILINEAR), byte for byte."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    tmp = _pass(img, *coeffs(img.shape[1], w), axis=1)          # horizontal first, stored as uint8
    return np.ascontiguousarray(_pass(tmp, *coeffs(img.shape[0], h), axis=0))


def resize_frames(frames, h, w):
    """uint8 [..., H0, W0, 3] -> uint8 [..., h, w, 3]"""
    frames = np.asarray(frames, dtype=np.uint8)
    flat = frames.reshape((-1,) + frames.shape[-3:])
    out = np.stack([resize(f, h, w) for f in flat])
    return out.reshape(frames.shape[:-3] + (h, w, 3))
