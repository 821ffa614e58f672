"""numpy restatement of the camera front end's centre crop and colour jitter (TEST INFRASTRUCTURE; the specification is DESIGN.md
section 1d): torchvision's CenterCrop(int) and ColorJitter on a PIL frame, i.e. Pillow's ImageEnhance (Image.blend against a
degenerate image) and Pillow's RGB <-> HSV conversions, byte for byte.  tests/test_colour_ref.py holds it to Pillow itself.

A frame's parameter record is 8 float32 numbers:
  [0:4]  the ops in the order they run: 0 = none, 1 = brightness, 2 = contrast, 3 = saturation, 4 = hue
         (torchvision's fn_idx + 1; an op that ColorJitter.get_params leaves out is 0)
  [4:7]  the brightness, contrast and saturation factors
  [7]    the hue byte shift, 0 .. 255: int(hue_factor * 255) truncated toward zero, mod 256
"""
import numpy as np

OP_NONE, OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE = 0, 1, 2, 3, 4
RECORD = 8
F32 = np.float32


def center_crop_origin(H0, W0, c):
    """(top, left) of torchvision's CenterCrop(c) window on an (H0, W0) frame; Python's round (halves to even)."""
    if c < 1 or c > H0 or c > W0:
        raise NotImplementedError(f"centre crop {c} of a {H0}x{W0} frame: torchvision pads with black, which is not built")
    return int(round((H0 - c) / 2.0)), int(round((W0 - c) / 2.0))


def center_crop(frames, c):
    """uint8 [..., H0, W0, 3] -> uint8 [..., c, c, 3]"""
    top, left = center_crop_origin(frames.shape[-3], frames.shape[-2], c)
    return np.ascontiguousarray(frames[..., top:top + c, left:left + c, :])


def luma(rgb):
    """Pillow's convert("L"): uint8 [..., 3] -> uint8 [...]"""
    p = rgb.astype(np.int64)
    return ((19595 * p[..., 0] + 38470 * p[..., 1] + 7471 * p[..., 2] + 0x8000) >> 16).astype(np.uint8)


def blend(deg, x, a):
    """Pillow's Image.blend(degenerate, image, a) per byte; `deg` and `x` broadcast.  The multiply and the add are rounded to
    fp32 one after the other (no fused multiply-add)."""
    a = F32(a)
    d = np.asarray(deg).astype(F32)
    t = (d + (a * (np.asarray(x).astype(F32) - d)).astype(F32)).astype(F32)
    if F32(0) <= a <= F32(1):
        return t.astype(np.int32).astype(np.uint8)
    out = t.astype(np.int32)
    out = np.where(t <= 0, 0, np.where(t >= 255, 255, out))
    return out.astype(np.uint8)


def rgb_to_hsv(rgb):
    """Pillow's convert("HSV") of an RGB image: uint8 [..., 3] -> uint8 [..., 3]"""
    p = rgb.astype(np.int32)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    maxc, minc = p.max(-1), p.min(-1)
    grey = maxc == minc
    cr = np.where(grey, 1, maxc - minc).astype(F32)
    s = cr / np.where(grey, 1, maxc).astype(F32)
    rc, gc, bc = [((maxc - ch).astype(F32) / cr).astype(np.float64) for ch in (r, g, b)]
    h = np.where(r == maxc, bc - gc, np.where(g == maxc, 2.0 + rc - bc, 4.0 + gc - rc)).astype(F32)
    h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(F32)
    H = np.clip((h.astype(np.float64) * 255.0).astype(np.int32), 0, 255)
    S = np.clip((s.astype(np.float64) * 255.0).astype(np.int32), 0, 255)
    out = np.stack([np.where(grey, 0, H), np.where(grey, 0, S), maxc], -1)
    return out.astype(np.uint8)


def hsv_to_rgb(hsv):
    """Pillow's convert("RGB") of an HSV image: uint8 [..., 3] -> uint8 [..., 3]"""
    p = hsv.astype(np.int32)
    H, S, V = p[..., 0], p[..., 1], p[..., 2]
    h6 = H.astype(F32).astype(np.float64) * 6.0 / 255.0
    i = np.floor(h6).astype(np.int32)
    f = (h6 - i.astype(F32).astype(np.float64)).astype(F32).astype(np.float64)
    fs = (S.astype(F32).astype(np.float64) / 255.0).astype(F32).astype(np.float64)
    v = V.astype(np.float64)

    def c_round(x):             # C's round(): halves away from zero
        return np.where(x >= 0, np.floor(x + 0.5), np.ceil(x - 0.5)).astype(np.int32)
    pp = np.clip(c_round(v * (1.0 - fs)), 0, 255)
    q = np.clip(c_round(v * (1.0 - fs * f)), 0, 255)
    t = np.clip(c_round(v * (1.0 - fs * (1.0 - f))), 0, 255)
    sel = i % 6
    table = [(V, t, pp), (q, V, pp), (pp, V, t), (pp, q, V), (t, pp, V), (V, pp, q)]
    out = np.empty(p.shape, dtype=np.int32)
    for ch in range(3):
        out[..., ch] = np.select([sel == k for k in range(6)], [table[k][ch] for k in range(6)])
    out = np.where((S == 0)[..., None], V[..., None], out)
    return out.astype(np.uint8)


def adjust_brightness(img, a):
    return blend(0, img, a)


def adjust_saturation(img, a):
    return blend(luma(img)[..., None], img, a)


def contrast_mean(img):
    """ImageEnhance.Contrast's grey level of one frame [h, w, 3]: int(mean(L) + 0.5)"""
    L = luma(img)
    return int(int(L.sum(dtype=np.int64)) / L.size + 0.5)


def adjust_contrast(img, a):
    return blend(contrast_mean(img), img, a)


def adjust_hue_shift(img, shift):
    hsv = rgb_to_hsv(img)
    hsv[..., 0] = (hsv[..., 0].astype(np.int32) + int(shift)) % 256
    return hsv_to_rgb(hsv)


def hue_shift(hue_factor):
    """The byte torchvision's PIL adjust_hue adds to the H channel, np.uint8 wrap-around included."""
    return int(float(hue_factor) * 255) % 256


def jitter_frame(img, rec):
    """One frame uint8 [h, w, 3] through its record."""
    rec = np.asarray(rec, dtype=F32)
    out = np.ascontiguousarray(img, dtype=np.uint8)
    for op in rec[:4].astype(np.int32):
        if op == OP_BRIGHTNESS:
            out = adjust_brightness(out, rec[4])
        elif op == OP_CONTRAST:
            out = adjust_contrast(out, rec[5])
        elif op == OP_SATURATION:
            out = adjust_saturation(out, rec[6])
        elif op == OP_HUE:
            out = adjust_hue_shift(out, int(rec[7]))
        elif op != OP_NONE:
            raise ValueError(f"op {op}")
    return out


def jitter_frames(frames, params):
    """uint8 [..., h, w, 3] with float32 params [number of frames, 8] (any leading shape) -> the jittered frames"""
    frames = np.asarray(frames, dtype=np.uint8)
    flat = frames.reshape((-1,) + frames.shape[-3:])
    params = np.asarray(params, dtype=F32).reshape(-1, RECORD)
    assert len(params) == len(flat)
    return np.stack([jitter_frame(f, r) for f, r in zip(flat, params)]).reshape(frames.shape)


def check_records(params, brightness, contrast, saturation, hue):
    """The sampler's contract: params float32 [n, 8] as input_pipeline.color_jitter(n, ...) returns them."""
    params = np.asarray(params)
    assert params.dtype == np.float32 and params.ndim == 2 and params.shape[1] == RECORD
    ranges = {OP_BRIGHTNESS: brightness, OP_CONTRAST: contrast, OP_SATURATION: saturation}
    for rec in params:
        ops = rec[:4].astype(np.int32)
        assert np.array_equal(ops, rec[:4])
        present = sorted(int(o) for o in ops if o != OP_NONE)
        want = [code for code, v in ranges.items() if v > 0] + ([OP_HUE] if hue > 0 else [])
        assert present == sorted(want), (present, want)
        for code, v in ranges.items():
            f = float(rec[3 + code])
            if v > 0:
                assert max(0.0, 1.0 - v) - 1e-6 <= f <= 1.0 + v + 1e-6
            else:
                assert f == 1.0
        assert rec[7] == int(rec[7]) and 0 <= rec[7] <= 255
        if hue > 0:
            sh = int(rec[7])
            assert sh <= int(hue * 255) or sh >= 256 - int(hue * 255)
        else:
            assert rec[7] == 0
