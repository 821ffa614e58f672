"""Host tests of the camera front end's centre crop and colour jitter: the numpy restatement tests/colour_ref.py (which
tests/test_gpu_colour.py holds the kernels to, byte for byte) against Pillow itself where it is installed and against Pillow's
recorded outputs (tests/golden/colour_jitter.npz) everywhere; the sampler input_pipeline.color_jitter; the new Options."""
import argparse
import os

import numpy as np
import pytest
import torch

import colour_ref as cr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "colour_jitter.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def cube():
    """all 2^24 colours as one 4096 x 4096 image"""
    v = np.arange(1 << 24, dtype=np.uint32)
    c = np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    c.setflags(write=False)
    return c


# ---- against Pillow
@pytest.mark.parametrize("which", ["hsv", "rgb", "luma"])
def test_conversions_equal_pillow_on_all_colours(cube, which):
    Image = pytest.importorskip("PIL.Image")
    if which == "hsv":
        want, got = np.asarray(Image.fromarray(cube, "RGB").convert("HSV")), cr.rgb_to_hsv(cube)
    elif which == "rgb":
        want, got = np.asarray(Image.fromarray(cube, "HSV").convert("RGB")), cr.hsv_to_rgb(cube)
    else:
        want, got = np.asarray(Image.fromarray(cube, "RGB").convert("L")), cr.luma(cube)
    assert int((got != want).sum()) == 0


def test_blend_equals_pillow_on_all_byte_pairs():
    Image = pytest.importorskip("PIL.Image")
    d, x = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    alphas = [float(a) for a in np.linspace(0.0, 2.0, 65)] + [float(np.nextafter(np.float32(1), np.float32(2))), 1.0009765625, 1.001]
    assert 0.0 in alphas and 1.0 in alphas and 2.0 in alphas and len(alphas) >= 64
    dimg, ximg = Image.fromarray(d, "L"), Image.fromarray(x, "L")
    for a in alphas:
        want = np.asarray(Image.blend(dimg, ximg, a))
        assert int((cr.blend(d, x, a) != want).sum()) == 0, a


def test_enhance_ops_and_hue_equal_pillow():
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageEnhance
    fr = np.random.default_rng(0).integers(0, 256, (37, 41, 3), dtype=np.uint8)
    im = Image.fromarray(fr, "RGB")
    for a in (0.0, 0.4, 1.0, 1.7, 3.0):
        assert np.array_equal(cr.adjust_brightness(fr, a), np.asarray(ImageEnhance.Brightness(im).enhance(a))), a
        assert np.array_equal(cr.adjust_saturation(fr, a), np.asarray(ImageEnhance.Color(im).enhance(a))), a
        assert np.array_equal(cr.adjust_contrast(fr, a), np.asarray(ImageEnhance.Contrast(im).enhance(a))), a
    for shift in (0, 1, 128, 243):
        h, s, v = im.convert("HSV").split()
        np_h = np.array(h, dtype=np.uint8)
        with np.errstate(over="ignore"):
            np_h += np.uint8(shift)
        want = np.asarray(Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB"))
        assert np.array_equal(cr.adjust_hue_shift(fr, shift), want), shift


# (H0, W0, c, top, left): even and odd differences; 70 -> 37 is 16.5 -> 16 (even neighbour below), 72 -> 37 is 17.5 -> 18
CROP_CASES = [(45, 72, 37, 4, 18), (70, 70, 37, 16, 16), (72, 72, 37, 18, 18), (38, 41, 37, 0, 2), (37, 37, 37, 0, 0), (9, 12, 4, 2, 4),
              (40, 39, 37, 2, 1)]


@pytest.mark.parametrize("h0,w0,c,top,left", CROP_CASES)
def test_crop_origin_and_window(h0, w0, c, top, left):
    assert cr.center_crop_origin(h0, w0, c) == (top, left)
    fr = np.random.default_rng(h0 * 100 + w0).integers(0, 256, (2, h0, w0, 3), dtype=np.uint8)
    got = cr.center_crop(fr, c)
    assert got.shape == (2, c, c, 3) and np.array_equal(got, fr[:, top:top + c, left:left + c])
    Image = pytest.importorskip("PIL.Image")
    want = np.asarray(Image.fromarray(fr[1], "RGB").crop((left, top, left + c, top + c)))
    assert np.array_equal(got[1], want)


def test_crop_larger_than_the_frame_is_refused():
    for h0, w0 in ((36, 72), (72, 36)):
        with pytest.raises(NotImplementedError):
            cr.center_crop_origin(h0, w0, 37)


# ---- against Pillow's recorded outputs
def test_golden_conversions_blend_and_crops(golden):
    cols = golden["colours"]
    assert np.array_equal(cr.rgb_to_hsv(cols), golden["hsv"])
    assert np.array_equal(cr.hsv_to_rgb(cols), golden["rgb"])
    assert np.array_equal(cr.luma(cols), golden["luma"])
    d, x = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    for a, want in zip(golden["alphas"], golden["blend"]):
        assert np.array_equal(cr.blend(d, x, a), want), a
    for i, (h0, w0, c) in enumerate(golden["crops"]):
        assert np.array_equal(cr.center_crop(golden[f"crop_in{i}"], int(c)), golden[f"crop_out{i}"]), (h0, w0, c)


def test_golden_jitter_by_record(golden):
    src, recs, want = golden["frames"], golden["records"], golden["jittered"]
    assert len(recs) >= 24 and len({tuple(r[:4]) for r in recs[:24]}) == 24          # all 24 orders
    for i, r in enumerate(recs):
        assert np.array_equal(cr.jitter_frame(src[i % len(src)], r), want[i]), (i, r)
    # no ops: unchanged
    none = [i for i, r in enumerate(recs) if not r[:4].any()]
    assert none and all(np.array_equal(want[i], src[i % len(src)]) for i in none)
    # jitter_frames is jitter_frame per frame, any leading shape
    fr = np.stack([src[i % len(src)] for i in range(4)]).reshape(2, 2, *src.shape[1:])
    assert np.array_equal(cr.jitter_frames(fr, recs[:4]), want[:4].reshape(fr.shape))


def test_contrast_mean_equals_integer_rule():
    """int(sum / count + 0.5), what the kernel computes as (2 sum + count) // (2 count)"""
    rng = np.random.default_rng(3)
    for _ in range(200):
        count = int(rng.integers(1, 5000))
        s = int(rng.integers(0, 255 * count + 1))
        assert int(s / count + 0.5) == (2 * s + count) // (2 * count)
    for count in (1, 2, 437, 4096 * 4096):
        for s in (0, count // 2, count // 2 + 1, 255 * count, 127 * count + count // 2, 127 * count + (count + 1) // 2):
            assert int(s / count + 0.5) == (2 * s + count) // (2 * count), (s, count)


# ---- the sampler
def test_sampler_is_repeatable_and_in_range():
    from agplace_amd import input_pipeline as ip
    a = ip.color_jitter(50, 0.4, 0.3, 0.2, 0.1, generator=torch.Generator().manual_seed(5))
    b = ip.color_jitter(50, 0.4, 0.3, 0.2, 0.1, generator=torch.Generator().manual_seed(5))
    c = ip.color_jitter(50, 0.4, 0.3, 0.2, 0.1, generator=torch.Generator().manual_seed(6))
    assert a.dtype == torch.float32 and tuple(a.shape) == (50, 8) and a.device.type == "cpu"
    assert torch.equal(a, b) and not torch.equal(a, c)
    cr.check_records(a.numpy(), 0.4, 0.3, 0.2, 0.1)
    assert len({tuple(r[:4].tolist()) for r in a}) > 10                     # the order is drawn per frame
    assert tuple(ip.color_jitter(0, 0.4).shape) == (0, 8)


def test_sampler_makes_torchvisions_draws():
    """ColorJitter.get_params: randperm(4), then one uniform_ per op that has a range, in the order b, c, s, h"""
    from agplace_amd import input_pipeline as ip
    got = ip.color_jitter(3, 0.4, 0.0, 0.2, 0.5, generator=torch.Generator().manual_seed(9))
    g = torch.Generator().manual_seed(9)
    for rec in got:
        order = torch.randperm(4, generator=g).tolist()
        b = float(torch.empty(1).uniform_(0.6, 1.4, generator=g))
        s = float(torch.empty(1).uniform_(0.8, 1.2, generator=g))          # contrast 0: no draw
        h = float(torch.empty(1).uniform_(-0.5, 0.5, generator=g))
        assert rec[:4].tolist() == [0 if fn == 1 else fn + 1 for fn in order]
        assert float(rec[4]) == b and float(rec[5]) == 1.0 and float(rec[6]) == s
        assert int(rec[7]) == int(h * 255) % 256
    # the global generator, as torchvision uses it
    torch.manual_seed(11)
    x = ip.color_jitter(2, 0.1, 0.1, 0.1, 0.1)
    torch.manual_seed(11)
    assert torch.equal(x, ip.color_jitter(2, 0.1, 0.1, 0.1, 0.1))


def test_sampler_absent_ops_draw_nothing_and_ranges_clamp():
    from agplace_amd import input_pipeline as ip
    g = torch.Generator().manual_seed(1)
    none = ip.color_jitter(4, generator=g)
    assert torch.equal(none[:, :4], torch.zeros(4, 4)) and torch.equal(none[:, 4:7], torch.ones(4, 3)) and not none[:, 7].any()
    # only the four randperm calls were made
    g2 = torch.Generator().manual_seed(1)
    for _ in range(4):
        torch.randperm(4, generator=g2)
    assert torch.equal(torch.rand(3, generator=g), torch.rand(3, generator=g2))
    # a strength above 1 clamps the lower end at 0: [max(0, 1 - v), 1 + v]
    big = ip.color_jitter(400, 3.0, 0.0, 0.0, 0.0, generator=torch.Generator().manual_seed(2))
    fb = big[:, 4]
    assert float(fb.min()) >= 0.0 and float(fb.max()) <= 4.0 and float(fb.min()) < 0.2 and float(fb.max()) > 3.8
    cr.check_records(big.numpy(), 3.0, 0.0, 0.0, 0.0)
    for bad in (dict(hue=0.6), dict(brightness=-0.1), dict(contrast=float("nan")), dict(saturation="1"), dict(hue=True)):
        with pytest.raises(ValueError):
            ip.color_jitter(1, **bad)
    with pytest.raises(ValueError):
        ip.color_jitter(-1)


def test_sampler_negative_hue_wraps():
    from agplace_amd import input_pipeline as ip
    recs = ip.color_jitter(300, 0.0, 0.0, 0.0, 0.1, generator=torch.Generator().manual_seed(4))
    sh = recs[:, 7].numpy().astype(int)
    lim = int(0.1 * 255)
    assert ((sh <= lim) | (sh >= 256 - lim)).all() and (sh >= 256 - lim).any() and ((sh > 0) & (sh <= lim)).any()
    assert cr.hue_shift(-0.05) == 256 - 12 == 244 and cr.hue_shift(0.05) == 12 and cr.hue_shift(-0.001) == 0 and cr.hue_shift(0.5) == 127
    assert cr.hue_shift(-0.5) == 129
    g = torch.Generator().manual_seed(4)
    for rec in recs[:20]:
        torch.randperm(4, generator=g)
        assert int(rec[7]) == cr.hue_shift(float(torch.empty(1).uniform_(-0.1, 0.1, generator=g)))


# ---- Options
def test_options_defaults_and_validation():
    from agplace_amd.options import Options
    o = Options()
    assert o.db_cropsize is None and o.q_jitter == 0.0 and o.db_jitter == 0.0
    assert o.image_mean == (0.485, 0.456, 0.406) and o.image_std == (0.229, 0.224, 0.225)
    o = Options(db_cropsize=384, q_jitter=0.3, db_jitter=1, image_mean=[0.5, 0.5, 0.5], image_std=(0.22, 0.22, 0.22))
    assert o.db_cropsize == 384 and o.image_mean == (0.5, 0.5, 0.5) and isinstance(o.image_mean, tuple)
    assert o.copy(db_cropsize=None).db_cropsize is None
    for bad in (dict(db_cropsize=0), dict(db_cropsize=2.5), dict(db_cropsize=True), dict(q_jitter=-0.1), dict(db_jitter=float("nan")),
                dict(q_jitter="0.1"), dict(image_mean=0.5), dict(image_mean=(0.5, 0.5)), dict(image_std=(0.2, 0.0, 0.2)),
                dict(image_std=(0.2, -1.0, 0.2)), dict(image_mean=(0.5, float("inf"), 0.5)), dict(image_std=("a", "b", "c"))):
        with pytest.raises(ValueError):
            Options(**bad)


def test_from_reference_opt_branches():
    from agplace_amd.options import Options, from_reference_opt
    kitti = from_reference_opt(argparse.Namespace(dataset="kitti360", db_cropsize=384, db_resize=224, q_resize=192, q_jitter=0.2,
                                                  db_jitter=0.1))
    assert kitti.db_cropsize == 384 and kitti.image_mean == (0.5,) * 3 and kitti.image_std == (0.22,) * 3
    assert (kitti.db_resize, kitti.q_resize, kitti.q_jitter, kitti.db_jitter) == (224, 192, 0.2, 0.1)
    # the nuScenes loader has the crop commented out and normalises with ImageNet's constants
    nusc = from_reference_opt(argparse.Namespace(dataset="nuscenes", db_cropsize=384, db_resize=224))
    d = Options()
    assert nusc.db_cropsize is None and nusc.image_mean == d.image_mean and nusc.image_std == d.image_std and nusc.db_resize == 224
    # any other namespace: as before
    plain = from_reference_opt(argparse.Namespace(db_cropsize=256, features_dim=128))
    assert plain.db_cropsize is None and plain.image_mean == d.image_mean and plain.features_dim == 128


def test_models_hand_the_normalisation_to_their_trunks():
    from agplace_amd.models_baseline.dbvanilla2d import DBVanilla2D
    from agplace_amd.network_mm.mm import MM
    from agplace_amd.options import Options
    o = Options(image_mean=(0.5,) * 3, image_std=(0.22,) * 3)
    assert (MM(opt=o).image_fe.fe.image_mean, MM(opt=o).image_fe.fe.image_std) == ((0.5,) * 3, (0.22,) * 3)
    assert all(e.fe.image_std == (0.22,) * 3 for e in DBVanilla2D("db", 256, opt=o).dbimage_fes)
    assert MM(opt=Options()).image_fe.fe.image_mean == (0.485, 0.456, 0.406)
