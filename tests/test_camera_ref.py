"""Camera front end, host side (no GPU): the numpy restatement of Pillow's 8-bit bilinear resampler (tests/camera_ref.py) against
Pillow itself and against Pillow outputs recorded in tests/golden/camera_resize.npz; torchvision's Resize(int) size rule; the new
Options fields; the library's pure-host helpers (agp_resize_ksize / agp_resize_coeffs / agp_resized_size) against camera_ref's
tables.  Everything is exact: no tolerance appears here."""
import ctypes as C

import numpy as np
import pytest

import camera_ref

# (H0, W0, h, w)
GEOMETRIES = [(256, 455, 192, 341), (37, 53, 16, 22), (20, 31, 20, 17), (9, 9, 9, 9), (16, 24, 32, 48), (300, 300, 256, 256),
              (5, 64, 3, 38), (256, 455, 256, 455),
              (64, 64, 16, 16),      # a 4x reduction: 9 taps
              (8, 8, 32, 32),        # a 4x enlargement
              (70, 130, 33, 67)]


def _frames(h0, w0, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h0, 0:w0]
    pat = np.stack([((yy + xx) % 2) * 255, (xx * 255) // max(w0 - 1, 1), (yy * 255) // max(h0 - 1, 1)], -1).astype(np.uint8)
    # all-0 and all-255 frames: the top of the accumulator and the clip
    return [rng.integers(0, 256, (h0, w0, 3), dtype=np.uint8), pat, np.zeros((h0, w0, 3), np.uint8), np.full((h0, w0, 3), 255, np.uint8)]


@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: "%dx%d-%dx%d" % g)
def test_camera_ref_resize_equals_pillow(geo):
    Image = pytest.importorskip("PIL.Image")
    h0, w0, h, w = geo
    for i, img in enumerate(_frames(h0, w0, 7)):
        want = np.asarray(Image.fromarray(img).resize((w, h), Image.BILINEAR))
        got = camera_ref.resize(img, h, w)
        assert got.dtype == np.uint8 and got.shape == (h, w, 3)
        assert np.array_equal(got, want), (geo, i, int((got != want).sum()))


def test_camera_ref_resize_equals_recorded_pillow_outputs(golden):
    fx = golden("camera_resize")
    geos = fx["geometries"]
    assert len(geos) >= 8
    for i, (h0, w0, h, w) in enumerate(geos.tolist()):
        src, want = fx[f"in{i}"], fx[f"out{i}"]
        assert src.shape[1:] == (h0, w0, 3) and want.shape[1:] == (h, w, 3)
        got = camera_ref.resize_frames(src, h, w)
        assert np.array_equal(got, want), ((h0, w0, h, w), int((got != want).sum()))


def test_resized_size_follows_torchvision():
    assert camera_ref.resized_size(256, 455, 192) == (192, 341)        # landscape: the nuScenes frame
    assert camera_ref.resized_size(455, 256, 192) == (341, 192)        # portrait
    assert camera_ref.resized_size(300, 300, 256) == (256, 256)        # square
    assert camera_ref.resized_size(100, 50, 192) == (384, 192)         # size larger than the input: an enlargement
    assert camera_ref.resized_size(85, 85, 64) == (64, 64)
    assert camera_ref.resized_size(80, 120, 64) == (64, 96)


def test_identity_axis_has_identity_coefficients():
    k, b = camera_ref.coeffs(9, 9)
    assert k.shape == (9, 3) and np.all(k[:, 0] == 1 << 22) and np.all(k[:, 1:] == 0)
    assert np.array_equal(b[:, 0], np.arange(9))


def test_options_resize_fields():
    from types import SimpleNamespace
    from agplace_amd.options import Options, from_reference_opt
    o = Options()
    assert (o.q_resize, o.db_resize) == (256, 256)
    for bad in (0, -3, 192.0, "192", None, True):
        with pytest.raises(ValueError):
            Options(q_resize=bad)
        with pytest.raises(ValueError):
            Options(db_resize=bad)
    o = from_reference_opt(SimpleNamespace(q_resize=192, db_resize=224))
    assert (o.q_resize, o.db_resize) == (192, 224)
    with pytest.raises(ValueError):
        from_reference_opt(SimpleNamespace(q_resize=0))


def _lib_tables(L, n_in, n_out):
    ks = L.agp_resize_ksize(n_in, n_out)
    k = np.full((n_out, ks), -1, dtype=np.int32)
    b = np.full((n_out, 2), -1, dtype=np.int32)
    p = C.POINTER(C.c_int32)
    assert L.agp_resize_coeffs(n_in, n_out, k.ctypes.data_as(p), b.ctypes.data_as(p)) == 0
    return ks, k, b


def test_library_host_helpers_equal_camera_ref():
    """The built library loads without a GPU; its tables are the ones the kernels read."""
    from agplace_amd import _lib
    L = _lib.load()
    for h0, w0, h, w in GEOMETRIES + [(72, 8, 8, 72), (1, 1, 1, 1), (16384, 3, 2048, 16384)]:
        for n_in, n_out in ((h0, h), (w0, w)):
            ks, k, b = _lib_tables(L, n_in, n_out)
            kr, br = camera_ref.coeffs(n_in, n_out)
            assert ks == camera_ref.ksize(n_in, n_out) == kr.shape[1]
            assert np.array_equal(k, kr) and np.array_equal(b, br), (n_in, n_out)
    oh, ow = C.c_int(), C.c_int()
    for h, w, size in [(256, 455, 192), (455, 256, 192), (300, 300, 256), (100, 50, 192), (1, 7, 3), (85, 85, 64), (80, 120, 64),
                       (1080, 1920, 256), (3, 16384, 2)]:
        assert L.agp_resized_size(h, w, size, C.byref(oh), C.byref(ow)) == 0
        assert (oh.value, ow.value) == camera_ref.resized_size(h, w, size)
    assert L.agp_resized_size(0, 5, 3, C.byref(oh), C.byref(ow)) == 1 and L.agp_resized_size(5, 5, 0, C.byref(oh), C.byref(ow)) == 1
    assert L.agp_resize_ksize(0, 4) == -1 and L.agp_resize_ksize(4, 16385) == -1
    assert L.agp_resize_coeffs(4, 4, None, None) == 1
