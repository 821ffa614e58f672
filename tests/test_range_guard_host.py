"""The fp16 range guard's host side (include/agplace_hip.h agp_range_flag_set / _get): no GPU needed."""
import ctypes
import threading

import pytest

from agplace_amd import _lib
from agplace_amd.options import Options


def test_symbols_are_exported_and_bound():
    lib = _lib.load()
    for name in ("agp_range_flag_set", "agp_range_flag_get"):
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None


def test_set_returns_the_previous_binding_and_get_reads_it():
    lib = _lib.load()
    w1, w2 = ctypes.c_uint32(0), ctypes.c_uint32(0)
    a1, a2 = ctypes.addressof(w1), ctypes.addressof(w2)
    prev = lib.agp_range_flag_set(a1)
    try:
        assert lib.agp_range_flag_get() == a1
        assert lib.agp_range_flag_set(a2) == a1
        assert lib.agp_range_flag_get() == a2
        assert lib.agp_range_flag_set(None) == a2
        assert lib.agp_range_flag_get() is None
    finally:
        lib.agp_range_flag_set(prev)
    assert lib.agp_range_flag_get() == prev


def test_binding_is_per_host_thread():
    lib = _lib.load()
    w = ctypes.c_uint32(0)
    prev = lib.agp_range_flag_set(ctypes.addressof(w))
    seen = {}

    def other():
        seen["before"] = lib.agp_range_flag_get()
        w2 = ctypes.c_uint32(0)
        lib.agp_range_flag_set(ctypes.addressof(w2))
        seen["own"] = lib.agp_range_flag_get() == ctypes.addressof(w2)
        lib.agp_range_flag_set(None)

    try:
        t = threading.Thread(target=other)
        t.start()
        t.join()
        assert seen["before"] is None          # a fresh thread starts unbound
        assert seen["own"]
        assert lib.agp_range_flag_get() == ctypes.addressof(w)     # the other thread's binding did not leak here
    finally:
        lib.agp_range_flag_set(prev)


def test_options_accept_the_guard():
    assert Options().fp16_range_guard is False
    assert Options(fp16_range_guard=True).fp16_range_guard is True
    with pytest.raises(ValueError):
        Options(fp16_range_guard=1)


def test_guard_binds_only_fp16_inference():
    from agplace_amd import range_guard
    on = Options(fp16_range_guard=True)
    assert range_guard.active(on, 4, False) and range_guard.active(on, 2, False)
    assert not range_guard.active(on, 3, False)
    assert not range_guard.active(on, 4, True)
    assert not range_guard.active(Options(), 4, False)
