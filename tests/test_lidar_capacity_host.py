"""The level capacity of the raw-points route, host side (no GPU): Options.voxel_capacity, the workspace size of
agp_sparse_build_points_cap and its refusals, which return before anything is launched."""
import ctypes
import types

import pytest

from agplace_amd import _lib
from agplace_amd.options import Options, from_reference_opt

AGP_E_BADARG = 1


def test_voxel_capacity_is_validated_like_its_neighbours():
    assert Options().voxel_capacity is None
    for v in (1, 8780, 16384, (1 << 30) - 1):
        assert Options(voxel_capacity=v).voxel_capacity == v
        assert Options().copy(voxel_capacity=v).voxel_capacity == v
    for v in (0, -1, 1 << 30, 1 << 40, True, False, 16384.0, "16384", (16384,)):
        with pytest.raises(ValueError, match="voxel_capacity"):
            Options(voxel_capacity=v)


def test_from_reference_opt_leaves_the_capacity_unset():
    ns = types.SimpleNamespace(voxel_capacity=4096, convnext_u8=True, quant_size=1.5, features_dim=256)
    o = from_reference_opt(ns)
    assert o.voxel_capacity is None and o.convnext_u8 is False
    assert o.quant_size == 1.5                                   # (fields the reference does carry are taken)
    assert from_reference_opt(ns).copy(voxel_capacity=4096).voxel_capacity == 4096


def _table_bytes(level_cap):
    slots = 64
    while slots < 2 * level_cap:
        slots *= 2
    return slots * 8


def test_workspace_table_part_follows_the_level_capacity_at_fixed_npoints():
    L = _lib.load()
    n, nb = 73001, 4
    caps = [1, 32, 33, 64, 8779, 8780, 16384, 16385, 73001, 100000, 1 << 20]
    sizes = [L.agp_sparse_points_cap_workspace_bytes(n, c, nb) for c in caps]
    # the table is the only part that depends on level_cap: a power of two >= 2 level_cap (>= 64) eight-byte slots, 256-byte aligned
    for c, s in zip(caps, sizes):
        assert s - sizes[0] == _table_bytes(c) - _table_bytes(1), (c, s)
    assert sizes[0] == sizes[1] < sizes[2] == sizes[3]          # 64 slots up to 32 rows, then 128
    # everything else is addressed by point rows: at a fixed level_cap the size grows with npoints by 32 bytes a row
    # (bucket keys 8, unique keys 8, sort scratch 16), each part rounded up to 256 bytes
    a, b = (L.agp_sparse_points_cap_workspace_bytes(m, 16384, nb) for m in (73001, 2 * 73001))
    assert abs((b - a) - 32 * 73001) < 3 * 256
    # at level_cap = npoints it is the uncapped workspace plus the two state words (a 256-byte slot each)
    assert L.agp_sparse_points_cap_workspace_bytes(n, n, nb) == L.agp_sparse_points_workspace_bytes(n, nb) + 512
    # a capped level is the smaller workspace, and the difference is the table's
    assert L.agp_sparse_points_workspace_bytes(n, nb) - L.agp_sparse_points_cap_workspace_bytes(n, 8780, nb) == \
        _table_bytes(n) - _table_bytes(8780) - 512
    # arguments outside the range are clamped like agp_sparse_points_workspace_bytes clamps them
    assert L.agp_sparse_points_cap_workspace_bytes(0, 0, 0) == L.agp_sparse_points_cap_workspace_bytes(1, 1, 1)
    assert L.agp_sparse_points_cap_workspace_bytes(n, 1 << 31, nb) == L.agp_sparse_points_cap_workspace_bytes(n, (1 << 30) - 1, nb)


def test_every_refusal_returns_before_a_launch():
    """Without a GPU a launch cannot succeed, so AGP_E_BADARG (and not a launch error) shows the refusal came first; the pointers
    are host buffers that a refused call never touches."""
    L = _lib.load()
    n, cap, nb = 64, 16, 2
    nbytes = L.agp_sparse_points_cap_workspace_bytes(n, cap, nb)
    bufs = {k: ctypes.create_string_buffer(4096) for k in ("pts", "off", "keys", "f", "seg", "bidx", "flag", "ws")}
    a = {k: ctypes.addressof(v) for k, v in bufs.items()}

    def call(npoints=n, level_cap=cap, nbatch=nb, quant=2.0, per=0, wsb=nbytes, **null):
        p = dict(a, **{k: None for k in null})
        return L.agp_sparse_build_points_cap(p["pts"], p["off"], npoints, level_cap, nbatch, quant, None, per, p["keys"], p["f"], p["seg"],
                                             p["bidx"], p["flag"], p["ws"], wsb, None)
    refused = [dict(level_cap=0), dict(level_cap=-5), dict(level_cap=1 << 30), dict(level_cap=1 << 40),
               dict(npoints=0), dict(npoints=-1), dict(npoints=1 << 30),
               dict(wsb=nbytes - 1), dict(wsb=0),
               # a larger level needs the larger table: the workspace of a smaller one is short
               dict(level_cap=4096, wsb=nbytes),
               dict(nbatch=0), dict(nbatch=0x7fff), dict(quant=0.0), dict(quant=float("nan")), dict(quant=float("inf")), dict(per=2),
               dict(pts=1), dict(off=1), dict(keys=1), dict(f=1), dict(seg=1), dict(bidx=1), dict(flag=1), dict(ws=1)]
    for kw in refused:
        assert call(**kw) == AGP_E_BADARG, kw
    # level_cap > npoints is legal: it is refused for no reason of its own (here only the workspace of the small level is short)
    big = L.agp_sparse_points_cap_workspace_bytes(n, 1000, nb)
    assert big > nbytes and call(level_cap=1000, wsb=big - 1) == AGP_E_BADARG


def test_header_exports_and_binding_table_name_the_new_entries():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "agplace_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("agp_sparse_build_points_cap", 16), ("agp_sparse_points_cap_workspace_bytes", 3)):
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", hdr)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == nargs


def test_level_capacity_argument_is_validated_before_the_device_is_touched():
    from agplace_amd.sparse import SparseTensor
    assert SparseTensor._level_capacity(None) is None and SparseTensor._level_capacity(8780) == 8780
    for v in (0, -3, 1 << 30, True, 16384.0, "1"):
        with pytest.raises(ValueError, match="level_capacity"):
            SparseTensor._level_capacity(v)
