"""tests/sparse_coord_ref.py pinned on the CPU: its two table builders against each other, its fp64 first convolution against the
project's oracle (oracle/sparse.py), its keys against a lexicographic sort, and the CONDITIONS its clouds must meet for
tests/test_gpu_sparse_coord_kernels.py to reach every path of conv0_mfma_kernel (csrc/sparse.hip): if a cloud stops meeting
them, the GPU test would silently stop covering a path."""
import numpy as np
import pytest
import torch

import sparse_coord_ref as C
from oracle import sparse as osp

OFFSETS = {
    "k3": C.offsets_centered(3, 1),
    "k5": C.offsets_centered(5, 1),
    "children": C.offsets_children(1),
    "mixed": C.offsets_mixed(16, seed=1),
}


@pytest.fixture(scope="module")
def clouds():
    return {name: C.CLOUDS[name](0) for name in ("thin", "slab", "edge")}


def test_offsets_are_in_the_projects_tap_order():
    """kidx = ix + k * iy + k * k * iz, as oracle/sparse.py:_offsets lists them"""
    for k, s in ((3, 1), (5, 1), (7, 1), (3, 2), (5, 4)):
        assert C.offsets_centered(k, s) == osp._offsets(k, s)
    for s in (1, 2, 4):
        assert C.offsets_children(s) == osp._offsets(2, s)
        assert C.offsets_up(s) == [(-a, -b, -c) for a, b, c in C.offsets_children(s)]
    m = C.offsets_mixed(16, seed=1)
    assert len(set(m)) == 16 and (0, 0, 0) in m
    assert min(min(o) for o in m) < 0 < max(max(o) for o in m)


@pytest.mark.parametrize("offs", sorted(OFFSETS))
@pytest.mark.parametrize("name", ["thin", "slab", "edge"])
def test_table_dict_equals_table_dense(clouds, name, offs):
    """Two methods, one table.  The edge cloud's dense volume is built on its translated copy (the bands next to +-32511 moved
    next to the origin: same row order, same differences inside the reach of the offsets)."""
    c, _ = clouds[name]
    n = c.shape[0]
    a = C.table_dict(c, c, OFFSETS[offs], n)
    cd = C.edge_translated(c) if name == "edge" else c
    if name == "edge":
        assert np.array_equal(np.lexsort(cd[:, ::-1].T), np.arange(n)) and np.unique(cd, axis=0).shape[0] == n
    b = C.table_dense(cd, cd, OFFSETS[offs], n)
    assert a.dtype == b.dtype == np.int32 and a.shape == (len(OFFSETS[offs]), n)
    assert np.array_equal(a, b)
    assert (a != n).any() and (a == n).any()
    if (0, 0, 0) in OFFSETS[offs]:
        assert np.array_equal(a[OFFSETS[offs].index((0, 0, 0))], np.arange(n))


def test_tables_between_levels_agree_too():
    """children (coarse outputs, fine inputs) and up (fine outputs, coarse inputs) tables, in != out"""
    lv, _ = C.levels("slab")
    for s in (1, 2):
        fine, coarse = lv[s], lv[2 * s]
        ch = C.table_dict(fine, coarse, C.offsets_children(s), fine.shape[0])
        assert np.array_equal(ch, C.table_dense(fine, coarse, C.offsets_children(s), fine.shape[0]))
        # every fine voxel is the child of exactly one coarse voxel
        hit = np.sort(ch[ch != fine.shape[0]])
        assert np.array_equal(hit, np.arange(fine.shape[0]))
        up = C.table_dict(coarse, fine, C.offsets_up(s), coarse.shape[0])
        assert np.array_equal(up, C.table_dense(coarse, fine, C.offsets_up(s), coarse.shape[0]))
        assert ((up != coarse.shape[0]).sum(0) == 1).all()


@pytest.mark.parametrize("ntaps,cout", [(125, 64), (27, 32)])
def test_conv0_ref64_equals_the_oracle_convolution(clouds, ntaps, cout):
    c, nb = clouds["thin"]
    k = round(ntaps ** (1 / 3))
    g = torch.Generator().manual_seed(ntaps)
    f = torch.randn((c.shape[0], 1), generator=g, dtype=torch.float64)
    w = torch.randn((ntaps, 1, cout), generator=g, dtype=torch.float64)
    x = osp.SpT([tuple(r) for r in c.tolist()], f, 1, nb)
    want = osp.conv(x, w, k).feats
    tab = C.table_dict(c, c, C.offsets_centered(k, 1), c.shape[0])
    got = C.conv0_ref64(tab, f[:, 0], w[:, 0, :])
    assert got.shape == want.shape and got.dtype == torch.float64
    torch.testing.assert_close(got, want, rtol=1e-12, atol=0.0)            # (both sum the taps in kidx order)
    # the epilogue
    scale, shift = torch.rand(cout, generator=g, dtype=torch.float64) + 0.5, torch.randn(cout, generator=g, dtype=torch.float64)
    got = C.conv0_ref64(tab, f[:, 0], w[:, 0, :], scale, shift, True)
    torch.testing.assert_close(got, torch.relu(want * scale + shift), rtol=1e-12, atol=0.0)


def test_tile_windows_put_slab_on_both_sides_of_the_lds_window(clouds):
    """Conditions on the INPUTS of the GPU test, not measurements: slab at kernel 5 has tiles whose window fits the 1536 keys of
    conv0_mfma_kernel's LDS copy and tiles whose window does not; thin, and slab at kernel 3, have none that does not."""
    slab_k = C.keys_of(clouds["slab"][0])
    thin_k = C.keys_of(clouds["thin"][0])
    w5 = C.tile_windows(slab_k, 2, 1)
    assert w5.shape[0] == (slab_k.shape[0] + 127) // 128
    assert int((w5 > C.C0_WK).sum()) >= 1 and int((w5 <= C.C0_WK).sum()) >= 1
    assert int(w5[:27].min()) >= 1330 and int(w5.max()) == 2532        # the slab's own 27 tiles
    assert int(C.tile_windows(slab_k, 1, 1).max()) <= C.C0_WK
    for r in (1, 2, 3):
        assert int(C.tile_windows(thin_k, r, 1).max()) <= C.C0_WK
    # by definition, on a cloud small enough to count by hand: 3 keys in one x-plane, window of reach 1 around each
    k = C.keys_of(np.array([[0, 0, 0, 0], [0, 0, 0, 1], [0, 5, 0, 0]]))
    assert C.tile_windows(k, 1, 1, rows=1).tolist() == [2, 2, 1]
    assert C.tile_windows(k, 1, 1, rows=2).tolist() == [2, 1]
    assert C.tile_windows(k, 1, 5, rows=3).tolist() == [3]


def test_cloud_conditions(clouds):
    """What the GPU test relies on: row counts off the tile size, an empty middle sample, a tile across two samples, the edge
    cloud at the limit, the big cloud past one round of the 1024-workgroup grid and past kernel_map_kernel's grid."""
    t, nb = clouds["thin"]
    off = C.seg_offsets(t, nb)
    assert nb == 3 and off[1] == off[2] and 800 < t.shape[0] < 900 and t.shape[0] % 128 and off[1] % 128
    # the inclusive upper bound of conv0_mfma_kernel's window shows only where the key keys[last] + span exists: never on thin
    # (by construction), on most tiles of slab -- the evidence that slab covers what thin cannot
    s, nbs = clouds["slab"]
    for r in (1, 2, 3):
        assert not C.window_end_keys_present(C.keys_of(t), r, 1).any()
    for r in (1, 2):
        assert int(C.window_end_keys_present(C.keys_of(s), r, 1)[:27].sum()) >= 10
    offs = C.seg_offsets(s, nbs)
    assert offs[1] == 3456 and offs[2] == offs[3] and s.shape[0] == 3456 + t.shape[0]
    e, _ = clouds["edge"]
    assert e[:, 1:].max() == C.LIMIT and e[:, 1:].min() == -C.LIMIT and 100 < e.shape[0] < 400
    corners = {(sx * C.LIMIT, sy * C.LIMIT, sz * C.LIMIT) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)}
    assert corners <= {tuple(r[1:]) for r in e.tolist() if r[0] == 0}
    b, nbb = C.big(0)
    assert nbb == 4 and b.shape[0] == 140000 and b.shape[0] > 1024 * 128 and b.shape[0] * 16 > 8192 * 256
    lv, _ = C.levels("thin")
    assert (lv[2][:, 1:] % 2 == 0).all() and (lv[4][:, 1:] % 4 == 0).all() and lv[4].shape[0] < lv[2].shape[0] < lv[1].shape[0]
    # same seed, same data
    assert np.array_equal(C.thin(0)[0], t) and not np.array_equal(C.thin(1)[0], t)


@pytest.mark.parametrize("name", ["thin", "slab", "edge"])
def test_keys_round_trip_and_sort_like_the_coordinates(clouds, name):
    from agplace_amd.sparse import coords as pc
    c, _ = clouds[name]
    k = C.keys_of(c)
    assert k.dtype == np.int64 and np.array_equal(C.coords_of(k), c)
    assert np.array_equal(k, pc._keys(torch.from_numpy(c)).numpy())         # the project's own linearisation
    assert (np.diff(k) > 0).all()                                          # rows sorted by (b, x, y, z) <=> keys increasing
    rng = np.random.default_rng(3)
    p = rng.permutation(c.shape[0])
    assert np.array_equal(np.argsort(k[p], kind="stable"), np.lexsort(c[p][:, ::-1].T))
    # a coordinate offset is a key offset
    o = C.offsets_mixed(16, seed=1)
    d = C.key_offsets(o)
    moved = c[:, None, :] + np.array([[0, *v] for v in o])[None]
    assert np.array_equal(C.keys_of(moved.reshape(-1, 4)).reshape(-1, 16), k[:, None] + d[None])
    assert (k < C.PAD_KEY).all()
