"""Pins the oracle of the geo kernels (tests/geo_ref.py): radius_ref against sklearn's radius_neighbors, and the proof that the
fixtures of tests/test_gpu_geo.py tell every deliberately wrong variant apart from the oracle.  No GPU."""
import numpy as np
import pytest

import geo_ref


def test_radius_ref_equals_sklearn_as_sets():
    """The reference's own call (datasets_ws_nuscenes.py:907-912) on a float32 UTM random walk, radii 10 and 25: equal sets,
    the pairs exactly on the boundary included (float32 grids produce them; both sides are inclusive and exact in fp64)."""
    neighbors = pytest.importorskip("sklearn.neighbors")
    q, db = geo_ref.sklearn_layout()
    knn = neighbors.NearestNeighbors(n_jobs=1)
    knn.fit(db)
    for radius in (10, 25):
        theirs = knn.radius_neighbors(q, radius=radius, return_distance=False)
        off, idx = geo_ref.radius_ref(q, db, radius)
        assert off[-1] == sum(len(t) for t in theirs)
        for i, t in enumerate(theirs):
            assert np.array_equal(np.sort(t), idx[off[i]:off[i + 1]]), (radius, i)
        on = 0
        for s in range(0, len(q), 512):
            d = q.astype(np.float64)[s:s + 512, None, :] - db.astype(np.float64)[None, :, :]
            on += int((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] == radius * radius).sum())
        print(f"radius {radius}: {off[-1]} pairs, {on} exactly on the boundary")


def test_three_four_five():
    db = np.asarray([(3.0, 4.0), (0.0, 5.0), (5.0, 0.0), (np.nextafter(5.0, 6.0), 0.0)])
    off, idx = geo_ref.radius_ref(np.zeros((1, 2)), db, 5.0)
    assert off.tolist() == [0, 3] and idx.tolist() == [0, 1, 2]


def test_radius_ref_rows_are_ascending_and_nan_has_no_neighbours():
    cases = {name: (q, db, r) for name, q, db, r in geo_ref.radius_cases()}
    q, db, r = cases["nan_inf_f32"]
    off, idx = geo_ref.radius_ref(q, db, r)
    lens = np.diff(off)
    assert lens[1] == 0 and lens[3] == 0 and lens[0] == 63 and not np.isin([7, 64], idx).any()
    for name, (q, db, r) in cases.items():
        off, idx = geo_ref.radius_ref(q, db, r)
        for row in geo_ref.csr_lists(off, idx):
            assert np.all(np.diff(row) > 0), name


def test_radius_fixtures_hold_the_required_cases():
    cases = {name: geo_ref.radius_ref(q, db, r) + (q, db) for name, q, db, r in geo_ref.radius_cases()}
    assert {db.shape[0] for n, (_, _, _, db) in cases.items() if n.startswith("walk")} == set(geo_ref.RADIUS_NB)
    assert {q.shape[0] for n, (_, _, q, _) in cases.items() if n.startswith("walk")} == set(geo_ref.RADIUS_NQ)
    assert {q.dtype for _, _, q, _ in cases.values()} == {np.dtype(np.float32), np.dtype(np.float64)}
    assert any((np.diff(off) == 0).any() and (np.diff(off) > 0).any() for off, _, _, _ in cases.values())
    off, _, q, db = cases["whole_database"]
    assert np.all(np.diff(off) == len(db))
    assert np.diff(cases["lists_of_64_and_65"][0]).tolist() == [64, 65, 0]
    assert np.diff(cases["duplicates"][0])[0] >= 4


def test_wrong_radius_variants_are_caught_by_the_fixtures():
    caught = {"exclusive": [], "float32": []}
    for name, q, db, r in geo_ref.radius_cases():
        off, idx = geo_ref.radius_ref(q, db, r)
        for key, kw in (("exclusive", dict(exclusive=True)), ("float32", dict(arith=np.float32))):
            o2, i2 = geo_ref.radius_ref(q, db, r, **kw)
            if not (np.array_equal(off, o2) and np.array_equal(idx, i2)):
                caught[key].append(name)
    assert {"boundary_f32_r10", "boundary_f32_r5", "boundary_f32_r15", "boundary_f64_r10", "three_four_five"} <= set(caught["exclusive"])
    assert "boundary_f64_r10" in caught["float32"]


@pytest.mark.parametrize("k", geo_ref.FIRST_HIT_K)
@pytest.mark.parametrize("nq", geo_ref.FIRST_HIT_Q)
def test_first_hit_ref_is_the_reference_loop(k, nq):
    """first_hit_ref < n  <=>  np.any(np.isin(pred[:n], positives)), the reference's test (test.py:77)."""
    pred, off, idx = geo_ref.first_hit_case(k, nq)
    first = geo_ref.first_hit_ref(pred, off, idx)
    for q in range(nq):
        for n in {1, 5, 20, 64, 65, k}:
            assert bool(np.any(np.isin(pred[q, :n], idx[off[q]:off[q + 1]]))) == bool(first[q] < min(n, k))


def test_first_hit_fixtures_and_wrong_variants():
    seen, lens = set(), set()
    skips = wraps = False
    for k in geo_ref.FIRST_HIT_K:
        for nq in geo_ref.FIRST_HIT_Q:
            pred, off, idx = geo_ref.first_hit_case(k, nq)
            first = geo_ref.first_hit_ref(pred, off, idx)
            seen |= {(int(f) if f < k - 1 else ("last" if f == k - 1 else "none")) for f in first}
            lens |= set(np.diff(off).tolist())
            assert (pred == -1).any() or k <= 4 or nq == 1
            skips |= not np.array_equal(first, geo_ref.first_hit_wrong_skips(pred, off, idx))
            wraps |= not np.array_equal(first, geo_ref.first_hit_wrong_wraps(pred, off, idx, geo_ref.N_DB))
    assert {0, 63, 64, "last", "none"} <= seen
    assert {0, 1, 64, 65, 5000} <= lens
    assert skips and wraps


def test_drop_listed_wrong_variants_are_caught_by_the_mining_fixture():
    fx = geo_ref.MiningFixture()
    off, idx = fx.soft_ref()
    lens = np.diff(off)[fx.sq]
    assert lens[2] == 0 and lens[0] >= 1100 and lens[1] == 80                # sq = [1, 0, 2, ...]
    in_sample = np.asarray([np.isin(fx.cand, idx[off[r]:off[r + 1]]).sum() for r in fx.sq])
    assert in_sample[1] == 81 and in_sample[0] == 100 and in_sample.max() == 100      # row 5 twice
    wide = np.isin(fx.cand_wide, idx[off[1]:off[2]]).sum()
    assert wide == 1100 and wide > 1024 - fx.negs
    k = fx.negs + int(in_sample.max())
    I = geo_ref.knn_positions_ref(fx.qfeat, fx.feat[fx.cand], k)
    assert np.isin(fx.cand[I[1, :64]], idx[off[0]:off[1]]).all()             # query 0: its first 64 candidates are all listed
    out, filled = geo_ref.drop_listed_ref(I, fx.cand, fx.sq, off, idx, fx.negs)
    assert np.all(filled == fx.negs)
    for variant in ("position", "first_copy"):
        o2, f2 = geo_ref.drop_listed_ref(I, fx.cand, fx.sq, off, idx, fx.negs, variant=variant)
        assert not np.array_equal(out, o2), variant
    # and the oracle is the reference's own route: setdiff1d, then the nearest of what is left
    for q in (0, 1, 2, 17):
        left = np.setdiff1d(fx.cand, idx[off[fx.sq[q]]:off[fx.sq[q] + 1]], assume_unique=True)
        sub = fx.cand[np.isin(fx.cand, left)]
        near = geo_ref.knn_positions_ref(fx.qfeat[q:q + 1], fx.feat[sub], fx.negs)[0]
        assert np.array_equal(out[q], sub[near])
