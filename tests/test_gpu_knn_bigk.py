"""-m gpu parity tests of the exact kNN for 128 < k <= 1024 (select_rerank_kernel<.., BIGK>, csrc/knn.hip): indices EQUAL to the
fp64 brute force of oracle/knn.py wherever the ordering is unambiguous, distances to fp32 rounding, ascending, ties by ascending
index, faiss padding.  Shapes are the smallest that reach each branch of the big-k path."""
import types

import numpy as np
import pytest
import torch

from oracle import knn
from oracle import mining as omining
from agplace_amd import _lib, retrieval

pytestmark = pytest.mark.gpu


def check_against_oracle(index, q, db, k, sel=None):
    """The contract of tests/test_gpu_knn.py::check_against_oracle; `sel`: judge only these query rows (the search takes all)."""
    D, I = index.search(q, k)
    assert D.dtype == np.float32 and I.dtype == np.int64 and D.shape == (q.shape[0], k) and I.shape == D.shape
    if sel is not None:
        D, I, q = D[sel], I[sel], q[sel]
    Dr, Ir, D64 = knn.knn_l2_fp64(q, db, k + 1)
    ok = knn.unambiguous_mask(D64, 1e-9)[:, :k]
    kk = min(k, db.shape[0])
    assert np.array_equal(I[:, :kk][ok[:, :kk]], Ir[:, :kk][ok[:, :kk]])
    np.testing.assert_allclose(D[:, :kk], Dr[:, :kk], rtol=2e-7, atol=1e-37)
    assert np.all(np.diff(D[:, :kk].astype(np.float64), axis=1) >= 0)
    assert np.all((I[:, :kk] >= 0) & (I[:, :kk] < db.shape[0]))
    assert all(len(set(r.tolist())) == kk for r in I[:, :kk])            # no label twice
    if k > db.shape[0]:
        assert np.all(I[:, db.shape[0]:] == -1) and np.all(D[:, db.shape[0]:] == knn.FLT_MAX)
    return D, I


def brute_force_full_sort(q, db, k):
    """fp64 direct sum over EVERY row, sorted by (distance, index).  For inputs that are all ties: oracle.knn.knn_l2_fp64
    shortlists k + 32 rows with argpartition first, which picks arbitrary members of a tie larger than that."""
    diff = q.astype(np.float64)[:, None, :] - db.astype(np.float64)[None]
    d = (diff * diff).sum(-1)
    order = np.lexsort((np.broadcast_to(np.arange(db.shape[0]), d.shape), d), axis=1)[:, :k]
    return np.take_along_axis(d, order, 1), order


@pytest.fixture(scope="module")
def small():
    """3000 x 64 database, 37 queries: shared by the cases that only vary k and the coarse form (never written to)."""
    rng = np.random.default_rng(3000 + 64)
    db = rng.standard_normal((3000, 64)).astype(np.float32)
    q = rng.standard_normal((37, 64)).astype(np.float32)
    return db, q


@pytest.fixture(scope="module")
def small_indexes(dev, small):
    db, _ = small
    out = {}
    for prec in (4, 3, 1):
        out[prec] = retrieval.IndexFlatL2(64, prec=prec)
        out[prec].add(db)
    return out


@pytest.mark.parametrize("k", [129, 256, 500, 1024])
@pytest.mark.parametrize("prec", [4, 3, 1])
def test_both_coarse_forms_several_k(dev, small, small_indexes, prec, k):
    """prec 4: packed 64-row groups (48 of them, fewer than every k here: T = INF); prec 3 / 1: generic 16-row groups (192:
    more than k = 129, fewer than the others).  k = 129 is the first k the small path refuses (AGP_E_BADARG before this path)."""
    db, q = small
    check_against_oracle(small_indexes[prec], q, db, k)


@pytest.mark.parametrize("k", [129, 256])
def test_packed_groups_above_k(dev, k):
    """The packed form with a finite threshold at a small width: 20000 rows = 314 groups of 64 > k, so the bound comes from the
    sorted per-thread minima (two per thread at most here) and most candidate groups contribute the one row of their minimum."""
    rng = np.random.default_rng(20000)
    db = rng.standard_normal((20000, 64)).astype(np.float32)
    q = rng.standard_normal((37, 64)).astype(np.float32)
    idx = retrieval.IndexFlatL2(64, prec=4)
    idx.add(db)
    check_against_oracle(idx, q, db, k)


def test_four_wave_coarse_kernel_in_front(dev):
    """The ragged shape of test_four_wave_coarse_kernel_ragged_shapes (d = 256, > 512 queries, >= 12 tiles per workgroup): the
    packed big-k selection behind coarse_f16_w4_kernel, 386 groups of 64 rows > k."""
    nb, nq, k = 24577, 513, 300
    rng = np.random.default_rng(nb + nq)
    db = (rng.standard_normal((nb, 256)) * 0.02).astype(np.float32)
    q = (rng.standard_normal((nq, 256)) * 0.02).astype(np.float32)
    db[127] = db[128] = db[nb - 1]
    q[5] = db[128]
    idx = retrieval.IndexFlatL2(256, prec=4)
    idx.add(db)
    sel = np.unique(np.concatenate([[5, nq - 1], rng.choice(nq, 40, replace=False)]))
    D, I = check_against_oracle(idx, q, db, k, sel=sel)
    row5 = int(np.nonzero(sel == 5)[0][0])
    assert list(I[row5, :3]) == [127, 128, nb - 1] and np.all(D[row5, :3] == 0)


@pytest.mark.parametrize("prec", [4, 3])
def test_fewer_groups_than_k(dev, prec):
    """nb = 700: 48 sixteen-row groups / 12 sixty-four-row groups < k = 200 -> no finite bound, every row is a candidate."""
    rng = np.random.default_rng(700)
    db = rng.standard_normal((700, 128)).astype(np.float32)
    q = rng.standard_normal((11, 128)).astype(np.float32)
    idx = retrieval.IndexFlatL2(128, prec=prec)
    idx.add(db)
    check_against_oracle(idx, q, db, 200)


@pytest.mark.parametrize("prec", [4, 3])
def test_k_above_ntotal_pads_like_faiss(dev, prec):
    rng = np.random.default_rng(150)
    db = rng.standard_normal((150, 64)).astype(np.float32)
    q = rng.standard_normal((5, 64)).astype(np.float32)
    idx = retrieval.IndexFlatL2(64, prec=prec)
    idx.add(db)
    D, I = check_against_oracle(idx, q, db, 300)
    assert np.all(I[:, 150:] == -1) and np.all(D[:, 150:] == np.float32(3.4028234663852886e38))
    assert np.all(I[:, :150] >= 0)


@pytest.mark.parametrize("prec", [4, 3])
def test_identical_rows_take_several_exact_rounds(dev, prec):
    """6000 identical rows, k = 1024: every row is a candidate (more than the 4096-entry buffer holds: the exact phase runs in
    rounds of one chunk behind the running best) and the tie rule leaves rows 0..1023."""
    rng = np.random.default_rng(6000)
    row = rng.standard_normal(64).astype(np.float32)
    db = np.tile(row, (6000, 1))
    q = np.concatenate([row[None], rng.standard_normal((3, 64)).astype(np.float32)])
    idx = retrieval.IndexFlatL2(64, prec=prec)
    idx.add(db)
    D, I = idx.search(q, 1024)
    assert np.array_equal(I, np.tile(np.arange(1024), (4, 1)))
    want = ((q.astype(np.float64) - row.astype(np.float64)) ** 2).sum(1).astype(np.float32)
    np.testing.assert_allclose(D, np.tile(want[:, None], (1, 1024)), rtol=2e-7, atol=0)
    assert np.all(D[0] == 0)


@pytest.mark.parametrize("prec", [4, 3])
def test_three_distinct_rows_two_thousand_copies_each(dev, prec):
    """db[i] = base[i % 3]: k = 600 is filled by the first 600 copies of the query's nearest base row, in index order."""
    rng = np.random.default_rng(2000)
    base = rng.standard_normal((3, 64)).astype(np.float32)
    db = base[np.arange(6000) % 3]
    q = np.concatenate([base, rng.standard_normal((4, 64)).astype(np.float32)])
    idx = retrieval.IndexFlatL2(64, prec=prec)
    idx.add(db)
    D, I = idx.search(q, 600)
    Dr, Ir = brute_force_full_sort(q, db, 600)
    assert np.array_equal(I, Ir)
    np.testing.assert_allclose(D, Dr.astype(np.float32), rtol=2e-7, atol=0)
    for j in range(3):                                  # the base rows themselves: copies j, j + 3, j + 6, ...
        assert np.array_equal(I[j], j + 3 * np.arange(600)) and np.all(D[j] == 0)


def test_more_than_one_window_of_group_minima(dev):
    """The generic coarse form writes one minimum per 16-row group; the launcher gives a thread VPT = 32 minima per window once
    there are more than 8 * 256 groups, so more than 32 * 256 = 8192 groups take a second window.  Relies on
    G = agp_knn_pad_rows(nb) / 16 > 8192 (asserted below with the launcher's own arithmetic)."""
    nb, d, nq, k = 140000, 32, 3, 700
    G = _lib.load().agp_knn_pad_rows(nb) // 16
    assert G > 8 * 256 and G > 32 * 256 and (G + 32 * 256 - 1) // (32 * 256) == 2
    rng = np.random.default_rng(nb)
    db = rng.standard_normal((nb, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    idx = retrieval.IndexFlatL2(d, prec=3)
    idx.add(db)
    check_against_oracle(idx, q, db, k)


@pytest.mark.parametrize("scale", [1e5, 3e-6])
def test_f16_coarse_pass_out_of_range_at_big_k(dev, scale):
    """The scalings of test_f16_coarse_pass_stays_exact_out_of_range (fp16 saturates / underflows: the window opens to
    everything) at k = 300."""
    rng = np.random.default_rng(11)
    db = (rng.standard_normal((700, 64)) * scale).astype(np.float32)
    q = (rng.standard_normal((9, 64)) * scale).astype(np.float32)
    idx = retrieval.IndexFlatL2(64, prec=4)
    idx.add(db)
    D, I = idx.search(q, 300)
    Dr, Ir, _ = knn.knn_l2_fp64(q, db, 300)
    assert np.array_equal(I, Ir)
    np.testing.assert_allclose(D, Dr, rtol=2e-7, atol=1e-37)


@pytest.mark.parametrize("prec", [4, 3])
def test_dispatch_boundary_128_129(dev, small, small_indexes, prec):
    """k = 128 (the small path's last) and k = 129 (the big path's first) on the same index and queries."""
    db, q = small
    D128, I128 = check_against_oracle(small_indexes[prec], q, db, 128)
    D129, I129 = check_against_oracle(small_indexes[prec], q, db, 129)
    _, _, D64 = knn.knn_l2_fp64(q, db, 130)
    ok = knn.unambiguous_mask(D64, 1e-9)[:, :128]
    assert np.array_equal(I128[ok], I129[:, :128][ok])
    assert np.array_equal(D128, D129[:, :128])


@pytest.mark.parametrize("k", [1025, 0, -3])
def test_limits_raise_before_any_launch(dev, small, monkeypatch, k):
    db, q = small
    idx = retrieval.IndexFlatL2(64)
    idx.add(db)

    def no_library():
        raise AssertionError("the library was touched for an out-of-range k")
    monkeypatch.setattr(retrieval._lib, "load", no_library)
    with pytest.raises(ValueError, match="1024"):
        idx.search(q, k)
    with pytest.raises(ValueError, match="1024"):
        idx.search_device(torch.from_numpy(q).to(dev), k)
    assert idx._prepared is None and not idx._ws


def test_compute_recall_with_recall_at_200(dev):
    """recall_values = [1, 20, 200]: positives planted at known ranks of the oracle's own neighbour lists (rank 0, inside the top
    20, inside the top 200, beyond it)."""
    rng = np.random.default_rng(200)
    db = rng.standard_normal((2500, 64)).astype(np.float32)
    q = rng.standard_normal((48, 64)).astype(np.float32)
    _, Ir, _ = knn.knn_l2_fp64(q, db, 400)
    ranks = [0, 7, 19, 20, 150, 199, 200, 399]
    positives = [np.array([Ir[i, ranks[i % len(ranks)]]]) for i in range(48)]
    ds = types.SimpleNamespace(queries_num=48, get_positives=lambda: positives)
    args = types.SimpleNamespace(features_dim=64, recall_values=[1, 20, 200])
    recalls, s = retrieval.compute_recall(args, q, db, ds)
    want, want_s = retrieval.recall_from_predictions(args, Ir[:, :200], ds)
    np.testing.assert_array_equal(recalls, want)
    assert s == want_s
    np.testing.assert_allclose(recalls, [100 / 8, 300 / 8, 600 / 8])


def test_mining_with_300_in_sample_soft_positives_is_one_search(dev, monkeypatch):
    """k = negs + 300 = 310: one batched search serves every query (the per-query fallback is for k > 1024 only)."""
    from agplace_amd import mining
    rng = np.random.default_rng(300)
    ndb, nq, d = 1500, 6, 64
    db = rng.standard_normal((ndb, d)).astype(np.float32)
    q = (db[rng.integers(0, ndb, nq)] + 0.1 * rng.standard_normal((nq, d))).astype(np.float32)
    sampled = rng.choice(ndb, size=800, replace=False)
    soft = [rng.choice(ndb, size=int(rng.integers(1, 30)), replace=False) for _ in range(nq)]
    soft[1] = np.unique(np.concatenate([soft[1], sampled[100:400]]))
    soft[3] = np.zeros(0, dtype=np.int64)
    assert np.isin(sampled, soft[1]).sum() >= 300
    calls = []
    real = retrieval.IndexFlatL2.search_device

    def spy(self, xq, k):
        calls.append((xq.shape[0], k))
        return real(self, xq, k)
    monkeypatch.setattr(retrieval.IndexFlatL2, "search_device", spy)
    got = mining.hardest_negatives_indexes(q, db, sampled, soft, 10, device=dev).cpu().numpy()
    want = np.stack([omining.hardest_negatives_indexes(q[i], db, np.setdiff1d(sampled, soft[i], assume_unique=True), 10)
                     for i in range(nq)])
    assert np.array_equal(got, want)
    assert len(calls) == 1 and calls[0][0] == nq and 310 <= calls[0][1] <= mining.MAX_K
