"""Host-side checks of the big-k kNN path (128 < k <= 1024): a numpy model of the selection kernel's threshold rule, the
constants the layers share, and the argument checks that run before any launch."""
import os
import re

import numpy as np
import pytest

from agplace_amd import _lib, mining, retrieval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS, S = 256, 4          # select_rerank_kernel<.., BIGK>: 256 threads, BIGK_S = 4 minima kept per thread (csrc/knn.hip)


def threshold_model(gmin, k):
    """Step (a) of the big-k selection: group g goes to thread g % 256, a thread keeps the S smallest of its groups' minima, the
    256 * S keys (absent ones = +inf, the kernel's KMAX) are sorted and T' is the min(k, G)-th smallest."""
    G = gmin.shape[0]
    keys = np.full((THREADS, S), np.inf)
    for t in range(THREADS):
        own = np.sort(gmin[t::THREADS])[:S]
        keys[t, :own.shape[0]] = own
    return np.sort(keys.reshape(-1))[min(k, G) - 1]


def key_sets(G, rng):
    yield "random", rng.standard_normal(G)
    yield "all equal", np.full(G, 1.25)
    yield "ascending", np.arange(G, dtype=np.float64)
    yield "descending", np.arange(G, dtype=np.float64)[::-1].copy()
    # the smallest values all dealt to ONE thread (it keeps only S of them: the bound comes from other threads' groups)
    one = rng.uniform(10, 20, G)
    one[0::THREADS] = rng.uniform(0, 1, one[0::THREADS].shape[0])
    yield "one thread owns the smallest", one
    # ... and to the first few threads
    few = rng.uniform(10, 20, G)
    for t in range(3):
        few[t::THREADS] = rng.uniform(0, 1, few[t::THREADS].shape[0])
    yield "three threads own the smallest", few
    yield "heavy ties", rng.integers(0, 3, G).astype(np.float64)


@pytest.mark.parametrize("G", [130, 255, 256, 257, 700, 1023, 1024, 1025, 1279, 1280, 2048, 2049, 8192, 8752, 20000])
@pytest.mark.parametrize("k", [129, 200, 256, 257, 700, 1000, 1024])
def test_threshold_rule_bounds_the_kth_group_minimum(G, k):
    """T' >= T_k (the k-th smallest group minimum) whenever G >= k, and T' is a real group's value, never the padding: G around
    256 * S = 1024 is where 'every group is kept' turns into 'every thread keeps S'.  G < k: the kernel ignores T' (T = INF)."""
    rng = np.random.default_rng(G * 1031 + k)
    for name, gmin in key_sets(G, rng):
        tp = threshold_model(gmin, k)
        assert np.isfinite(tp), (name, "the min(k, G)-th key is padding")
        if G >= k:
            tk = np.sort(gmin)[k - 1]
            assert tp >= tk, (name, tp, tk)
            assert (gmin <= tp).sum() >= k, name               # at least k groups inside the window
        else:
            assert tp == gmin.max(), name                      # G < k <= 1024: every group is kept, the G-th key is the largest


def test_one_minimum_per_thread_would_not_reach_big_k():
    """Why the small path's rule (the k-th smallest of ONE minimum per thread) stops at 256 and S = 4 is needed: with more than
    256 groups and k > 256 the 256 kept keys run out."""
    gmin = np.random.default_rng(0).standard_normal(5000)
    keys = np.sort(np.array([gmin[t::THREADS].min() for t in range(THREADS)]))
    assert keys.shape[0] == THREADS < 300                                    # 256 keys have no 300th smallest
    assert threshold_model(gmin, 300) >= np.sort(gmin)[299]


def test_constants_agree_across_the_layers():
    assert mining.MAX_K == retrieval.MAX_K == 1024
    hdr = open(os.path.join(ROOT, "include", "agplace_hip.h")).read()
    m = re.search(r"^#define AGP_KNN_MAX_K (\d+)\s*$", hdr, flags=re.M)
    assert m, "AGP_KNN_MAX_K not found in the header"
    assert int(m.group(1)) == retrieval.MAX_K
    src = open(os.path.join(ROOT, "agplace_amd", "csrc", "knn.hip")).read()
    assert "MAX_K_BIG = AGP_KNN_MAX_K" in src
    ent = int(re.search(r"constexpr int MAX_ENT_BIG = (\d+);", src).group(1))
    chunk = int(re.search(r"constexpr int MAX_ENT_CHUNK_BIG = (\d+);", src).group(1))
    s = int(re.search(r"constexpr int BIGK_S = (\d+);", src).group(1))
    assert ent >= chunk + retrieval.MAX_K and ent & (ent - 1) == 0          # a round takes one chunk behind k running-best entries
    assert s == S and THREADS * s >= retrieval.MAX_K
    assert ent * 12 + THREADS * s * 4 <= 64 * 1024                          # static LDS of one workgroup


def test_workspace_does_not_depend_on_k():
    """agp_knn_workspace_bytes is still sufficient for k up to 1024: the search's workspace holds the query planes and the
    group minima; the running best lives in LDS."""
    L = _lib.load()
    for nq, nb, d in ((37, 3000, 64), (513, 24577, 256), (3, 140000, 32), (5, 150, 64)):
        sizes = {L.agp_knn_workspace_bytes(nq, nb, d, k) for k in (1, 20, 128, 129, 1024)}
        assert len(sizes) == 1 and sizes.pop() > 0


@pytest.mark.parametrize("k", [1025, 0, -1, 10 ** 6])
def test_out_of_range_k_is_a_value_error_before_the_library_is_touched(monkeypatch, k):
    idx = retrieval.IndexFlatL2(32, device="cpu")
    idx.add(np.zeros((4, 32), np.float32))

    def no_library():
        raise AssertionError("the library was touched for an out-of-range k")
    monkeypatch.setattr(retrieval._lib, "load", no_library)
    with pytest.raises(ValueError, match="1024"):
        idx.search(np.zeros((2, 32), np.float32), k)
    import torch
    with pytest.raises(ValueError, match="1024"):
        idx.search_device(torch.zeros(2, 32), k)
    with pytest.raises(ValueError, match="1024"):
        idx.search(np.zeros((2, 32), np.float32), 2.5)


def test_mining_batches_every_query_up_to_the_new_limit(monkeypatch):
    """The split of hardest_negatives_indexes: a query goes to the batched search while negs + (its in-sample soft positives)
    <= MAX_K, and on its own beyond -- checked on the host with a stand-in index that answers from an fp64 brute force."""
    import torch
    from oracle import knn, mining as omining
    calls = []

    class FakeIndex:
        def __init__(self, d, device="cpu", prec=None):
            self.db = None

        def add(self, xb):
            self.db = xb.cpu().numpy()

        def search_device(self, xq, k):
            retrieval._check_k(k)
            calls.append((xq.shape[0], k))
            D, I, _ = knn.knn_l2_fp64(xq.cpu().numpy(), self.db, k)
            return torch.from_numpy(D), torch.from_numpy(I)
    monkeypatch.setattr(mining, "IndexFlatL2", FakeIndex)
    rng = np.random.default_rng(5)
    ndb, nq, d = 2600, 4, 32
    db = rng.standard_normal((ndb, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    sampled = rng.permutation(ndb)[:2400]
    soft = [sampled[:300], np.zeros(0, np.int64), sampled[50:1150], sampled[5:1019]]     # 300, 0, 1100, 1014 in the sample
    got = mining.hardest_negatives_indexes(q, db, sampled, soft, 10, device="cpu").numpy()
    want = np.stack([omining.hardest_negatives_indexes(q[i], db, np.setdiff1d(sampled, soft[i], assume_unique=True), 10)
                     for i in range(nq)])
    assert np.array_equal(got, want)
    # queries 0, 1, 3 (k = 10 + 1014 = 1024) in one search; query 2 (10 + 1100 > 1024) alone with k = negs
    assert sorted(calls) == [(1, 10), (3, 1024)]
