"""-m gpu: agp_mine_topk_listed (csrc/mining.hip) and the full / random mining routes built on it (agplace_amd/mining.py:
nearest_listed, NegCache, compute_triplets_full, compute_triplets_random) against numpy restatements kept in this file.

The judge of the kernel: fp64 brute-force distances, then np.lexsort on (row, distance) over the distinct valid candidates.
The judges of the two mining functions restate reference datasets/datasets_ws_nuscenes.py:1295-1322 and :1264-1289 line by
line, the random draws passed in.  Indices are compared with array_equal.  out_dist may differ from the judge's fp32-rounded
value by one fp32 ulp: the two fp64 sums differ only in summation order (about d * 2^-53 relative), so their fp32 roundings can
differ only at a rounding boundary.  Every fixture asserts, on the judge's side, that two distinct candidates of a query whose
vectors are not bit-identical lie at fp64 distances at least 1e-9 apart (relative): far more than the summation order can move."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A5A5A5A5A
NGUARD = 8
FLT_MAX = np.float32(3.4028234663852886e38)


def _guarded(n, dtype, dev, fill=None):
    """(whole buffer, the n-element window behind NGUARD guard words and in front of NGUARD more)."""
    word = GUARD if dtype == torch.int64 else 0x5A5A5A5A
    buf = torch.full((n + 2 * NGUARD,), word, dtype=torch.int32 if dtype == torch.float32 else dtype, device=dev)
    if dtype == torch.float32:
        buf = buf.view(torch.float32)
    win = buf[NGUARD:NGUARD + n]
    if fill is not None:
        win.fill_(fill)
    return buf, win


def _guards_intact(buf, n):
    if buf.dtype == torch.float32:
        buf = buf.view(torch.int32)
    word = GUARD if buf.dtype == torch.int64 else 0x5A5A5A5A
    return bool((buf[:NGUARD] == word).all()) and bool((buf[NGUARD + n:] == word).all())


# ---------------------------------------------------------------------------------------------------------------- judges

def _dist64(qv, xb, rows):
    diff = qv.astype(np.float64)[None, :] - xb[rows].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return (diff * diff).sum(1)


def _assert_separated(dd, rows, xb):
    """The fixture condition: distinct candidates that are not the same vector are at least 1e-9 (relative) apart."""
    fin = np.isfinite(dd)
    d, r = dd[fin], rows[fin]
    order = np.lexsort((r, d))
    d, r = d[order], r[order]
    for a in range(len(d) - 1):
        if xb[r[a]].tobytes() == xb[r[a + 1]].tobytes():
            assert d[a] == d[a + 1]
        else:
            assert d[a + 1] - d[a] >= 1e-9 * d[a + 1], (r[a], r[a + 1], d[a], d[a + 1])


def topk_ref(xq, xb, cand, excl, exempt, k):
    """(idx [Q, k], dist fp32 [Q, k], filled): the k smallest of the distinct valid candidates under (fp64 distance, row); a
    non-finite distance counts as +inf.  excl: per query an array of excluded rows, or None."""
    nq, ncols = cand.shape
    idx = np.full((nq, k), -1, dtype=np.int64)
    dist = np.full((nq, k), FLT_MAX, dtype=np.float32)
    filled = np.zeros(nq, dtype=np.int32)
    for q in range(nq):
        row = cand[q]
        ok = (row >= 0) & (row < len(xb))
        if excl is not None:
            ok &= ~(np.isin(row, excl[q]) & (np.arange(ncols) >= exempt))
        rows = np.unique(row[ok])
        dd = _dist64(xq[q], xb, rows)
        _assert_separated(dd, rows, xb)
        key = np.where(np.isfinite(dd), dd, np.inf)
        take = np.lexsort((rows, key))[:k]
        filled[q] = len(take)
        idx[q, :len(take)] = rows[take]
        with np.errstate(over="ignore"):
            dist[q, :len(take)] = dd[take].astype(np.float32)
    return idx, dist, filled


def _within_one_ulp(got, want):
    fin = np.isfinite(want)
    same_kind = np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    gap = np.abs(got[fin].view(np.int32).astype(np.int64) - want[fin].view(np.int32).astype(np.int64))     # both >= 0: ordered bits
    return same_kind and bool((gap <= 1).all())


def _launch(dev, xq, xb, cand, excl, rows, exempt, k, with_dist=True):
    """The C entry on guarded outputs; excl a list of lists (the exclusion CSR's rows) or None.  (idx, dist, filled) as numpy."""
    from agplace_amd import _lib, geo
    from agplace_amd._lib import check, ptr
    nq, ncols = cand.shape
    xq_d, xb_d, cand_d = torch.from_numpy(xq).to(dev), torch.from_numpy(xb).to(dev), torch.from_numpy(cand).to(dev)
    ibuf, idx = _guarded(nq * k, torch.int64, dev, fill=-7)
    dbuf, dist = _guarded(nq * k, torch.float32, dev, fill=-7.0)
    fbuf, filled = _guarded(nq, torch.int32, dev, fill=-7)
    off_p = idx_p = rows_p = None
    if excl is not None:
        pos = geo.Positives.from_lists(excl, dev, sort=True)
        keep = pos.indices if pos.indices.numel() else torch.zeros(1, dtype=torch.int64, device=dev)
        rows_d = torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(dev)
        off_p, idx_p, rows_p = ptr(pos.offsets), ptr(keep), ptr(rows_d)
    check(_lib.load().agp_mine_topk_listed(ptr(xq_d), nq, ptr(xb_d), len(xb), xq.shape[1], ptr(cand_d), ncols, rows_p, off_p, idx_p,
                                           exempt, k, ptr(idx), ptr(dist) if with_dist else None, ptr(filled), _lib.stream()),
          "agp_mine_topk_listed")
    torch.cuda.synchronize()
    assert _guards_intact(ibuf, nq * k) and _guards_intact(dbuf, nq * k) and _guards_intact(fbuf, nq)
    return idx.view(nq, k).cpu().numpy(), dist.view(nq, k).cpu().numpy(), filled.cpu().numpy()


# ------------------------------------------------------------------------------------------------------- the kernel alone

Q, N, NCOLS, K, EXEMPT = 5, 300, 70, 10, 10
TWINS = ((17, 203), (40, 41))                      # database rows with bit-identical vectors


@functools.lru_cache(maxsize=None)
def _kernel_case(d):
    """Q = 5 queries over N = 300 rows, 70 columns of which the first 10 are exempt; the exclusion CSR has 8 rows of which the
    queries use rows [6, 2, 0, 3, 5]."""
    rng = np.random.default_rng(1000 + d)
    xb = rng.standard_normal((N, d)).astype(np.float32)
    for a, b in TWINS:
        xb[b] = xb[a]
    xq = rng.standard_normal((Q, d)).astype(np.float32)
    xq[0] = xb[17] + 0.05 * rng.standard_normal(d).astype(np.float32)          # the twins 17 / 203 lead query 0's result
    xq[1] = xb[41] + 0.05 * rng.standard_normal(d).astype(np.float32)
    cand = np.full((Q, NCOLS), -1, dtype=np.int64)
    lists = [np.zeros(0, dtype=np.int64) for _ in range(8)]
    rows = np.asarray([6, 2, 0, 3, 5])
    # query 0: twins in either order, the same row twice within the sample (88), once exempt and once in the sample (120),
    # an excluded row that survives in an exempt column (55; also listed in the sample, where it is dropped), padding, entries
    # >= N and < -1, and an exclusion list that takes a dozen sampled rows
    sample = rng.permutation(np.setdiff1d(np.arange(N), [17, 203, 88, 120, 55]))[:50]
    cand[0, :EXEMPT] = [120, 55, -1, 7, 9, -1, 300, -5, 11, 13]
    cand[0, EXEMPT:] = np.concatenate([[203, 88, 17, 120, 88, 55, N, 5000, -2, -1], sample])
    lists[6] = np.concatenate([[55, 7], sample[:12]])                           # 7 is exempt too
    # query 1: an EMPTY exclusion list; the twins 40 / 41 listed larger row first
    cand[1, :EXEMPT] = [41, 40, 3, -1, -1, -1, -1, -1, -1, -1]
    cand[1, EXEMPT:] = rng.permutation(np.setdiff1d(np.arange(N), [40, 41, 3]))[:60]
    # query 2: an exclusion list that removes most of the row (all but 6 of the sample), the exempt columns keep 4 of the excluded and 3 more
    s2 = rng.permutation(N)[:60]
    cand[2, :EXEMPT] = [s2[0], s2[1], s2[2], s2[3], 250, 251, 252, -1, -1, -1]
    cand[2, EXEMPT:] = s2
    lists[0] = np.concatenate([s2[:54], [250]])
    # query 3: 7 distinct valid candidates (5, 290, 0, 299, 123, 64, 200) among repeats, padding and out-of-range entries
    cand[3, :EXEMPT] = [5, 5, -1, 290, -1, -1, -1, -1, -1, -1]
    cand[3, EXEMPT:EXEMPT + 14] = [0, 299, 123, 64, 200, 200, 0, 150, 151, 300, 301, -3, 2 ** 40, -2 ** 40]
    lists[3] = np.asarray([150, 151, 152])
    # query 4: nothing valid: padding, out of range, and excluded rows only (none in an exempt column)
    cand[4, EXEMPT:EXEMPT + 6] = [30, 31, 32, N, -9, 31]
    cand[4, :3] = [-1, N + 7, -4]
    lists[5] = np.asarray([29, 30, 31, 32, 33])
    lists[1], lists[2] = np.arange(N), np.zeros(0, dtype=np.int64)                    # row 1 unused; row 2 (query 1) empty
    lists[4], lists[7] = np.arange(0, N, 2), np.asarray([1])
    excl_q = [lists[r] for r in rows]
    return xq, xb, cand, lists, rows, topk_ref(xq, xb, cand, excl_q, EXEMPT, K)


@pytest.mark.parametrize("d", [32, 96, 256])
def test_topk_listed_equals_the_judge(dev, d):
    from agplace_amd import mining
    xq, xb, cand, lists, rows, (want_idx, want_dist, want_filled) = _kernel_case(d)
    idx, dist, filled = _launch(dev, xq, xb, cand, lists, rows, EXEMPT, K)
    assert np.array_equal(filled, want_filled) and np.array_equal(idx, want_idx)
    assert _within_one_ulp(dist, want_dist)
    # what the fixture is there to show
    assert want_filled.tolist() == [K, K, K, 7, 0]
    assert want_idx[0, :2].tolist() == [17, 203] and want_idx[1, :2].tolist() == [40, 41]          # twins: the smaller row first
    assert np.isin(55, topk_ref(xq, xb, cand, [lists[r] for r in rows], EXEMPT, NCOLS)[0][0])       # excluded row 55 survives
    assert not np.isin(55, topk_ref(xq, xb, cand, [lists[r] for r in rows], 0, NCOLS)[0][0])        # only through its exempt column
    assert (idx[3, 7:] == -1).all() and (dist[3, 7:] == FLT_MAX).all() and (idx[4] == -1).all() and (dist[4] == FLT_MAX).all()
    # without out_dist, and through the wrapper (lists addressed by exclude_rows; a Positives; one list per query)
    idx2, _, filled2 = _launch(dev, xq, xb, cand, lists, rows, EXEMPT, K, with_dist=False)
    assert np.array_equal(idx2, idx) and np.array_equal(filled2, filled)
    for exclude, exclude_rows in ((lists, rows), ([lists[r] for r in rows], None)):
        got, got_filled = mining.nearest_listed(xq, xb, cand, K, exclude, exclude_rows, EXEMPT, device=dev)
        assert got.dtype == torch.int64 and got_filled.dtype == torch.int32
        assert np.array_equal(got.cpu().numpy(), want_idx) and np.array_equal(got_filled.cpu().numpy(), want_filled)
    # no exclusion at all, every column
    want = topk_ref(xq, xb, cand, None, 0, K)
    got, got_filled = mining.nearest_listed(xq, xb, cand, K, device=dev)
    assert np.array_equal(got.cpu().numpy(), want[0]) and np.array_equal(got_filled.cpu().numpy(), want[2])


def test_topk_listed_all_columns_decide(dev):
    """The full-width check of query 0's exempt row: with k = ncols every distinct valid candidate is returned, 55 among them."""
    xq, xb, cand, lists, rows, _ = _kernel_case(32)
    want = topk_ref(xq, xb, cand, [lists[r] for r in rows], EXEMPT, NCOLS)
    idx, dist, filled = _launch(dev, xq, xb, cand, lists, rows, EXEMPT, NCOLS)
    assert np.array_equal(idx, want[0]) and np.array_equal(filled, want[2]) and _within_one_ulp(dist, want[1])
    assert 55 in idx[0] and (np.bincount(idx[0][idx[0] >= 0]) <= 1).all()


@functools.lru_cache(maxsize=None)
def _edge_case(nq, ncols):
    n, d = 600, 32
    rng = np.random.default_rng(7 * ncols + nq)
    xb = rng.standard_normal((n, d)).astype(np.float32)
    xq = rng.standard_normal((nq, d)).astype(np.float32)
    cand = rng.integers(-1, n, size=(nq, ncols)).astype(np.int64)             # repeats once ncols is large, some padding
    excl = [rng.permutation(n)[:n // 3] for _ in range(nq)]
    return xq, xb, cand, excl


@pytest.mark.parametrize("nq,ncols,k", [(3, 1, 10), (3, 257, 10), (3, 4096, 10), (3, 257, 1), (3, 257, 128), (3, 4096, 128),
                                        (1, 257, 10), (1, 1, 1)])
def test_topk_listed_edges_of_k_columns_and_queries(dev, nq, ncols, k):
    xq, xb, cand, excl = _edge_case(nq, ncols)
    exempt = min(4, ncols - 1)
    want = topk_ref(xq, xb, cand, excl, exempt, k)
    runs = [_launch(dev, xq, xb, cand, excl, np.arange(nq), exempt, k) for _ in range(2)]
    idx, dist, filled = runs[0]
    assert np.array_equal(idx, want[0]) and np.array_equal(filled, want[2]) and _within_one_ulp(dist, want[1])
    for a, b in zip(runs[0], runs[1]):                                         # the same call twice: identical bits
        assert a.tobytes() == b.tobytes()


def test_a_nan_row_comes_last_and_once(dev):
    xq, xb, cand, _ = _edge_case(3, 257)
    xb = xb.copy()
    xb[77, 5] = np.nan
    xb[301] = np.inf                                                            # inf - finite = inf: non-finite too, the larger row
    cand = cand[:, :20].copy()
    cand[:, 3] = cand[:, 11] = 77                                               # listed twice
    cand[:, 0] = 301
    k = 20
    want = topk_ref(xq, xb, cand, None, 0, k)
    idx, dist, filled = _launch(dev, xq, xb, cand, None, None, 0, k)
    assert np.array_equal(idx, want[0]) and np.array_equal(filled, want[2]) and _within_one_ulp(dist, want[1])
    for q in range(3):
        f = filled[q]
        assert idx[q, f - 2:f].tolist() == [77, 301] and (idx[q] == 77).sum() == 1
        assert np.isnan(dist[q, f - 2]) and np.isinf(dist[q, f - 1]) and np.isfinite(dist[q, :f - 2]).all()
    short = _launch(dev, xq, xb, cand, None, None, 0, 5)                        # and it is not among a shorter result
    assert not np.isin([77, 301], short[0]).any()


# ------------------------------------------------------------------------------------------------ the two mining functions

def _best_ref(query_features, database_features, hard):
    """get_best_positive_index (:1241-1248): an IndexFlatL2 over the query's hard positives, k = 1, the first on ties."""
    dd = _dist64(query_features, database_features, hard)
    return int(hard[int(np.argmin(dd))])


def _hardest_ref(query_features, database_features, neg_samples, negs):
    """get_hardest_negatives_indexes (:1250-1258): an IndexFlatL2 over cache[neg_samples], the `negs` nearest, the earlier
    entry first on ties (a stable sort)."""
    dd = _dist64(query_features, database_features, neg_samples)
    _assert_separated(dd, neg_samples, database_features)
    neg_nums = np.argsort(dd, kind="stable")[:negs]                             # :1255
    return neg_samples[neg_nums].astype(np.int32)                               # :1257


def full_ref(query_features, database_features, sampled_queries_indexes, hard, soft, draws, neg_cache, negs):
    """compute_triplets_full (:1295-1322), the draws of :1310 passed in; neg_cache (a list of arrays) is updated in place."""
    triplets = []
    for i, query_index in enumerate(sampled_queries_indexes):                   # :1306
        qf = query_features[i]                                                  # :1307
        best_positive_index = _best_ref(qf, database_features, hard[query_index])            # :1308
        neg_indexes = draws[i]                                                  # :1310
        soft_positives = soft[query_index]                                      # :1312
        neg_indexes = np.setdiff1d(neg_indexes, soft_positives, assume_unique=True)           # :1313
        neg_indexes = np.unique(np.concatenate([neg_cache[query_index], neg_indexes]))        # :1315
        neg_indexes = _hardest_ref(qf, database_features, neg_indexes, negs)    # :1317
        neg_cache[query_index] = neg_indexes                                    # :1319
        triplets.append((query_index, best_positive_index, *neg_indexes))       # :1320
    return np.asarray(triplets, dtype=np.int64)                                 # :1322


def random_ref(query_features, database_features, sampled_queries_indexes, hard, soft, draws, negs):
    """compute_triplets_random (:1264-1289), the draws of :1284 passed in."""
    triplets = []
    for i, query_index in enumerate(sampled_queries_indexes):                   # :1278
        qf = query_features[i]                                                  # :1279
        best_positive_index = _best_ref(qf, database_features, hard[query_index])            # :1280
        soft_positives = soft[query_index]                                      # :1283
        neg_indexes = draws[i]                                                  # :1284
        neg_indexes = np.setdiff1d(neg_indexes, soft_positives, assume_unique=True)[:negs]    # :1285
        triplets.append((query_index, best_positive_index, *neg_indexes))       # :1287
    return np.asarray(triplets, dtype=np.int64)                                 # :1289


class _Mining:
    """N = 400 database rows, 40 queries, d = 64, negs = 10: continuous features (no ties), per query 3..30 soft positives of
    which the first few are hard; three overlapping refreshes of 12 sampled queries with their own draws of S = 60."""
    n, nq_all, d, negs, q, s = 400, 40, 64, 10, 12, 60

    def __init__(self):
        rng = np.random.default_rng(20240)
        self.feat = rng.standard_normal((self.n, self.d)).astype(np.float32)
        self.soft = [np.sort(rng.choice(self.n, size=rng.integers(3, 31), replace=False)) for _ in range(self.nq_all)]
        self.hard = [np.sort(rng.choice(s, size=rng.integers(1, 4), replace=False)) for s in self.soft]
        near = np.asarray([h[0] for h in self.hard])
        self.qfeat_all = (self.feat[near] + 0.8 * rng.standard_normal((self.nq_all, self.d))).astype(np.float32)
        perm = rng.permutation(self.nq_all)
        self.refreshes = [perm[:12], perm[6:18], np.concatenate([perm[[0, 1, 2, 7, 8, 9]], perm[20:26]])]
        self.draws = [np.stack([rng.choice(self.n, size=self.s, replace=False) for _ in range(self.q)]) for _ in self.refreshes]
        # the cache the first refresh starts from: mostly empty; query perm[0] holds a SOFT POSITIVE of its own next to it in
        # feature space (the reference does not filter the cache, so it must stay a negative), query perm[6] a short list
        a, b = int(perm[0]), int(perm[6])
        self.start = [np.empty((0,), dtype=np.int32) for _ in range(self.nq_all)]
        self.start[a] = np.asarray([self.hard[a][0], 5, 6], dtype=np.int32)
        self.start[b] = np.asarray([(self.soft[b][0] + 1) % self.n], dtype=np.int32)
        self.kept = (a, int(self.hard[a][0]))


@functools.lru_cache(maxsize=None)
def _mining():
    return _Mining()


@functools.lru_cache(maxsize=None)
def _full_want():
    """The restatement's table and cache after each of the three refreshes: computed once, never changed."""
    fx = _mining()
    cache = [x.copy() for x in fx.start]
    out = []
    for sq, draws in zip(fx.refreshes, fx.draws):
        table = full_ref(fx.qfeat_all[sq], fx.feat, sq, fx.hard, fx.soft, draws, cache, fx.negs)
        out.append((table, [x.copy() for x in cache]))
    return out


def _raise(*a, **k):
    raise AssertionError("the device route went through host lists")


@pytest.mark.parametrize("positives", ["lists", "Positives"])
def test_compute_triplets_full_over_three_refreshes(dev, monkeypatch, positives):
    from agplace_amd import geo, mining
    fx = _mining()
    hard, soft = fx.hard, fx.soft
    if positives == "Positives":
        hard, soft = geo.Positives.from_lists(fx.hard, dev, sort=True), geo.Positives.from_lists(fx.soft, dev, sort=True)
        monkeypatch.setattr(mining, "_csr", _raise)                             # no host loop over the queries on this route
        monkeypatch.setattr(geo.Positives, "to_lists", _raise)
        monkeypatch.setattr(geo.Positives, "_host_copy", _raise)
        monkeypatch.setattr(geo.Positives, "from_lists", _raise)
    cache = mining.NegCache.from_lists(fx.start, fx.negs, device=dev)
    for (sq, draws), (want_table, want_cache) in zip(zip(fx.refreshes, fx.draws), _full_want()):
        got = mining.compute_triplets_full(fx.qfeat_all[sq], fx.feat, sq, hard, soft, draws, cache, fx.negs, device=dev)
        assert got.dtype == torch.int64 and got.shape == (fx.q, 2 + fx.negs)
        assert np.array_equal(got.cpu().numpy(), want_table)
        mine = cache.to_lists()
        assert all(a.dtype == np.int32 and np.array_equal(a, b) for a, b in zip(mine, want_cache))
    # the unfiltered cache entry did stay a negative of its query in the first refresh
    q, row = fx.kept
    first = _full_want()[0][0]
    assert row in first[first[:, 0] == q][0, 2:] and row in fx.soft[q]
    assert len(set(fx.refreshes[0]) & set(fx.refreshes[1])) == 6 and len(set(fx.refreshes[0]) & set(fx.refreshes[2])) == 6


def test_full_with_one_shared_draw_equals_partial(dev):
    """An empty cache and every query given the SAME draw: the candidates are compute_triplets_partial's, so are the negatives
    and their order (continuous features: no ties for the two tie rules to differ on)."""
    from agplace_amd import mining
    fx = _mining()
    sq, draw = fx.refreshes[0], fx.draws[0][0]
    cache = mining.NegCache(fx.nq_all, fx.negs, device=dev)
    got = mining.compute_triplets_full(fx.qfeat_all[sq], fx.feat, sq, fx.hard, fx.soft, np.tile(draw, (fx.q, 1)), cache, fx.negs,
                                       device=dev)
    want = mining.compute_triplets_partial(fx.qfeat_all[sq], fx.feat, sq, fx.hard, fx.soft, draw, fx.negs, device=dev)
    assert torch.equal(got, want)


def test_full_with_too_few_candidates_raises_and_keeps_the_cache(dev):
    from agplace_amd import geo, mining
    fx = _mining()
    sq = fx.refreshes[0]
    rng = np.random.default_rng(5)
    draws = np.stack([rng.choice(fx.n, size=12, replace=False) for _ in range(fx.q)])
    soft = [x.copy() for x in fx.soft]
    soft[sq[4]] = np.sort(np.concatenate([draws[4][:5], np.setdiff1d(fx.soft[sq[4]], draws[4])]))   # 5 of its 12 are soft positives
    start = [x.copy() for x in fx.start]
    for i in sq:
        if i != sq[4]:
            start[i] = np.arange(20, 30, dtype=np.int32)                      # everyone else has candidates to spare
    start[sq[4]] = np.empty((0,), dtype=np.int32)
    for s in (soft, geo.Positives.from_lists(soft, dev, sort=True)):
        cache = mining.NegCache.from_lists(start, fx.negs, device=dev)
        before = cache.table.clone()
        with pytest.raises(ValueError, match="^fewer candidate negatives than negs_num_per_query for some query$"):
            mining.compute_triplets_full(fx.qfeat_all[sq], fx.feat, sq, fx.hard, s, draws, cache, fx.negs, device=dev)
        assert torch.equal(cache.table, before)


@pytest.mark.parametrize("positives", ["lists", "Positives"])
def test_compute_triplets_random_equals_the_restatement(dev, monkeypatch, positives):
    from agplace_amd import geo, mining
    fx = _mining()
    sq = fx.refreshes[1]
    rng = np.random.default_rng(77)
    draws = [rng.choice(fx.n, size=fx.negs + len(fx.soft[i]), replace=False) for i in sq]                    # :1284
    # one query's draw holds ALL its soft positives, so exactly `negs` entries are left
    i5 = sq[5]
    others = rng.choice(np.setdiff1d(np.arange(fx.n), fx.soft[i5]), size=fx.negs, replace=False)
    draws[5] = rng.permutation(np.concatenate([fx.soft[i5], others]))
    assert len(np.setdiff1d(draws[5], fx.soft[i5])) == fx.negs
    want = random_ref(fx.qfeat_all[sq], fx.feat, sq, fx.hard, fx.soft, draws, fx.negs)
    width = max(len(x) for x in draws) + 3
    table = np.full((fx.q, width), -1, dtype=np.int64)
    for i, x in enumerate(draws):
        table[i, :len(x)] = x
    hard, soft = fx.hard, fx.soft
    if positives == "Positives":
        hard, soft = geo.Positives.from_lists(fx.hard, dev, sort=True), geo.Positives.from_lists(fx.soft, dev, sort=True)
    got_lists = mining.compute_triplets_random(fx.qfeat_all[sq], fx.feat, sq, hard, soft, draws, fx.negs, device=dev)
    if positives == "Positives":
        monkeypatch.setattr(mining, "_csr", _raise)
        monkeypatch.setattr(geo.Positives, "to_lists", _raise)
        monkeypatch.setattr(geo.Positives, "_host_copy", _raise)
        monkeypatch.setattr(geo.Positives, "from_lists", _raise)
    got_table = mining.compute_triplets_random(fx.qfeat_all[sq], fx.feat, sq, hard, soft, torch.from_numpy(table).to(dev), fx.negs,
                                               device=dev)
    assert got_table.dtype == torch.int64 and got_table.shape == (fx.q, 2 + fx.negs)
    assert np.array_equal(got_lists.cpu().numpy(), want) and np.array_equal(got_table.cpu().numpy(), want)
    short = [x.copy() for x in draws]
    short[5] = short[5][short[5] != others[0]]                                  # one non-positive fewer: not enough for that query
    with pytest.raises(ValueError, match="^fewer candidate negatives than negs_num_per_query for some query$"):
        mining.compute_triplets_random(fx.qfeat_all[sq], fx.feat, sq, hard, soft, short, fx.negs, device=dev)
