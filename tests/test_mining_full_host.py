"""Host side of full / random mining (agplace_amd/mining.py, agp_mine_topk_listed in csrc/mining.hip): argument checks that
return before any launch, the wrappers' own refusals, and the NegCache container.  No GPU."""
import numpy as np
import pytest
import torch

from agplace_amd import _lib, geo, mining

BADARG = 1
P = 0x1000          # a non-null address: every call below is refused before it could be read


def _call(L, a):
    return L.agp_mine_topk_listed(a["xq"], a["nq"], a["xb"], a["nb"], a["d"], a["cand"], a["ncols"], a["row"], a["off"], a["idx"],
                                  a["exempt"], a["k"], a["out_idx"], a["out_dist"], a["filled"], None)


OK = dict(xq=P, nq=4, xb=P, nb=100, d=32, cand=P, ncols=70, row=P, off=P, idx=P, exempt=10, k=10, out_idx=P, out_dist=P, filled=P)


@pytest.mark.parametrize("bad", [
    dict(k=0), dict(k=129), dict(k=-1),
    dict(ncols=0), dict(ncols=4097),
    dict(d=0), dict(d=-4),
    dict(nq=-1), dict(nb=-1), dict(exempt=-1),
    dict(filled=None), dict(out_idx=None), dict(cand=None), dict(xq=None), dict(xb=None),
    dict(row=None), dict(off=None), dict(idx=None), dict(row=None, off=None), dict(off=None, idx=None), dict(row=None, idx=None),
], ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_topk_listed_refuses_before_a_launch(bad):
    assert _call(_lib.load(), {**OK, **bad}) == BADARG


def test_topk_listed_takes_the_limits_and_nothing_to_do():
    L = _lib.load()
    # nq == 0: OK without a launch (no GPU here, a launch would fail), at the limits, with and without the optional arguments
    assert _call(L, {**OK, "nq": 0}) == 0
    assert _call(L, {**OK, "nq": 0, "k": 128, "ncols": 4096, "exempt": 0}) == 0
    assert _call(L, {**OK, "nq": 0, "k": 1, "ncols": 1, "row": None, "off": None, "idx": None, "out_dist": None}) == 0
    assert _call(L, {**OK, "nq": 0, "nb": 0, "xb": None}) == 0
    assert mining.MINE_MAX_K == 128 and mining.MINE_MAX_COLS == 4096


def test_limits_are_named_in_the_header():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "agplace_hip.h")).read()
    assert int(re.search(r"#define AGP_MINE_MAX_K (\d+)", hdr).group(1)) == mining.MINE_MAX_K
    assert int(re.search(r"#define AGP_MINE_MAX_COLS (\d+)", hdr).group(1)) == mining.MINE_MAX_COLS


class _Sentinel(Exception):
    pass


@pytest.fixture
def no_library(monkeypatch):
    """Any call into the library fails the test: the wrappers below must refuse first."""
    def boom():
        raise _Sentinel
    monkeypatch.setattr(_lib, "load", boom)


def test_nearest_listed_refuses_before_the_library(no_library):
    q, db = np.zeros((3, 8), dtype=np.float32), np.zeros((20, 8), dtype=np.float32)
    cand = np.zeros((3, 12), dtype=np.int64)
    for k in (0, 129, -1):
        with pytest.raises(ValueError, match="between 1 and 128"):
            mining.nearest_listed(q, db, cand, k, device="cpu")
    with pytest.raises(ValueError, match="between 1 and 4096 candidate columns"):
        mining.nearest_listed(q, db, np.zeros((3, 4097), dtype=np.int64), 10, device="cpu")
    with pytest.raises(ValueError, match="between 1 and 4096 candidate columns"):
        mining.nearest_listed(q, db, np.zeros((3, 0), dtype=np.int64), 10, device="cpu")
    with pytest.raises(ValueError, match="one row of candidates per query"):
        mining.nearest_listed(q, db, np.zeros((4, 12), dtype=np.int64), 10, device="cpu")
    with pytest.raises(ValueError, match="features must be"):
        mining.nearest_listed(q, np.zeros((20, 9), dtype=np.float32), cand, 10, device="cpu")
    with pytest.raises(ValueError, match="exclusion lists for 3 queries"):
        mining.nearest_listed(q, db, cand, 10, exclude=[[1], [2]], device="cpu")
    with pytest.raises(ValueError, match="exclude_rows for 3 queries"):
        mining.nearest_listed(q, db, cand, 10, exclude=[[1], [2]], exclude_rows=np.asarray([0, 1]), device="cpu")
    with pytest.raises(IndexError):
        mining.nearest_listed(q, db, cand, 10, exclude=[[1], [2]], exclude_rows=np.asarray([0, 1, 2]), device="cpu")
    with pytest.raises(ValueError, match="exclude_rows without exclude"):
        mining.nearest_listed(q, db, cand, 10, exclude_rows=np.arange(3), device="cpu")
    with pytest.raises(ValueError, match="exempt_cols"):
        mining.nearest_listed(q, db, cand, 10, exempt_cols=-1, device="cpu")
    with pytest.raises(_Sentinel):                                          # and a good call does reach the library
        mining.nearest_listed(q, db, cand, 10, exclude=[[1], [2], []], exempt_cols=2, device="cpu")


def test_triplet_functions_refuse_before_the_library(no_library):
    q, db = np.zeros((3, 8), dtype=np.float32), np.zeros((50, 8), dtype=np.float32)
    lists = [np.asarray([1, 2]), np.asarray([3]), np.zeros(0, dtype=np.int64), np.asarray([4])]
    pos = geo.Positives.from_lists(lists, "cpu", sort=True)
    samp = np.arange(36, dtype=np.int64).reshape(3, 12)
    cache = mining.NegCache(4, 5, device="cpu")
    for p in (lists, pos):
        with pytest.raises(ValueError, match="duplicate entries in sampled_queries_indexes"):
            mining.compute_triplets_full(q, db, np.asarray([1, 3, 1]), p, p, samp, cache, 5, device="cpu")
        with pytest.raises(ValueError, match="duplicate entries in sampled_queries_indexes"):
            mining.compute_triplets_random(q, db, np.asarray([2, 2, 0]), p, p, samp, 5, device="cpu")
        with pytest.raises(ValueError, match=r"sampled_negatives must be \[3, S\]"):
            mining.compute_triplets_full(q, db, np.asarray([1, 3, 0]), p, p, samp[:2], cache, 5, device="cpu")
        with pytest.raises(ValueError, match=r"drawn_negatives must be \[3, W\]"):
            mining.compute_triplets_random(q, db, np.asarray([1, 3, 0]), p, p, samp[:2], 5, device="cpu")
        with pytest.raises(ValueError, match="rows of query features"):
            mining.compute_triplets_full(q, db, np.asarray([1, 3]), p, p, samp[:2], cache, 5, device="cpu")
        with pytest.raises(IndexError):
            mining.compute_triplets_full(q, db, np.asarray([1, 4, 0]), p, p, samp, cache, 5, device="cpu")
        with pytest.raises(ValueError, match="neg_cache holds 5 negatives"):
            mining.compute_triplets_full(q, db, np.asarray([1, 3, 0]), p, p, samp, cache, 6, device="cpu")
        with pytest.raises(ValueError, match="between 1 and 4096 candidate columns"):
            mining.compute_triplets_full(q, db, np.asarray([1, 3, 0]), p, p, np.zeros((3, 4092), dtype=np.int64), cache, 5,
                                         device="cpu")
        with pytest.raises(ValueError, match="between 1 and 128"):
            mining.compute_triplets_full(q, db, np.asarray([1, 3, 0]), p, p, samp, mining.NegCache(4, 129, device="cpu"), 129,
                                         device="cpu")
    assert bool((cache.table == -1).all())
    with pytest.raises(ValueError, match="2 draws for 3 sampled queries"):
        mining.compute_triplets_random(q, db, np.asarray([1, 3, 0]), lists, lists, [np.arange(6), np.arange(7)], 5, device="cpu")


def test_neg_cache_round_trips_lists():
    ref = [np.empty((0,), dtype=np.int32), np.asarray([7, 3, 9, 1, 4], dtype=np.int32), np.asarray([2, 8], dtype=np.int32),
           np.empty((0,), dtype=np.int32)]
    c = mining.NegCache.from_lists(ref, 5, device="cpu")
    assert len(c) == 4 and c.negs == 5 and c.table.dtype == torch.int64 and c.device.type == "cpu"
    assert c.table.tolist() == [[-1] * 5, [7, 3, 9, 1, 4], [2, 8, -1, -1, -1], [-1] * 5]
    back = c.to_lists()
    assert all(b.dtype == np.int32 and np.array_equal(a, b) for a, b in zip(ref, back))
    fresh = mining.NegCache(3, 4, device="cpu")
    assert fresh.table.shape == (3, 4) and all(len(x) == 0 and x.dtype == np.int32 for x in fresh.to_lists())
    assert fresh.rows(np.asarray([2, 0])).tolist() == [[-1] * 4] * 2
    fresh.update(np.asarray([2, 0]), torch.tensor([[5, 6, 7, 8], [1, 2, 3, 4]]))
    assert [x.tolist() for x in fresh.to_lists()] == [[1, 2, 3, 4], [], [5, 6, 7, 8]]
    got = fresh.rows(torch.tensor([2]))
    got[0, 0] = 99                                                          # a copy: the cache does not follow
    assert fresh.table[2, 0] == 5
    with pytest.raises(ValueError, match="more than negs"):
        mining.NegCache.from_lists([np.arange(6)], 5, device="cpu")
