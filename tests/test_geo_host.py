"""Host side of the geo feature (agplace_amd/geo.py, csrc/geo.hip): argument checks that return before any launch, the
Positives container, the recall arithmetic from a first-hit column, and the promise that lists still take the old routes.
No GPU."""
import ctypes

import numpy as np
import pytest
import torch

from agplace_amd import _lib, geo, mining, retrieval

BADARG = 1
P = 0x1000          # a non-null address: every call below is refused before it could be read


def test_radius_entries_refuse_null_pointers_and_negative_sizes():
    L = _lib.load()
    ok = dict(q=P, nq=4, db=P, nb=4, r2=1.0, counts=P)
    for bad in (dict(q=None), dict(db=None), dict(counts=None), dict(nq=-1), dict(nb=-1), dict(nq=2 ** 31), dict(nb=2 ** 31)):
        a = {**ok, **bad}
        assert L.agp_radius_count(a["q"], a["nq"], a["db"], a["nb"], a["r2"], a["counts"], None) == BADARG, bad
    ok = dict(q=P, nq=4, db=P, nb=4, r2=1.0, off=P, idx=P)
    for bad in (dict(q=None), dict(db=None), dict(off=None), dict(idx=None), dict(nq=-1), dict(nb=-1), dict(nq=2 ** 31)):
        a = {**ok, **bad}
        assert L.agp_radius_fill(a["q"], a["nq"], a["db"], a["nb"], a["r2"], a["off"], a["idx"], None) == BADARG, bad
    # nothing to do: OK without a launch (no GPU here, a launch would fail)
    assert L.agp_radius_count(P, 0, P, 4, 1.0, P, None) == 0 and L.agp_radius_count(P, 4, P, 0, 1.0, P, None) == 0
    assert L.agp_radius_fill(P, 0, P, 4, 1.0, P, P, None) == 0 and L.agp_radius_fill(P, 4, P, 0, 1.0, P, P, None) == 0


def test_first_hit_refuses_bad_arguments_and_k_outside_1_1024():
    L = _lib.load()
    ok = dict(pred=P, nq=4, k=20, off=P, idx=P, first=P)
    for bad in (dict(pred=None), dict(off=None), dict(idx=None), dict(first=None), dict(nq=-1), dict(k=0), dict(k=-3),
                dict(k=1025)):
        a = {**ok, **bad}
        assert L.agp_recall_first_hit(a["pred"], a["nq"], a["k"], a["off"], a["idx"], a["first"], None) == BADARG, bad
    assert L.agp_recall_first_hit(P, 0, 1024, P, P, P, None) == 0
    assert retrieval.MAX_K == geo._MAX_K == 1024


def test_drop_listed_refuses_bad_arguments():
    L = _lib.load()
    ok = dict(I=P, nq=4, k=20, cand=P, nc=100, row=P, off=P, idx=P, negs=10, out=P, filled=P)
    for bad in (dict(I=None), dict(cand=None), dict(row=None), dict(off=None), dict(idx=None), dict(out=None), dict(filled=None),
                dict(nq=-1), dict(nc=-1), dict(k=0), dict(k=1025), dict(negs=0), dict(negs=-1), dict(negs=1025)):
        a = {**ok, **bad}
        assert L.agp_mine_drop_listed(a["I"], a["nq"], a["k"], a["cand"], a["nc"], a["row"], a["off"], a["idx"], a["negs"],
                                      a["out"], a["filled"], None) == BADARG, bad
    assert L.agp_mine_drop_listed(P, 0, 20, P, 100, P, P, P, 10, P, P, None) == 0


def test_python_wrappers_refuse_before_the_library():
    pos = geo.Positives.from_lists([[1, 2], []], device="cpu", sort=True)
    with pytest.raises(ValueError, match="between 1 and 1024"):
        geo.first_hit(torch.zeros((2, 1025), dtype=torch.int64), pos)
    with pytest.raises(ValueError, match="between 1 and 1024"):
        geo.first_hit(torch.zeros((2, 0), dtype=torch.int64), pos)
    with pytest.raises(ValueError, match="do not match"):
        geo.first_hit(torch.zeros((3, 5), dtype=torch.int64), pos)
    with pytest.raises(ValueError, match=r"\[n, 2\]"):
        geo.radius_neighbors(np.zeros((3, 3)), np.zeros((3, 2)), 1.0, device="cpu")
    with pytest.raises(ValueError, match="float32 or float64"):
        geo.radius_neighbors(np.zeros((3, 2), dtype=np.int64), np.zeros((3, 2)), 1.0, device="cpu")
    with pytest.raises(ValueError, match="radius"):
        geo.radius_neighbors(np.zeros((3, 2)), np.zeros((3, 2)), float("nan"), device="cpu")
    empty = geo.radius_neighbors(np.zeros((3, 2)), np.zeros((0, 2)), 5.0, device="cpu")       # no database: no launch
    assert len(empty) == 3 and empty.is_sorted and empty.lengths().tolist() == [0, 0, 0]


def test_positives_round_trips():
    lists = [np.asarray([5, 3, 3, 9]), np.zeros(0, dtype=np.int64), np.asarray([7]), np.asarray([2, 1])]
    p = geo.Positives.from_lists(lists, device="cpu")
    assert not p.is_sorted and len(p) == 4
    assert p.offsets.tolist() == [0, 4, 4, 5, 7] and p.indices.tolist() == [5, 3, 3, 9, 7, 2, 1]
    assert p.lengths().tolist() == [4, 0, 1, 2]
    back = p.to_lists()
    assert all(b.dtype == np.int64 and np.array_equal(b, a) for a, b in zip(lists, back))
    assert np.array_equal(p[0], lists[0]) and np.array_equal(p[-1], lists[3]) and len(p[1]) == 0
    assert [len(x) for x in p] == [4, 0, 1, 2]
    assert [i for i, x in enumerate(p) if len(x) == 0] == [1]              # the reference's filter for queries without positives
    with pytest.raises(IndexError):
        p[4]
    assert p._host_copy() is p._host_copy()                                 # made once
    s = p.sorted_unique()
    assert s.is_sorted and s.sorted_unique() is s
    assert [x.tolist() for x in s.to_lists()] == [[3, 5, 9], [], [7], [1, 2]]
    assert [x.tolist() for x in geo.Positives.from_lists(lists, device="cpu", sort=True)] == [[3, 5, 9], [], [7], [1, 2]]
    sel = s.select(torch.tensor([3, 0, 0, 1]))
    assert [x.tolist() for x in sel] == [[1, 2], [3, 5, 9], [3, 5, 9], []] and sel.is_sorted
    none = geo.Positives.from_lists([[], []], device="cpu", sort=True)
    assert len(none) == 2 and none.indices.numel() == 0 and none.to_lists()[1].dtype == np.int64


class _Args:
    def __init__(self, recall_values):
        self.recall_values = recall_values


class _DS:
    def __init__(self, positives, queries_num):
        self._p, self.queries_num = positives, queries_num

    def get_positives(self):
        return self._p


@pytest.mark.parametrize("recall_values", [[1, 5, 10, 20], [10, 1, 20, 5], [20], [5, 5, 1]])
def test_recall_arithmetic_from_a_hand_made_first_hit(recall_values):
    """recalls_from_first_hit against the reference loop (retrieval.recall_from_predictions with lists) on predictions built to
    have exactly the hand-made first-hit columns; 20 = no hit."""
    first = np.asarray([0, 0, 1, 4, 5, 9, 10, 19, 20, 20, 3, 0, 12], dtype=np.int32)
    k = 20
    pred = np.arange(k, dtype=np.int64)[None, :].repeat(len(first), 0) + 100
    lists = []
    for q, f in enumerate(first):
        lists.append(np.asarray([pred[q, f], pred[q, min(f + 2, k - 1)]]) if f < k else np.asarray([7]))
    want = retrieval.recall_from_predictions(_Args(recall_values), pred, _DS(lists, 17))
    got = geo.recalls_from_first_hit(torch.from_numpy(first), k, recall_values, 17)
    assert np.array_equal(got[0], want[0]) and got[0].dtype == want[0].dtype and got[1] == want[1]


class _Sentinel(Exception):
    pass


def _boom(*a, **k):
    raise _Sentinel


def test_lists_reach_the_old_recall_loop(monkeypatch):
    monkeypatch.setattr(geo, "recall_at", _boom)
    monkeypatch.setattr(geo, "first_hit", _boom)
    pred = np.asarray([[4, 2, 9], [1, 1, 1]], dtype=np.int64)
    recalls, s = retrieval.recall_from_predictions(_Args([1, 3]), pred, _DS([np.asarray([9]), np.asarray([5])], 2))
    assert recalls.tolist() == [0.0, 50.0] and s == "R@1: 0.0, R@3: 50.0"
    # and a Positives takes the device route
    with pytest.raises(_Sentinel):
        retrieval.recall_from_predictions(_Args([1, 3]), pred, _DS(geo.Positives.from_lists([[9], [5]], "cpu", sort=True), 2))


def test_lists_reach_the_old_mining_code(monkeypatch):
    q, db = np.zeros((2, 8), dtype=np.float32), np.zeros((6, 8), dtype=np.float32)
    lists = [np.asarray([1, 2]), np.asarray([3])]
    monkeypatch.setattr(mining, "_hardest_negatives_device", _boom)
    monkeypatch.setattr(mining, "_compute_triplets_partial_device", _boom)
    # lists: the host CSR builder, then the host loop and the search over the sample
    seen = []
    monkeypatch.setattr(mining, "_csr", lambda lists_, dev: seen.append(len(lists_)) or _boom())
    with pytest.raises(_Sentinel):
        mining.best_positive_indexes(q, db, lists, device="cpu")
    with pytest.raises(_Sentinel):
        mining.compute_triplets_partial(q, db, np.asarray([1, 0]), lists, lists, np.arange(6), 2, device="cpu")
    assert seen == [2, 2]

    class Index:
        def __init__(self, *a, **k):
            raise _Sentinel
    monkeypatch.setattr(mining, "IndexFlatL2", Index)
    monkeypatch.setattr(np, "unique", lambda *a, **k: seen.append("unique") or _boom())
    with pytest.raises(_Sentinel):
        mining.hardest_negatives_indexes(q, db, np.arange(6), lists, 2, device="cpu")
    assert seen[-1] == "unique"                                            # the per-query host loop, as before
    # a Positives goes the other way
    pos = geo.Positives.from_lists(lists, "cpu", sort=True)
    monkeypatch.undo()
    monkeypatch.setattr(mining, "_hardest_negatives_device", _boom)
    monkeypatch.setattr(mining, "_csr", lambda *a: pytest.fail("host CSR on the device route"))
    with pytest.raises(_Sentinel):
        mining.hardest_negatives_indexes(q, db, np.arange(6), pos, 2, device="cpu")
