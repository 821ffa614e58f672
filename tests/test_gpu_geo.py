"""-m gpu: the geo kernels (csrc/geo.hip) and their host layer (agplace_amd/geo.py, the Positives routes of retrieval and
mining) against the numpy oracle of tests/geo_ref.py.  Every comparison is exact: integer equality, `==` on the recall floats."""
import functools

import numpy as np
import pytest
import torch

import geo_ref

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A5A5A5A5A
NGUARD = 8


def _guarded(n, dtype, dev, fill=None):
    """(whole buffer, the n-element window behind NGUARD guard words and in front of NGUARD more)."""
    word = GUARD if dtype == torch.int64 else 0x5A5A5A5A
    buf = torch.full((n + 2 * NGUARD,), word, dtype=dtype, device=dev)
    win = buf[NGUARD:NGUARD + n]
    if fill is not None:
        win.fill_(fill)
    return buf, win


def _guards_intact(buf, n):
    word = GUARD if buf.dtype == torch.int64 else 0x5A5A5A5A
    return bool((buf[:NGUARD] == word).all()) and bool((buf[NGUARD + n:] == word).all())


@functools.lru_cache(maxsize=None)
def _radius_cases():
    return {name: (q, db, r, geo_ref.radius_ref(q, db, r)) for name, q, db, r in geo_ref.radius_cases()}


RADIUS_NAMES = [c[0] for c in geo_ref.radius_cases()]


@pytest.mark.parametrize("name", RADIUS_NAMES)
def test_radius_count_and_fill_equal_the_oracle(dev, name):
    from agplace_amd import _lib
    from agplace_amd._lib import check, ptr
    q, db, r, (off_ref, idx_ref) = _radius_cases()[name]
    L = _lib.load()
    qd = torch.from_numpy(q).to(dev, torch.float64).contiguous()
    dbd = torch.from_numpy(db).to(dev, torch.float64).contiguous()
    nq, nb, r2 = len(q), len(db), float(r) * float(r)
    cbuf, counts = _guarded(nq, torch.int64, dev)
    check(L.agp_radius_count(ptr(qd), nq, ptr(dbd), nb, r2, ptr(counts), _lib.stream()), "agp_radius_count")
    assert np.array_equal(counts.cpu().numpy(), np.diff(off_ref))
    assert _guards_intact(cbuf, nq)
    off = torch.from_numpy(off_ref).to(dev)
    total = int(off_ref[-1])
    runs = []
    for _ in range(2):
        ibuf, idx = _guarded(total, torch.int64, dev, fill=-7)
        check(L.agp_radius_fill(ptr(qd), nq, ptr(dbd), nb, r2, ptr(off), ptr(ibuf[NGUARD:]), _lib.stream()), "agp_radius_fill")
        assert _guards_intact(ibuf, total)
        runs.append(idx.cpu().numpy())
    assert np.array_equal(runs[0], idx_ref)
    assert runs[0].tobytes() == runs[1].tobytes()


@pytest.mark.parametrize("name", RADIUS_NAMES)
def test_radius_neighbors_returns_the_oracles_lists(dev, name):
    from agplace_amd import geo
    q, db, r, (off_ref, idx_ref) = _radius_cases()[name]
    p = geo.radius_neighbors(q, db, r, device=dev)
    assert p.is_sorted and len(p) == len(q)
    assert np.array_equal(p.offsets.cpu().numpy(), off_ref) and np.array_equal(p.indices.cpu().numpy(), idx_ref)
    p2 = geo.radius_neighbors(torch.from_numpy(q).to(dev), torch.from_numpy(db), r, device=dev)      # tensors, either side
    assert torch.equal(p2.offsets, p.offsets) and torch.equal(p2.indices, p.indices)
    assert all(np.array_equal(a, b) for a, b in zip(p, geo_ref.csr_lists(off_ref, idx_ref)))


class _Args:
    features_dim = 64

    def __init__(self, recall_values):
        self.recall_values = recall_values


class _DS:
    def __init__(self, positives, queries_num):
        self._p, self.queries_num = positives, queries_num

    def get_positives(self):
        return self._p


@pytest.mark.parametrize("nq", geo_ref.FIRST_HIT_Q)
@pytest.mark.parametrize("k", geo_ref.FIRST_HIT_K)
def test_first_hit_and_recall_equal_the_oracle(dev, k, nq):
    from agplace_amd import _lib, geo, retrieval
    from agplace_amd._lib import check, ptr
    pred, off, idx = geo_ref.first_hit_case(k, nq)
    want = geo_ref.first_hit_ref(pred, off, idx)
    pos = geo.Positives(torch.from_numpy(off).to(dev), torch.from_numpy(idx).to(dev), is_sorted=True)
    pred_d = torch.from_numpy(pred).to(dev)
    fbuf, first = _guarded(nq, torch.int32, dev)
    check(_lib.load().agp_recall_first_hit(ptr(pred_d), nq, k, ptr(pos.offsets), ptr(pos.indices), ptr(first), _lib.stream()),
          "agp_recall_first_hit")
    assert np.array_equal(first.cpu().numpy(), want) and _guards_intact(fbuf, nq)
    assert np.array_equal(geo.first_hit(pred, pos).cpu().numpy(), want)
    # an unsorted CSR is sorted on the device first
    shuffled = [np.random.default_rng(q).permutation(np.repeat(x, 2)) for q, x in enumerate(geo_ref.csr_lists(off, idx))]
    assert np.array_equal(geo.first_hit(pred_d, geo.Positives.from_lists(shuffled, dev)).cpu().numpy(), want)
    lists = geo_ref.csr_lists(off, idx)
    values = [[1, 5, 10, 20], [10, 1, 20, 5]] if k >= 20 else [[1], [1, 1]]
    for rv in values:
        theirs = retrieval.recall_from_predictions(_Args(rv), pred[:, :max(rv)], _DS(lists, nq + 3))
        for p_in in (pred_d[:, :max(rv)], pred[:, :max(rv)]):
            mine = geo.recall_at(p_in, pos, rv, nq + 3)
            assert np.array_equal(mine[0], theirs[0]) and mine[1] == theirs[1]
        routed = retrieval.recall_from_predictions(_Args(rv), pred_d[:, :max(rv)], _DS(pos, nq + 3))
        assert np.array_equal(routed[0], theirs[0]) and routed[1] == theirs[1]


@functools.lru_cache(maxsize=None)
def _fx():
    return geo_ref.MiningFixture()


@functools.lru_cache(maxsize=None)
def _fx_positives():
    from agplace_amd import geo
    fx = _fx()
    soft = geo.radius_neighbors(fx.qutm, fx.utm, 25.0)
    hard = geo.radius_neighbors(fx.qutm, fx.utm, 10.0)
    for p, (off, idx) in ((soft, fx.soft_ref()), (hard, fx.hard_ref())):
        assert np.array_equal(p.offsets.cpu().numpy(), off) and np.array_equal(p.indices.cpu().numpy(), idx)
    return soft, hard


def test_compute_recall_with_positives_equals_lists(dev):
    from agplace_amd import retrieval
    fx = _fx()
    soft, _ = _fx_positives()
    args = _Args([1, 5, 10, 20])
    near = np.asarray([x[0] if len(x) else 0 for x in geo_ref.csr_lists(*fx.soft_ref())])
    qf = fx.feat[near] + 0.3 * fx.qfeat_all                 # descriptors next to one of the query's positives, where it has any
    a = retrieval.compute_recall(args, qf, fx.feat, _DS(soft, len(qf)))
    b = retrieval.compute_recall(args, qf, fx.feat, _DS(soft.to_lists(), len(qf)))
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    assert 0.0 < a[0][-1]


def _raise(*a, **k):
    raise AssertionError("the device route went through host lists")


@pytest.mark.parametrize("which", ["sample_of_1000", "wide_sample_single_query_route"])
def test_triplets_with_positives_equal_the_lists_route(dev, monkeypatch, which):
    from agplace_amd import geo, mining
    fx = _fx()
    soft, hard = _fx_positives()
    sq, cand = (fx.sq, fx.cand) if which == "sample_of_1000" else (fx.sq_wide, fx.cand_wide)
    qf = fx.qfeat_all[sq]
    soft_l, hard_l = soft.to_lists(), hard.to_lists()
    want = mining.compute_triplets_partial(qf, fx.feat, sq, hard_l, soft_l, cand, fx.negs, device=dev)
    monkeypatch.setattr(mining, "_csr", _raise)
    monkeypatch.setattr(geo.Positives, "to_lists", _raise)
    monkeypatch.setattr(geo.Positives, "_host_copy", _raise)
    got = mining.compute_triplets_partial(qf, fx.feat, sq, hard, soft, cand, fx.negs, device=dev)
    assert got.shape == (len(sq), 2 + fx.negs) and torch.equal(got, want)
    only = mining.hardest_negatives_indexes(qf, fx.feat, cand, soft.select(torch.from_numpy(sq).to(dev)), fx.negs, device=dev)
    assert torch.equal(only, want[:, 2:])
    # no negative is one of the query's soft positives; the query without positives has no best positive
    for i in (0, 1, 2):
        assert not np.isin(got[i, 2:].cpu().numpy(), soft_l[sq[i]]).any()
    assert int(got[2, 1]) == -1 and sq[2] == 2


@pytest.mark.parametrize("k", [64, 82, 110])
def test_drop_listed_equals_the_oracle(dev, k):
    """The kernel alone on the search's own labels: k = 64 and 82 leave query 0 (81 listed candidates in front) short."""
    from agplace_amd import _lib, retrieval
    from agplace_amd._lib import check, ptr
    fx = _fx()
    soft, _ = _fx_positives()
    cand_t = torch.from_numpy(fx.cand).to(dev)
    index = retrieval.IndexFlatL2(fx.feat.shape[1], device=dev)
    index.add(torch.from_numpy(fx.feat).to(dev).index_select(0, cand_t))
    _, I = index.search_device(torch.from_numpy(fx.qfeat).to(dev), k)
    nq, negs = len(fx.sq), fx.negs
    obuf, out = _guarded(nq * negs, torch.int64, dev, fill=-1)
    fbuf, filled = _guarded(nq, torch.int32, dev)
    rows = torch.from_numpy(fx.sq).to(dev)
    check(_lib.load().agp_mine_drop_listed(ptr(I), nq, k, ptr(cand_t), len(fx.cand), ptr(rows), ptr(soft.offsets), ptr(soft.indices),
                                           negs, ptr(out), ptr(filled), _lib.stream()), "agp_mine_drop_listed")
    off, idx = fx.soft_ref()
    want_out, want_filled = geo_ref.drop_listed_ref(I.cpu().numpy(), fx.cand, fx.sq, off, idx, negs)
    assert np.array_equal(filled.cpu().numpy(), want_filled) and np.array_equal(out.view(nq, negs).cpu().numpy(), want_out)
    assert _guards_intact(obuf, nq * negs) and _guards_intact(fbuf, nq)
    assert int(want_filled[1]) == {64: 0, 82: 1, 110: negs}[k]


def test_too_few_candidates_is_the_old_error(dev):
    from agplace_amd import mining
    fx = _fx()
    soft, hard = _fx_positives()
    cand = np.arange(12)                                    # all in cluster A: query 0 has no negative among them
    with pytest.raises(ValueError, match="^fewer candidate negatives than negs_num_per_query for some query$"):
        mining.compute_triplets_partial(fx.qfeat_all[:3], fx.feat, np.arange(3), hard, soft, cand, fx.negs, device=dev)
    with pytest.raises(ValueError, match="^fewer candidate negatives than negs_num_per_query for some query$"):
        mining.compute_triplets_partial(fx.qfeat_all[:3], fx.feat, np.arange(3), hard.to_lists(), soft.to_lists(), cand, fx.negs,
                                        device=dev)
