"""Batched triplet mining on the GPU.

The reference mines per query in a python loop (`compute_triplets_partial_sep`,
datasets/datasets_ws_nuscenes.py:1372-1410): for each of `cache_refresh_rate` sampled queries it
builds TWO faiss indexes (best positive :1241-1248, hardest negatives :1250-1258) from rows of a
host-side feature cache.  Here the cache stays on the device and the whole refresh is
    * one `agp_mine_best_positive` launch over the ragged positive lists, and
    * one `agp_knn_search` over the sampled database rows with k = negs + (most soft positives any
      query has inside the sample), followed by dropping each query's soft positives;
results are identical to the per-query loop: same candidate order (np.setdiff1d(..., assume_unique=True) keeps the
random sample's order), same tie rule (earlier candidate wins), exact distances.

The other two modes of `--mining` give every query candidates of its OWN, so no shared search serves them:
    * `full` (compute_triplets_full, :1295-1322): a private random sample minus the soft positives, merged with the negatives the
      query kept last time (`NegCache`, the reference's self.neg_cache), searched, written back.  One `agp_mine_topk_listed`
      launch (`nearest_listed`) over the [Q, negs + S] table of candidates;
    * `random` (compute_triplets_random, :1264-1289): the first `negs` of a private draw that are not soft positives: tensor ops.
The random draws stay with the caller, as `sampled_database_indexes` does for `partial`.
"""
import numpy as np
import torch

from . import _lib
from ._lib import check, ptr
from .geo import Positives
from .retrieval import IndexFlatL2, MAX_K      # MAX_K: agp_knn_search's limit on k

MINE_MAX_K = 128        # AGP_MINE_MAX_K (include/agplace_hip.h): agp_mine_topk_listed's limit on k
MINE_MAX_COLS = 4096    # AGP_MINE_MAX_COLS: its limit on the columns of the candidate table
_TOO_FEW = "fewer candidate negatives than negs_num_per_query for some query"


def _dev(x, device, dtype):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    return x.to(device=device, dtype=dtype).contiguous()


def _csr(lists, device):
    lens = [len(x) for x in lists]
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    flat = np.concatenate([np.asarray(x, dtype=np.int64).reshape(-1) for x in lists]) if off[-1] else \
        np.zeros(0, dtype=np.int64)
    return torch.from_numpy(off).to(device), torch.from_numpy(flat).to(device)


def best_positive_indexes(query_features, database_features, hard_positives_per_query, device="cuda"):
    """[Q] int64: for query i the row of `database_features` among hard_positives_per_query[i] nearest
    in feature space (reference get_best_positive_index, :1241-1248); -1 for an empty list.
    hard_positives_per_query: a list of Q index arrays, or a geo.Positives with Q rows, which is read where it lies."""
    dev = torch.device(device)
    xq = _dev(query_features, dev, torch.float32)
    xb = _dev(database_features, dev, torch.float32)
    if isinstance(hard_positives_per_query, Positives):
        if len(hard_positives_per_query) != xq.shape[0]:
            raise ValueError("best_positive_indexes: one list of hard positives per query is needed")
        off, idx = hard_positives_per_query.offsets.to(dev), hard_positives_per_query.indices.to(dev)
    else:
        off, idx = _csr(hard_positives_per_query, dev)
    if idx.numel() == 0:
        idx = torch.zeros(1, dtype=torch.int64, device=dev)
    out = torch.empty(xq.shape[0], dtype=torch.int64, device=dev)
    check(_lib.load().agp_mine_best_positive(ptr(xq), xq.shape[0], ptr(xb), xb.shape[0], xq.shape[1], ptr(off), ptr(idx),
                                             ptr(out), None, _lib.stream()), "agp_mine_best_positive")
    return out


def hardest_negatives_indexes(query_features, database_features, sampled_database_indexes, soft_positives_per_query,
                              negs_num_per_query=10, device="cuda"):
    """[Q, negs] int64 database rows: per query the `negs` nearest rows of
    np.setdiff1d(sampled_database_indexes, soft_positives, assume_unique=True) (reference :1394-1404 + :1250-1258).
    Candidates keep the order of `sampled_database_indexes` (setdiff1d with assume_unique=True does not sort), so
    equal distances resolve to the earlier SAMPLED row, as an index built over that array would.
    One batched search with k = negs + (most in-sample soft positives of any query) serves every query whose soft
    positives leave k <= MAX_K (1024); a query with more in-sample soft positives than that is searched on its own
    over its own candidate set, like the reference does for every query.
    soft_positives_per_query: a list of Q index arrays, or a geo.Positives with Q rows; the latter stays on the device (no host
    loop over the queries: agp_mine_drop_listed removes the listed rows from the search's result)."""
    dev = torch.device(device)
    xq = _dev(query_features, dev, torch.float32)
    xb = _dev(database_features, dev, torch.float32)
    if isinstance(soft_positives_per_query, Positives):
        if len(soft_positives_per_query) != xq.shape[0]:
            raise ValueError("hardest_negatives_indexes: one list of soft positives per query is needed")
        return _hardest_negatives_device(xq, xb, sampled_database_indexes, soft_positives_per_query,
                                         torch.arange(xq.shape[0], device=dev), negs_num_per_query)
    cand = np.asarray(sampled_database_indexes, dtype=np.int64).reshape(-1)      # the sample's own order
    nq, nc = xq.shape[0], cand.shape[0]
    order = np.argsort(cand, kind="stable")
    sorted_c = cand[order]
    # soft positives that actually lie in the sample, as candidate POSITIONS per query
    hits_per_q = []
    for soft in soft_positives_per_query:
        soft = np.unique(np.asarray(soft, dtype=np.int64).reshape(-1))
        if soft.size == 0 or nc == 0:
            hits_per_q.append(np.zeros(0, dtype=np.int64))
            continue
        lo, hi = np.searchsorted(sorted_c, soft, "left"), np.searchsorted(sorted_c, soft, "right")
        if np.all(hi - lo <= 1):
            hits = order[lo[hi > lo]]
        else:                                   # a sampled row listed twice: every copy is a soft positive
            hits = np.concatenate([order[a:b] for a, b in zip(lo, hi)]) if lo.size else np.zeros(0, dtype=np.int64)
        hits_per_q.append(np.sort(hits))
    counts = np.array([h.size for h in hits_per_q], dtype=np.int64)
    if nq and nc - int(counts.max(initial=0)) < negs_num_per_query:
        raise ValueError("fewer candidate negatives than negs_num_per_query for some query")
    out = torch.empty((nq, negs_num_per_query), dtype=torch.int64, device=dev)
    cand_t = torch.from_numpy(cand).to(dev)
    batched = np.nonzero(counts <= MAX_K - negs_num_per_query)[0]
    single = np.nonzero(counts > MAX_K - negs_num_per_query)[0]
    if batched.size:
        most = int(counts[batched].max())
        k = min(nc, negs_num_per_query + most)
        index = IndexFlatL2(xq.shape[1], device=dev)
        index.add(xb.index_select(0, cand_t))
        bt = torch.from_numpy(batched).to(dev)
        xqb = xq if batched.size == nq else xq.index_select(0, bt)
        _, I = index.search_device(xqb, k)                                      # [Qb,k] positions in cand, nearest first
        nb = batched.size
        if most:
            pos_q = np.concatenate([np.full(hits_per_q[q].size, i, dtype=np.int64) for i, q in enumerate(batched)])
            pos_c = np.concatenate([hits_per_q[q] for q in batched])
            keys = torch.from_numpy(pos_q * nc + pos_c).to(dev)
            rowkey = torch.arange(nb, device=dev).view(-1, 1) * nc + I
            keep = ~torch.isin(rowkey, keys)
        else:
            keep = torch.ones_like(I, dtype=torch.bool)
        rank = torch.cumsum(keep, 1) - 1                                        # rank among kept entries
        sel = keep & (rank < negs_num_per_query)
        rows = bt.view(-1, 1).expand_as(I)
        out[rows[sel], rank[sel]] = cand_t[I[sel]]
    for q in single:
        mask = np.ones(nc, dtype=bool)
        mask[hits_per_q[q]] = False
        sub = cand[mask]                                                        # sampled order, soft positives removed
        sub_t = torch.from_numpy(sub).to(dev)
        index = IndexFlatL2(xq.shape[1], device=dev)
        index.add(xb.index_select(0, sub_t))
        _, I = index.search_device(xq[q:q + 1], negs_num_per_query)
        out[q] = sub_t[I[0]]
    return out


def _hardest_negatives_device(xq, xb, sampled_database_indexes, soft, row_of_q, negs):
    """hardest_negatives_indexes with the soft positives as a device CSR: query i's list is row row_of_q[i] of `soft` (int64
    on the device), so the sampled queries' lists are never gathered.  Same result as the list route."""
    dev = xq.device
    soft = soft.sorted_unique()
    if soft.device != dev:
        soft = Positives(soft.offsets.to(dev), soft.indices.to(dev), True)
    cand_t = sampled_database_indexes if torch.is_tensor(sampled_database_indexes) else \
        torch.from_numpy(np.ascontiguousarray(np.asarray(sampled_database_indexes, dtype=np.int64).reshape(-1)))
    cand_t = cand_t.to(device=dev, dtype=torch.int64).reshape(-1).contiguous()            # the sample's own order
    nq, nc, ndb = xq.shape[0], cand_t.shape[0], xb.shape[0]
    out = torch.empty((nq, negs), dtype=torch.int64, device=dev)
    if nq == 0:
        return out
    # in-sample soft positives per query: how often every database row was sampled, gathered through the CSR, summed per row
    times = torch.bincount(cand_t, minlength=ndb) if nc else torch.zeros(max(ndb, 1), dtype=torch.int64, device=dev)
    idx = soft.indices
    w = torch.where((idx >= 0) & (idx < times.numel()), times[idx.clamp(0, times.numel() - 1)], torch.zeros_like(idx))
    run = torch.zeros(idx.numel() + 1, dtype=torch.int64, device=dev)
    torch.cumsum(w, 0, out=run[1:])
    counts = (run[soft.offsets[1:]] - run[soft.offsets[:-1]])[row_of_q]                   # [nq]
    most_all = int(counts.max())                                                          # the one host read that chooses k
    if nc - most_all < negs:
        raise ValueError("fewer candidate negatives than negs_num_per_query for some query")
    L = _lib.load()
    pos_idx = idx if idx.numel() else torch.zeros(1, dtype=torch.int64, device=dev)
    if most_all <= MAX_K - negs:
        bt, xqb, rows_b, most = None, xq, row_of_q, most_all
        single = []
    else:
        fits = counts <= MAX_K - negs
        bt = torch.nonzero(fits).view(-1)
        single = torch.nonzero(~fits).view(-1).tolist()
        xqb, rows_b = xq.index_select(0, bt), row_of_q.index_select(0, bt).contiguous()
        most = int(counts[bt].max()) if bt.numel() else 0
    if xqb.shape[0]:
        k = min(nc, negs + most)
        index = IndexFlatL2(xq.shape[1], device=dev)
        index.add(xb.index_select(0, cand_t))
        _, I = index.search_device(xqb, k)                                                # [Qb,k] positions in cand, nearest first
        nqb = xqb.shape[0]
        out_b = out if bt is None else torch.empty((nqb, negs), dtype=torch.int64, device=dev)
        filled = torch.empty(nqb, dtype=torch.int32, device=dev)
        check(L.agp_mine_drop_listed(ptr(I), nqb, k, ptr(cand_t), nc, ptr(rows_b), ptr(soft.offsets), ptr(pos_idx), negs,
                                     ptr(out_b), ptr(filled), _lib.stream()), "agp_mine_drop_listed")
        if int(filled.min()) < negs:
            raise RuntimeError("hardest_negatives_indexes: the batched search left a query short of negatives")
        if bt is not None:
            out[bt] = out_b
    for q in single:                                     # today's single-query route, the query's list read on the device
        r = int(row_of_q[q])
        mine = idx[int(soft.offsets[r]):int(soft.offsets[r + 1])]                         # ascending, not empty
        at = torch.searchsorted(mine, cand_t).clamp(max=mine.numel() - 1)
        sub_t = cand_t[mine[at] != cand_t]                                                # sampled order, soft positives removed
        index = IndexFlatL2(xq.shape[1], device=dev)
        index.add(xb.index_select(0, sub_t))
        _, I = index.search_device(xq[q:q + 1], negs)
        out[q] = sub_t[I[0]]
    return out


def compute_triplets_partial(query_features, database_features, sampled_queries_indexes, hard_positives_per_query,
                             soft_positives_per_query, sampled_database_indexes, negs_num_per_query=10, device="cuda"):
    """The triplet table of `compute_triplets_partial_sep` (:1372-1410): int64 [Q, 2 + negs] rows
    (query_index, best_positive_index, neg_indexes...).  `query_features[i]` belongs to
    sampled_queries_indexes[i]; the two per-query lists are indexed by the GLOBAL query index, as
    in the reference dataset object.  Either list may be a geo.Positives over all queries: it is then read on the device
    (the hard rows gathered by tensor indexing, the soft rows addressed in place), with the result of the same lists."""
    sq = np.asarray(sampled_queries_indexes, dtype=np.int64)
    if isinstance(hard_positives_per_query, Positives) or isinstance(soft_positives_per_query, Positives):
        return _compute_triplets_partial_device(query_features, database_features, sq, hard_positives_per_query,
                                                soft_positives_per_query, sampled_database_indexes, negs_num_per_query, device)
    hard = [hard_positives_per_query[i] for i in sq]
    soft = [soft_positives_per_query[i] for i in sq]
    best = best_positive_indexes(query_features, database_features, hard, device)
    negs = hardest_negatives_indexes(query_features, database_features, sampled_database_indexes, soft,
                                     negs_num_per_query, device)
    return torch.cat([torch.from_numpy(sq).to(best.device).view(-1, 1), best.view(-1, 1), negs], 1)


def _compute_triplets_partial_device(query_features, database_features, sq, hard_positives_per_query, soft_positives_per_query,
                                     sampled_database_indexes, negs_num_per_query, device):
    dev = torch.device(device)
    xq = _dev(query_features, dev, torch.float32)
    xb = _dev(database_features, dev, torch.float32)
    for p in (hard_positives_per_query, soft_positives_per_query):
        if sq.size and not (0 <= sq.min() and sq.max() < len(p)):
            raise IndexError("compute_triplets_partial: sampled query index outside the lists of positives")
    sq_t = torch.from_numpy(sq).to(dev)
    if isinstance(hard_positives_per_query, Positives):
        hard = hard_positives_per_query.select(sq_t.to(hard_positives_per_query.device))
    else:
        hard = [hard_positives_per_query[i] for i in sq]
    best = best_positive_indexes(xq, xb, hard, dev)
    if isinstance(soft_positives_per_query, Positives):
        negs = _hardest_negatives_device(xq, xb, sampled_database_indexes, soft_positives_per_query, sq_t, negs_num_per_query)
    else:
        negs = hardest_negatives_indexes(xq, xb, sampled_database_indexes, [soft_positives_per_query[i] for i in sq],
                                         negs_num_per_query, dev)
    return torch.cat([sq_t.view(-1, 1), best.view(-1, 1), negs], 1)


def compute_triplets_partial_sharded(query_features, database_features, sampled_queries_indexes, hard_positives_per_query,
                                     soft_positives_per_query, sampled_database_indexes, negs_num_per_query=10, device="cuda"):
    """Data-parallel cache refresh (the loop it shards: reference datasets_ws_nuscenes.py:1398-1410).
    Every rank holds the whole feature cache (the all-gather of the sharded cache extraction is the exchange step) and
    the same sampled index arrays (same seed); rank r mines its contiguous shard of the sampled queries
    (parallel.shard_range) and the [Q_r, 2 + negs] tables are all-gathered: every rank returns the full table, equal to
    compute_triplets_partial on one rank."""
    from . import parallel
    import torch.distributed as dist
    sq = np.asarray(sampled_queries_indexes, dtype=np.int64)
    rank = dist.get_rank() if dist.is_initialized() else 0
    world = dist.get_world_size() if dist.is_initialized() else 1
    lo, hi = parallel.shard_range(len(sq), rank, world)
    qf = query_features[lo:hi]
    local, err = None, None
    try:
        if hi > lo:
            local = compute_triplets_partial(qf, database_features, sq[lo:hi], hard_positives_per_query, soft_positives_per_query,
                                             sampled_database_indexes, negs_num_per_query, device)
        else:
            local = torch.zeros((0, 2 + negs_num_per_query), dtype=torch.int64, device=torch.device(device))
    except ValueError as e:          # e.g. too few candidate negatives for one of THIS shard's queries only
        err = f"rank {rank}: {e}"
    # a failure on one rank must fail every rank BEFORE the gather (the others would wait in the collective for ever)
    errs = [e for e in parallel.all_gather_object(err) if e]
    if errs:
        raise ValueError("compute_triplets_partial_sharded: " + "; ".join(errs))
    return parallel.all_gather_rows(local)


# ---------------------------------------------------------------------------------------------- full and random mining

def _exclusion_on(exclude, dev):
    """`exclude` (a Positives or a list of index arrays) as a Positives with ascending rows on `dev`."""
    if not isinstance(exclude, Positives):
        exclude = Positives.from_lists(exclude, dev)
    exclude = exclude.sorted_unique()
    if exclude.device != dev:
        exclude = Positives(exclude.offsets.to(dev), exclude.indices.to(dev), True)
    return exclude


def _topk_listed(xq, xb, cand, k, exclude, rows, exempt_cols):
    """The launch behind nearest_listed, its arguments checked and on one device: exclude a sorted Positives or None."""
    nq, ncols = cand.shape
    dev = xq.device
    idx = torch.empty((nq, k), dtype=torch.int64, device=dev)
    filled = torch.empty(nq, dtype=torch.int32, device=dev)
    off_p = idx_p = rows_p = None
    if exclude is not None:
        keep = exclude.indices if exclude.indices.numel() else torch.zeros(1, dtype=torch.int64, device=dev)
        off_p, idx_p, rows_p = ptr(exclude.offsets), ptr(keep), ptr(rows)
    check(_lib.load().agp_mine_topk_listed(ptr(xq), nq, ptr(xb) if xb.shape[0] else None, xb.shape[0], xq.shape[1], ptr(cand),
                                           ncols, rows_p, off_p, idx_p, exempt_cols, k, ptr(idx), None, ptr(filled),
                                           _lib.stream()), "agp_mine_topk_listed")
    return idx, filled


def _check_topk_shapes(what, xq, xb, cand, k):
    if xq.dim() != 2 or xb.dim() != 2 or xq.shape[1] != xb.shape[1] or xq.shape[1] == 0:
        raise ValueError(f"{what}: features must be [Q, d] and [N, d] with one d > 0, got {tuple(xq.shape)} and {tuple(xb.shape)}")
    if cand.dim() != 2 or cand.shape[0] != xq.shape[0]:
        raise ValueError(f"{what}: one row of candidates per query is needed, got {tuple(cand.shape)} for {xq.shape[0]} queries")
    if not 1 <= k <= MINE_MAX_K:
        raise ValueError(f"{what}: k must lie between 1 and {MINE_MAX_K}, got {k}")
    if not 1 <= cand.shape[1] <= MINE_MAX_COLS:
        raise ValueError(f"{what}: between 1 and {MINE_MAX_COLS} candidate columns are supported, got {cand.shape[1]}")


def nearest_listed(query_features, database_features, candidates, k, exclude=None, exclude_rows=None, exempt_cols=0,
                   device="cuda"):
    """(idx int64 [Q, k], filled int32 [Q]) on the device: per query the k nearest DISTINCT rows of `database_features` among
    row q of `candidates` (int64 [Q, ncols], any order, padded with -1), nearest first; one agp_mine_topk_listed launch.
    An entry counts when it lies in [0, N) and is not in the query's exclusion list: `exclude` (a geo.Positives or a list of
    index arrays) read at row exclude_rows[q] (default q).  The first `exempt_cols` columns are never excluded.
    Order: (exact fp64 squared distance, database row), both ascending, so equal distances resolve to the SMALLER row, whatever
    the order of the columns; a row listed twice counts once; a candidate at a non-finite distance comes behind every finite one.
    filled[q] = how many distinct valid candidates there were, at most k; idx[q, filled[q]:] = -1.
    1 <= k <= 128, 1 <= ncols <= 4096; ValueError otherwise, and for shapes that do not agree."""
    dev = torch.device(device)
    xq = _dev(query_features, dev, torch.float32)
    xb = _dev(database_features, dev, torch.float32)
    cand = _dev(candidates, dev, torch.int64)
    k, exempt_cols = int(k), int(exempt_cols)
    _check_topk_shapes("nearest_listed", xq, xb, cand, k)
    if exempt_cols < 0:
        raise ValueError(f"nearest_listed: exempt_cols must be >= 0, got {exempt_cols}")
    nq = xq.shape[0]
    rows = None
    if exclude is None:
        if exclude_rows is not None:
            raise ValueError("nearest_listed: exclude_rows without exclude")
    else:
        exclude = _exclusion_on(exclude, dev)
        if exclude_rows is None:
            if len(exclude) != nq:
                raise ValueError(f"nearest_listed: {len(exclude)} exclusion lists for {nq} queries (give exclude_rows to address them)")
            rows = torch.arange(nq, dtype=torch.int64, device=dev)
        else:
            rows = _dev(exclude_rows, dev, torch.int64).reshape(-1)
            if rows.numel() != nq:
                raise ValueError(f"nearest_listed: {rows.numel()} exclude_rows for {nq} queries")
            if nq and not (0 <= int(rows.min()) and int(rows.max()) < len(exclude)):
                raise IndexError("nearest_listed: exclude_rows outside the exclusion lists")
    return _topk_listed(xq, xb, cand, k, exclude, rows, exempt_cols)


class NegCache:
    """The negatives every query kept at its last `full` refresh (the reference's self.neg_cache, :1026 and :1315-1319) as ONE
    device table: int64 [queries_num, negs], -1 where a query has not been mined yet."""

    def __init__(self, queries_num, negs=10, device="cuda"):
        self.table = torch.full((int(queries_num), int(negs)), -1, dtype=torch.int64, device=torch.device(device))

    @property
    def negs(self):
        return self.table.shape[1]

    @property
    def device(self):
        return self.table.device

    def __len__(self):
        return self.table.shape[0]

    def _index(self, sq):
        if not torch.is_tensor(sq):
            sq = torch.from_numpy(np.ascontiguousarray(np.asarray(sq, dtype=np.int64).reshape(-1)))
        return sq.to(device=self.device, dtype=torch.int64)

    def rows(self, sq):
        """int64 [len(sq), negs]: the cached negatives of the given queries (a copy)."""
        return self.table.index_select(0, self._index(sq))

    def update(self, sq, negs):
        """Row sq[i] = negs[i] (int64 [len(sq), negs])."""
        self.table[self._index(sq)] = negs.to(device=self.device, dtype=torch.int64)

    def to_lists(self):
        """The reference's form: per query an int32 array, the -1 entries dropped (empty before the query's first refresh)."""
        host = self.table.cpu().numpy()
        return [row[row >= 0].astype(np.int32) for row in host]

    @classmethod
    def from_lists(cls, lists, negs=10, device="cuda"):
        host = np.full((len(lists), int(negs)), -1, dtype=np.int64)
        for i, x in enumerate(lists):
            x = np.asarray(x, dtype=np.int64).reshape(-1)
            if x.size > negs:
                raise ValueError(f"NegCache.from_lists: list {i} has {x.size} entries, more than negs = {negs}")
            host[i, :x.size] = x
        cache = cls(0, negs, device)
        cache.table = torch.from_numpy(host).to(torch.device(device))
        return cache


def _sampled_queries(what, sampled_queries_indexes, xq, *per_query):
    sq = np.asarray(sampled_queries_indexes, dtype=np.int64).reshape(-1)
    if xq.shape[0] != sq.size:
        raise ValueError(f"{what}: {xq.shape[0]} rows of query features for {sq.size} sampled queries")
    if np.unique(sq).size != sq.size:
        raise ValueError(f"{what}: duplicate entries in sampled_queries_indexes")
    for p in per_query:
        if sq.size and not (0 <= sq.min() and sq.max() < len(p)):
            raise IndexError(f"{what}: sampled query index outside the per-query lists")
    return sq


def _best_of_sampled(xq, xb, hard_positives_per_query, sq, sq_t, dev):
    if isinstance(hard_positives_per_query, Positives):
        hard = hard_positives_per_query.select(sq_t.to(hard_positives_per_query.device))
    else:
        hard = [hard_positives_per_query[i] for i in sq]
    return best_positive_indexes(xq, xb, hard, dev)


def _soft_of_sampled(soft_positives_per_query, sq, sq_t, dev):
    """(sorted Positives on dev, the row of every sampled query in it): a Positives over all queries is read where it lies."""
    if isinstance(soft_positives_per_query, Positives):
        return _exclusion_on(soft_positives_per_query, dev), sq_t
    soft = Positives.from_lists([soft_positives_per_query[i] for i in sq], dev, sort=True)
    return soft, torch.arange(sq.size, dtype=torch.int64, device=dev)


def compute_triplets_full(query_features, database_features, sampled_queries_indexes, hard_positives_per_query,
                          soft_positives_per_query, sampled_negatives, neg_cache, negs_num_per_query=10, device="cuda"):
    """The triplet table of the reference's `full` mining (compute_triplets_full, :1295-1322): int64 [Q, 2 + negs] rows
    (query_index, best_positive_index, neg_indexes...), and `neg_cache` updated with the negatives found.
    sampled_negatives int64 [Q, S]: row i is query i's own np.random.choice(database_num, neg_samples_num, replace=False).
    Per query the candidates are its cached negatives (never filtered, as in the reference) and its sample minus its soft
    positives; the `negs` nearest distinct ones are taken, the smaller row first at equal distance -- what the reference's
    search over np.unique(...) gives.  One nearest_listed launch over cat([neg_cache.rows(sq), sampled_negatives], 1).
    The per-query lists are indexed by the GLOBAL query index and may be lists or geo.Positives, as in
    compute_triplets_partial; with two Positives no host loop runs over the queries.
    ValueError: duplicate sampled queries (the reference's sequential cache update would make one depend on the other), or a
    query with fewer than `negs` distinct candidates; neg_cache is then left as it was."""
    dev = torch.device(device)
    negs = int(negs_num_per_query)
    xq = _dev(query_features, dev, torch.float32)
    xb = _dev(database_features, dev, torch.float32)
    sq = _sampled_queries("compute_triplets_full", sampled_queries_indexes, xq, hard_positives_per_query, soft_positives_per_query,
                          neg_cache)
    samp = _dev(sampled_negatives, dev, torch.int64)
    if samp.dim() != 2 or samp.shape[0] != sq.size:
        raise ValueError(f"compute_triplets_full: sampled_negatives must be [{sq.size}, S], got {tuple(samp.shape)}")
    if neg_cache.negs != negs:
        raise ValueError(f"compute_triplets_full: neg_cache holds {neg_cache.negs} negatives per query, negs_num_per_query is {negs}")
    sq_t = torch.from_numpy(sq).to(dev)
    cand = torch.cat([neg_cache.rows(sq_t).to(dev), samp], 1)
    _check_topk_shapes("compute_triplets_full", xq, xb, cand, negs)
    best = _best_of_sampled(xq, xb, hard_positives_per_query, sq, sq_t, dev)
    soft, rows = _soft_of_sampled(soft_positives_per_query, sq, sq_t, dev)
    found, filled = _topk_listed(xq, xb, cand, negs, soft, rows, negs)
    if sq.size and int(filled.min()) < negs:
        raise ValueError(_TOO_FEW)
    neg_cache.update(sq_t, found)
    return torch.cat([sq_t.view(-1, 1), best.view(-1, 1), found], 1)


def compute_triplets_random(query_features, database_features, sampled_queries_indexes, hard_positives_per_query,
                            soft_positives_per_query, drawn_negatives, negs_num_per_query=10, device="cuda"):
    """The triplet table of the reference's `random` mining (compute_triplets_random, :1264-1289): int64 [Q, 2 + negs].
    drawn_negatives: per sampled query its np.random.choice(database_num, negs + len(soft_positives), replace=False), as a list
    of arrays or an int64 [Q, W] table padded with -1.  The negatives are the first `negs` entries of each row, in the row's
    order, that are database rows and not soft positives of the query: np.setdiff1d(draw, soft, assume_unique=True)[:negs].
    Tensor operations on [Q, W] only; lists and geo.Positives as in compute_triplets_full.  ValueError for duplicate sampled
    queries and for a draw with fewer than `negs` such entries."""
    dev = torch.device(device)
    negs = int(negs_num_per_query)
    xq = _dev(query_features, dev, torch.float32)
    xb = _dev(database_features, dev, torch.float32)
    sq = _sampled_queries("compute_triplets_random", sampled_queries_indexes, xq, hard_positives_per_query, soft_positives_per_query)
    if negs < 1:
        raise ValueError(f"compute_triplets_random: negs_num_per_query must be >= 1, got {negs}")
    if isinstance(drawn_negatives, (list, tuple)):
        if len(drawn_negatives) != sq.size:
            raise ValueError(f"compute_triplets_random: {len(drawn_negatives)} draws for {sq.size} sampled queries")
        host = np.full((sq.size, max([negs] + [len(x) for x in drawn_negatives])), -1, dtype=np.int64)
        for i, x in enumerate(drawn_negatives):
            host[i, :len(x)] = np.asarray(x, dtype=np.int64).reshape(-1)
        drawn_negatives = host
    drawn = _dev(drawn_negatives, dev, torch.int64)
    if drawn.dim() != 2 or drawn.shape[0] != sq.size:
        raise ValueError(f"compute_triplets_random: drawn_negatives must be [{sq.size}, W], got {tuple(drawn.shape)}")
    sq_t = torch.from_numpy(sq).to(dev)
    best = _best_of_sampled(xq, xb, hard_positives_per_query, sq, sq_t, dev)
    soft, rows = _soft_of_sampled(soft_positives_per_query, sq, sq_t, dev)
    nb = max(int(xb.shape[0]), 1)
    # membership through ONE ascending key array: (list row) * nb + (database row) over the CSR's in-range entries
    inside = (soft.indices >= 0) & (soft.indices < nb)
    keys = (soft.rows() * nb + soft.indices)[inside]
    keep = (drawn >= 0) & (drawn < xb.shape[0])
    if keys.numel():
        mine = rows.view(-1, 1) * nb + drawn.clamp(0, nb - 1)
        at = torch.searchsorted(keys, mine).clamp(max=keys.numel() - 1)
        keep &= keys[at] != mine
    rank = torch.cumsum(keep, 1) - 1                                                # rank among kept entries, in the row's order
    if sq.size and int(keep.sum(1).min()) < negs:
        raise ValueError(_TOO_FEW)
    sel = keep & (rank < negs)
    out = torch.empty((sq.size, negs), dtype=torch.int64, device=dev)
    at_row = torch.arange(sq.size, device=dev).view(-1, 1).expand_as(drawn)
    out[at_row[sel], rank[sel]] = drawn[sel]
    return torch.cat([sq_t.view(-1, 1), best.view(-1, 1), out], 1)
