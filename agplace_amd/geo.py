"""Geographic positives on the device: radius search, the CSR that holds its result, recall@N from that CSR.

The reference builds its ground truth on the host with sklearn (`NearestNeighbors.radius_neighbors` over the 2-D UTM coordinates,
datasets/datasets_ws_nuscenes.py:907-912 and :1032-1037: `soft_positives_per_query` at 25 m, `hard_positives_per_query` at 10 m,
`get_positives()`), then scores with a per-query `np.isin` loop (test.py:73-83) and mines from Python lists (:1372-1410).  Here
the lists are ONE device-resident ragged array, `Positives`, built once by `radius_neighbors` (csrc/geo.hip) and read where it
lies by `recall_at` (agp_recall_first_hit) and by the miner (agplace_amd/mining.py: agp_mine_best_positive,
agp_mine_drop_listed).  A `Positives` still indexes and iterates like the reference's list of arrays, so code that reads
`soft_positives_per_query[i]` or filters queries with `len(p) == 0` keeps working on the same object.

One difference from sklearn: it returns every list in tree order, this search in ASCENDING database rows.  The sets are equal.
Only agp_mine_best_positive's tie rule (the first of two candidates at exactly equal feature distance, in list order) can see
the order, and only between two hard positives whose descriptors are at exactly the same distance from the query.
"""
import numpy as np
import torch

from . import _lib
from ._lib import check, ptr

_MAX_K = 1024      # AGP_KNN_MAX_K (include/agplace_hip.h): the widest prediction row agp_recall_first_hit takes


def _as_tensor(x, device, dtype):
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(x))
    return x.to(device=device, dtype=dtype).contiguous()


class Positives:
    """Per-query lists of database rows as a device CSR: row i is indices[offsets[i] : offsets[i + 1]].

    offsets int64 [n + 1], indices int64 [total], both on one device.  `is_sorted` says that every row is ascending without
    repeats -- what the kernels' binary search needs; `radius_neighbors` produces such rows, `sorted_unique()` makes them.
    len(), [i] and iteration serve numpy int64 arrays from a host copy that is made once, on first use."""

    def __init__(self, offsets, indices, is_sorted=False):
        if offsets.dtype != torch.int64 or indices.dtype != torch.int64 or offsets.dim() != 1 or indices.dim() != 1:
            raise ValueError("Positives: offsets and indices must be 1-D int64 tensors")
        if offsets.numel() < 1 or offsets.device != indices.device:
            raise ValueError("Positives: offsets needs n + 1 entries on the device of indices")
        self.offsets = offsets.contiguous()
        self.indices = indices.contiguous()
        self.is_sorted = bool(is_sorted)
        self._host = None

    @property
    def device(self):
        return self.offsets.device

    @classmethod
    def from_lists(cls, lists, device="cuda", sort=False):
        """The CSR of a list of index arrays (the reference's soft_positives_per_query and its kin), rows in the given order.
        sort=True returns sorted_unique() of it.  The lists' own order is not examined: is_sorted is set only by sorting."""
        lens = np.fromiter((len(x) for x in lists), dtype=np.int64, count=len(lists))
        off = np.zeros(len(lists) + 1, dtype=np.int64)
        np.cumsum(lens, out=off[1:])
        flat = np.concatenate([np.asarray(x, dtype=np.int64).reshape(-1) for x in lists]) if off[-1] else np.zeros(0, dtype=np.int64)
        dev = torch.device(device)
        p = cls(torch.from_numpy(off).to(dev), torch.from_numpy(flat).to(dev))
        return p.sorted_unique() if sort else p

    def lengths(self):
        """int64 [n] on the device: the length of every row."""
        return self.offsets[1:] - self.offsets[:-1]

    def rows(self):
        """int64 [total] on the device: the row that owns every entry of `indices`."""
        n = self.offsets.numel() - 1
        return torch.repeat_interleave(torch.arange(n, device=self.device), self.lengths(), output_size=self.indices.numel())

    def sorted_unique(self):
        """Every row ascending, repeats removed: `self` when is_sorted, else one device sort on the key row * n_db + index."""
        if self.is_sorted:
            return self
        n = self.offsets.numel() - 1
        if self.indices.numel() == 0:
            return Positives(self.offsets, self.indices, True)
        if int(self.indices.min()) < 0:
            raise ValueError("Positives.sorted_unique: negative database row")
        n_db = int(self.indices.max()) + 1
        key = torch.unique(self.rows() * n_db + self.indices)           # sorted
        row = torch.div(key, n_db, rounding_mode="floor")
        off = torch.zeros(n + 1, dtype=torch.int64, device=self.device)
        torch.cumsum(torch.bincount(row, minlength=n), 0, out=off[1:])
        return Positives(off, key - row * n_db, True)

    def select(self, rows):
        """The CSR of the given rows (int64 tensor on the device, repeats allowed), in that order: torch indexing on the device."""
        lens = self.lengths()[rows]
        off = torch.zeros(rows.numel() + 1, dtype=torch.int64, device=self.device)
        torch.cumsum(lens, 0, out=off[1:])
        total = int(off[-1])
        src = torch.repeat_interleave(self.offsets[:-1][rows] - off[:-1], lens, output_size=total) + \
            torch.arange(total, device=self.device)
        return Positives(off, self.indices[src], self.is_sorted)

    # ---- the reference's list-of-arrays view
    def _host_copy(self):
        if self._host is None:
            self._host = (self.offsets.cpu().numpy(), self.indices.cpu().numpy())
        return self._host

    def to_lists(self):
        """A list of numpy int64 arrays, one per row (what sklearn's radius_neighbors returns, rows ascending)."""
        off, idx = self._host_copy()
        return [idx[off[i]:off[i + 1]] for i in range(len(off) - 1)]

    def __len__(self):
        return self.offsets.numel() - 1

    def __getitem__(self, i):
        off, idx = self._host_copy()
        n = len(off) - 1
        i = int(i)
        if not -n <= i < n:
            raise IndexError(i)
        i %= n
        return idx[off[i]:off[i + 1]]

    def __iter__(self):
        off, idx = self._host_copy()
        return (idx[off[i]:off[i + 1]] for i in range(len(off) - 1))


def _utm(x, device):
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if x.dim() != 2 or x.shape[1] != 2:
        raise ValueError(f"radius_neighbors: expected [n, 2] coordinates, got {tuple(x.shape)}")
    if x.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"radius_neighbors: coordinates must be float32 or float64, got {x.dtype}")
    return x.to(device=device, dtype=torch.float64).contiguous()       # float32 widens exactly, as sklearn widens it


def radius_neighbors(queries_utms, database_utms, radius, device="cuda"):
    """Positives: for every query the database rows within `radius` (same unit as the coordinates), ascending.

    queries_utms [nq, 2], database_utms [nb, 2]: arrays or tensors, float32 or float64 (the reference stores float32 UTM metres;
    they are widened to fp64 on the way in, as sklearn does).  Row b is in query q's list when
    dx*dx + dy*dy <= radius*radius in fp64 without fused multiply-add -- inclusive at the boundary, bit for bit the numpy
    expression, which is also what sklearn's radius_neighbors decides on these inputs.  A NaN or infinite coordinate has no
    neighbours.  sklearn returns each list in tree order; these are ascending (see the module docstring for the one place
    that can tell).

    Two launches (count, fill) with ONE host read between them -- the total, to size `indices` -- so this function is not
    capturable in a graph; it belongs to dataset construction, not to a step."""
    dev = torch.device(device)
    q, db = _utm(queries_utms, dev), _utm(database_utms, dev)
    r = float(radius)
    if not r >= 0.0:
        raise ValueError(f"radius_neighbors: radius must be >= 0, got {radius!r}")
    r2 = r * r
    nq, nb = q.shape[0], db.shape[0]
    L = _lib.load()
    off = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    if nq == 0 or nb == 0:
        return Positives(off, torch.zeros(0, dtype=torch.int64, device=dev), True)
    counts = torch.empty(nq, dtype=torch.int64, device=dev)
    check(L.agp_radius_count(ptr(q), nq, ptr(db), nb, r2, ptr(counts), _lib.stream()), "agp_radius_count")
    torch.cumsum(counts, 0, out=off[1:])
    total = int(off[-1])
    idx = torch.empty(total, dtype=torch.int64, device=dev)
    if total:
        check(L.agp_radius_fill(ptr(q), nq, ptr(db), nb, r2, ptr(off), ptr(idx), _lib.stream()), "agp_radius_fill")
    return Positives(off, idx, True)


def _nonnull(idx):
    """pos_idx of an all-empty CSR: the entries take no null pointer, and no row reads it."""
    return idx if idx.numel() else torch.zeros(1, dtype=torch.int64, device=idx.device)


def first_hit(predictions, positives):
    """int32 [Q] on the device: per query the first column of `predictions` (int64 [Q, k], 1 <= k <= 1024) that is one of the
    query's positives, k if none is.  Entries < 0 never match."""
    positives = positives.sorted_unique()
    pred = _as_tensor(predictions, positives.device, torch.int64)
    if pred.dim() != 2 or pred.shape[0] != len(positives):
        raise ValueError(f"first_hit: predictions {tuple(pred.shape)} do not match {len(positives)} lists of positives")
    nq, k = pred.shape
    if not 1 <= k <= _MAX_K:
        raise ValueError(f"first_hit: predictions must have between 1 and {_MAX_K} columns, got {k}")
    first = torch.empty(nq, dtype=torch.int32, device=pred.device)
    check(_lib.load().agp_recall_first_hit(ptr(pred), nq, k, ptr(positives.offsets), ptr(_nonnull(positives.indices)), ptr(first),
                                           _lib.stream()), "agp_recall_first_hit")
    return first


def recalls_from_first_hit(first, k, recall_values, queries_num):
    """The arithmetic of reference test.py:73-83 from the first-hit column of every query (a device tensor, k = no hit):
    per query the FIRST i in list order with a hit inside pred[:recall_values[i]] adds one to recalls[i:]."""
    rv = torch.tensor([min(int(n), k) for n in recall_values], dtype=torch.int64, device=first.device)
    hit = first.to(torch.int64).view(-1, 1) < rv.view(1, -1)                        # [Q, R]
    any_hit = hit.any(1)
    where = torch.argmax(hit.to(torch.uint8), 1)                                    # the first i that holds
    per_value = torch.bincount(where[any_hit], minlength=len(recall_values))
    recalls = torch.cumsum(per_value, 0).cpu().numpy().astype(np.float64)           # whole numbers: the loop's `+= 1`, exactly
    recalls = recalls / queries_num * 100
    recalls_str = ", ".join([f"R@{val}: {rec:.1f}" for val, rec in zip(recall_values, recalls)])
    return recalls, recalls_str


def recall_at(predictions, positives, recall_values, queries_num=None):
    """(recalls, recalls_str) of reference test.py:73-83 with the positives on the device.

    predictions int64 [Q, k] (tensor or array; k >= max(recall_values) in the reference, a shorter row is used whole, as
    `pred[:n]` does), positives a `Positives` with Q rows, recall_values in any order, queries_num the divisor (default Q).
    One agp_recall_first_hit launch, a few tensor operations on [Q, len(recall_values)], one copy of len(recall_values) numbers."""
    first = first_hit(predictions, positives)
    nq, k = first.shape[0], int(predictions.shape[1])
    return recalls_from_first_hit(first, k, list(recall_values), nq if queries_num is None else queries_num)
