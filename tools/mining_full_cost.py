"""What one refresh of `full` mining costs, the device route against what a user had before it: python tools/mining_full_cost.py
[--queries 4000] [--database 100000] [--sample 1000] [--negs 10] [--repeats 5] [--loop-repeats 1].

One seeded setting (d = 256 descriptors, every query next to one of its hard positives; per query 5..60 soft positives, a
private draw of `sample` database rows, and a negative cache left by one earlier refresh), two routes to the same table:
  * mining.compute_triplets_full with the positives as geo.Positives: one agp_mine_best_positive and one agp_mine_topk_listed
    launch over the [Q, negs + sample] candidate table (its kernel time alone is reported too, from events on the stream);
  * the loop a user of the library had to write (the reference's :1295-1322 with the library's index in faiss's place): the
    batched best positive, then per query np.setdiff1d / np.unique on the host, an upload of the candidate rows, a row gather,
    one retrieval.IndexFlatL2 build and one search.
Wall times of calls that end in a device synchronise, after a warm-up (the loop's warm-up is its first 32 queries): the median
of `repeats` for the device route, of `loop-repeats` for the loop.  The two tables are compared (`same`).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from agplace_amd import geo, mining, retrieval  # noqa: E402


def timed(fn, repeats, warm=True):
    """(median ms, [min, max], the last result); every call bracketed by device synchronisations."""
    if warm:
        fn()
    ms = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ms), 3), [round(min(ms), 3), round(max(ms), 3)], out


def loop_route(xq, xb, sq, hard, soft, draws, cache_lists, negs, dev, only=None):
    """The per-query loop over the same candidate sets; cache_lists is read, not written."""
    best = mining.best_positive_indexes(xq, xb, [hard[i] for i in sq], dev)
    rows = []
    for i, query_index in enumerate(sq[:only]):
        cand = np.setdiff1d(draws[i], soft[query_index], assume_unique=True)
        cand = np.unique(np.concatenate([cache_lists[query_index], cand]))
        cand_t = torch.from_numpy(cand).to(dev)
        index = retrieval.IndexFlatL2(xq.shape[1], device=dev)
        index.add(xb.index_select(0, cand_t))
        _, I = index.search_device(xq[i:i + 1], negs)
        rows.append(cand_t[I[0]])
    n = len(rows)
    return torch.cat([torch.from_numpy(sq[:n]).to(dev).view(-1, 1), best[:n].view(-1, 1), torch.stack(rows)], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=4000)
    ap.add_argument("--database", type=int, default=100000)
    ap.add_argument("--sample", type=int, default=1000)
    ap.add_argument("--negs", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-repeats", type=int, default=1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mining_full_cost: needs a GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    nq, nb, s, negs, d = a.queries, a.database, a.sample, a.negs, 256
    queries_num = nq + nq // 4                                                  # the sampled queries are a subset of all queries
    soft = [np.sort(rng.choice(nb, size=rng.integers(5, 61), replace=False)) for _ in range(queries_num)]
    hard = [x[:3] for x in soft]
    db_f = rng.standard_normal((nb, d)).astype(np.float32)
    sq = rng.choice(queries_num, size=nq, replace=False)
    q_f = (db_f[[hard[i][0] for i in sq]] + 0.9 * rng.standard_normal((nq, d))).astype(np.float32)
    xq, xb = torch.from_numpy(q_f).to(dev), torch.from_numpy(db_f).to(dev)
    soft_p, hard_p = geo.Positives.from_lists(soft, dev, sort=True), geo.Positives.from_lists(hard, dev, sort=True)
    draw = lambda: np.stack([rng.choice(nb, size=s, replace=False) for _ in range(nq)])      # noqa: E731
    # an earlier refresh fills the cache of the sampled queries
    start = mining.NegCache(queries_num, negs, device=dev)
    mining.compute_triplets_full(xq, xb, sq, hard_p, soft_p, draw(), start, negs, device=dev)
    start_lists = start.to_lists()
    draws = draw()
    draws_t = torch.from_numpy(draws).to(dev)
    res = {"metric": "mining_full_cost", "queries": nq, "database": nb, "d": d, "sample": s, "negs": negs,
           "repeats": a.repeats, "loop_repeats": a.loop_repeats, "device": torch.cuda.get_device_name(0),
           "cores": {"cpu_count": os.cpu_count(), "usable": len(os.sched_getaffinity(0)), "torch_threads": torch.get_num_threads()}}

    def device_route(draws_in):
        cache = mining.NegCache(queries_num, negs, device=dev)
        cache.table.copy_(start.table)
        return mining.compute_triplets_full(xq, xb, sq, hard_p, soft_p, draws_in, cache, negs, device=dev)
    ms, span, got = timed(lambda: device_route(draws_t), a.repeats)
    res.update(device_ms=ms, device_min_max=span)
    ms, span, _ = timed(lambda: device_route(draws), a.repeats)                 # the draws uploaded from numpy inside the call
    res.update(device_from_numpy_draws_ms=ms, device_from_numpy_draws_min_max=span)

    # the kernel alone
    cand = torch.cat([start.rows(sq), draws_t], 1)
    rows = torch.from_numpy(sq).to(dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * a.repeats)]
    mining._topk_listed(xq, xb, cand, negs, soft_p, rows, negs)
    for r in range(a.repeats):
        ev[2 * r].record()
        mining._topk_listed(xq, xb, cand, negs, soft_p, rows, negs)
        ev[2 * r + 1].record()
    torch.cuda.synchronize()
    res["topk_listed_kernel_ms"] = round(statistics.median(ev[2 * r].elapsed_time(ev[2 * r + 1]) for r in range(a.repeats)), 3)

    loop_route(xq, xb, sq, hard, soft, draws, start_lists, negs, dev, only=32)  # warm-up
    ms, span, want = timed(lambda: loop_route(xq, xb, sq, hard, soft, draws, start_lists, negs, dev), a.loop_repeats, warm=False)
    res.update(loop_ms=ms, loop_min_max=span, loop_over_device=round(ms / res["device_ms"], 1), same=bool(torch.equal(want, got)))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
