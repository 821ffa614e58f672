"""What the geographic ground truth costs around the kernels, host routes against the device CSR: python tools/geo_eval_cost.py
[--queries 4096] [--database 20000] [--repeats 5].

One seeded layout (a 2-D random walk of float32 UTM points, queries perturbed from it; d = 256 descriptors, six queries in ten
next to one of their positives', the rest next to any row's), three comparisons, each the median wall time of `repeats` calls
that end in a device synchronise, after one warm-up call:
  * radius search at 25 m: geo.radius_neighbors (count, prefix sum, the host read of the total, fill), and sklearn's
    NearestNeighbors.radius_neighbors (fit + query) if sklearn can be imported;
  * recall@[1, 5, 10, 20] from [Q, 20] predictions: the reference's loop (retrieval.recall_from_predictions with lists and numpy
    predictions) against geo.recall_at with a Positives (predictions on the device, and uploaded from numpy);
  * one miner refresh, mining.compute_triplets_partial at 4000 sampled queries, 1000 sampled rows, negs = 10: lists against
    Positives.
The host routes are the code as it was before the device CSR existed, run here in the same process.  Results of the two routes
are compared and reported (`same`).  Prints one JSON line."""
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


def timed(fn, repeats):
    """(median ms, [min, max], the last result); every call bracketed by device synchronisations."""
    fn()
    ms = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ms), 3), [round(min(ms), 3), round(max(ms), 3)], out


class Args:
    recall_values = [1, 5, 10, 20]


class DS:
    def __init__(self, positives, queries_num):
        self.positives, self.queries_num = positives, queries_num

    def get_positives(self):
        return self.positives


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--database", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("geo_eval_cost: needs a GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    nq, nb, d, k = a.queries, a.database, 256, 20
    db_utm = (np.cumsum(rng.normal(0.0, 3.0, size=(nb, 2)), 0) + np.asarray([368000.0, 140000.0])).astype(np.float32)
    q_utm = (db_utm[rng.integers(0, nb, nq)] + rng.normal(0.0, 8.0, size=(nq, 2))).astype(np.float32)
    res = {"metric": "geo_eval_cost", "queries": nq, "database": nb, "repeats": a.repeats,
           "cores": {"cpu_count": os.cpu_count(), "usable": len(os.sched_getaffinity(0)), "torch_threads": torch.get_num_threads()}}

    # ---- radius search
    ms, span, soft = timed(lambda: geo.radius_neighbors(q_utm, db_utm, 25.0, device=dev), a.repeats)
    res["radius_25m"] = {"device_ms": ms, "device_min_max": span, "pairs": int(soft.indices.numel())}
    q_dev, db_dev = torch.from_numpy(q_utm).to(dev), torch.from_numpy(db_utm).to(dev)
    ms, span, _ = timed(lambda: geo.radius_neighbors(q_dev, db_dev, 25.0, device=dev), a.repeats)
    res["radius_25m"].update(device_inputs_on_device_ms=ms, device_inputs_on_device_min_max=span)
    try:
        from sklearn.neighbors import NearestNeighbors

        def sk():
            knn = NearestNeighbors(n_jobs=-1)
            knn.fit(db_utm)
            return knn.radius_neighbors(q_utm, radius=25.0, return_distance=False)
        ms, span, theirs = timed(sk, a.repeats)
        same = all(np.array_equal(np.sort(t), m) for t, m in zip(theirs, soft))
        res["radius_25m"].update(sklearn_ms=ms, sklearn_min_max=span, same_sets=bool(same))
    except ImportError:
        res["radius_25m"]["sklearn_ms"] = None
    hard = geo.radius_neighbors(q_utm, db_utm, 10.0, device=dev)
    soft_l, hard_l = soft.to_lists(), hard.to_lists()

    # ---- recall
    db_f = rng.standard_normal((nb, d)).astype(np.float32)
    # six queries in ten sit next to one of their positives, the others anywhere: hits at every column and misses, so the
    # host loop runs one to four np.isin per query as it does on real predictions
    near = np.asarray([x[rng.integers(0, len(x))] if len(x) and rng.random() < 0.6 else rng.integers(0, nb) for x in soft_l])
    q_f = (db_f[near] + 0.9 * rng.standard_normal((nq, d))).astype(np.float32)
    index = retrieval.IndexFlatL2(d, device=dev)
    index.add(db_f)
    _, pred_dev = index.search_device(torch.from_numpy(q_f).to(dev), k)
    pred_np = pred_dev.cpu().numpy()
    ms_h, span_h, want = timed(lambda: retrieval.recall_from_predictions(Args, pred_np, DS(soft_l, nq)), a.repeats)
    ms_d, span_d, got = timed(lambda: retrieval.recall_from_predictions(Args, pred_dev, DS(soft, nq)), a.repeats)
    ms_u, span_u, got_u = timed(lambda: geo.recall_at(pred_np, soft, Args.recall_values, nq), a.repeats)
    res["recall_q%d_k%d" % (nq, k)] = {
        "host_loop_ms": ms_h, "host_loop_min_max": span_h, "device_ms": ms_d, "device_min_max": span_d,
        "device_from_numpy_predictions_ms": ms_u, "device_from_numpy_predictions_min_max": span_u,
        "host_over_device": round(ms_h / ms_d, 1), "recalls": want[1],
        "same": bool(np.array_equal(want[0], got[0]) and want[1] == got[1] and np.array_equal(want[0], got_u[0]))}

    # ---- one miner refresh
    nsq, nc, negs = min(4000, nq), 1000, 10
    sq = rng.choice(nq, size=nsq, replace=False)
    cand = rng.choice(nb, size=nc, replace=False)
    qf_dev, dbf_dev = torch.from_numpy(q_f[sq]).to(dev), torch.from_numpy(db_f).to(dev)
    ms_h, span_h, want = timed(lambda: mining.compute_triplets_partial(qf_dev, dbf_dev, sq, hard_l, soft_l, cand, negs, device=dev),
                               a.repeats)
    ms_d, span_d, got = timed(lambda: mining.compute_triplets_partial(qf_dev, dbf_dev, sq, hard, soft, cand, negs, device=dev),
                              a.repeats)
    res["miner_refresh_q%d_c%d_negs%d" % (nsq, nc, negs)] = {
        "lists_ms": ms_h, "lists_min_max": span_h, "positives_ms": ms_d, "positives_min_max": span_d,
        "lists_over_positives": round(ms_h / ms_d, 1), "same": bool(torch.equal(want, got))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
