"""Neighbours: the top-``cutoff`` most similar items for batches of query items of a synthetic shape (ML-20M by
default: 26,744 items), on the device (``DeviceRecommender.similar_items_arrays``: ``irs_serve_neighbors``, nothing
but the query indices goes up) and on the host the way a user does it today from the downloaded operand, in the same
process.

Models: iALS ``K = 64`` with ``cosine`` and with ``dot`` (factors), cosine item-kNN (``top_k`` 100; sparse float64
``W``), EASE (dense float32 ``W``).  Batches: 1, 64, 1,024 and all items.  Per (model, metric, batch) one JSON line:

  create_ms      making the DeviceRecommender (validation, upload), once per model
  device_ms      wall time of one ``similar_items_arrays`` call: the median of ``--repeats`` calls after ``--warmup``
                 warm-up calls of the same shape (the first cosine call of a server also makes the inverse norms: it
                 is a warm-up call); ``device_min_ms`` / ``device_max_ms`` the spread
  upload/score/mask/rank_ms   stream time by phase of the last call (``last_phases()``)
  host_ms        wall time of the host path for the same queries, median of up to three runs after one warm-up:
                 factors - the float32 table normalised once (not timed; ``dot``: as it is), then per 1,024 queries
                 one BLAS product against the whole table (BLAS's own threads), self to -inf, ``argpartition``
                 and a sort of the kept ``cutoff``, the rows of the piece in slices on ``--threads`` threads;
                 sparse ``W`` - per query the stored row of the scipy CSR without the item itself, a stable sort by
                 weight; dense ``W`` - the rows as the factor path ranks its products
  items_per_s, host_items_per_s, speedup (host_ms / device_ms)
  same           sparse and dense ``W``: whether both paths list the same items in the same order with the same
                 float32 scores (ties: candidate order on both sides); factors: the fraction of queries with the same
                 first neighbour (float32 sums in another order)

Run it under a time limit sized to the step, e.g.

    timeout -k 10 1100 python scripts/similar_items_bench.py
    timeout -k 10 300 python scripts/similar_items_bench.py --shape ml100k --models ials,knn
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import scipy.sparse as sps

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from irspack_amd.recommenders.dense_slim import DenseSLIMRecommender  # noqa: E402
from irspack_amd.recommenders.ials import IALSRecommender  # noqa: E402
from irspack_amd.recommenders.knn import CosineKNNRecommender  # noqa: E402
from irspack_amd.serving import DeviceRecommender  # noqa: E402
from irspack_amd.synthetic import make_interactions  # noqa: E402

PIECE = 1024


def fit(name: str, X: sps.csr_matrix):
    if name == "knn":
        return CosineKNNRecommender(X, top_k=100).learn()
    if name == "ease":
        return DenseSLIMRecommender(X, reg=500.0).learn()
    return IALSRecommender(X, n_components=64, alpha0=0.1, reg=1e-2, train_epochs=2).learn()


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0


def rank_dense(S: np.ndarray, ids: np.ndarray, cutoff: int):
    """the ``cutoff`` best columns of every row of a host score block, self left out: (idx, score)"""
    S[np.arange(ids.size), ids] = -np.inf
    keep = min(cutoff, S.shape[1] - 1)
    part = np.argpartition(-S, keep - 1, axis=1)[:, :keep]
    vals = np.take_along_axis(S, part, axis=1)
    order = np.argsort(-vals, axis=1, kind="stable")
    return np.take_along_axis(part, order, axis=1), np.take_along_axis(vals, order, axis=1)


def rank_pieces(block_of, ids: np.ndarray, cutoff: int, pool: ThreadPoolExecutor, threads: int):
    """per PIECE queries: ``block_of(q)`` (the host score block of the queries ``q``; BLAS runs on its own
    threads), then the rows of the block ranked in ``threads`` slices on the pool"""
    idx, val = [], []
    for b in range(0, ids.size, PIECE):
        q = ids[b:b + PIECE]
        S = block_of(q)
        step = max(1, -(-q.size // threads))
        out = list(pool.map(lambda lo: rank_dense(S[lo:lo + step], q[lo:lo + step], cutoff), range(0, q.size, step)))
        idx += [o[0] for o in out]
        val += [o[1] for o in out]
    return np.concatenate(idx), np.concatenate(val)


def host_factors(table: np.ndarray, ids: np.ndarray, cutoff: int, pool: ThreadPoolExecutor, threads: int):
    return rank_pieces(lambda q: table[q] @ table.T, ids, cutoff, pool, threads)


def host_dense_rows(W: np.ndarray, ids: np.ndarray, cutoff: int, pool: ThreadPoolExecutor, threads: int):
    return rank_pieces(lambda q: W[q].astype(np.float32), ids, cutoff, pool, threads)


def host_sparse_rows(W: sps.csr_matrix, ids: np.ndarray, cutoff: int):
    out = []
    for q in ids:
        lo, hi = W.indptr[q], W.indptr[q + 1]
        cols, vals = W.indices[lo:hi], W.data[lo:hi]
        live = cols != q
        cols, vals = cols[live], vals[live]
        best = np.argsort(-vals, kind="stable")[:cutoff]
        out.append((cols[best], vals[best].astype(np.float32)))
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml20m")
    ap.add_argument("--models", default="ials,knn,ease")
    ap.add_argument("--batches", default="1,64,1024,all")
    ap.add_argument("--cutoff", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    X = sps.csr_matrix(make_interactions(args.shape), dtype=np.float64)
    n_users, n_items = X.shape
    rng = np.random.default_rng(0)
    pool = ThreadPoolExecutor(args.threads)
    for name in args.models.split(","):
        model, fit_s = timed(lambda: fit(name, X))
        dev, create_s = timed(lambda: DeviceRecommender(model))
        for metric in (("cosine", "dot") if name == "ials" else ("weight",)):
            if name == "ials":
                table = np.ascontiguousarray(model.get_item_embedding(), dtype=np.float32)
                if metric == "cosine":
                    norm = np.linalg.norm(table.astype(np.float64), axis=1)
                    table = (table / np.where(norm > 0, norm, 1.0)[:, None]).astype(np.float32)
                host = lambda ids: host_factors(table, ids, args.cutoff, pool, args.threads)  # noqa: E731
            elif name == "knn":
                Wc = sps.csr_matrix(model.W, dtype=np.float64)
                Wc.sort_indices()
                host = lambda ids: host_sparse_rows(Wc, ids, args.cutoff)  # noqa: E731
            else:
                Wd = model.W
                host = lambda ids: host_dense_rows(Wd, ids, args.cutoff, pool, args.threads)  # noqa: E731
            for batch in args.batches.split(","):
                n = n_items if batch == "all" else min(int(batch), n_items)
                ids = np.arange(n_items) if batch == "all" else np.sort(rng.choice(n_items, size=n, replace=False))
                for _ in range(args.warmup):
                    dev.similar_items_arrays(ids, args.cutoff, metric=metric)
                times = []
                for _ in range(args.repeats):
                    got, s = timed(lambda: dev.similar_items_arrays(ids, args.cutoff, metric=metric))
                    times.append(s)
                device_s = float(np.median(times))
                phases = dev.last_phases()
                host(ids)
                th = []
                for _ in range(3 if n <= PIECE else 1):
                    want, s = timed(lambda: host(ids))
                    th.append(s)
                host_s = float(np.median(th))
                idx, score, length = got
                if name == "knn":
                    same = all(np.array_equal(idx[r, :length[r]], w[0]) and np.array_equal(score[r, :length[r]], w[1])
                               for r, w in enumerate(want))
                elif name == "ease":
                    same = bool((length == idx.shape[1]).all() and np.array_equal(idx, want[0])
                                and np.array_equal(score, want[1]))
                else:
                    same = float(np.mean(idx[:, 0] == want[0][:, 0]))
                print(json.dumps(dict(
                    model=name, kind=dev.kind, metric=metric, shape=args.shape, n_users=n_users, n_items=n_items,
                    nnz=int(X.nnz), batch=n, cutoff=args.cutoff, fit_s=round(fit_s, 2),
                    create_ms=round(create_s * 1e3, 1), device_ms=round(device_s * 1e3, 3),
                    device_min_ms=round(min(times) * 1e3, 3), device_max_ms=round(max(times) * 1e3, 3),
                    repeats=args.repeats, **{f"{k}_ms": round(v, 3) for k, v in phases.items()},
                    host_ms=round(host_s * 1e3, 3), items_per_s=round(n / device_s), host_items_per_s=round(n / host_s),
                    speedup=round(host_s / device_s, 2), same=same, host_threads=args.threads,
                    omp_threads=os.environ.get("OMP_NUM_THREADS"))), flush=True)
        dev.close()
        del model, dev, got, want
    pool.shutdown()


if __name__ == "__main__":
    main()
