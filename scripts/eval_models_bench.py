"""Time of ``Evaluator.get_scores(model, [20])`` over all users of a synthetic shape, ML-20M by default, for
the five recommenders the evaluator scores on the device since the dense-similarity and factor calls: SLIM
(sparse float32 weights), DenseSLIM / EASE and EDLAE (dense float32 weights), truncated SVD and NMF (factors).

Per model one JSON line: the device call's wall time (second call: the first one pays the code-object load and
the allocations), its stream time by phase - uploads, scoring, masking, ranking; ``last_call_phases``, for the
dense and the factor calls -, for the dense call the ``W`` row segments the score kernel reads (stored profile
entries x n_items x itemsize) over its time, and beside it the ``fused=False`` block loop - the model's own
host scores per 128 users, uploaded and ranked - timed on the first ``--host-users`` users and scaled to all.

The models are fitted by the package (NMF: ``--nmf-iter`` iterations; the time of an evaluation does not turn
on the quality of the fit).  Run it under a time limit sized to the step, e.g.

    timeout -k 10 900 python scripts/eval_models_bench.py
    timeout -k 10 300 python scripts/eval_models_bench.py --models truncsvd,nmf --host-users 4096
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sps

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from irspack_amd.evaluation import Evaluator  # noqa: E402
from irspack_amd.recommenders import (DenseSLIMRecommender, EDLAERecommender, NMFRecommender,  # noqa: E402
                                      SLIMRecommender, TruncatedSVDRecommender)
from irspack_amd.recommenders.nmf import NMFModel  # noqa: E402
from irspack_amd.synthetic import holdout_split, make_interactions  # noqa: E402
from irspack_amd.utils import nmf_fit  # noqa: E402


def fit(name: str, X: sps.csr_matrix, k: int, nmf_iter: int):
    if name == "slim":
        return SLIMRecommender(X).learn()
    if name == "dense_slim":
        return DenseSLIMRecommender(X, reg=500.0).learn()
    if name == "edlae":
        return EDLAERecommender(X, reg=500.0, dropout_p=0.1).learn()
    if name == "truncsvd":
        return TruncatedSVDRecommender(X, n_components=k).learn()
    model = NMFRecommender(X, n_components=k)
    model.W, model.H, n_iter = nmf_fit(model.X_train_all, k, model.alpha, model.l1_ratio, init="random", tol=0.0,
                                       max_iter=nmf_iter)
    model.nmf_model = NMFModel(model.H, n_iter, model.alpha, model.l1_ratio)
    return model


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml20m")
    ap.add_argument("--models", default="slim,dense_slim,edlae,truncsvd,nmf")
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--nmf-iter", type=int, default=5)
    ap.add_argument("--cutoff", type=int, default=20)
    ap.add_argument("--host-users", type=int, default=2048)
    args = ap.parse_args()
    X_train, X_test = holdout_split(sps.csr_matrix(make_interactions(args.shape), dtype=np.float64))
    n_users, n_items = X_train.shape
    n_host = min(n_users, max(args.host_users, 1))
    device, host = Evaluator(X_test, cutoff=args.cutoff), Evaluator(X_test[:n_host], cutoff=args.cutoff, fused=False)
    for name in args.models.split(","):
        model, fit_s = timed(lambda: fit(name, X_train, args.k, args.nmf_iter))
        path = device._device_path(model)
        _, first_s = timed(lambda: device.get_score(model))
        got, call_s = timed(lambda: device.get_score(model))
        out = dict(model=name, shape=args.shape, n_users=n_users, n_items=n_items, nnz=int(X_train.nnz), path=path,
                   fit_s=round(fit_s, 3), first_call_ms=round(first_s * 1e3, 1), call_ms=round(call_s * 1e3, 1),
                   users_per_s=round(n_users / call_s), ndcg=round(got["ndcg"], 6))
        if path in ("dense_similarity", "factors"):
            phases = device.core.last_call_phases()
            out.update({n: round(v, 2) for n, v in phases.items()})
            if path == "dense_similarity" and phases["score_ms"] > 0:
                seg_bytes = float(X_train.nnz) * n_items * model.W.dtype.itemsize
                out.update(score_w_bytes=seg_bytes, score_tb_per_s=round(seg_bytes / phases["score_ms"] / 1e9, 2))
            if path == "factors":
                out.update(k=args.k)
        want, host_s = timed(lambda: host.get_score(model))
        scaled = host_s * n_users / n_host
        out.update(host_users=n_host, host_loop_s=round(host_s, 3), host_loop_all_users_s=round(scaled, 2),
                   host_users_per_s=round(n_host / host_s), speedup=round(scaled / call_s, 1),
                   host_threads=os.environ.get("OMP_NUM_THREADS"))
        print(json.dumps(out), flush=True)
        del model


if __name__ == "__main__":
    main()
