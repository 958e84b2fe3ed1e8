"""Time of ``EvaluatorWithColdUser.get_scores(model, [20])`` on a synthetic shape, ML-20M by default, with the last
20 % of the users held out as cold users: the models are fitted on the other 80 %, the cold users' rows are split
into the input the model folds in and the ground truth.

Per model one JSON line: the kind ``_device_path`` names (``similarity``: cosine kNN; ``dense_similarity``:
DenseSLIM; ``factors``: truncated SVD, NMF, iALS, Mult-VAE), nDCG@20, the device path's wall time (second call:
the first one pays the code-object load and the allocations), the stream time by phase of its last device call -
uploads, scoring, masking, ranking; ``last_call_phases``, for the dense and the factor calls, so without the
fold-in, which the wall time holds - and beside it the ``fused=False`` block loop - the model's own host scores
per ``mb_size`` users, padded, uploaded and ranked - timed on the first ``--host-users`` cold users and scaled to
all of them.

The models are fitted by the package (NMF: ``--nmf-iter`` iterations, Mult-VAE and iALS: ``--epochs``; the time of
an evaluation does not turn on the quality of the fit).  Run it under a time limit sized to the step, e.g.

    timeout -k 10 900 python scripts/eval_cold_bench.py
    timeout -k 10 300 python scripts/eval_cold_bench.py --models truncsvd,nmf,ials --host-users 1024
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sps

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from irspack_amd.evaluation import EvaluatorWithColdUser  # noqa: E402
from irspack_amd.recommenders import (CosineKNNRecommender, DenseSLIMRecommender, IALSRecommender,  # noqa: E402
                                      MultVAERecommender, NMFRecommender, TruncatedSVDRecommender)
from irspack_amd.recommenders.nmf import NMFModel  # noqa: E402
from irspack_amd.synthetic import holdout_split, make_interactions  # noqa: E402
from irspack_amd.utils import nmf_fit  # noqa: E402


def fit(name: str, X: sps.csr_matrix, k: int, nmf_iter: int, epochs: int):
    if name == "knn":
        return CosineKNNRecommender(X, top_k=100).learn()
    if name == "dense_slim":
        return DenseSLIMRecommender(X, reg=500.0).learn()
    if name == "truncsvd":
        return TruncatedSVDRecommender(X, n_components=k).learn()
    if name == "ials":
        return IALSRecommender(X, n_components=k, alpha0=0.1, reg=1e-2, train_epochs=epochs,
                               solver_type="CHOLESKY").learn()
    if name == "multvae":
        return MultVAERecommender(X, dim_z=k, enc_hidden_dims=k, train_epochs=epochs).learn()
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
    ap.add_argument("--models", default="knn,dense_slim,truncsvd,nmf,ials,multvae")
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--nmf-iter", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--cutoff", type=int, default=20)
    ap.add_argument("--host-users", type=int, default=2048)
    args = ap.parse_args()
    X = sps.csr_matrix(make_interactions(args.shape), dtype=np.float64)
    n_train = X.shape[0] - X.shape[0] // 5
    X_train = X[:n_train]
    cold_input, cold_truth = holdout_split(X[n_train:])
    n_cold, n_items = cold_input.shape
    n_host = min(n_cold, max(args.host_users, 1))
    device = EvaluatorWithColdUser(cold_input, cold_truth, cutoff=args.cutoff)
    host = EvaluatorWithColdUser(cold_input[:n_host], cold_truth[:n_host], cutoff=args.cutoff, fused=False)
    for name in args.models.split(","):
        model, fit_s = timed(lambda: fit(name, X_train, args.k, args.nmf_iter, args.epochs))
        path = device._device_path(model)
        _, first_s = timed(lambda: device.get_score(model))
        got, call_s = timed(lambda: device.get_score(model))
        out = dict(model=name, shape=args.shape, n_train_users=n_train, n_cold_users=n_cold, n_items=n_items,
                   cold_nnz=int(cold_input.nnz), path=path, fit_s=round(fit_s, 3),
                   first_call_ms=round(first_s * 1e3, 1), call_ms=round(call_s * 1e3, 1),
                   users_per_s=round(n_cold / call_s), ndcg=round(got["ndcg"], 6))
        if path in ("dense_similarity", "factors"):
            out.update({n: round(v, 2) for n, v in device.core.last_call_phases().items()})
        want, host_s = timed(lambda: host.get_score(model))
        scaled = host_s * n_cold / n_host
        out.update(host_users=n_host, host_ndcg=round(want["ndcg"], 6), host_loop_s=round(host_s, 3),
                   host_loop_all_users_s=round(scaled, 2), host_users_per_s=round(n_host / host_s),
                   speedup=round(scaled / call_s, 1), host_threads=os.environ.get("OMP_NUM_THREADS"))
        print(json.dumps(out), flush=True)
        del model


if __name__ == "__main__":
    main()
