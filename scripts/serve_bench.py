"""Serving: top-``cutoff`` lists for batches of known users of a synthetic shape (ML-20M by default), through the
fused device path (``irspack_amd.serving.DeviceRecommender``: scores, exclusions and top-k on the device) and
through the two-step path as it ran before (``model.get_score_remove_seen`` on the host, then
``retrieve_recommend_from_score``: the whole score block over PCIe), in the same process.

Models: cosine item-kNN (``top_k`` 100; sparse float64 weights), EASE (dense float32 weights), iALS ``K = 64``
(factors).  Batches: 1, 64, 1,024, 16,384 and all users.  Per (model, batch) one JSON line:

  create_ms           making the DeviceRecommender (validation, canonical copy, upload), once per model
  fused_ms            wall time of one ``recommend_known_arrays`` call, the median of ``--repeats`` calls after
                      ``--warmup`` warm-up calls of the same shape (host gather + device call + copies home)
  upload/score/mask/rank_ms   stream time by phase of the last call (``irs_serve_last_phases``)
  mapper_ms           wall time of ``IDMapper.recommend_for_known_user_batch`` for the same users, forced to the
                      device path (``DEVICE_MIN_BATCH`` zeroed): the cache key of the call (``key_ms`` of it: the
                      fingerprint of the copied operands, for iALS the download of both tables), the device call
                      and the ``(item_id, score)`` lists.  This is the call ``DEVICE_MIN_BATCH`` routes, so the
                      crossover is read from ``mapper_ms`` against ``two_step_ms`` (which lacks the ID lists: a
                      lower bound of the mapper's own two-step call)
  two_step_ms         wall time of the two-step path for the same users.  Batches above 4,096 rows go through in
                      4,096-row pieces (the host block of 16,384 rows is 3.5 GB of float64, of all users 29.6 GB),
                      every piece of them by default.  ``--two-step-pieces N`` (N > 0) runs at most N pieces and
                      scales the time to the batch (``two_step_scaled: true``, ``two_step_rows`` rows measured),
                      for a quick look: the host product of one EASE piece alone takes seconds.
  users_per_s, two_step_users_per_s, speedup
  same                whether the two paths returned the same lists on the rows both computed (similarity models:
                      indices and scores must agree exactly; iALS: float32 sums in another order, so ``same`` is
                      reported as the fraction of equal top-1 items)

Run it under a time limit sized to the step, e.g.

    timeout -k 10 1150 python scripts/serve_bench.py
    timeout -k 10 300 python scripts/serve_bench.py --shape ml100k --models knn,ials
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sps

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from irspack_amd.recommenders.dense_slim import DenseSLIMRecommender  # noqa: E402
from irspack_amd.recommenders.ials import IALSRecommender  # noqa: E402
from irspack_amd.recommenders.knn import CosineKNNRecommender  # noqa: E402
from irspack_amd.serving import DeviceRecommender  # noqa: E402
from irspack_amd.synthetic import make_interactions  # noqa: E402
from irspack_amd.serving import model_operands  # noqa: E402
from irspack_amd.utils import IDMapper, id_mapping, retrieve_recommend_from_score  # noqa: E402

PIECE = 4096


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


def two_step(model, users: np.ndarray, cutoff: int):
    out = []
    for b in range(0, users.size, PIECE):
        score = model.get_score_remove_seen(users[b:b + PIECE])
        out += retrieve_recommend_from_score(score, [], cutoff, 1)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml20m")
    ap.add_argument("--models", default="knn,ease,ials")
    ap.add_argument("--batches", default="1,64,1024,16384,all")
    ap.add_argument("--cutoff", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--two-step-pieces", type=int, default=0)
    args = ap.parse_args()
    X = sps.csr_matrix(make_interactions(args.shape), dtype=np.float64)
    n_users, n_items = X.shape
    rng = np.random.default_rng(0)
    mapper = IDMapper(list(range(n_users)), list(range(n_items)))
    for kind in id_mapping.DEVICE_MIN_BATCH:  # (the device path at every size: the crossover is what is measured)
        id_mapping.DEVICE_MIN_BATCH[kind] = 0
    for name in args.models.split(","):
        model, fit_s = timed(lambda: fit(name, X))
        dev, create_s = timed(lambda: DeviceRecommender(model))
        for batch in args.batches.split(","):
            n = n_users if batch == "all" else min(int(batch), n_users)
            users = np.arange(n_users) if batch == "all" else np.sort(rng.choice(n_users, size=n, replace=False))
            reps = args.repeats if n <= 16384 else max(1, args.repeats // 2)
            for _ in range(args.warmup if n <= 16384 else 1):
                dev.recommend_known_arrays(users, args.cutoff)
            times = []
            for _ in range(reps):
                got, s = timed(lambda: dev.recommend_known_arrays(users, args.cutoff))
                times.append(s)
            fused_s = float(np.median(times))
            phases = dev.last_phases()
            ids = users.tolist()
            mapper.recommend_for_known_user_batch(model, ids, cutoff=args.cutoff)  # (makes the cached copy)
            tm = []
            for _ in range(3 if n <= 16384 else 1):
                mapped, s = timed(lambda: mapper.recommend_for_known_user_batch(model, ids, cutoff=args.cutoff))
                tm.append(s)
            mapper_s = float(np.median(tm))
            _, key_s = timed(lambda: id_mapping._operand_key(*model_operands(model)))
            rows2 = min(n, args.two_step_pieces * PIECE) if args.two_step_pieces > 0 else n
            if n <= PIECE:  # (small batches: one warm-up, then the median, like the fused path)
                two_step(model, users, args.cutoff)
                t2 = []
                for _ in range(min(reps, 3)):
                    want, s = timed(lambda: two_step(model, users[:rows2], args.cutoff))
                    t2.append(s)
                two_s = float(np.median(t2))
            else:
                want, two_s = timed(lambda: two_step(model, users[:rows2], args.cutoff))
            scaled = two_s * n / rows2
            idx, score, length = got
            if name == "ials":
                same = float(np.mean([len(w) > 0 and length[r] > 0 and w[0][0] == idx[r, 0]
                                      for r, w in enumerate(want)]))
            else:
                same = all([(int(i), float(s)) for i, s in zip(idx[r, :length[r]], score[r, :length[r]])] == w
                           for r, w in enumerate(want))
            print(json.dumps(dict(
                model=name, kind=dev.kind, shape=args.shape, n_users=n_users, n_items=n_items, nnz=int(X.nnz),
                batch=n, cutoff=args.cutoff, fit_s=round(fit_s, 2), create_ms=round(create_s * 1e3, 1),
                fused_ms=round(fused_s * 1e3, 3), fused_min_ms=round(min(times) * 1e3, 3),
                fused_max_ms=round(max(times) * 1e3, 3), repeats=reps,
                **{f"{k}_ms": round(v, 3) for k, v in phases.items()},
                mapper_ms=round(mapper_s * 1e3, 3), key_ms=round(key_s * 1e3, 3),
                mapper_same=[[i for i, _ in row] for row in mapped[:64]] == [idx[r, :length[r]].tolist()
                                                                             for r in range(min(n, 64))],
                users_per_s=round(n / fused_s), two_step_ms=round(scaled * 1e3, 2), two_step_rows=rows2,
                two_step_scaled=rows2 < n, two_step_piece_rows=PIECE if n > PIECE else n,
                two_step_users_per_s=round(n / scaled), speedup=round(scaled / fused_s, 2), same=same,
                host_threads=os.environ.get("OMP_NUM_THREADS"))), flush=True)
        dev.close()
        del model, dev, mapped, got, want


if __name__ == "__main__":
    main()
