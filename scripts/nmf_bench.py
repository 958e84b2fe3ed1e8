"""Device time of an NMF fit (irs_nmf_fit) at a synthetic shape, ML-20M by default, for n_components = 64 and
512: milliseconds per iteration by phase from ``stats`` (sparse x block products, Gram matrices, coordinate
sweeps, the violation reduce and its copy; HIP events), the set-up once, and the wall time of ``nmf_fit``.  The
start is the ``random`` init, so that only the fit is timed; ``max_iter`` iterations with ``tol = 0``.

``--host`` adds scikit-learn's ``NMF`` on the host's threads from the same start, at the same ``max_iter`` with
``tol = 0`` on the same matrix (float32), and the largest difference of the two ``W @ H`` on a sample of rows.

One JSON line per point.  Run it under a time limit sized to the step, e.g.

    timeout -k 10 300 python scripts/nmf_bench.py
    timeout -k 10 900 python scripts/nmf_bench.py --k 64 --host
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from irspack_amd.synthetic import make_interactions  # noqa: E402
from irspack_amd.utils import nmf_fit  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml20m")
    ap.add_argument("--k", default="64,512")
    ap.add_argument("--max-iter", type=int, default=5)
    ap.add_argument("--alpha", type=float, default=1e-2)
    ap.add_argument("--l1-ratio", type=float, default=1e-2)
    ap.add_argument("--host", action="store_true")
    args = ap.parse_args()
    X = make_interactions(args.shape).astype(np.float32)
    n_it = args.max_iter
    nmf_fit(X[:2000], 8, init="random", tol=0.0, max_iter=1)  # (the first call of a process pays the code-object load)
    for k in (int(v) for v in args.k.split(",")):
        stats = {}
        t0 = time.perf_counter()
        W, H, n_iter = nmf_fit(X, k, args.alpha, args.l1_ratio, init="random", tol=0.0, max_iter=n_it, stats=stats)
        wall = time.perf_counter() - t0
        violations = stats.pop("violations")
        per_iter = {n.replace("_ms", "_ms_per_iter"): round(stats[n] / n_iter, 3)
                    for n in ("spmm_ms", "gram_ms", "sweep_ms", "d2h_ms")}
        out = dict(shape=args.shape, n_users=X.shape[0], n_items=X.shape[1], nnz=int(X.nnz), k=k, n_iter=n_iter,
                   wall_s=round(wall, 3), setup_ms=round(stats["setup_ms"], 2), **per_iter,
                   device_ms_per_iter=round(sum(per_iter.values()), 3),
                   violation_ratio_last=float(violations[-1] / violations[0]))
        if args.host:
            from sklearn.decomposition import NMF

            avg = np.sqrt(X.mean() / k)
            rng = np.random.RandomState(42)
            H0 = np.abs(avg * rng.standard_normal(size=(k, X.shape[1]))).astype(np.float32)
            W0 = np.abs(avg * rng.standard_normal(size=(X.shape[0], k))).astype(np.float32)
            model = NMF(k, init="custom", alpha_W=args.alpha, l1_ratio=args.l1_ratio, tol=0.0, max_iter=n_it)
            t0 = time.perf_counter()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                Ws = model.fit_transform(X, W=W0, H=H0)
            host_s = time.perf_counter() - t0
            rows = np.arange(0, X.shape[0], max(1, X.shape[0] // 512))
            S, Ss = W[rows] @ H, Ws[rows] @ model.components_
            out.update(host_threads=os.environ.get("OMP_NUM_THREADS"), sklearn_float32_wall_s=round(host_s, 3),
                       sklearn_ms_per_iter=round(host_s * 1e3 / n_it, 1), speedup_wall=round(host_s / wall, 2),
                       score_max_diff_over_max=float(np.abs(S - Ss).max() / np.abs(Ss).max()))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
