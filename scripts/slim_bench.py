"""Device time of a SLIM fit (irs_slim_fit) at a synthetic shape, ML-20M by default: the three phase
times (Gram matrix with upload and transpose, coordinate descent, emit; HIP events), the sweeps run
summed over the columns and the coordinate changes applied, at the constructor defaults of
SLIMRecommender and at one weakly regularised point (alpha = 1e-3, l1_ratio = 0.5).

One JSON line per point.  Derived rates: ``visits_per_s`` = sweeps_total * n_items / descent time
(coordinate visits), ``axpy_gbs`` = updates_total * 4 n_items bytes / descent time (each change reads one
column of G).

    python scripts/slim_bench.py [--shape ml20m] [--points default,weak] [--n-iter 100] [--allow-negative]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from irspack_amd.synthetic import make_interactions  # noqa: E402
from irspack_amd.utils import _slim  # noqa: E402

POINTS = {"default": (0.05, 0.01), "weak": (1e-3, 0.5)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml20m")
    ap.add_argument("--points", default="default,weak")
    ap.add_argument("--n-iter", type=int, default=100)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--allow-negative", action="store_true")
    args = ap.parse_args()
    X = make_interactions(args.shape)
    n_users, n_items = X.shape
    for name in args.points.split(","):
        alpha, l1_ratio = POINTS[name]
        stats = {}
        t0 = time.perf_counter()
        W = _slim(X, not args.allow_negative, 1, args.n_iter, n_users * alpha * (1 - l1_ratio),
                  n_users * alpha * l1_ratio, args.tol, -1, None, stats)
        wall = time.perf_counter() - t0
        descent_s = max(stats["descent_ms"], 1e-6) / 1e3
        print(json.dumps(dict(
            shape=args.shape, n_users=n_users, n_items=n_items, nnz=int(X.nnz), point=name, alpha=alpha,
            l1_ratio=l1_ratio, positive_only=not args.allow_negative, n_iter=args.n_iter, tol=args.tol,
            gram_ms=round(stats["gram_ms"], 3), descent_ms=round(stats["descent_ms"], 3),
            emit_ms=round(stats["emit_ms"], 3), wall_s=round(wall, 3), sweeps_total=stats["sweeps_total"],
            updates_total=stats["updates_total"], w_nnz=int(W.nnz),
            visits_per_s=stats["sweeps_total"] * n_items / descent_s,
            axpy_gbs=stats["updates_total"] * 4.0 * n_items / descent_s / 1e9)), flush=True)


if __name__ == "__main__":
    main()
