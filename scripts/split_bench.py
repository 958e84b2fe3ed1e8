"""Device time of the row-wise hold-out split (irs_split_rowwise) at a synthetic shape, ML-20M by default: the five
phase times (upload, select, scan, scatter, copy back; HIP events), their sum, the wall time of the Python call and the
rows per kernel class, once for a ratio split and once for a fixed-n split.

One JSON line per split: the call with the smallest wall time out of ``--repeat`` (after one untimed call, which pays
for the first use of the device).

    python scripts/split_bench.py [--shape ml20m] [--dtype float64] [--ratio 0.2] [--n-test 10] [--repeat 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from irspack_amd.synthetic import make_interactions  # noqa: E402
from irspack_amd.utils import (rowwise_train_test_split_by_fixed_n,  # noqa: E402
                               rowwise_train_test_split_by_ratio)

PHASES = ("upload_ms", "select_ms", "scan_ms", "scatter_ms", "d2h_ms")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml20m")
    ap.add_argument("--dtype", default="float64")
    ap.add_argument("--ratio", type=float, default=0.2)
    ap.add_argument("--n-test", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--seed", type=int, default=42)
    args = ap.parse_args()
    X = make_interactions(args.shape, dtype=np.dtype(args.dtype))
    n_users, n_items = X.shape
    rowwise_train_test_split_by_fixed_n(X[:1000], args.seed, 1)  # first use of the device
    calls = {
        "ratio": lambda stats: rowwise_train_test_split_by_ratio(X, args.seed, args.ratio, False, stats=stats),
        "fixed_n": lambda stats: rowwise_train_test_split_by_fixed_n(X, args.seed, args.n_test, stats=stats),
    }
    for name, call in calls.items():
        best = None
        for _ in range(max(args.repeat, 1)):
            stats = {}
            t0 = time.perf_counter()
            X_train, X_test = call(stats)
            wall = time.perf_counter() - t0
            if best is None or wall < best[0]:
                best = (wall, stats, int(X_train.nnz), int(X_test.nnz))
        wall, stats, nnz_train, nnz_test = best
        print(json.dumps(dict(
            shape=args.shape, dtype=args.dtype, n_users=n_users, n_items=n_items, nnz=int(X.nnz), split=name,
            ratio=args.ratio if name == "ratio" else None, n_test=args.n_test if name == "fixed_n" else None,
            nnz_train=nnz_train, nnz_test=nnz_test, **{p: round(stats[p], 3) for p in PHASES},
            device_ms=round(sum(stats[p] for p in PHASES), 3), wall_ms=round(wall * 1e3, 3),
            rows_empty=stats["rows_empty"], rows_wave=stats["rows_wave"], rows_lds=stats["rows_lds"],
            rows_stream=stats["rows_stream"])), flush=True)


if __name__ == "__main__":
    main()
