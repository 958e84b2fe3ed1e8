"""Device time of a truncated SVD fit (irs_truncsvd_*) at a synthetic shape, ML-20M by default, for
n_components = 64 and 512: the phase times from ``stats`` (set-up, sparse x block products, Gram matrices,
Cholesky and triangular inverse, block rotations, copies home; HIP events; the host eigenproblems and the test
matrix beside them), the wall time of ``truncated_svd`` and the achieved bytes/s of the sparse x block
passes on the count ``nnz * (8 + 4 l_pad)`` bytes per pass, beside the copy and gather ceilings
``irs_measure_ceilings`` measures.

``--host`` adds scikit-learn's ``TruncatedSVD`` on the host's threads for scale.

One JSON line per point.  Run it under a time limit sized to the step, e.g.

    timeout -k 10 300 python scripts/truncsvd_bench.py
    timeout -k 10 900 python scripts/truncsvd_bench.py --k 64 --host
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from irspack_amd import _lib  # noqa: E402
from irspack_amd.synthetic import make_interactions  # noqa: E402
from irspack_amd.utils import truncated_svd  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml20m")
    ap.add_argument("--k", default="64,512")
    ap.add_argument("--host", action="store_true")
    args = ap.parse_args()
    X = make_interactions(args.shape)
    ceil = _lib.measure_ceilings()
    truncated_svd(X[:2000], 8)  # (the first call of a process pays the code-object load)
    for k in (int(v) for v in args.k.split(",")):
        stats = {}
        t0 = time.perf_counter()
        z, s, c = truncated_svd(X, k, 0, stats=stats)
        wall = time.perf_counter() - t0
        pass_bytes = float(X.nnz) * (8 + 4 * stats["l_pad"])
        gbs = pass_bytes * stats["n_spmm"] / max(stats["spmm_ms"], 1e-9) / 1e6
        device_ms = sum(stats[n] for n in ("setup_ms", "spmm_ms", "gram_ms", "chol_ms", "apply_ms", "d2h_ms"))
        out = dict(shape=args.shape, n_users=X.shape[0], n_items=X.shape[1], nnz=int(X.nnz), k=k,
                   wall_s=round(wall, 3), device_ms=round(device_ms, 2),
                   **{n: round(float(v), 3) for n, v in stats.items()},
                   eigh_share_of_wall=round(stats["eigh_ms"] / 1e3 / wall, 4), spmm_gbs=round(gbs, 1),
                   copy_gbs=round(ceil["copy_gbs"], 1), gather256_gbs=round(ceil["gather256_gbs"], 1),
                   gather512_gbs=round(ceil["gather512_gbs"], 1),
                   spmm_fraction_of_copy=round(gbs / ceil["copy_gbs"], 4), sigma_1=float(s[0]), sigma_k=float(s[-1]))
        if args.host:
            from sklearn.decomposition import TruncatedSVD

            t0 = time.perf_counter()
            svd = TruncatedSVD(n_components=k, random_state=0)
            svd.fit_transform(X.astype(np.float32))
            host_s = time.perf_counter() - t0
            out.update(host_threads=os.environ.get("OMP_NUM_THREADS"), sklearn_float32_wall_s=round(host_s, 3),
                       speedup=round(host_s / wall, 2),
                       sigma_max_diff_over_sigma_1=float(np.abs(svd.singular_values_ - s).max() / s[0]))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
