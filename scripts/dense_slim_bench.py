"""Device time of an EASE / EDLAE fit (irs_dense_slim_fit) at a synthetic shape, ML-20M by default: the
phase times from ``stats`` (Gram matrix with upload and transpose, Cholesky factor, inverse from the
factor, finalize, device-to-host copy; HIP events), the wall time of ``learn()`` and the achieved TF/s on
the algorithmic count ``I^3`` (factor + triangular inverse + product, ``I^3 / 3`` each) over the three
dense phases, beside the measured fp32 MFMA ceiling (``irs_measure_ceilings``).

``--host`` runs the comparison leg instead: the reference's own formulation on the host (scipy sparse
product, ``scipy.linalg.inv`` on float32, with the threads the BLAS is given) beside a device fit of the
same matrix; ``--host-items N`` restricts both to the N most popular items when the full size does not fit
the time limit.

One JSON line per point.  Run it under a time limit sized to the step, e.g.

    timeout -k 10 300 python scripts/dense_slim_bench.py
    timeout -k 10 900 python scripts/dense_slim_bench.py --points ease --host --host-items 8000
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sps

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from irspack_amd import _lib  # noqa: E402
from irspack_amd.recommenders import DenseSLIMRecommender, EDLAERecommender  # noqa: E402
from irspack_amd.synthetic import make_interactions  # noqa: E402
from irspack_amd.utils import dense_slim_weight  # noqa: E402

POINTS = {"ease": (1.0, None), "edlae": (1.0, 0.1)}


def host_fit(X, reg, dropout_p):
    """the reference's arithmetic (dense_slim.py:39-53 / edlae.py:49-66) restated"""
    import scipy.linalg

    Xf = X.astype(np.float32)
    P = np.asarray((Xf.T @ Xf).todense())
    idx = np.arange(P.shape[0])
    lam = np.float32(reg) if dropout_p is None else dropout_p / (1 - dropout_p) * np.diag(P) + reg
    P[idx, idx] += lam
    P = scipy.linalg.inv(P, overwrite_a=True)
    P *= -(1 / np.diag(P))[np.newaxis, :]
    P[idx, idx] = 0
    return P


def device_point(X, name, ceiling):
    reg, dropout_p = POINTS[name]
    rec = DenseSLIMRecommender(X, reg=reg) if dropout_p is None else EDLAERecommender(X, reg=reg, dropout_p=dropout_p)
    t0 = time.perf_counter()
    rec.learn()
    wall = time.perf_counter() - t0
    stats = {}
    ds = 0.0 if dropout_p is None else np.float32(dropout_p / (1 - dropout_p))
    same = dense_slim_weight(X, reg, ds, stats=stats).tobytes() == rec.W.tobytes()
    n = X.shape[1]
    dense_s = (stats["factor_ms"] + stats["invert_ms"]) / 1e3
    tflops = float(n) ** 3 / max(dense_s, 1e-9) / 1e12
    return dict(point=name, reg=reg, dropout_p=dropout_p, n_users=X.shape[0], n_items=n, nnz=int(X.nnz),
                n_pad=stats["n_pad"], gram_ms=round(stats["gram_ms"], 3), factor_ms=round(stats["factor_ms"], 3),
                invert_ms=round(stats["invert_ms"], 3), finalize_ms=round(stats["finalize_ms"], 3),
                d2h_ms=round(stats["d2h_ms"], 3), learn_wall_s=round(wall, 3), second_call_same_bytes=same,
                tflops_on_I3=round(tflops, 3), mfma_f32_ceiling_tflops=ceiling,
                fraction_of_ceiling=round(tflops / ceiling, 4) if ceiling else None), rec.W


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml20m")
    ap.add_argument("--points", default="ease,edlae")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--host-items", type=int, default=0)
    args = ap.parse_args()
    X = make_interactions(args.shape)
    ceiling = round(_lib.measure_ceilings()["mfma_f32_tflops"], 2)
    if not args.host:
        for name in args.points.split(","):
            out, _ = device_point(X, name, ceiling)
            print(json.dumps(dict(shape=args.shape, **out)), flush=True)
    else:
        Xh = X
        if args.host_items:
            pop = np.asarray((X != 0).sum(axis=0)).ravel()
            Xh = sps.csr_matrix(X[:, np.sort(np.argsort(-pop, kind="stable")[:args.host_items])])
        for name in args.points.split(","):
            reg, dropout_p = POINTS[name]
            out, W = device_point(Xh, name, ceiling)
            t0 = time.perf_counter()
            Wh = host_fit(Xh, reg, dropout_p)
            host_s = time.perf_counter() - t0
            print(json.dumps(dict(shape=args.shape, leg="host", host_threads=os.environ.get("OMP_NUM_THREADS"),
                                  host_wall_s=round(host_s, 3), device_learn_wall_s=out["learn_wall_s"],
                                  speedup=round(host_s / out["learn_wall_s"], 2),
                                  max_abs_diff=float(np.abs(Wh - W).max()), **{k: out[k] for k in (
                                      "point", "n_users", "n_items", "nnz", "gram_ms", "factor_ms", "invert_ms",
                                      "finalize_ms", "d2h_ms")})), flush=True)


if __name__ == "__main__":
    main()
