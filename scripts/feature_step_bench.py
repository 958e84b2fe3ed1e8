"""ms per epoch of the feature-aware iALS epoch at the ML-20M shape (K = 64, binary interactions):
the plain irs_ials_step, the native irs_ials_feature_step, and the host-ridge path
(IALSTrainer._step_host_ridge: F x F ridge solve in scipy), at three feature sizes:

  a  users 32 dense + 200 one-hot columns, items 20 one-hot columns
  b  1,024 one-hot columns per side
  c  4,096 one-hot columns per side

One JSON line per configuration; ``gram_llt_ms`` is the one-off Gram + Cholesky of both sides
(the first feature epoch minus a later one).

    python scripts/feature_step_bench.py [--epochs 5] [--configs a,b,c] [--solver CG]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sps

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from irspack_amd import _lib  # noqa: E402
from irspack_amd.recommenders._ials_core import (IALSModelConfigBuilder, IALSSolverConfigBuilder,  # noqa: E402
                                                  IALSTrainer, LossType, SolverType)
from irspack_amd.synthetic import make_interactions  # noqa: E402


def one_hot(n, f, seed):
    rng = np.random.default_rng(seed)
    return sps.csr_matrix((np.ones(n, np.float32), (np.arange(n), rng.integers(0, f, n))), shape=(n, f))


def features(name, n_users, n_items):
    if name == "a":
        dense = sps.csr_matrix(np.random.default_rng(1).standard_normal((n_users, 32)).astype(np.float32))
        return sps.hstack([dense, one_hot(n_users, 200, 2)], format="csr"), one_hot(n_items, 20, 3)
    F = {"b": 1024, "c": 4096}[name]
    return one_hot(n_users, F, 4), one_hot(n_items, F, 5)


def timed(fn, n):
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    return (time.perf_counter() - t0) / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--configs", default="a,b,c")
    ap.add_argument("--solver", default="CG", choices=["CG", "CHOLESKY"])
    args = ap.parse_args()
    X = make_interactions("ml20m")
    mc = (IALSModelConfigBuilder().set_K(64).set_alpha0(0.1).set_reg(0.05).set_nu(1.0)
          .set_loss_type(LossType.ORIGINAL).set_lambda_user_feature(1.0).set_lambda_item_feature(1.0)
          .build())
    sc = IALSSolverConfigBuilder().set_solver_type(SolverType[args.solver]).set_max_cg_steps(3).build()
    s = sc._struct()
    for name in args.configs.split(","):
        uf, itf = features(name, *X.shape)
        t = IALSTrainer(mc, X, uf, itf)
        plain = lambda: _lib.check(_lib.lib().irs_ials_step(t._h, C.byref(s)))  # noqa: E731
        plain()
        plain_ms = timed(plain, args.epochs)
        first_ms = timed(lambda: t.step(sc), 1)  # builds and factorises both ridge systems
        native_ms = timed(lambda: t.step(sc), args.epochs)
        h = IALSTrainer(mc, X, uf, itf)
        h._step_host_ridge(sc)  # (its host Gram + LLT)
        host_ms = timed(lambda: h._step_host_ridge(sc), args.epochs)
        print(json.dumps({"config": name, "n_feat": [uf.shape[1], itf.shape[1]], "solver": args.solver,
                          "plain_ms": round(plain_ms, 3), "native_feature_ms": round(native_ms, 3),
                          "host_ridge_ms": round(host_ms, 3),
                          "gram_llt_ms": round(first_ms - native_ms, 3)}), flush=True)
        del t, h


if __name__ == "__main__":
    main()
