"""Records which profiled regions one iALS epoch launches, and how often, per configuration:
``ials_launch_names.json``, the golden of tests/test_gpu_ials_routes.py.  The factor tests prove that a
half-step's results are right; they would not notice a route that fell back to a slower kernel family.

Needs a GPU and the built library.  Row chunks of 64 entries keep the matrix small; the chunk size is
read once per process, so it is set here before the library loads:

    python tests/golden/make_ials_launch_names.py            # writes the golden
    python tests/golden/make_ials_launch_names.py --print    # prints the same JSON (what the test runs)

Shape: 300 users x 2304 items.  A row folds its partial Gramians only above 32 chunks, i.e. above 2048
entries at 64 per chunk, so one user holds 2200 items (split and folded; also above the 2048 entries at
which iALS++ gives a row a whole workgroup); a few users hold 100 - 200 (split, not folded), three items
are held by half of the users (split on the item side), the rest are short, and one user has none.
"""
import json
import os
import sys

os.environ["IRSPACK_AMD_IALS_CHUNK"] = "64"
os.environ["IRSPACK_AMD_IALS_CHUNK_LONG"] = "64"

import numpy as np  # noqa: E402
import scipy.sparse as sps  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
GOLDEN = os.path.join(HERE, "ials_launch_names.json")

N_USERS, N_ITEMS = 300, 2304

# (name, K, solver, subspace dimension, weighted data, switches set while the trainer is created)
CONFIGS = (
    [(f"K{K}_{s}_binary", K, s, 0, False, {}) for s in ("CHOLESKY", "CG") for K in (16, 64, 128, 192, 320)]
    + [("K64_CHOLESKY_weighted", 64, "CHOLESKY", 0, True, {})]
    + [(f"K64_IALSPP_sub{d}", 64, "IALSPP", d, False, {}) for d in (1, 16, 64)]
    + [(f"K128_IALSPP_sub{d}", 128, "IALSPP", d, False, {}) for d in (64, 96)]
    + [("K64_CHOLESKY_unit0", 64, "CHOLESKY", 0, False, {"IRSPACK_AMD_IALS_UNIT": "0"}),
       ("K128_CHOLESKY_wave128_0", 128, "CHOLESKY", 0, False, {"IRSPACK_AMD_IALS_WAVE128": "0"})]
)


def interactions(weighted):
    rng = np.random.default_rng(20261019)
    M = sps.random(N_USERS, N_ITEMS, density=0.012, format="lil", random_state=rng, dtype=np.float64)
    M[0, rng.choice(N_ITEMS, 2200, replace=False)] = 1.0
    for u, n in ((1, 200), (2, 130), (3, 100), (4, 65), (5, 64)):
        M[u, rng.choice(N_ITEMS, n, replace=False)] = 1.0
    for i in (7, 8, 9):
        M[rng.choice(N_USERS, 150, replace=False), i] = 1.0
    M[17, :] = 0.0
    M = M.tocsr()
    M.eliminate_zeros()
    M.sort_indices()
    M.data = rng.uniform(0.5, 3.0, M.nnz) if weighted else np.ones(M.nnz)
    return M.astype(np.float32)


def run_config(cfg, epochs=1, profile=True):
    """-> ({region: launches} of `epochs` epochs, user factors, item factors)"""
    from irspack_amd.recommenders._ials_core import (IALSModelConfigBuilder, IALSSolverConfigBuilder,
                                                      IALSTrainer, SolverType)

    _, K, solver, sub, weighted, switches = cfg
    mc = IALSModelConfigBuilder().set_K(K).set_alpha0(0.1).set_reg(1e-2).set_random_seed(42).build()
    sb = IALSSolverConfigBuilder().set_n_threads(1).set_solver_type(SolverType[solver]).set_max_cg_steps(3)
    if solver == "IALSPP":
        sb = sb.set_ialspp_subspace_dimension(sub).set_ialspp_iteration(1)
    sc = sb.build()
    saved = {k: os.environ.get(k) for k in switches}
    os.environ.update(switches)
    try:
        t = IALSTrainer(mc, interactions(weighted), device=0)  # (the switches are read here)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    t.profile(bool(profile))
    for _ in range(epochs):
        t.step(sc)
    prof = t.profile_read()
    t.profile(False)
    return {name: rec["launches"] for name, rec in sorted(prof.items())}, t.user.copy(), t.item.copy()


def record():
    return {cfg[0]: run_config(cfg)[0] for cfg in CONFIGS}


if __name__ == "__main__":
    out = json.dumps(record(), indent=1, sort_keys=True)
    if "--print" in sys.argv:
        print(out)
    else:
        with open(GOLDEN, "w") as f:
            f.write(out + "\n")
        print("wrote", GOLDEN)
