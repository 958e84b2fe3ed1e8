"""Records what the truncated SVD, the NMF fit, EASE / EDLAE, SLIM, BPR / WARP, Mult-VAE and the iALS feature ridge
return, per configuration: ``sparse_block_results.json``, the golden of tests/test_gpu_sparse_block_golden.py.
Recorded before the host code these fits share (the matrix checks, the phase spans, the segment plan and the
launches of the product, Gram, Cholesky and inverse kernels) moved into csr_checks.hpp, phase_spans.hpp,
sparse_block_plan.hpp, sparse_block.hpp and tile_solver_calls.hpp.  No kernel changed in that move, and every sum
of these paths has a fixed order, so every output is the same bytes before and after.

Needs a GPU and the built library:

    python tests/golden/make_sparse_block_results.py            # writes the golden
    python tests/golden/make_sparse_block_results.py --print    # prints the same JSON (what the test runs)

Per configuration: the SHA-256 of every output array and the integer outputs (``n_iter``, ``l_pad``, ``n_spmm``).

X is 1100 x 520, about 2 % dense, small integers; column 5 has exactly 1024 entries, column 6 has 1025 and column 7
all 1100: in X^T these are the row that just fits one segment, the 1024 + 1 split and the 1024 + 76 split.  X^T
(520 x 1100) takes the truncated SVD's ``transposed`` orientation and puts the split rows into the matrix itself.
The widths l = 1, 64, 65, 129, 257, 513 pad to 64, 64, 128, 192, 320, 576 columns: every instance of the product
kernels and 1, 1, 2, 3, 5, 9 block columns of the Cholesky and inverse loops.  Nothing between the calls is computed
by a host library (no eigen-decomposition): the matrices handed to ``apply`` and ``finish`` are fixed non-zero
multiples of 1 / 8, so the record depends on the device code and this file alone.
"""
import ctypes as C
import hashlib
import json
import os
import sys
import warnings

import numpy as np
import scipy.sparse as sps

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
GOLDEN = os.path.join(HERE, "sparse_block_results.json")

N_USERS, N_ITEMS = 1100, 520
SVD_WIDTHS = (1, 64, 65, 129, 257, 513)
TRANSFORM_K = (64, 65, 513)
NMF_K = (1, 65, 257, 513)
EASE_ITEMS = (1, 64, 65, 129, 321)
FEW = 48  # users of the BPR / WARP / Mult-VAE / iALS configurations
PHASE_SWITCHES = ("IRSPACK_AMD_BPR_PHASES", "IRSPACK_AMD_MULTVAE_PHASES")


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def matrix() -> sps.csr_matrix:
    rs = np.random.RandomState(20240)
    dense = (rs.random_sample((N_USERS, N_ITEMS)) < 0.02) * rs.randint(1, 4, size=(N_USERS, N_ITEMS))
    for col, count in ((5, 1024), (6, 1025), (7, N_USERS)):
        dense[:, col] = 0
        dense[rs.permutation(N_USERS)[:count], col] = rs.randint(1, 4, size=count)
    X = sps.csr_matrix(dense.astype(np.float32))
    X.sort_indices()
    assert [int(n) for n in np.diff(X.tocsc().indptr)[5:8]] == [1024, 1025, N_USERS]
    return X


def eighths(rs, shape) -> np.ndarray:
    return np.ascontiguousarray(rs.choice([-2, -1, 1, 2], size=shape) / 8.0, dtype=np.float32)


def svd_stages(A, l):
    """range (n_iter = 1), apply, project, finish through the C ABI, with fixed matrices between the calls"""
    from irspack_amd import _lib
    from irspack_amd._lib import check, lib, ptr

    n_users, n_items = A.shape
    _, indptr, indices, data = _lib.csr_arrays(A, np.float32)
    rs = np.random.RandomState(1000 + l)
    n = min(n_users, n_items)
    l2, k = max(1, l - 1), max(1, l - 2)
    omega = np.ascontiguousarray(rs.normal(size=(n, l)), dtype=np.float32)
    M, rot = eighths(rs, (l, l2)), eighths(rs, (l2, k))
    fptr = lambda a: ptr(a, C.c_float)  # noqa: E731
    out = {}
    h = C.c_void_p()
    check(lib().irs_truncsvd_create(n_users, n_items, ptr(indptr, C.c_int64), ptr(indices, C.c_int32), fptr(data),
                                    _lib.default_device(), C.byref(h)))
    try:
        G = np.zeros((l, l), dtype=np.float32)
        check(lib().irs_truncsvd_range(h, fptr(omega), n, l, 1, fptr(G)))
        out["range_gram"] = sha(G)
        G = np.zeros((l2, l2), dtype=np.float32)
        check(lib().irs_truncsvd_apply(h, fptr(M), l2, fptr(G)))
        out["apply_gram"] = sha(G)
        G = np.zeros((l2, l2), dtype=np.float32)
        check(lib().irs_truncsvd_project(h, fptr(G)))
        out["project_gram"] = sha(G)
        z, comps = np.zeros((n_users, k), dtype=np.float32), np.zeros((k, n_items), dtype=np.float32)
        check(lib().irs_truncsvd_finish(h, fptr(rot), k, fptr(z), fptr(comps)))
        out["z"], out["components"] = sha(z), sha(comps)
        st = _lib.TruncSvdStatsStruct()
        check(lib().irs_truncsvd_stats(h, C.cast(C.byref(st), C.c_void_p)))
        out["n_spmm"], out["l_pad"] = int(st.n_spmm), int(st.l_pad)
    finally:
        lib().irs_truncsvd_destroy(h)
    return out


def nmf(A, k, update_H, with_stats):
    from irspack_amd.utils import _nmf_call

    rs = np.random.RandomState(2000 + k)
    W = np.ascontiguousarray(rs.randint(0, 9, size=(A.shape[0], k)) / 8.0, dtype=np.float32)
    H = np.ascontiguousarray(rs.randint(0, 9, size=(k, A.shape[1])) / 8.0, dtype=np.float32)
    stats = {} if with_stats else None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        n_iter = _nmf_call(A, W, H, 0.001, 0.5, 0.0, 2, update_H, None, stats)
    out = {"W": sha(W), "H": sha(H), "n_iter": int(n_iter)}
    if with_stats:  # (the violation sums come back only with the statistics; the times are not recorded)
        out["violations"] = sha(stats["violations"])
    return out


def trainer_state(make, switch, value):
    os.environ[switch] = value
    try:
        t = make()
        t.run_epochs(2)
        state = t.get_state()
        t.close()
    finally:
        os.environ.pop(switch, None)
    return {name: sha(v) if isinstance(v, np.ndarray) else int(v) for name, v in sorted(state.items())}


def ials_feature_ridge(A):
    from irspack_amd.recommenders._ials_core import (IALSModelConfigBuilder, IALSSolverConfigBuilder, IALSTrainer,
                                                      LossType, SolverType)

    rs = np.random.RandomState(77)
    F = sps.csr_matrix(((rs.random_sample((A.shape[0], 129)) < 0.3) * rs.randint(1, 4, size=(A.shape[0], 129)))
                       .astype(np.float32))
    mc = (IALSModelConfigBuilder().set_K(32).set_alpha0(0.1).set_reg(0.05).set_nu(1.0).set_init_stdev(0.1)
          .set_random_seed(1).set_loss_type(LossType.ORIGINAL).set_lambda_user_feature(0.5)
          .set_lambda_item_feature(0.3).build())
    sc = IALSSolverConfigBuilder().set_n_threads(1).set_solver_type(SolverType.CHOLESKY).set_max_cg_steps(3).build()
    t = IALSTrainer(mc, A, F, None)
    for _ in range(2):
        t.step(sc)  # (irs_ials_feature_step)
    return {"user": sha(t.user), "item": sha(t.item), "user_feature_weight": sha(t.user_feature_weight)}


def record():
    from irspack_amd.recommenders.bpr import BPRFMTrainer
    from irspack_amd.recommenders.multvae import MultVAETrainer
    from irspack_amd.utils import _slim, dense_slim_weight, truncated_svd_transform

    for name in PHASE_SWITCHES:
        os.environ.pop(name, None)
    X = matrix()
    Xt = sps.csr_matrix(X.T)
    Xt.sort_indices()
    out = {}
    for name, A in (("X", X), ("Xt", Xt)):
        for l in SVD_WIDTHS:
            out[f"svd_{name}_l{l}"] = svd_stages(A, l)
    for k in TRANSFORM_K:
        comps = eighths(np.random.RandomState(3000 + k), (k, N_USERS))
        out[f"transform_33rows_k{k}"] = {"z": sha(truncated_svd_transform(Xt[:33], comps))}
        out[f"transform_1row_k{k}"] = {"z": sha(truncated_svd_transform(Xt[7:8], comps))}
    for k in NMF_K:
        for update_H in (1, 0):
            for with_stats in (0, 1):
                out[f"nmf_k{k}_updateH{update_H}_stats{with_stats}"] = nmf(X, k, bool(update_H), bool(with_stats))
    out["nmf_Xt_k65_updateH1_stats0"] = nmf(Xt, 65, True, False)
    for n in EASE_ITEMS:
        out[f"ease_{n}items"] = {"W": sha(dense_slim_weight(X[:, :n], 10.0))}
    out["edlae_129items"] = {"W": sha(dense_slim_weight(X[:, :129], 10.0, 0.25))}
    for positive_only in (1, 0):
        W = _slim(X[:, :65], bool(positive_only), 1, 5, 0.1, 0.01, 0.0, -1, None)
        out[f"slim_65items_positive{positive_only}"] = {"indptr": sha(W.indptr.astype(np.int64)),
                                                        "indices": sha(W.indices.astype(np.int32)), "data": sha(W.data)}
    few = sps.csr_matrix(X[:FEW])
    for loss in ("bpr", "warp"):
        for value in ("0", "1"):
            out[f"{loss}_phases{value}"] = trainer_state(
                lambda: BPRFMTrainer(few, 16, 1e-4, 1e-4, loss=loss, learning_rate=0.05, batch_size=256, random_seed=3,
                                     max_sampled=5), "IRSPACK_AMD_BPR_PHASES", value)
    for value in ("0", "1"):
        out[f"multvae_phases{value}"] = trainer_state(
            lambda: MultVAETrainer(few, 8, 24, None, 0.5, 0.0, 0.2, 3, 16, 1e-3, random_seed=5),
            "IRSPACK_AMD_MULTVAE_PHASES", value)
    out["ials_feature_ridge_F129"] = ials_feature_ridge(few)
    return out


if __name__ == "__main__":
    text = json.dumps(record(), indent=1, sort_keys=True)
    if "--print" in sys.argv:
        print(text)
    else:
        with open(GOLDEN, "w") as f:
            f.write(text + "\n")
        print("wrote", GOLDEN)
