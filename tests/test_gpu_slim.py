"""GPU tests of SLIM (``irs_slim_fit``: ``slim_weight_*`` and ``SLIMRecommender``).

The arbiter is the float64 numpy restatement of the recurrence (``tests/_slim_restatement.py``: ascending
coordinate order, exact Gauss-Seidel).  The bar of a configuration is measured, not fixed: the same
restatement runs in float32, and a GPU column may be at most 4 x as far from float64 as the worst
float32-restatement column of that configuration (floor 1e-5); the factor is room for another summation
order inside the axpy and the Gram pass, not for another algorithm.  Error of a column:
``max|w_gpu - w_f64| / max|w_f64|``; a column that is all zero in float64 must be all zero."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sps

from _slim_restatement import gram, kkt_residual, slim_column
from conftest import record_parity
from irspack_amd import _lib
from irspack_amd.synthetic import make_interactions
from irspack_amd.utils import slim_weight_allow_negative, slim_weight_positive_only

pytestmark = pytest.mark.gpu

X_SMALL = sps.csr_matrix(
    np.asarray([[1, 1, 2, 3, 4], [0, 1, 0, 1, 0], [0, 0, 1, 0, 0], [0, 0, 0, 0, 0]], dtype=float))


def fit(X, positive_only, l2, l1, n_iter=100, tol=0.0, top_k=-1, stats=None):
    f = slim_weight_positive_only if positive_only else slim_weight_allow_negative
    return f(X, 1, n_iter, l2, l1, tol, top_k, stats=stats)


def coeffs(n_users, alpha, l1_ratio):
    return n_users * alpha * (1 - l1_ratio), n_users * alpha * l1_ratio  # slim.py:89-91


def assert_well_formed(W, n_items):
    assert sps.isspmatrix_csc(W) and W.dtype == np.float32 and W.shape == (n_items, n_items)
    assert W.indptr[0] == 0 and W.indptr[-1] == W.nnz and (np.diff(W.indptr) >= 0).all()
    assert (W.data != 0).all() and np.isfinite(W.data).all()
    for j in range(n_items):
        rows = W.indices[W.indptr[j]:W.indptr[j + 1]]
        assert (np.diff(rows) > 0).all() and j not in rows
    assert (W.diagonal() == 0).all()


def same_bytes(A, B):
    return (A.indptr.tobytes() == B.indptr.tobytes() and A.indices.tobytes() == B.indices.tobytes()
            and A.data.tobytes() == B.data.tobytes())


_ML100K = {}


def ml100k(ratings=False):
    if ratings not in _ML100K:
        X = make_interactions("ml100k").astype(np.float64)
        if ratings:
            X.data = np.random.default_rng(17).integers(1, 6, size=X.nnz).astype(np.float64)
        _ML100K[ratings] = (X, gram(X), gram(X, np.float32))
    return _ML100K[ratings]


def sample_columns(X, n=12, seed=3):
    """n columns by a seeded generator, the most and the least popular item among them"""
    pop = np.asarray((X != 0).sum(axis=0)).ravel()
    cols = {int(pop.argmax()), int(pop.argmin())}
    rng = np.random.default_rng(seed)
    while len(cols) < n:
        cols.add(int(rng.integers(0, X.shape[1])))
    return sorted(cols)


def column_errors(W, G64, G32, cols, l2, l1, n_iter, positive_only):
    """(gpu error, float32-restatement error, float64 column, gpu column) per sampled column"""
    out = []
    for j in cols:
        w64 = slim_column(G64, j, l2, l1, n_iter, 0.0, positive_only)
        w32 = slim_column(G32, j, l2, l1, n_iter, 0.0, positive_only).astype(np.float64)
        wg = np.asarray(W[:, [j]].todense()).ravel().astype(np.float64)
        scale = np.abs(w64).max()
        if scale == 0:
            out.append((0.0 if not wg.any() else np.inf, 0.0 if not w32.any() else np.inf, w64, wg))
        else:
            out.append((np.abs(wg - w64).max() / scale, np.abs(w32 - w64).max() / scale, w64, wg))
    return out


# ------------------------------------------------------------------ 1. the reference's own tests
@pytest.mark.parametrize("positive_only", [True, False])
def test_reference_elasticnet_case(positive_only):
    """tests/recommenders/test_slim.py of the reference: X_small, alpha = 0.1, l1_ratio = 0.5, n_iter = 100,
    tol = 0, every column against sklearn's ElasticNet (rtol 1e-2, the reference's) and against float64."""
    linear_model = pytest.importorskip("sklearn.linear_model")
    alpha, l1_ratio = 0.1, 0.5
    X = X_SMALL
    l2, l1 = coeffs(X.shape[0], alpha, l1_ratio)
    W = fit(X, positive_only, l2, l1, n_iter=100, tol=0.0)
    assert_well_formed(W, 5)
    Wd = np.asarray(W.todense(), dtype=np.float64)
    G64 = gram(X)
    worst = 0.0
    for j in range(5):
        Xd = X.toarray()
        y = Xd[:, j].copy()
        Xd[:, j] = 0.0
        en = linear_model.ElasticNet(alpha=alpha, l1_ratio=l1_ratio, fit_intercept=False, positive=positive_only,
                                     max_iter=100, tol=1e-8)
        en.fit(Xd, y)
        np.testing.assert_allclose(Wd[:, j], en.coef_, rtol=1e-2)
        w64 = slim_column(G64, j, l2, l1, 100, 0.0, positive_only)
        scale = np.abs(w64).max()
        if scale == 0:
            assert not Wd[:, j].any()
        else:
            worst = max(worst, np.abs(Wd[:, j] - w64).max() / scale)
            assert (Wd[:, j] != 0).tolist() == (w64 != 0).tolist()
    record_parity("test_reference_elasticnet_case", f"positive_only={positive_only}", worst_col_err_vs_f64=worst)
    assert worst <= 1e-5


def test_reference_top_k_case():
    """the reference's top_k = 1 test: alpha = 1e-4, l1_ratio = 0 - at most one positive entry per column,
    equal to the unrestricted column's maximum"""
    X = X_SMALL
    l2, l1 = coeffs(X.shape[0], 1e-4, 0.0)
    W_all = np.asarray(fit(X, True, l2, l1, 100, 0.0).todense())
    W_one = fit(X, True, l2, l1, 100, 0.0, top_k=1)
    assert_well_formed(W_one, 5)
    W_one = np.asarray(W_one.todense())
    assert ((W_one > 0).sum(axis=0) <= 1).all() and (W_one >= 0).all()
    np.testing.assert_array_equal(W_one.max(axis=0), W_all.max(axis=0))


# ------------------------------------------------------------------ 2. same order, same sweeps, at size
CONFIGS = [(0.05, 0.01, 100), (1e-3, 0.5, 100), (0.01, 0.5, 100), (1e-3, 0.5, 3)]
SIZE_CASES = [(False, c) for c in CONFIGS] + [(True, CONFIGS[0])]


@pytest.mark.parametrize("positive_only", [True, False])
@pytest.mark.parametrize("ratings, config", SIZE_CASES)
def test_matches_float64_restatement_at_ml100k(ratings, config, positive_only):
    """(1e-3, 0.5, 3) is unconverged on purpose: only an implementation that keeps the order passes."""
    alpha, l1_ratio, n_iter = config
    X, G64, G32 = ml100k(ratings)
    l2, l1 = coeffs(X.shape[0], alpha, l1_ratio)
    W = fit(X, positive_only, l2, l1, n_iter, 0.0)
    assert_well_formed(W, X.shape[1])
    cols = sample_columns(X)
    res = column_errors(W, G64, G32, cols, np.float32(l2), np.float32(l1), n_iter, positive_only)
    gpu_worst, f32_worst = max(r[0] for r in res), max(r[1] for r in res)
    bar = max(4.0 * f32_worst, 1e-5)
    record_parity("test_matches_float64_restatement_at_ml100k",
                  f"ratings={ratings} alpha={alpha} l1_ratio={l1_ratio} n_iter={n_iter} positive_only={positive_only}",
                  n_cols=len(cols), gpu_worst_col_err=gpu_worst, f32_restatement_worst_col_err=f32_worst, bar=bar,
                  nnz=int(W.nnz))
    assert gpu_worst <= bar, (gpu_worst, f32_worst)
    for (_, _, w64, wg), j in zip(res, cols):
        big = np.abs(w64) > bar
        assert (wg[big] != 0).all(), j


# ------------------------------------------------------------------ 3. optimality, independent of order
@pytest.mark.parametrize("positive_only", [True, False])
def test_kkt_residual(positive_only):
    alpha, l1_ratio, n_iter, tol = 0.01, 0.5, 400, 1e-7
    X, G64, G32 = ml100k(False)
    l2, l1 = coeffs(X.shape[0], alpha, l1_ratio)
    W = fit(X, positive_only, l2, l1, n_iter, tol)
    cols = sample_columns(X)
    l2f, l1f = float(np.float32(l2)), float(np.float32(l1))
    gpu, f32 = [], []
    for j in cols:
        wg = np.asarray(W[:, [j]].todense()).ravel()
        w32 = slim_column(G32, j, np.float32(l2), np.float32(l1), n_iter, tol, positive_only)
        gpu.append(kkt_residual(G64, j, wg, l2f, l1f, positive_only))
        f32.append(kkt_residual(G64, j, w32, l2f, l1f, positive_only))
    bar = max(4.0 * max(f32), 1e-5 * l1f)
    record_parity("test_kkt_residual", f"positive_only={positive_only}", n_cols=len(cols), l1=l1f,
                  gpu_worst_residual=max(gpu), f32_restatement_worst_residual=max(f32), bar=bar)
    assert max(gpu) <= bar, (max(gpu), max(f32))


# ------------------------------------------------------------------ 4. tol
def test_tol():
    X, _, _ = ml100k(False)
    l2, l1 = coeffs(X.shape[0], 1e-3, 0.5)  # the unconverged configuration
    assert same_bytes(fit(X, False, l2, l1, n_iter=50, tol=1e9), fit(X, False, l2, l1, n_iter=1, tol=0.0))
    assert not same_bytes(fit(X, False, l2, l1, n_iter=7, tol=0.0), fit(X, False, l2, l1, n_iter=6, tol=0.0))


# ------------------------------------------------------------------ 5. top_k
def test_top_k_keeps_the_largest_values():
    X, _, _ = ml100k(False)
    l2, l1 = coeffs(X.shape[0], 1e-3, 0.5)
    W_all = fit(X, False, l2, l1, 20, 0.0)
    W_top = fit(X, False, l2, l1, 20, 0.0, top_k=5)
    assert_well_formed(W_top, X.shape[1])
    assert (W_all.data < 0).any()  # by value, not by magnitude, is a real distinction here
    n_cut = 0
    for j in range(X.shape[1]):
        rows = W_all.indices[W_all.indptr[j]:W_all.indptr[j + 1]]
        vals = W_all.data[W_all.indptr[j]:W_all.indptr[j + 1]]
        if rows.size > 5:
            keep = np.sort(np.lexsort((rows, -vals))[:5])  # largest values, ties: the lower row
            rows, vals = rows[keep], vals[keep]
            n_cut += 1
        np.testing.assert_array_equal(W_top.indices[W_top.indptr[j]:W_top.indptr[j + 1]], rows)
        np.testing.assert_array_equal(W_top.data[W_top.indptr[j]:W_top.indptr[j + 1]], vals)
    assert n_cut > 0
    assert fit(X, False, l2, l1, 2, 0.0, top_k=0).nnz == 0


# ------------------------------------------------------------------ 6. reproducibility, the second path
@pytest.fixture()
def lds_switch():
    old = os.environ.get("IRSPACK_AMD_SLIM_LDS")
    yield
    if old is None:
        os.environ.pop("IRSPACK_AMD_SLIM_LDS", None)
    else:
        os.environ["IRSPACK_AMD_SLIM_LDS"] = old


@pytest.mark.parametrize("positive_only", [True, False])
def test_reproducible_and_global_path_identical(positive_only, lds_switch):
    """Two calls: the same bytes.  IRSPACK_AMD_SLIM_LDS=0 (the running vector in global memory): the same
    bytes too - every element of the running vector sees the same operations in the same order on both
    paths, only where it is kept differs.  The library reports which path a call took
    (``irs_slim_last_launch``): the switch flips it, both run 256 threads at this size."""
    X, _, _ = ml100k(True)
    l2, l1 = coeffs(X.shape[0], 1e-3, 0.5)
    os.environ.pop("IRSPACK_AMD_SLIM_LDS", None)
    on, off = {}, {}
    A = fit(X, positive_only, l2, l1, 10, 0.0, stats=on)
    B = fit(X, positive_only, l2, l1, 10, 0.0)
    assert A.nnz > 0 and same_bytes(A, B)
    os.environ["IRSPACK_AMD_SLIM_LDS"] = "0"
    assert same_bytes(A, fit(X, positive_only, l2, l1, 10, 0.0, stats=off))
    assert on["lds_r"] is True and off["lds_r"] is False
    assert on["threads"] == 256 and off["threads"] == 256
    assert on["lds_bytes"] == 400 + 4 * X.shape[1] and off["lds_bytes"] == 400
    assert (on["sweeps_total"], on["updates_total"]) == (off["sweeps_total"], off["updates_total"])


@pytest.mark.parametrize("positive_only", [True, False])
def test_ml100k_bytes_are_the_recorded_ones(positive_only):
    """The 256-thread result at the ML-100K shape is held to the bytes recorded before the launch decision moved
    into slim_host_plan.hpp (tests/golden/slim_ml100k_sha256.json): a change to the descent for the wide
    shapes must leave this one as it was."""
    import hashlib
    import json

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "slim_ml100k_sha256.json")) as f:
        want = json.load(f)[f"positive_only={positive_only}"]
    X, _, _ = ml100k(True)
    l2, l1 = coeffs(X.shape[0], 1e-3, 0.5)
    W = fit(X, positive_only, l2, l1, 10, 0.0)
    assert W.data.dtype == np.float32
    got = hashlib.sha256(W.indptr.astype(np.int32).tobytes() + W.indices.astype(np.int32).tobytes()
                         + W.data.tobytes()).hexdigest()
    assert (int(W.nnz), got) == (want["nnz"], want["sha256"])


# ------------------------------------------------------------------ 7. edges
@pytest.mark.parametrize("positive_only", [True, False])
def test_untouched_item_and_empty_user(positive_only):
    """an item nobody touched with l2 = 0 (G_ff + l2 == 0), a user without interactions, I not a multiple
    of 64: finite output, the item's row and column empty, every column equal to float64's"""
    X = make_interactions("tiny").astype(np.float64)[:, :157].tolil()
    X[:, 40] = 0
    X[7, :] = 0
    X = X.tocsr()
    W = fit(X, positive_only, 0.0, 2.0, 30, 0.0)
    assert_well_formed(W, 157)
    Wd = np.asarray(W.todense(), dtype=np.float64)
    assert not Wd[40, :].any() and not Wd[:, 40].any()
    G64, G32 = gram(X), gram(X, np.float32)
    res = column_errors(W, G64, G32, range(157), np.float32(0.0), np.float32(2.0), 30, positive_only)
    gpu_worst, f32_worst = max(r[0] for r in res), max(r[1] for r in res)
    record_parity("test_untouched_item_and_empty_user", f"positive_only={positive_only}",
                  gpu_worst_col_err=gpu_worst, f32_restatement_worst_col_err=f32_worst)
    assert gpu_worst <= max(4.0 * f32_worst, 1e-5)


def test_single_item_and_empty_matrix():
    W = fit(sps.csr_matrix(np.ones((3, 1))), True, 0.1, 0.1, 5, 0.0)
    assert W.shape == (1, 1) and W.nnz == 0
    W = fit(sps.csr_matrix((4, 6)), False, 0.0, 0.0, 5, 0.0)
    assert W.shape == (6, 6) and W.nnz == 0 and W.indptr.tolist() == [0] * 7


def test_above_the_lds_threshold():
    """70,000 items: the running vector (280 KB) cannot live in LDS, the kernel keeps it in global memory
    without the switch.  Items without interactions never move (G_ff = 0, l2 > 0), so the fit restricted to
    the touched items is the fit of the compacted matrix, which goes through the LDS path; float64
    arbitrates a few columns of it.  Needs 39 GB for the two dense I x I arrays: skipped (and said so) when
    the device reports less free memory."""
    n_items, n_users = 70_000, 400
    rng = np.random.default_rng(23)
    touched = np.sort(rng.choice(n_items, size=300, replace=False))
    dense = (rng.random((n_users, touched.size)) < 0.03).astype(np.float64)
    small = sps.csr_matrix(dense)
    coo = small.tocoo()
    big = sps.csr_matrix((coo.data, (coo.row, touched[coo.col])), shape=(n_users, n_items))
    l2, l1 = 0.5, 0.25
    stats = {}
    try:
        W_big = fit(big, False, l2, l1, 4, 0.0, stats=stats)
    except RuntimeError as exc:
        if "device memory" in str(exc):
            pytest.skip(f"NOT RUN: {exc}")
        raise
    print("test_above_the_lds_threshold: RUN (the device had the memory)")
    assert stats["lds_r"] is False and stats["threads"] == 256
    W_small = fit(small, False, l2, l1, 4, 0.0)
    assert W_small.nnz > 0 and W_big.nnz == W_small.nnz
    sub = W_big[touched][:, touched].tocsc()
    sub.sort_indices()
    assert same_bytes(sub, W_small)
    G64, G32 = gram(small), gram(small, np.float32)
    res = column_errors(W_small, G64, G32, range(0, 300, 25), np.float32(l2), np.float32(l1), 4, False)
    assert max(r[0] for r in res) <= max(4.0 * max(r[1] for r in res), 1e-5)


def test_bare_c_abi_rejects_duplicates_and_bad_indptr():
    """duplicate column indices within a row are an invalid-argument status (documented in the header:
    rejected, not summed); a non-monotone indptr is a status, not a wild read; the Python wrapper sums
    duplicates before the call"""
    lib = _lib.lib()
    data = np.ones(4, dtype=np.float32)

    def call(indptr, indices):
        indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int32)
        h = C.c_void_p()
        st = lib.irs_slim_fit(len(indptr) - 1, 3, _lib.ptr(indptr, C.c_int64), _lib.ptr(indices, C.c_int32),
                              _lib.ptr(data, C.c_float), 1, 2, 0.1, 0.1, 0.0, -1, 0, C.byref(h))
        if st == 0:
            lib.irs_slim_destroy(h)
        return st

    assert call([0, 2, 4], [0, 1, 1, 2]) == 0
    assert call([0, 2, 4], [1, 1, 1, 2]) == 1
    assert "duplicate" in lib.irs_last_error().decode()
    assert call([0, 3, 2, 4], [0, 1, 1, 2]) == 1
    assert call([5, 2, 4], [0, 1, 1, 2]) == 1
    dup = sps.csr_matrix((np.ones(4), np.array([1, 1, 0, 2]), np.array([0, 2, 4])), shape=(2, 3))
    summed = sps.csr_matrix(dup.toarray())
    assert same_bytes(fit(dup, False, 0.1, 0.1, 5, 0.0), fit(summed, False, 0.1, 0.1, 5, 0.0))


# ------------------------------------------------------------------ 8. the recommender end to end
def test_recommender_end_to_end():
    from irspack_amd.evaluation import Evaluator
    from irspack_amd.recommenders import BaseSimilarityRecommender, SLIMRecommender

    X = make_interactions("tiny").astype(np.float64)
    rng = np.random.default_rng(1)
    held = sps.csr_matrix((rng.random(X.shape) < 0.03).astype(np.float64))
    rec = SLIMRecommender(X, alpha=1e-3, l1_ratio=0.5, n_threads=1).learn()
    W = rec.W
    assert_well_formed(W, X.shape[1])
    assert W.nnz > 0
    users = np.array([0, 5, 17, 299])
    np.testing.assert_array_equal(rec.get_score(users), np.asarray((X[users] @ W).todense()))

    class Handmade(BaseSimilarityRecommender):
        def _learn(self):
            self._W = W.copy()

    ev = Evaluator(held, cutoff=10)
    got, want = ev.get_score(rec), ev.get_score(Handmade(X).learn())
    assert got == want and got["ndcg"] > 0
    neg = SLIMRecommender(X, alpha=1e-3, l1_ratio=0.5, positive_only=False, top_k=3, n_iter=5).learn().W
    assert (np.diff(neg.indptr) <= 3).all()
