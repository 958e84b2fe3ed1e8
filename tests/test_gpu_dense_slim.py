"""GPU tests of EASE / EDLAE (``irs_dense_slim_fit``: ``dense_slim_weight``, ``DenseSLIMRecommender``,
``EDLAERecommender``).

The arbiter is the float64 numpy restatement (``tests/_dense_slim_restatement.py``).  The bar of a case is
measured, not fixed: the same restatement runs in float32 through scipy's LU inverse (the reference's own
arithmetic), and the GPU may be at most 4 x as far from float64 as that - the multiple ``test_gpu_slim.py``
uses against its float32 restatement.  Error of a matrix: the worst column of
``||W[:, j] - W64[:, j]|| / ||W64[:, j]||`` over ALL columns; a column that is exactly zero in float64 must be
exactly zero on the GPU."""
import ctypes as C
import pickle
import time

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sps

from _dense_slim_restatement import (ease_weights, optimality_residual, regularised_gram, weights_from_inverse,
                                     worst_column_error)
from conftest import record_parity
from irspack_amd import _lib
from irspack_amd.synthetic import holdout_split, make_interactions
from irspack_amd.utils import dense_slim_weight

pytestmark = pytest.mark.gpu

_ML100K = {}


def ml100k(ratings=False):
    """the matrices of test_gpu_slim.ml100k: binary, or with 1..5 ratings from the same seeded generator"""
    if ratings not in _ML100K:
        X = make_interactions("ml100k").astype(np.float64)
        if ratings:
            X.data = np.random.default_rng(17).integers(1, 6, size=X.nnz).astype(np.float64)
        _ML100K[ratings] = X
    return _ML100K[ratings]


def scale_of(dropout_p):
    return np.float32(dropout_p / (1 - dropout_p))  # edlae.py:55-56 on a float32 diagonal


# (name, reg, dropout_p): the defaults and the corners of the reference's default_tune_range
CASES = [("ease", 1.0, None), ("ease", 100.0, None), ("ease", 1e4, None),
         ("edlae", 1.0, 0.1), ("edlae", 1.0, 0.99), ("edlae", 1e4, 0.0)]


# ------------------------------------------------------------------ 1. parity at the ML-100K shape
@pytest.mark.parametrize("ratings", [False, True])
@pytest.mark.parametrize("model, reg, dropout_p", CASES)
def test_matches_float64_restatement_at_ml100k(model, reg, dropout_p, ratings):
    X = ml100k(ratings)
    ds = np.float32(0.0) if dropout_p is None else scale_of(dropout_p)
    W = dense_slim_weight(X, reg, ds)
    n = X.shape[1]
    assert W.dtype == np.float32 and W.shape == (n, n) and W.flags.c_contiguous
    assert np.isfinite(W).all() and (np.diag(W) == 0).all()
    W64 = ease_weights(X, reg, ds, np.float64)
    W32 = ease_weights(X, reg, ds, np.float32)
    gpu, f32 = worst_column_error(W, W64), worst_column_error(W32, W64)
    P64 = regularised_gram(X, np.float32(reg), ds, np.float64)
    r_gpu, r_f32 = optimality_residual(P64, W), optimality_residual(P64, W32)
    record_parity("test_matches_float64_restatement_at_ml100k",
                  f"{model} reg={reg} dropout_p={dropout_p} ratings={ratings}", n_cols=n, gpu_worst_col_err=gpu,
                  f32_restatement_worst_col_err=f32, bar=4.0 * f32, gpu_optimality_residual=r_gpu,
                  f32_restatement_optimality_residual=r_f32)
    assert gpu <= 4.0 * f32, (gpu, f32)
    assert r_gpu <= 4.0 * r_f32, (r_gpu, r_f32)


# ------------------------------------------------------------------ 2. exact properties
def test_two_calls_give_identical_bytes_and_edlae_zero_dropout_is_ease():
    X = ml100k(True)
    A = dense_slim_weight(X, 100.0)
    B = dense_slim_weight(X, 100.0)
    assert A.tobytes() == B.tobytes() and A.any()
    assert dense_slim_weight(X, 100.0, scale_of(0.0)).tobytes() == A.tobytes()
    E1 = dense_slim_weight(X, 1.0, scale_of(0.1))
    assert E1.tobytes() == dense_slim_weight(X, 1.0, scale_of(0.1)).tobytes()
    assert E1.tobytes() != dense_slim_weight(X, 1.0).tobytes()


# ------------------------------------------------------------------ 3. shapes that cross the tile logic
@pytest.mark.parametrize("n_items", [1, 63, 64, 65, 129, 1000])
def test_tile_boundaries(n_items):
    rng = np.random.default_rng(100 + n_items)
    n_users = max(40, n_items // 2)
    X = sps.csr_matrix((rng.random((n_users, n_items)) < 0.08) * rng.integers(1, 6, size=(n_users, n_items)),
                       dtype=np.float64)
    stats = {}
    W = dense_slim_weight(X, 10.0, stats=stats)
    assert stats["n_pad"] == -(-n_items // 64) * 64
    assert W.shape == (n_items, n_items) and W.dtype == np.float32 and (np.diag(W) == 0).all()
    W64, W32 = ease_weights(X, 10.0, 0.0, np.float64), ease_weights(X, 10.0, 0.0, np.float32)
    gpu, f32 = worst_column_error(W, W64), worst_column_error(W32, W64)
    record_parity("test_tile_boundaries", f"n_items={n_items}", gpu_worst_col_err=gpu,
                  f32_restatement_worst_col_err=f32, bar=4.0 * f32)
    assert gpu <= 4.0 * f32, (gpu, f32)


def test_untouched_item_empty_user_and_empty_matrix():
    """an item without interactions: at reg > 0 its row and column of W are exactly zero; a user without
    interactions changes nothing; an empty matrix gives W = 0"""
    X = make_interactions("tiny").astype(np.float64)[:, :157].tolil()
    X[:, 40] = 0
    X[7, :] = 0
    X = X.tocsr()
    W = dense_slim_weight(X, 10.0)
    assert not W[40, :].any() and not W[:, 40].any() and W.any()
    W64, W32 = ease_weights(X, 10.0, 0.0, np.float64), ease_weights(X, 10.0, 0.0, np.float32)
    gpu, f32 = worst_column_error(W, W64), worst_column_error(W32, W64)
    record_parity("test_untouched_item_empty_user_and_empty_matrix", "tiny[:, :157]", gpu_worst_col_err=gpu,
                  f32_restatement_worst_col_err=f32, bar=4.0 * f32)
    assert gpu <= 4.0 * f32, (gpu, f32)
    keep = np.setdiff1d(np.arange(X.shape[0]), [7])
    assert dense_slim_weight(X[keep], 10.0).tobytes() == W.tobytes()
    E = dense_slim_weight(sps.csr_matrix((4, 6)), 1.0)
    assert E.shape == (6, 6) and not E.any()


# ------------------------------------------------------------------ 4. errors
def test_singular_system_is_a_linalg_error_and_leaves_the_output_alone():
    X = make_interactions("tiny").astype(np.float32)[:, :157].tolil()
    X[:, 40] = 0
    X = sps.csr_matrix(X.tocsr())
    X.eliminate_zeros()
    with pytest.raises(np.linalg.LinAlgError, match="not positive definite") as info:
        dense_slim_weight(X, 0.0)
    assert "column 40" in str(info.value)
    assert issubclass(np.linalg.LinAlgError, ValueError)
    # the bare call: status 2, the caller's array untouched
    lib = _lib.lib()
    indptr, indices = X.indptr.astype(np.int64), X.indices.astype(np.int32)
    data = X.data.astype(np.float32)
    W = np.full((157, 157), 7.0, dtype=np.float32)
    st = lib.irs_dense_slim_fit(X.shape[0], 157, _lib.ptr(indptr, C.c_int64), _lib.ptr(indices, C.c_int32),
                                _lib.ptr(data, C.c_float), 0.0, 0.0, 0, _lib.ptr(W, C.c_float), None)
    assert st == 2 and "not positive definite" in lib.irs_last_error().decode()
    assert (W == 7.0).all()


def test_edlae_dropout_one_and_duplicates_through_the_bare_abi():
    from irspack_amd.recommenders import EDLAERecommender

    with pytest.raises(ZeroDivisionError):
        EDLAERecommender(ml100k(False), dropout_p=1.0).learn()
    lib = _lib.lib()
    data = np.ones(4, dtype=np.float32)

    def call(indptr, indices):
        indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int32)
        W = np.zeros((3, 3), dtype=np.float32)
        return lib.irs_dense_slim_fit(len(indptr) - 1, 3, _lib.ptr(indptr, C.c_int64), _lib.ptr(indices, C.c_int32),
                                      _lib.ptr(data, C.c_float), 1.0, 0.0, 0, _lib.ptr(W, C.c_float), None)

    assert call([0, 2, 4], [0, 1, 1, 2]) == 0
    assert call([0, 2, 4], [1, 1, 1, 2]) == 1
    assert "duplicate" in lib.irs_last_error().decode()
    # the Python wrapper sums duplicates before the call
    dup = sps.csr_matrix((np.ones(4), np.array([1, 1, 0, 2]), np.array([0, 2, 4])), shape=(2, 3))
    assert dense_slim_weight(dup, 1.0).tobytes() == dense_slim_weight(sps.csr_matrix(dup.toarray()), 1.0).tobytes()


# ------------------------------------------------------------------ 5. the recommenders end to end
@pytest.mark.parametrize("model", ["ease", "edlae"])
def test_recommender_end_to_end(model):
    from irspack_amd.evaluation import Evaluator
    from irspack_amd.recommenders import DenseSLIMRecommender, EDLAERecommender

    X_train, X_test = holdout_split(ml100k(False))
    if model == "ease":
        rec, reg, ds = DenseSLIMRecommender(X_train).learn(), 1, np.float32(0.0)
    else:
        rec, reg, ds = EDLAERecommender(X_train).learn(), 1.0, scale_of(0.1)
    n = X_train.shape[1]
    W = rec.W
    assert isinstance(W, np.ndarray) and W.dtype == np.float32 and W.shape == (n, n) and W.flags.c_contiguous
    W64, W32 = ease_weights(X_train, reg, ds, np.float64), ease_weights(X_train, reg, ds, np.float32)
    S64, S32 = np.asarray(X_train @ W64), np.asarray(X_train @ W32.astype(np.float64))
    users = np.array([0, 5, 17, 299, X_train.shape[0] - 1])

    def score_error(S, rows):  # worst user row, relative to that row of the float64 scores
        num, den = np.linalg.norm(S - S64[rows], axis=1), np.linalg.norm(S64[rows], axis=1)
        return float((num / np.maximum(den, 1e-300)).max())

    all_rows = np.arange(X_train.shape[0])
    bar = 4.0 * score_error(S32, all_rows)
    got = rec.get_score(users)
    block = rec.get_score_block(10, 200)
    assert np.isfinite(got).all() and np.isfinite(block).all()
    e_users, e_block = score_error(got, users), score_error(block, np.arange(10, 200))
    seen = rec.get_score_remove_seen(users)
    mask = np.asarray(X_train[users].todense()) != 0
    assert np.isneginf(seen[mask]).all() and np.isfinite(seen[~mask]).all()
    np.testing.assert_array_equal(seen[~mask], got[~mask])
    assert e_users <= bar and e_block <= bar, (e_users, e_block, bar)

    ev = Evaluator(X_test, cutoff=20, masked_interactions=X_train)
    res = ev.get_score(rec)  # a dense W: the block loop over get_score_block
    ndcg_gpu, valid = res["ndcg"], res["valid_user"]
    ndcg_64 = ev.get_scores_from_score_matrix(S64, [20])["ndcg@20"]
    ndcg_32 = ev.get_scores_from_score_matrix(S32, [20])["ndcg@20"]
    record_parity("test_recommender_end_to_end", model, score_err_users=e_users, score_err_block=e_block,
                  score_bar=bar, ndcg_gpu=ndcg_gpu, ndcg_f64=ndcg_64, ndcg_f32=ndcg_32, valid_user=valid)
    assert ndcg_gpu > 0 and valid > 0
    assert abs(ndcg_gpu - ndcg_64) <= 4.0 * abs(ndcg_32 - ndcg_64) + 1.0 / valid

    again = pickle.loads(pickle.dumps(rec))
    assert again.W.tobytes() == W.tobytes()
    np.testing.assert_array_equal(again.get_score(users), got)


# ------------------------------------------------------------------ 6. many tiles
def test_eight_thousand_items_sampled_columns():
    """ML-20M restricted to its 8,000 most popular items, reg = 100: 125 x 125 tiles.  16 columns against
    float64 ``solve`` of those columns only (column j of W is -B[:, j] / B[j, j] with P B[:, j] = e_j); the
    bar from the float32 restatement on the host."""
    t0 = time.perf_counter()
    X = make_interactions("ml20m")
    pop = np.asarray((X != 0).sum(axis=0)).ravel()
    top = np.sort(np.argsort(-pop, kind="stable")[:8000])
    X = sps.csr_matrix(X[:, top], dtype=np.float64)
    t1 = time.perf_counter()
    stats = {}
    W = dense_slim_weight(X, 100.0, stats=stats)
    t2 = time.perf_counter()
    n = X.shape[1]
    assert W.shape == (n, n) and np.isfinite(W).all() and (np.diag(W) == 0).all()
    cols = np.sort(np.random.default_rng(3).choice(n, size=16, replace=False))
    cols[0], cols[-1] = 0, n - 1  # the first and the last tile
    P64 = regularised_gram(X, 100.0, 0.0, np.float64)
    E = np.zeros((n, 16))
    E[cols, np.arange(16)] = 1.0
    Bc = np.linalg.solve(P64, E)
    W64c = -Bc / Bc[cols, np.arange(16)][np.newaxis, :]
    W64c[cols, np.arange(16)] = 0.0
    W32c = weights_from_inverse(scipy.linalg.inv(regularised_gram(X, 100.0, 0.0, np.float32)))[:, cols]
    gpu, f32 = worst_column_error(W[:, cols], W64c), worst_column_error(W32c, W64c)
    record_parity("test_eight_thousand_items_sampled_columns", "ml20m top 8000, reg=100", n_cols=16,
                  gpu_worst_col_err=gpu, f32_restatement_worst_col_err=f32, bar=4.0 * f32,
                  generate_s=t1 - t0, fit_wall_s=t2 - t1, test_wall_s=time.perf_counter() - t0, **stats)
    assert gpu <= 4.0 * f32, (gpu, f32)
