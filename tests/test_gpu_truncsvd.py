"""GPU tests of the randomized truncated SVD (``irs_truncsvd_*``: ``utils.truncated_svd``,
``TruncatedSVDRecommender``).

The arbiter is the float64 restatement of scikit-learn's randomized ``TruncatedSVD``
(``tests/_truncsvd_restatement.py``, pinned to scikit-learn by ``test_truncsvd_surface.py``), ``R64``.  The bar of
a case is measured, not fixed: the same restatement in float32, ``R32``, is the reference's own arithmetic on
float32 input, and the GPU may be at most 4 x as far from ``R64`` as ``R32`` is.  Where ``R32`` happens to be
nearly exact the bar has a floor of 4 x 2^-24 x the largest magnitude of the compared array (one float32 rounding
of the output, times the same factor); where ``R32`` is far off it is capped at 1e-4 of that magnitude.  Compared: the score matrix ``z @ components_`` (max abs difference) and
the singular values (max difference over ``sigma_1``).  Single components are not compared vector by vector:
neighbouring singular values of these matrices are as close as 6e-6 of ``sigma_1``."""
import pickle
import time

import numpy as np
import pytest
import scipy.sparse as sps

from _truncsvd_restatement import randomized_truncated_svd, score_error, sigma_error
from conftest import random_csr, record_parity
from irspack_amd.synthetic import holdout_split, make_interactions
from irspack_amd.utils import truncated_svd

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
_CACHE = {}


def ml100k(kind="binary"):
    if kind not in _CACHE:
        X = sps.csr_matrix(make_interactions("ml100k"), dtype=np.float64)
        if kind == "ratings":
            X.data = np.random.default_rng(17).integers(1, 6, size=X.nnz).astype(np.float64)
        if kind == "transposed":
            X = X.T.tocsr()
        _CACHE[kind] = X
    return _CACHE[kind]


def check_outputs(X, k, z, s, c):
    assert z.shape == (X.shape[0], k) and s.shape == (k,) and c.shape == (k, X.shape[1])
    for a in (z, s, c):
        assert a.dtype == np.float32 and a.flags.c_contiguous and np.isfinite(a).all()
    assert (np.diff(s) <= 0).all()
    live = s > 0
    # the entry of largest magnitude of every component is positive
    top = c[np.arange(k), np.abs(c).argmax(axis=1)]
    assert (top[live] > 0).all() and not c[~live].any() and not z[:, ~live].any()
    return live


def compare(test, config, X, k, seed=0, full_rank=True, uncapped=False, **kw):
    """``uncapped``: the case is there for its measured bar, so ``R32`` taking the 1e-4 cap fails it (a
    precondition on the CPU side: change the case, not the bar)"""
    z, s, c = truncated_svd(X, k, seed, **kw)
    live = check_outputs(X, k, z, s, c)
    z64, s64, c64 = randomized_truncated_svd(X, k, seed, np.float64, **kw)
    z32, s32, c32 = randomized_truncated_svd(X, k, seed, np.float32, **kw)
    e_gpu, top = score_error(z, c, z64, c64)
    e_r32, _ = score_error(z32, c32, z64, c64)
    g_gpu, g_r32 = sigma_error(s, s64), sigma_error(s32, s64)
    # (the cap: where the reference does not normalise, n_iter <= 2, R32 is 1e-2 away and its bar alone
    # would ask nothing; 1e-4 relative is this project's tolerance on scores everywhere else)
    bar, sbar = max(min(4.0 * e_r32, 1e-4 * top), 4.0 * EPS * top), max(min(4.0 * g_r32, 1e-4), 4.0 * EPS)
    ortho = float(np.abs(c[live].astype(np.float64) @ c[live].astype(np.float64).T - np.eye(int(live.sum()))).max())
    record_parity(test, config, n_live=int(live.sum()), score_err_gpu=e_gpu, score_err_r32=e_r32, score_bar=bar,
                  score_ratio=e_gpu / max(e_r32, 1e-300), score_max=top, sigma_err_gpu=g_gpu, sigma_err_r32=g_r32,
                  sigma_bar=sbar, sigma_ratio=g_gpu / max(g_r32, 1e-300), ortho=ortho)
    if uncapped:
        assert 4.0 * e_r32 <= 1e-4 * top and 4.0 * g_r32 <= 1e-4, (e_r32, top, g_r32)
    assert e_gpu <= bar, (e_gpu, e_r32, bar)
    assert g_gpu <= sbar, (g_gpu, g_r32, sbar)
    assert ortho <= 1e-5, ortho
    if full_rank:
        assert live.all()
    return z, s, c


# ------------------------------------------------------------------ 1. parity at the ML-100K shape
@pytest.mark.parametrize("seed", [0, 7])
@pytest.mark.parametrize("k", [4, 64, 128, 512])
def test_matches_float64_restatement_at_ml100k(k, seed):
    compare("test_matches_float64_restatement_at_ml100k", f"k={k} seed={seed}", ml100k(), k, seed)


def test_transposed_shape():
    compare("test_transposed_shape", "1682 x 943, k=64", ml100k("transposed"), 64)


def test_float_valued_matrix():
    compare("test_float_valued_matrix", "ratings 1..5, k=64", ml100k("ratings"), 64)


@pytest.mark.parametrize("n_iter", [0, 2])
def test_fewer_power_iterations(n_iter):
    compare("test_fewer_power_iterations", f"n_iter={n_iter} k=64", ml100k(), 64, n_iter=n_iter)


def test_no_oversampling():
    compare("test_no_oversampling", "n_oversamples=0 k=64", ml100k(), 64, n_oversamples=0)


def wide_matrix():
    if "wide" not in _CACHE:
        _CACHE["wide"] = random_csr(700, 600, 0.1, 2)
    return _CACHE["wide"]


@pytest.mark.parametrize("k", [300, 500])
def test_two_chunk_sketch_width(k):
    """l = k + 10 = 310 and 510, l_pad = 320 and 512: a lane of the sparse product holds two float4 of a row, the
    second one masked past lane 15 at 320 and on every lane at 512 (ML-100K at k = 256 would reach 320 too, but
    there R32 itself is 2.3e-4 from R64 and the bar would be the cap)"""
    compare("test_two_chunk_sketch_width", f"700 x 600 k={k}", wide_matrix(), k, uncapped=True)


@pytest.mark.parametrize("shape", [(20000, 64), (64, 20000)])
def test_tall_block_at_k4(shape):
    """20,000 rows at l_pad = 64: the Gram pass over that side has 313 chunks of 64 rows for 256 slabs at most,
    so 157 slabs of two chunks - the second pass of the kernel's row loop - of which the last has one chunk, and
    that chunk 32 rows.  The transpose puts the 20,000 rows on the other side's Gram and apply"""
    X = random_csr(shape[0], shape[1], 0.05, 4)
    compare("test_tall_block_at_k4", f"{shape[0]} x {shape[1]} k=4", X, 4)


# ------------------------------------------------------------------ 2. rank deficiency
def test_x_small_with_defaults(X_small):
    """4 x 5 with an empty row, rank 3, n_components = 4: the fourth component is a zero row"""
    z, s, c = compare("test_rank_deficiency", "X_small k=4", X_small, 4, full_rank=False)
    assert (s > 0).sum() == 3


def test_tripled_columns():
    rng = np.random.default_rng(11)
    B = (rng.random((300, 20)) < 0.3) * rng.integers(1, 6, size=(300, 20))
    X = sps.csr_matrix(np.hstack([B, B, B]), dtype=np.float64)
    z, s, c = compare("test_rank_deficiency", "300 x 60 of rank 20, k=30", X, 30, full_rank=False)
    assert (s > 0).sum() == 20


def test_zero_matrix_and_sketch_wider_than_the_matrix():
    z, s, c = truncated_svd(sps.csr_matrix((30, 12)), 5)
    assert not z.any() and not s.any() and not c.any()
    explicit = sps.csr_matrix((np.zeros(3), np.array([0, 1, 2]), np.array([0, 3] + [3] * 29)), shape=(30, 12))
    assert not truncated_svd(explicit, 5)[2].any()
    rng = np.random.default_rng(5)
    X = sps.csr_matrix((rng.random((9, 7)) < 0.5) * rng.integers(1, 6, size=(9, 7)), dtype=np.float64)
    compare("test_rank_deficiency", "9 x 7, k=6: l=16 clipped to 7", X, 6, full_rank=False)


# ------------------------------------------------------------------ 3. determinism
def test_two_calls_give_identical_bytes():
    X = ml100k("ratings")
    a, b = truncated_svd(X, 64, 3), truncated_svd(X, 64, 3)
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes() and u.any()
    assert a[0].tobytes() != truncated_svd(X, 64, 4)[0].tobytes()


# ------------------------------------------------------------------ 4. the recommender end to end
def test_recommender_end_to_end():
    from irspack_amd.evaluation import Evaluator
    from irspack_amd.recommenders import BaseRecommender, TruncatedSVDRecommender

    X_train, X_test = holdout_split(ml100k())
    rec = TruncatedSVDRecommender(X_train, n_components=32, random_seed=1).learn()
    z, c = rec.z, rec.decomposer.components_
    assert z.shape == (X_train.shape[0], 32) and c.shape == (32, X_train.shape[1])
    assert rec.decomposer.singular_values_.shape == (32,)
    zd, sd, cd = truncated_svd(X_train, 32, 1)
    assert z.tobytes() == zd.tobytes() and c.tobytes() == cd.tobytes()
    S = z @ c
    users = np.array([0, 5, 17, 299, X_train.shape[0] - 1])
    np.testing.assert_array_equal(rec.get_score(users), z[users] @ c)
    np.testing.assert_array_equal(rec.get_score_block(10, 200), z[10:200] @ c)
    np.testing.assert_array_equal(rec.get_user_embedding(), z)
    np.testing.assert_array_equal(rec.get_item_embedding(), c.T)
    np.testing.assert_array_equal(rec.get_score_from_user_embedding(z[users]), z[users] @ c)
    np.testing.assert_array_equal(rec.get_score_from_item_embedding(users, c.T), z[users] @ c)
    cold = rec.get_score_cold_user(X_train[users])
    np.testing.assert_array_equal(cold, np.asarray(X_train[users] @ c.T) @ c)
    np.testing.assert_allclose(cold, S[users], rtol=0, atol=1e-4 * np.abs(S).max())
    np.testing.assert_array_equal(rec.decomposer.transform(X_train[users]), np.asarray(X_train[users] @ c.T))
    seen = rec.get_score_remove_seen(users)
    mask = np.asarray(X_train[users].todense()) != 0
    assert np.isneginf(seen[mask]).all() and np.isfinite(seen[~mask]).all()

    class Fixed(BaseRecommender):
        def get_score_block(self, begin, end):
            return S[begin:end]

        def get_score(self, user_indices):
            return S[user_indices]

    ev = Evaluator(X_test, cutoff=20, masked_interactions=X_train)
    got, want = ev.get_score(rec), ev.get_score(Fixed(X_train))
    assert got == want and got["ndcg"] > 0 and got["valid_user"] > 0
    record_parity("test_recommender_end_to_end", "k=32", ndcg=got["ndcg"], valid_user=got["valid_user"])

    again = pickle.loads(pickle.dumps(rec))
    assert again.z.tobytes() == z.tobytes()
    np.testing.assert_array_equal(again.get_score(users), rec.get_score(users))


# ------------------------------------------------------------------ 5. the ML-20M shape
def test_ml20m_shape_k64():
    t0 = time.perf_counter()
    X = make_interactions("ml20m")
    t1 = time.perf_counter()
    stats = {}
    z, s, c = truncated_svd(X, 64, 0, stats=stats)
    t2 = time.perf_counter()
    live = check_outputs(X, 64, z, s, c)
    assert live.all()
    c64 = c.astype(np.float64)
    ortho = float(np.abs(c64 @ c64.T - np.eye(64)).max())
    record_parity("test_ml20m_shape_k64", f"{X.shape[0]} x {X.shape[1]}, nnz={X.nnz}", ortho=ortho,
                  sigma_1=float(s[0]), sigma_k=float(s[-1]), generate_s=t1 - t0, fit_wall_s=t2 - t1, **stats)
    assert ortho <= 1e-5, ortho
