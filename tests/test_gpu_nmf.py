"""GPU tests of the coordinate-descent NMF (``irs_nmf_fit``: ``utils.nmf_fit``, ``utils.nmf_transform``,
``NMFRecommender``).

The arbiter is the float64 restatement of scikit-learn's ``cd`` solver (``tests/_nmf_restatement.py``, pinned to
scikit-learn by ``test_nmf_surface.py``), ``R64``.  Unless a test says otherwise the GPU, ``R64`` and the same
restatement in float32, ``R32``, start from the same float32 ``W0 / H0`` (scikit-learn's ``_initialize_nmf`` where
scikit-learn is there, else the restatement's ``random`` init) and run ``max_iter`` iterations with ``tol = 0``.
The bar of a case is measured, not fixed: the GPU may be at most 4 x as far from ``R64`` as ``R32`` is, with a
floor of 4 x 2^-24 x the largest magnitude of the compared array and a cap of 1e-4 of it (a case that takes the
cap says so in its parity line).  Compared: ``W @ H``, ``W`` and ``H``, max abs difference each, and the violation
sum of every iteration, relative to ``R64``'s (``violation_bars``).

The probes of section 8 need no bar: with one non-zero per column of ``H`` and small integers in ``X`` every
sum of one transform step is exact in float32, and the GPU is compared for equality."""
import contextlib
import pickle
import time
import warnings

import numpy as np
import pytest
import scipy.sparse as sps

from _nmf_restatement import factor_errors, frobenius_objective, nmf_cd, random_init
from _nmf_restatement import nmf_transform as restated_transform
from _truncsvd_restatement import randomized_truncated_svd
from conftest import random_csr, record_parity
from irspack_amd.synthetic import holdout_split, make_interactions
from irspack_amd.utils import ConvergenceWarning, nmf_fit, nmf_transform, nndsvd_init

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def ml100k():
    return cached("ml100k", lambda: sps.csr_matrix(make_interactions("ml100k"), dtype=np.float64))


def base_matrix():
    """300 x 200 with an empty row and an empty column"""
    def make():
        X = random_csr(300, 200, 0.05, 1, empty_rows=(3,)).tolil()
        X[:, 7] = 0  # (an empty column whether or not the draw left one)
        X = sps.csr_matrix(X.tocsr(), dtype=np.float32)
        X.eliminate_zeros()
        assert X[3].nnz == 0 and X[:, 7].nnz == 0
        return X
    return cached("base", make)


def start(X, k, init=None):
    """the shared float32 start: scikit-learn's own initialisation where it is installed"""
    X64 = sps.csr_matrix(X, dtype=np.float64)
    try:
        from sklearn.decomposition._nmf import _initialize_nmf
        W0, H0 = _initialize_nmf(X64, k, init, random_state=42)
    except ImportError:
        W0, H0 = random_init(X64, k)
    return np.ascontiguousarray(W0, dtype=np.float32), np.ascontiguousarray(H0, dtype=np.float32)


def bar_of(e_r32, top):
    return max(min(4.0 * e_r32, 1e-4 * top), 4.0 * EPS * top), bool(4.0 * e_r32 > 1e-4 * top)


def check_factors(X, k, W, H):
    assert W.shape == (X.shape[0], k) and H.shape == (k, X.shape[1])
    for a in (W, H):
        assert a.dtype == np.float32 and a.flags.c_contiguous and np.isfinite(a).all() and (a >= 0).all()


def one_blas_thread():
    """The restatement sweeps one coordinate at a time, a matrix-vector product each (3,120 of them on 3,000 x 520
    at k = 520): a threaded BLAS spends several times the product itself on handing it out.  Where threadpoolctl
    is installed the restatement runs on one thread, which is also the order of sums closest to the Cython loop;
    BLAS does not thread the products of the smaller cases, whose references are the same bytes either way."""
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:
        return contextlib.nullcontext()
    return threadpool_limits(limits=1, user_api="blas")


def violation_bars(h32, h64):
    """per iteration: 4 x the relative distance of ``R32``'s violation sum from ``R64``'s, with a floor of
    16 x 2^-24 (``R32`` is sometimes exact by accident; the sum is one-signed over k-term float32 dot products,
    hence 16 where the factors have 4) and the 1e-4 cap"""
    return np.maximum(np.minimum(4.0 * np.abs(h32 / h64 - 1.0), 1e-4), 16.0 * EPS)


def compare(test, config, X, k, alpha=1e-2, l1_ratio=1e-2, max_iter=3, init=None, uncapped=False):
    """``uncapped``: the case is there for its measured bar, so ``R32`` taking the 1e-4 cap on any compared array
    fails it (a precondition on the CPU side: change the matrix, not the bar)"""
    W0, H0 = start(X, k, init)
    stats = {}
    W, H, n_iter = nmf_fit(X, k, alpha, l1_ratio, tol=0.0, max_iter=max_iter, W0=W0, H0=H0, stats=stats)
    check_factors(X, k, W, H)
    assert n_iter == max_iter and stats["violations"].shape == (max_iter,)
    with one_blas_thread():
        W64, H64, _, h64 = nmf_cd(X, W0, H0, alpha, l1_ratio, 0.0, max_iter, np.float64)
        W32, H32, _, h32 = nmf_cd(X, W0, H0, alpha, l1_ratio, 0.0, max_iter, np.float32)
    fields, failures, cap_taken = {}, [], []
    for name, (e_gpu, top), (e_r32, _) in zip(("WH", "W", "H"), factor_errors(W, H, W64, H64),
                                              factor_errors(W32, H32, W64, H64)):
        bar, capped = bar_of(e_r32, top)
        fields.update({f"{name}_err_gpu": e_gpu, f"{name}_err_r32": e_r32, f"{name}_bar": bar, f"{name}_max": top,
                       f"{name}_bar_is_the_1e-4_cap": capped})
        if capped:
            cap_taken.append((name, e_r32, top))
        if not e_gpu <= bar:
            failures.append((name, e_gpu, e_r32, bar))
    fields.update(violation_rel_err=None, violation_rel_err_r32=None, violation_bar=None)
    if (h64 > 0).all():  # (else there is no relative distance: recorded as null, not asserted)
        v_gpu, v_r32, v_bar = np.abs(stats["violations"] / h64 - 1.0), np.abs(h32 / h64 - 1.0), violation_bars(h32, h64)
        fields.update(violation_rel_err=float(v_gpu.max()), violation_rel_err_r32=float(v_r32.max()),
                      violation_bar=float(v_bar.min()), violation_rel_err_by_iteration=[float(v) for v in v_gpu],
                      violation_rel_err_r32_by_iteration=[float(v) for v in v_r32],
                      violation_bar_by_iteration=[float(v) for v in v_bar])
        for it in np.flatnonzero(~(v_gpu <= v_bar)):
            failures.append((f"violation of iteration {it + 1}", float(v_gpu[it]), float(v_r32[it]), float(v_bar[it])))
    record_parity(test, config, **fields)
    if uncapped:
        assert not cap_taken, cap_taken
    assert not failures, failures
    return W, H


# ------------------------------------------------------------------ 1. parity on the smallest shapes that can break
@pytest.mark.parametrize("k", [1, 3, 8, 17, 64, 65, 130])
def test_matches_float64_restatement_at_every_width(k):
    """widths round every padding and block boundary; rows that do not fill a workgroup, an empty row and column"""
    compare("test_matches_float64_restatement_at_every_width", f"300 x 200 k={k}", base_matrix(), k)


@pytest.mark.parametrize("k", [70, 100])
def test_more_items_than_users(k):
    """70 x 130: k = min(shape) (NNDSVDa) and k > min(shape) (the random init)"""
    X = random_csr(70, 130, 0.1, 2)
    compare("test_more_items_than_users", f"70 x 130 k={k}", X, k)


def test_row_longer_than_a_product_segment():
    """a row of 1,300 entries is cut into two segments of the sparse product (1,024 each at most)"""
    X = random_csr(40, 1500, 0.02, 5).tolil()
    rng = np.random.default_rng(9)
    cols = np.sort(rng.choice(1500, size=1300, replace=False))
    X[0, cols] = rng.uniform(0.5, 3.0, size=1300)
    X = sps.csr_matrix(X.tocsr(), dtype=np.float32)
    assert X[0].nnz > 1024 and X.shape[0] < X.shape[1]
    compare("test_row_longer_than_a_product_segment", "40 x 1500, 1300 in row 0, k=8", X, 8)
    compare("test_row_longer_than_a_product_segment", "its transpose, k=8", sps.csr_matrix(X.T), 8)


@pytest.mark.parametrize("k", [256, 257, 320, 512, 513, 576])
def test_matches_float64_restatement_at_wide_k(k):
    """k_pad = 256 is the widest one-chunk product (every lane on); 320 (k = 257, 320) and 512 are the two-chunk
    one with the second chunk partly masked and full; 576 (k = 513, 576) is the three-chunk one.  257 and 513
    leave k % 16 = k % 4 = 1 to the sweep.  k > min(shape): the random start"""
    compare("test_matches_float64_restatement_at_wide_k", f"300 x 200 k={k}", base_matrix(), k)


@pytest.mark.parametrize("shape", [(20000, 64), (64, 20000)])
def test_tall_block_at_k3(shape):
    """20,000 rows at k_pad = 64: the Gram pass of that side has 313 chunks of 64 rows for 256 slabs at most, so
    157 slabs of two chunks - the second pass of the kernel's row loop - of which the last has one chunk, and
    that chunk 32 rows; its sweep leaves 313 partial violations, more than the 256 threads that add them"""
    X = random_csr(shape[0], shape[1], 0.05, 4)
    compare("test_tall_block_at_k3", f"{shape[0]} x {shape[1]} k=3", X, 3)


def test_gram_slabs_of_two_chunks_with_off_diagonal_tiles():
    """k = 520, k_pad = 576: 45 tiles, so 2048 // 45 = 45 slabs at most for the 47 chunks of 3,000 rows: 24 slabs
    of two chunks, the last with one chunk of 56 rows"""
    X = random_csr(3000, 80, 0.05, 6)
    compare("test_gram_slabs_of_two_chunks_with_off_diagonal_tiles", "3000 x 80 k=520", X, 520, uncapped=True)


def test_split_rows_on_both_sides():
    """two rows and two columns longer than a product segment: X and X^T have two split rows each (the second
    one's partial slots do not start at 0), and one buffer of partial rows serves both products"""
    def make():
        X = random_csr(1500, 1500, 0.01, 7).tolil()
        rng = np.random.default_rng(13)
        for r, n in ((0, 1300), (2, 1100)):
            X[r, np.sort(rng.choice(1500, size=n, replace=False))] = rng.uniform(0.5, 3.0, size=n)
        for c, n in ((1, 1200), (4, 1400)):
            X[np.sort(rng.choice(1500, size=n, replace=False)), c] = rng.uniform(0.5, 3.0, size=n)
        return sps.csr_matrix(X.tocsr(), dtype=np.float32)
    X = cached("split_both", make)
    for M in (X, sps.csr_matrix(X.T)):
        assert (np.diff(M.indptr) > 1024).sum() == 2 and np.diff(M.indptr).max() <= 2048
    compare("test_split_rows_on_both_sides", "1500 x 1500, rows 0, 2 and columns 1, 4 split, k=8", X, 8)


def test_binary_matrix():
    X = random_csr(300, 200, 0.05, 3, binary=True)
    compare("test_binary_matrix", "300 x 200 binary k=17", X, 17)


@pytest.mark.parametrize("alpha,l1_ratio", [(1e-2, 0.0), (1e-2, 1.0), (0.0, 0.5)])
def test_regulariser_corners(alpha, l1_ratio):
    compare("test_regulariser_corners", f"alpha={alpha} l1_ratio={l1_ratio} k=17", base_matrix(), 17, alpha, l1_ratio)


@pytest.mark.parametrize("k,alpha,l1_ratio", [(8, 1e-2, 1e-2), (64, 1e-2, 1e-2), (64, 1e-6, 0.5)])
def test_ml100k_shape_ten_iterations(k, alpha, l1_ratio):
    compare("test_ml100k_shape_ten_iterations", f"k={k} alpha={alpha} l1_ratio={l1_ratio}", ml100k(), k, alpha,
            l1_ratio, max_iter=10)


# ------------------------------------------------------------------ 2. sklearn's exact comparisons
def test_zero_hessian_leaves_the_column_alone():
    """a zero row of H and alpha = 0: HHt[t, t] == 0, so the first sweep must not touch column t of W"""
    X = base_matrix()
    W0, H0 = start(X, 8)
    H0[5] = 0.0
    W, H, n_iter = nmf_fit(X, 8, 0.0, 0.0, tol=0.0, max_iter=1, W0=W0, H0=H0)
    assert n_iter == 1
    assert W[:, 5].tobytes() == W0[:, 5].tobytes() and W[:, 5].any()
    assert W[:, 4].tobytes() != W0[:, 4].tobytes()


def test_stopping_test_is_sklearns():
    X = base_matrix_for_stopping()
    W0, H0 = start(X, 8)
    W64, H64, n64, h64 = nmf_cd(X, W0, H0, 1e-2, 1e-2, 0.1, 200, np.float64)
    ratio = h64 / h64[0]
    # the precondition, on the float64 history alone: the decision is not within rounding of tol
    assert n64 >= 2 and abs(ratio[n64 - 1] - 0.1) > 0.01 and abs(ratio[n64 - 2] - 0.1) > 0.01, ratio
    stats = {}
    with warnings.catch_warnings():
        warnings.simplefilter("error", ConvergenceWarning)  # (stopped before max_iter: no warning)
        W, H, n_iter = nmf_fit(X, 8, 1e-2, 1e-2, tol=0.1, max_iter=200, W0=W0, H0=H0, stats=stats)
    rel = float(np.abs(stats["violations"][:n64] / h64 - 1.0).max()) if n_iter >= n64 else None
    record_parity("test_stopping_test_is_sklearns", "300 x 200 k=8 tol=0.1", n_iter_gpu=n_iter, n_iter_f64=n64,
                  ratios_f64=[float(r) for r in ratio], violation_rel_err=rel)
    assert n_iter == n64 and stats["violations"].shape == (n64,)
    assert rel <= 1e-3


def base_matrix_for_stopping():
    # the issue's matrix as it is drawn (no column zeroed)
    return cached("stopping", lambda: random_csr(300, 200, 0.05, 1, empty_rows=(3,)))


def test_max_iter_warns_in_sklearns_words():
    X = base_matrix()
    with pytest.warns(ConvergenceWarning, match=r"^Maximum number of iterations 2 reached\. Increase it to improve "
                                                r"convergence\.$"):
        nmf_fit(X, 8, 1e-2, 1e-2, init="random", max_iter=2)
    with warnings.catch_warnings():
        warnings.simplefilter("error", ConvergenceWarning)
        nmf_fit(X, 8, 1e-2, 1e-2, init="random", max_iter=2, tol=0.0)


# ------------------------------------------------------------------ 3. transform
def test_transform_of_held_out_rows():
    X = base_matrix()
    train, held = X[:260], X[260:]
    W0, H0 = start(train, 8)
    _, H64, _, _ = nmf_cd(train, W0, H0, 1e-2, 1e-2, 0.0, 5, np.float64)
    H = np.ascontiguousarray(H64, dtype=np.float32)
    T = nmf_transform(held, H, 1e-2, 1e-2, tol=0.0, max_iter=5)
    assert T.shape == (40, 8) and T.dtype == np.float32 and (T >= 0).all() and T.any()
    T64, _, _ = restated_transform(held, H, 1e-2, 1e-2, 0.0, 5, np.float64)
    T32, _, _ = restated_transform(held, H, 1e-2, 1e-2, 0.0, 5, np.float32)
    e_gpu, e_r32, top = float(np.abs(T - T64).max()), float(np.abs(T32 - T64).max()), float(np.abs(T64).max())
    bar, capped = bar_of(e_r32, top)
    record_parity("test_transform_of_held_out_rows", "40 rows k=8", W_err_gpu=e_gpu, W_err_r32=e_r32, W_bar=bar,
                  W_max=top, **{"W_bar_is_the_1e-4_cap": capped})
    assert e_gpu <= bar, (e_gpu, e_r32, bar)


# ------------------------------------------------------------------ 4. determinism
def test_two_calls_give_identical_bytes():
    X = base_matrix()
    runs = []
    for _ in range(2):
        stats = {}
        W, H, _ = nmf_fit(X, 65, 1e-2, 1e-2, tol=0.0, max_iter=4, stats=stats)
        runs.append((W, H, stats["violations"]))
    for u, v in zip(*runs):
        assert u.tobytes() == v.tobytes() and u.any()


# ------------------------------------------------------------------ 5. the default initialisation end to end
def test_default_init_reaches_sklearns_objective():
    """ML-100K shape, k = 16, everything else the defaults: 200 iterations (scikit-learn does not converge there
    either).  The start differs from scikit-learn's by the float32 SVD and NNDSVD cuts at 1e-6, so the factors
    are not compared; the Frobenius objective is, against ``R64`` from scikit-learn's start.  Allowed relative
    gap: 4 x the gap ``R64`` itself shows between two CPU starts - scikit-learn's, and the one built from the
    float32 restatement of the randomized SVD - with a floor of 1e-6."""
    X = ml100k()
    k = 16
    mean = X.mean()

    def cpu_start(dtype):
        z, s, comps = randomized_truncated_svd(X, k, 42, dtype, n_iter=7)  # (k < 0.1 min(shape): 7)
        z, s, comps = z.astype(np.float64), s.astype(np.float64), comps.astype(np.float64)
        W0, H0 = nndsvd_init(z / s, s, comps, mean, "nndsvda")
        return W0.astype(np.float32), H0.astype(np.float32)

    objective = {}
    for name, dtype in (("f64_start", np.float64), ("f32_start", np.float32)):
        W0, H0 = cpu_start(dtype)
        W, H, n, _ = nmf_cd(X, W0, H0, 0.0, 0.0, 1e-4, 200, np.float64)
        assert n == 200
        objective[name] = frobenius_objective(X, W, H)
    with pytest.warns(ConvergenceWarning):
        W, H, n_iter = nmf_fit(X, k)
    check_factors(X, k, W, H)
    assert n_iter == 200
    got = frobenius_objective(X, W, H)
    ref = objective["f64_start"]
    cpu_gap = abs(objective["f32_start"] - ref) / ref
    gap, allowed = abs(got - ref) / ref, max(4.0 * cpu_gap, 1e-6)
    record_parity("test_default_init_reaches_sklearns_objective", "ml100k k=16 200 iterations", objective_gpu=got,
                  objective_f64=ref, objective_f64_from_f32_start=objective["f32_start"], gap_gpu=gap, gap_cpu=cpu_gap,
                  allowed=allowed)
    assert gap <= allowed, (gap, cpu_gap)


# ------------------------------------------------------------------ 6. the recommender end to end
def test_recommender_end_to_end():
    from irspack_amd.evaluation import Evaluator
    from irspack_amd.recommenders import NMFRecommender

    X_train, X_test = holdout_split(ml100k())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", ConvergenceWarning)
        rec = NMFRecommender(X_train, n_components=16).learn()
    W, H = rec.W, rec.H
    check_factors(X_train, 16, W, H)
    model = rec.nmf_model
    assert model.components_ is H and model.n_components_ == 16 and 1 <= model.n_iter_ <= 200
    users = np.array([0, 5, 17, 299, X_train.shape[0] - 1])
    np.testing.assert_array_equal(rec.get_score(users), W[users] @ H)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", ConvergenceWarning)
        cold = rec.get_score_cold_user(X_train[users])
        np.testing.assert_array_equal(model.transform(X_train[users]) @ H, cold)
    assert cold.shape == (5, X_train.shape[1]) and np.isfinite(cold).all() and (cold >= 0).all() and cold.any()
    got = Evaluator(X_test, cutoff=20, masked_interactions=X_train).get_score(rec)
    assert got["ndcg"] > 0 and got["valid_user"] > 0
    record_parity("test_recommender_end_to_end", "nmf k=16", ndcg=got["ndcg"], valid_user=got["valid_user"],
                  n_iter=model.n_iter_)
    again = pickle.loads(pickle.dumps(rec))
    np.testing.assert_array_equal(again.get_score(users), rec.get_score(users))


# ------------------------------------------------------------------ 7. the ML-20M shape
def test_ml20m_shape_k64():
    t0 = time.perf_counter()
    X = make_interactions("ml20m")
    t1 = time.perf_counter()
    stats = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", ConvergenceWarning)
        W, H, n_iter = nmf_fit(X, 64, 1e-2, 1e-2, max_iter=2, stats=stats)
    t2 = time.perf_counter()
    check_factors(X, 64, W, H)
    assert n_iter == 2 and W.any() and H.any()
    violations = stats.pop("violations")
    assert np.isfinite(violations).all()
    record_parity("test_ml20m_shape_k64", f"{X.shape[0]} x {X.shape[1]}, nnz={X.nnz}", generate_s=t1 - t0,
                  fit_wall_s=t2 - t1, violations=[float(v) for v in violations], **stats)


# ------------------------------------------------------------------ 8. exact probes of one transform step
def probe_components(k):
    """``H`` (k x (4 k + 5)) with one non-zero per column: item j < 4 k belongs to component j % k, 1.0 in an even
    component and 2.0 in an odd one; the last five items are zero columns.  ``H H^T`` is diagonal, 4 and 16"""
    n_items = 4 * k + 5
    H = np.zeros((k, n_items), dtype=np.float32)
    j = np.arange(4 * k)
    H[j % k, j] = np.where((j % k) % 2 == 0, 1.0, 2.0)
    return H


def probe_matrix(n_rows, n_items, seed, long_rows=()):
    """5 % dense with integer values 1 .. 5; ``long_rows``: (row, number of entries) to overwrite"""
    rng = np.random.default_rng(seed)
    X = random_csr(n_rows, n_items, 0.05, seed).tolil()
    for r, n in long_rows:
        cols = np.sort(rng.choice(n_items, size=n, replace=False))
        X.rows[r], X.data[r] = cols.tolist(), [1.0] * n
    X = sps.csr_matrix(X.tocsr(), dtype=np.float32)
    X.data = rng.integers(1, 6, size=X.nnz).astype(np.float32)
    return X


def exact_probe(test, config, X, k):
    """One transform step (a product, a Gram pass, a sweep from ``W = 0``) on sums that are exact in float32:
    ``W[i, t] == XH[i, t] / G[t, t]`` and the violation is the sum of ``XH``, as a double, whatever the order"""
    H = probe_components(k)
    X64, H64 = sps.csr_matrix(X, dtype=np.float64), H.astype(np.float64)
    XH, G = np.asarray(X64 @ H64.T), H64 @ H64.T
    diag = np.diag(G)
    want = XH / diag
    # the preconditions of "exact": integer sums a float32 holds, a diagonal G, a division without rounding
    assert XH.max() < 2 ** 24 and (XH == np.rint(XH)).all() and XH.any()
    assert not (G - np.diag(diag)).any() and set(diag) <= {4.0, 16.0}
    assert (want * diag == XH).all() and (want.astype(np.float32) == want).all()
    r64, _, h64 = restated_transform(X, H, 0.0, 0.0, 0.0, 1, np.float64)
    assert np.array_equal(r64, want) and h64[0] == XH.sum()
    stats = {}
    W = nmf_transform(X, H, 0.0, 0.0, tol=0.0, max_iter=1, stats=stats)
    assert W.shape == want.shape and W.dtype == np.float32 and stats["violations"].shape == (1,)
    violation = float(stats["violations"][0])
    exact = bool(np.array_equal(W, want) and (W >= 0).all() and violation == XH.sum())
    record_parity(test, config, exact=exact, XH_max=float(XH.max()), violation=violation,
                  violation_expected=float(XH.sum()), n_mismatches=int((W != want).sum()))
    if not np.array_equal(W, want):
        i, t = (int(v) for v in np.argwhere(W != want)[0])
        print(f"first mismatch at (i, t) = ({i}, {t}): got {W[i, t]!r}, expected {want[i, t]!r}; XH = {XH[i, t]!r}, "
              f"G[t, t] = {diag[t]!r}, entries in row i = {X[i].nnz}")
    assert np.array_equal(W, want)
    assert (W >= 0).all()
    assert violation == XH.sum(), (violation, XH.sum())
    return W


@pytest.mark.parametrize("k", [1, 17, 64, 65, 256, 257, 320, 512, 513, 576])
def test_one_transform_step_is_exact(k):
    """every instantiation of the product (k_pad 64, 128, 256, 320, 512, 576: lanes per row 16, 32, 64 and two
    and three chunks a lane) and a sweep with and without a coordinate tail.  At k = 576 row 0 has 2,100 entries
    (three segments) and row 5 has 1,100 (two segments whose partial slots start at 3)"""
    n_items = 4 * k + 5
    long_rows = ((0, 2100), (5, 1100)) if k == 576 else ()
    X = probe_matrix(70, n_items, 100 + k, long_rows)
    if long_rows:
        assert X[0].nnz == 2100 and X[5].nnz == 1100
    exact_probe("test_one_transform_step_is_exact", f"70 x {n_items} k={k}", X, k)


def test_violation_total_over_313_workgroups_is_exact():
    """20,000 rows: the sweep leaves 313 partial sums for 256 adding threads, so the first 57 threads take a
    second one; the total of integers does not depend on the order"""
    t0 = time.perf_counter()
    X = probe_matrix(20000, 17, 3)
    assert time.perf_counter() - t0 < 1.0
    exact_probe("test_violation_total_over_313_workgroups_is_exact", "20000 x 17 k=3", X, 3)
