"""NMFRecommender without a GPU: the Python surface is the reference's (``recommenders/nmf.py:32-72``), the C ABI
declares and exports ``irs_nmf_fit``, its argument checks come before any device work, and the numpy restatement
that arbitrates the GPU tests (``tests/_nmf_restatement.py``) and the NNDSVD host function reproduce
scikit-learn."""
import ctypes as C
import inspect
import os
import re
import warnings

import numpy as np
import pytest
import scipy.sparse as sps

from _nmf_restatement import nmf_cd, nmf_transform, random_init
from irspack_amd.utils import nmf_fit, nndsvd_init  # (the parent commit fails here)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = inspect.Parameter.empty


def _params(fn, kind):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values() if p.kind is kind]


def test_recommender_has_the_reference_surface(X_small):
    from irspack_amd import recommenders
    from irspack_amd.recommenders import BaseRecommender, NMFRecommender

    assert "NMFRecommender" in recommenders.__all__
    assert issubclass(NMFRecommender, BaseRecommender)
    assert _params(NMFRecommender.__init__, inspect.Parameter.POSITIONAL_OR_KEYWORD) == [
        ("self", EMPTY), ("X_train_all", EMPTY), ("n_components", 64), ("alpha", 1e-2), ("l1_ratio", 1e-2),
        ("beta_loss", "frobenius"), ("init", None)]
    rec = NMFRecommender(X_small)
    assert (rec.n_components, rec.alpha, rec.l1_ratio, rec.beta_loss, rec.init) == (64, 1e-2, 1e-2, "frobenius", None)
    for name in ("get_score", "get_score_cold_user", "_learn"):
        assert name in vars(NMFRecommender), name
    # what sklearn's "cd" solver refuses, at learn() and before any device work
    with pytest.raises(ValueError, match="beta_loss"):
        NMFRecommender(X_small, n_components=2, beta_loss="kullback-leibler").learn()
    with pytest.raises(ValueError, match="init"):
        NMFRecommender(X_small, n_components=2, init="nndsvdb").learn()


def test_utils_signatures_and_host_answers(X_small):
    from irspack_amd import utils

    P, K = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY
    assert _params(utils.nmf_fit, P) == [("X", EMPTY), ("n_components", EMPTY), ("alpha", 0.0), ("l1_ratio", 0.0)]
    assert _params(utils.nmf_fit, K) == [("init", None), ("random_state", 42), ("tol", 1e-4), ("max_iter", 200),
                                         ("W0", None), ("H0", None), ("device", None), ("stats", None)]
    assert _params(utils.nmf_transform, P) == [("X", EMPTY), ("H", EMPTY), ("alpha", 0.0), ("l1_ratio", 0.0)]
    assert _params(utils.nmf_transform, K)[:2] == [("tol", 1e-4), ("max_iter", 200)]
    assert issubclass(utils.ConvergenceWarning, UserWarning) and utils.ConvergenceWarning.__name__ == "ConvergenceWarning"
    # an all-zero matrix is answered on the host as scikit-learn answers it: zero factors after one iteration
    for k in (2, 7):
        W, H, n_iter = nmf_fit(sps.csr_matrix((6, 5)), k)
        assert (W.shape, H.shape, n_iter) == ((6, k), (k, 5), 1)
        for a in (W, H):
            assert a.dtype == np.float32 and a.flags.c_contiguous and not a.any()
    with pytest.raises(ValueError, match="both or neither"):
        nmf_fit(X_small, 2, W0=np.ones((4, 2)))
    with pytest.raises(ValueError, match="Negative values"):
        nmf_fit(-X_small, 2)
    with pytest.raises(ValueError, match="n_components <= min"):
        nmf_fit(X_small, 5, init="nndsvd")
    with pytest.raises(ValueError, match="Invalid init"):
        nmf_fit(X_small, 2, init="custom")
    src = open(os.path.join(ROOT, "irspack_amd", "utils", "__init__.py")).read()
    assert not re.search(r"^\s*(import|from)\s+sklearn", src, re.M)  # the library does not import scikit-learn


def test_zero_matrix_is_sklearns_answer():
    sklearn_decomposition = pytest.importorskip("sklearn.decomposition")
    for k in (2, 7):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m = sklearn_decomposition.NMF(k, random_state=42)
            W = m.fit_transform(sps.csr_matrix((6, 5)))
        assert not W.any() and not m.components_.any() and m.n_iter_ == 1


def test_symbols_declared_listed_and_exported():
    from irspack_amd import _lib

    header = open(os.path.join(ROOT, "include", "irspack_amd.h")).read()
    declared = set(re.findall(r"\b(irs_[a-z0-9_]+)\s*\(", header))
    s = "irs_nmf_fit"
    assert s in declared and s in _lib.EXPORTED_SYMBOLS and s in _lib.ARGTYPES and hasattr(_lib.lib(), s)
    assert _lib.lib().irs_abi_version() == 4  # an additive change
    assert C.sizeof(_lib.NmfStatsStruct) == 40


def test_c_abi_checks_come_before_device_work():
    """Status 1 (invalid argument) with its message from every check, where no device is visible too (a status 2
    there would mean the device was asked first), and the outputs untouched."""
    from irspack_amd import _lib

    lib = _lib.lib()
    base = dict(indptr=np.array([0, 2, 3, 3], dtype=np.int64), indices=np.array([0, 2, 1], dtype=np.int32),
                data=np.ones(3, dtype=np.float32), cols=4, k=2, W=None, H=None, regs=(0.0, 0.0, 0.0, 0.0), tol=1e-4,
                max_iter=5)

    def call(**kw):
        a = dict(base, **kw)
        rows, k = len(a["indptr"]) - 1, a["k"]
        W = np.full((rows, max(k, 1)), 0.5, dtype=np.float32) if a["W"] is None else a["W"]
        H = np.full((max(k, 1), a["cols"]), 0.25, dtype=np.float32) if a["H"] is None else a["H"]
        W_in, H_in = W.copy(), H.copy()
        n_iter = C.c_int64(-7)
        viol = np.full(8, -1.0)
        st = lib.irs_nmf_fit(rows, a["cols"], _lib.ptr(a["indptr"], C.c_int64), _lib.ptr(a["indices"], C.c_int32),
                             _lib.ptr(a["data"], C.c_float), k, _lib.ptr(W, C.c_float), _lib.ptr(H, C.c_float),
                             *a["regs"], a["tol"], a["max_iter"], 1, 0, C.byref(n_iter), _lib.ptr(viol, C.c_double),
                             None)
        assert W.tobytes() == W_in.tobytes() and H.tobytes() == H_in.tobytes()
        assert n_iter.value == -7 and (viol == -1.0).all()
        return st, lib.irs_last_error().decode()

    # the shared cases in the words of irs_truncsvd_create
    assert call(indptr=np.array([0, 3, 2, 3], dtype=np.int64)) == (1, "malformed indptr.")
    assert call(cols=2) == (1, "column index out of range.")
    assert call(indices=np.array([0, -1, 1], dtype=np.int32)) == (1, "column index out of range.")
    st, msg = call(indices=np.array([2, 2, 1], dtype=np.int32))
    assert st == 1 and "duplicate column index" in msg
    st, msg = call(indices=np.array([2, 0, 1], dtype=np.int32))
    assert st == 1 and "sorted" in msg
    for bad in (np.nan, np.inf):
        st, msg = call(data=np.array([1.0, bad, 1.0], dtype=np.float32))
        assert st == 1 and "non-finite" in msg
    assert call(data=np.array([1.0, -1.0, 1.0], dtype=np.float32)) == (1, "the matrix holds a negative value.")
    assert call(k=0) == (1, "k must be >= 1.")
    assert call(max_iter=0) == (1, "max_iter must be >= 1.")
    assert call(tol=-1e-3) == (1, "tol must be >= 0.")
    for i in range(4):
        regs = [0.0] * 4
        regs[i] = -1.0
        assert call(regs=tuple(regs)) == (1, "the regularisers must be finite and >= 0.")
    for bad in (np.nan, np.inf, -0.5):
        W = np.full((3, 2), 0.5, dtype=np.float32)
        W[1, 1] = bad
        assert call(W=W) == (1, "the initial W must be finite and non-negative.")
        H = np.full((2, 4), 0.5, dtype=np.float32)
        H[0, 3] = bad
        assert call(H=H) == (1, "the initial H must be finite and non-negative.")


def _ml100k():
    from irspack_amd.synthetic import make_interactions

    return sps.csr_matrix(make_interactions("ml100k"), dtype=np.float64)


def _close(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == np.float64
    diff, top = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    print(what, got.shape, "max abs diff", diff, "of", top)
    assert diff <= 1e-10 * top, (what, diff, top)


def _sklearn_fit(X, k, alpha, l1_ratio, max_iter, init=None, tol=0.0):
    from sklearn.decomposition import NMF

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = NMF(k, init=init, l1_ratio=l1_ratio, alpha_W=alpha, random_state=42, tol=tol, max_iter=max_iter)
        W = m.fit_transform(X)
    return m, W


@pytest.mark.parametrize("max_iter", [3, 10])
@pytest.mark.parametrize("alpha,l1_ratio", [(1e-2, 1e-2), (1e-6, 0.5)])
@pytest.mark.parametrize("k", [8, 64])
def test_float64_restatement_is_sklearn_at_ml100k(k, alpha, l1_ratio, max_iter):
    """W, H and n_iter_ of the restatement against scikit-learn's, to 1e-10 of the largest magnitude"""
    pytest.importorskip("sklearn.decomposition")
    from sklearn.decomposition._nmf import _initialize_nmf

    X = _ml100k()
    assert X.shape == (943, 1682)
    m, W_ref = _sklearn_fit(X, k, alpha, l1_ratio, max_iter)
    W0, H0 = _initialize_nmf(X, k, None, random_state=42)
    W, H, n_iter, history = nmf_cd(X, W0, H0, alpha, l1_ratio, 0.0, max_iter)
    _close(W, W_ref, "W")
    _close(H, m.components_, "H")
    assert n_iter == m.n_iter_ == max_iter and history.shape == (max_iter,)


def test_float64_restatement_is_sklearn_on_small_cases(X_small):
    pytest.importorskip("sklearn.decomposition")
    from sklearn.decomposition._nmf import _initialize_nmf

    # X_small with the defaults, running to sklearn's own stop
    m, W_ref = _sklearn_fit(X_small, 2, 1e-2, 1e-2, 200, tol=1e-4)
    W0, H0 = _initialize_nmf(X_small, 2, None, random_state=42)
    W, H, n_iter, _ = nmf_cd(X_small, W0, H0, 1e-2, 1e-2, 1e-4, 200)
    _close(W, W_ref, "X_small W")
    _close(H, m.components_, "X_small H")
    assert n_iter == m.n_iter_
    # the random init, k > min(shape): init=None falls to it
    rng = np.random.default_rng(3)
    X = sps.csr_matrix((rng.random((30, 12)) < 0.3) * rng.integers(1, 6, size=(30, 12)), dtype=np.float64)
    m, W_ref = _sklearn_fit(X, 15, 1e-3, 0.3, 7)
    W0, H0 = random_init(X, 15)
    Wi, Hi = _initialize_nmf(X, 15, None, random_state=42)
    _close(W0, Wi, "random W0")
    _close(H0, Hi, "random H0")
    W, H, n_iter, _ = nmf_cd(X, W0, H0, 1e-3, 0.3, 0.0, 7)
    _close(W, W_ref, "random W")
    _close(H, m.components_, "random H")
    assert n_iter == m.n_iter_
    # transform on other rows
    Xc = sps.csr_matrix((rng.random((9, 12)) < 0.3) * rng.integers(1, 6, size=(9, 12)), dtype=np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        T_ref = m.transform(Xc)
    T, _, _ = nmf_transform(Xc, m.components_, 1e-3, 0.3, 0.0, 7)
    _close(T, T_ref, "transform")


@pytest.mark.parametrize("variant", ["nndsvd", "nndsvda", "nndsvdar"])
def test_nndsvd_host_function_is_sklearns(variant):
    """fed scikit-learn's own ``_randomized_svd`` output, against ``_initialize_nmf``, to 1e-12"""
    pytest.importorskip("sklearn.decomposition")
    from sklearn.decomposition._nmf import _initialize_nmf
    from sklearn.utils.extmath import _randomized_svd

    for X, k in ((_ml100k(), 16), (_ml100k()[:200, :90], 40)):
        U, S, Vt = _randomized_svd(X, k, random_state=42)
        W0, H0 = nndsvd_init(U, S, Vt, X.mean(), variant, np.random.RandomState(42))
        W_ref, H_ref = _initialize_nmf(X, k, variant, random_state=42)
        for got, ref in ((W0, W_ref), (H0, H_ref)):
            assert got.shape == ref.shape and (got >= 0).all()
            assert float(np.abs(got - ref).max()) <= 1e-12 * float(np.abs(ref).max())
        # the sign of a singular pair does not matter
        flip = np.where(np.arange(k) % 2 == 0, -1.0, 1.0)
        W1, H1 = nndsvd_init(U * flip, S, Vt * flip[:, None], X.mean(), variant, np.random.RandomState(42))
        assert W1.tobytes() == W0.tobytes() and H1.tobytes() == H0.tobytes()
    # a zero singular triplet gives a zero column and row (nndsvd), not 0 / 0
    U, S, Vt = np.zeros((5, 2)), np.array([2.0, 0.0]), np.zeros((2, 4))
    U[:, 0], Vt[0] = 0.5, 0.5
    W0, H0 = nndsvd_init(U, S, Vt, 0.1, "nndsvd")
    assert np.isfinite(W0).all() and not W0[:, 1].any() and not H0[1].any()
