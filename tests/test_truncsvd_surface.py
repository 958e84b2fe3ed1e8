"""TruncatedSVDRecommender without a GPU: the Python surface is the reference's
(``recommenders/truncsvd.py:48-77``), the C ABI declares and exports ``irs_truncsvd_*``, its argument checks
come before any device work, and the numpy / scipy restatement that arbitrates the GPU tests reproduces
scikit-learn's randomized ``TruncatedSVD``."""
import ctypes as C
import inspect
import os
import re
import warnings

import numpy as np
import pytest
import scipy.sparse as sps

from _truncsvd_restatement import randomized_truncated_svd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["irs_truncsvd_create", "irs_truncsvd_range", "irs_truncsvd_apply", "irs_truncsvd_project",
           "irs_truncsvd_finish", "irs_truncsvd_stats", "irs_truncsvd_destroy"]


def _positional(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()
            if p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]


def test_recommender_has_the_reference_surface(X_small):
    from irspack_amd import recommenders
    from irspack_amd.recommenders import BaseRecommender, TruncatedSVDRecommender

    empty = inspect.Parameter.empty
    assert "TruncatedSVDRecommender" in recommenders.__all__
    assert issubclass(TruncatedSVDRecommender, BaseRecommender)
    assert _positional(TruncatedSVDRecommender.__init__) == [("self", empty), ("X_train_all", empty),
                                                             ("n_components", 4), ("random_seed", 0)]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        rec = TruncatedSVDRecommender(X_small)
    assert (rec.n_components, rec.random_seed) == (4, 0)
    with pytest.raises(RuntimeError, match="^z fetched before fit$"):
        rec.z  # noqa: B018
    with pytest.raises(RuntimeError, match=r"^decomposer fetched before fit\.$"):
        rec.decomposer  # noqa: B018
    for k in (5, 9):
        with pytest.warns(UserWarning, match=r"n_components >= than X_train_all.shape\[1\]. Set it to "
                                             r"X_train_all.shape\[1\] - 1."):
            assert TruncatedSVDRecommender(X_small, n_components=k).n_components == 4
    with pytest.raises(AssertionError):
        TruncatedSVDRecommender(sps.csr_matrix(np.ones((3, 1))))
    for name in ("get_score", "get_score_block", "get_score_cold_user", "get_user_embedding",
                 "get_score_from_user_embedding", "get_item_embedding", "get_score_from_item_embedding"):
        assert name in vars(TruncatedSVDRecommender), name


def test_truncated_svd_signature_and_zero_matrix():
    from irspack_amd import utils

    empty = inspect.Parameter.empty
    sig = inspect.signature(utils.truncated_svd)
    assert _positional(utils.truncated_svd) == [("X", empty), ("n_components", empty), ("random_seed", 0)]
    assert [(p.name, p.default) for p in sig.parameters.values() if p.kind is inspect.Parameter.KEYWORD_ONLY] == \
        [("n_iter", 5), ("n_oversamples", 10), ("device", None), ("stats", None)]
    # an all-zero matrix is answered on the host: every output zero, no error
    z, s, c = utils.truncated_svd(sps.csr_matrix((7, 5)), 3)
    assert (z.shape, s.shape, c.shape) == ((7, 3), (3,), (3, 5))
    for a in (z, s, c):
        assert a.dtype == np.float32 and a.flags.c_contiguous and not a.any()
    with pytest.raises(ValueError):
        utils.truncated_svd(sps.csr_matrix((7, 5)), 6)


def test_symbols_declared_listed_and_exported():
    from irspack_amd import _lib

    header = open(os.path.join(ROOT, "include", "irspack_amd.h")).read()
    declared = set(re.findall(r"\b(irs_[a-z0-9_]+)\s*\(", header))
    for s in SYMBOLS:
        assert s in declared and s in _lib.EXPORTED_SYMBOLS and s in _lib.ARGTYPES and hasattr(_lib.lib(), s), s
    assert _lib.lib().irs_abi_version() == 4  # an additive change
    assert C.sizeof(_lib.TruncSvdStatsStruct) == 72


def test_c_abi_checks_come_before_device_work():
    """Status 1 (invalid argument) from every check, where no device is visible too: a status 2 there would
    mean the device was asked first."""
    from irspack_amd import _lib

    lib = _lib.lib()
    indptr = np.array([0, 2, 3, 3], dtype=np.int64)
    indices = np.array([0, 2, 1], dtype=np.int32)
    data = np.ones(3, dtype=np.float32)
    f = lambda a: _lib.ptr(a, C.c_float)  # noqa: E731

    def create(indptr=indptr, indices=indices, data=data, cols=4):
        h = C.c_void_p()
        st = lib.irs_truncsvd_create(len(indptr) - 1, cols, _lib.ptr(indptr, C.c_int64), _lib.ptr(indices, C.c_int32),
                                     f(data), 0, C.byref(h))
        msg = lib.irs_last_error().decode()
        if st != 0:
            assert not h.value
        return st, msg, h

    assert create(indptr=np.array([0, 3, 2, 3], dtype=np.int64))[:2] == (1, "malformed indptr.")
    assert create(cols=2)[:2] == (1, "column index out of range.")
    assert create(indices=np.array([0, -1, 1], dtype=np.int32))[:2] == (1, "column index out of range.")
    st, msg, _ = create(indices=np.array([2, 2, 1], dtype=np.int32))
    assert st == 1 and "duplicate column index" in msg
    st, msg, _ = create(indices=np.array([2, 0, 1], dtype=np.int32))
    assert st == 1 and "sorted" in msg
    for bad in (np.nan, np.inf):
        st, msg, _ = create(data=np.array([1.0, bad, 1.0], dtype=np.float32))
        assert st == 1 and "non-finite" in msg

    st, _, h = create()  # 3 users x 4 items: sklearn works on X^T, the test matrix has n_users = 3 rows
    assert st == 0 and h.value
    try:
        G = np.zeros((4, 4), dtype=np.float32)
        om = np.ones((4, 4), dtype=np.float32)
        assert lib.irs_truncsvd_range(h, f(om), 3, 0, 5, f(G)) == 1  # l < 1
        assert lib.irs_truncsvd_range(h, f(om), 4, 2, 5, f(G)) == 1  # rows: n_items, the wrong side
        assert "rows" in lib.irs_last_error().decode()
        assert lib.irs_truncsvd_range(h, f(om), 3, 4, 5, f(G)) == 1  # l > min(n_users, n_items)
        assert lib.irs_truncsvd_range(h, f(om), 3, 2, -1, f(G)) == 1
        z, c = np.zeros((3, 4), dtype=np.float32), np.zeros((4, 4), dtype=np.float32)
        assert lib.irs_truncsvd_finish(h, f(om), 2, f(z), f(c)) == 1  # k > l2 (no basis yet)
        assert "k > l2" in lib.irs_last_error().decode()
        assert lib.irs_truncsvd_apply(h, f(om), 1, f(G)) == 1
        assert lib.irs_truncsvd_project(h, f(G)) == 1
        assert not G.any() and not z.any() and not c.any()
    finally:
        assert lib.irs_truncsvd_destroy(h) == 0


def _ml100k():
    from irspack_amd.synthetic import make_interactions

    return sps.csr_matrix(make_interactions("ml100k"), dtype=np.float64)


@pytest.mark.parametrize("case", ["k4", "k64", "transposed", "X_small"])
def test_float64_restatement_is_sklearn(case, X_small):
    """z, components_ and singular_values_ of the restatement against scikit-learn's, to 1e-10 of the largest
    magnitude (bit for bit with scikit-learn 1.7.2; the slack is for another LAPACK build)."""
    sklearn_decomposition = pytest.importorskip("sklearn.decomposition")
    X, k, seed = {"k4": (_ml100k, 4, 0), "k64": (_ml100k, 64, 3), "transposed": (lambda: _ml100k().T.tocsr(), 64, 0),
                  "X_small": (lambda: X_small, 4, 0)}[case]
    X = X()
    if case != "X_small":
        assert X.shape == ((943, 1682) if case != "transposed" else (1682, 943))
    svd = sklearn_decomposition.TruncatedSVD(n_components=k, random_state=seed)
    z_ref = svd.fit_transform(X)
    z, s, comps = randomized_truncated_svd(X, k, seed, np.float64)
    for got, ref in ((z, z_ref), (comps, svd.components_), (s, svd.singular_values_)):
        assert got.shape == ref.shape and got.dtype == np.float64
        diff = float(np.abs(got - ref).max())
        print(case, got.shape, "max abs diff", diff, "of", float(np.abs(ref).max()))
        assert diff <= 1e-10 * np.abs(ref).max()
    assert randomized_truncated_svd(X, k, seed, np.float32)[0].dtype == np.float32
