"""SLIM without a GPU: the Python surface is the reference's (``_util_cpp.pyi:31-48``,
``recommenders/slim.py:59-78``), the C ABI declares and exports the calls, the argument checks of
``util.hpp:233-236`` come before any device work, and the chunked numpy restatement that arbitrates the
GPU tests is the plain loop bit for bit."""
import inspect
import os
import re

import numpy as np
import pytest
import scipy.sparse as sps

from _slim_restatement import gram, slim_column, slim_column_plain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLIM_SYMBOLS = ["irs_slim_fit", "irs_slim_nnz", "irs_slim_fetch", "irs_slim_last_stats", "irs_slim_destroy"]


def _positional(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()
            if p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]


def test_slim_functions_have_the_reference_signature():
    from irspack_amd import utils

    empty = inspect.Parameter.empty
    want = [("X", empty), ("n_threads", empty), ("n_iter", empty), ("l2_coeff", empty), ("l1_coeff", empty),
            ("tol", empty), ("top_k", -1)]
    for name in ("slim_weight_allow_negative", "slim_weight_positive_only"):
        assert _positional(getattr(utils, name)) == want, name


def test_slim_recommender_has_the_reference_signature():
    from irspack_amd import recommenders
    from irspack_amd.recommenders import BaseSimilarityRecommender, SLIMRecommender

    assert "SLIMRecommender" in recommenders.__all__
    assert issubclass(SLIMRecommender, BaseSimilarityRecommender)
    empty = inspect.Parameter.empty
    assert _positional(SLIMRecommender.__init__) == [
        ("self", empty), ("X_train_all", empty), ("alpha", 0.05), ("l1_ratio", 0.01), ("positive_only", True),
        ("n_iter", 100), ("tol", 1e-4), ("top_k", None), ("n_threads", None)]
    rec = SLIMRecommender(sps.csr_matrix(np.eye(3)), n_threads=2)
    assert (rec.alpha, rec.l1_ratio, rec.positive_only, rec.n_iter, rec.tol, rec.top_k, rec.n_threads) == \
        (0.05, 0.01, True, 100, 1e-4, None, 2)
    with pytest.raises(RuntimeError):
        rec.W  # noqa: B018 (fetched before fit)


def test_slim_symbols_declared_and_exported():
    from irspack_amd import _lib

    header = open(os.path.join(ROOT, "include", "irspack_amd.h")).read()
    declared = set(re.findall(r"\b(irs_[a-z0-9_]+)\s*\(", header))
    lib = _lib.lib()
    for s in SLIM_SYMBOLS:
        assert s in declared and s in _lib.EXPORTED_SYMBOLS and hasattr(lib, s), s


@pytest.mark.parametrize("positive_only", [True, False])
@pytest.mark.parametrize("bad, message", [
    (dict(n_threads=0), "n_threads must be > 0."),
    (dict(n_iter=0), "n_iter must be > 0."),
    (dict(l2_coeff=-1.0), "l2_coeff must be > 0."),
    (dict(l1_coeff=-1.0), "l1_coeff must be > 0."),
])
def test_slim_argument_checks_come_before_device_work(positive_only, bad, message):
    """util.hpp:233-236, with the reference's wording; ValueError also where no device is visible (a
    RuntimeError there would mean the device was asked first)."""
    from irspack_amd import utils

    fit = utils.slim_weight_positive_only if positive_only else utils.slim_weight_allow_negative
    kw = dict(n_threads=1, n_iter=1, l2_coeff=0.0, l1_coeff=0.0, tol=0.0)
    kw.update(bad)
    with pytest.raises(ValueError, match=re.escape(message)):
        fit(sps.csr_matrix(np.eye(4, 5)), **kw)


def test_slim_c_abi_checks_come_before_device_work():
    """The bare C call: its three argument checks and the matrix validation are statuses (1 = invalid
    argument) raised before the device is touched."""
    import ctypes as C

    from irspack_amd import _lib

    lib = _lib.lib()
    indptr = np.array([0, 2, 3], dtype=np.int64)
    indices = np.array([0, 2, 1], dtype=np.int32)
    data = np.ones(3, dtype=np.float32)

    def call(indptr=indptr, indices=indices, n_iter=1, l2=0.0, l1=0.0, cols=3):
        h = C.c_void_p()
        st = lib.irs_slim_fit(len(indptr) - 1, cols, _lib.ptr(indptr, C.c_int64), _lib.ptr(indices, C.c_int32),
                              _lib.ptr(data, C.c_float), 1, n_iter, l2, l1, 0.0, -1, 0, C.byref(h))
        assert h.value is None
        return st, lib.irs_last_error().decode()

    assert call(n_iter=0) == (1, "n_iter must be > 0.")
    assert call(l2=-1.0) == (1, "l2_coeff must be > 0.")
    assert call(l1=-1.0) == (1, "l1_coeff must be > 0.")
    assert call(indptr=np.array([0, 3, 2], dtype=np.int64)) == (1, "malformed indptr.")
    assert call(indptr=np.array([1, 2, 3], dtype=np.int64))[0] == 1
    assert call(cols=2) == (1, "column index out of range.")
    assert call(indices=np.array([0, -1, 1], dtype=np.int32)) == (1, "column index out of range.")
    st, msg = call(indices=np.array([2, 2, 1], dtype=np.int32))
    assert st == 1 and "duplicate column index" in msg
    st, msg = call(indices=np.array([2, 0, 1], dtype=np.int32))
    assert st == 1 and "sorted" in msg


@pytest.mark.parametrize("positive_only", [True, False])
@pytest.mark.parametrize("l2, l1, n_iter, tol", [(0.5, 0.3, 30, 0.0), (0.0, 0.0, 5, 0.0), (2.0, 1.0, 50, 1e-3)])
def test_chunked_restatement_is_the_plain_loop(positive_only, l2, l1, n_iter, tol):
    rng = np.random.default_rng(5)
    X = (rng.random((60, 37)) < 0.25) * rng.integers(1, 6, size=(60, 37))
    X[:, 11] = 0  # an item without interactions: G_ff + l2 == 0 when l2 == 0
    G = gram(X)
    for j in range(G.shape[0]):
        a = slim_column_plain(G, j, l2, l1, n_iter, tol, positive_only)
        for chunk, dense_fraction in ((8, 2.0), (256, 2.0), (16, 0.1)):  # 2.0: never the plain sweep
            b = slim_column(G, j, l2, l1, n_iter, tol, positive_only, chunk=chunk, dense_fraction=dense_fraction)
            assert a.tobytes() == b.tobytes(), (j, chunk)
        assert np.isfinite(a).all() and a[j] == 0 and a[11] == 0
