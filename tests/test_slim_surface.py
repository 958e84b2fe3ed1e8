"""SLIM without a GPU: the Python surface is the reference's (``_util_cpp.pyi:31-48``,
``recommenders/slim.py:59-78``), the C ABI declares and exports the calls, the argument checks of
``util.hpp:233-236`` come before any device work, and the chunked numpy restatement that arbitrates the
GPU tests is the plain loop bit for bit (also at the chunk widths of the wide workgroups), and embedding a
matrix into a wider catalogue of items without interactions changes nothing (the lemma
``tests/test_gpu_slim_wide.py`` rests on)."""
import inspect
import os
import re

import numpy as np
import pytest
import scipy.sparse as sps

from _slim_restatement import gram, slim_column, slim_column_plain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLIM_SYMBOLS = ["irs_slim_fit", "irs_slim_nnz", "irs_slim_fetch", "irs_slim_last_stats", "irs_slim_last_launch",
                "irs_slim_destroy"]


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


@pytest.mark.parametrize("positive_only", [True, False])
@pytest.mark.parametrize("l2, l1, n_iter, tol", [(5.0, 0.5, 4, 0.0), (0.0, 0.0, 3, 0.0), (2.0, 1.0, 6, 1e-3)])
def test_chunked_restatement_is_the_plain_loop_at_the_wide_chunks(positive_only, l2, l1, n_iter, tol):
    """The chunk widths of the device's three workgroup sizes (and 64, one wave) on a problem of several
    chunks of each: 1,340 coordinates, so the last chunk is partial at every width; target columns at the
    seams of the 512- and 1024-wide chunks, at both ends and on the item without interactions.
    ``dense_fraction = 2.0``: never the plain sweep inside ``slim_column``."""
    rng = np.random.default_rng(7)
    X = (rng.random((300, 1340)) < 0.04) * rng.integers(1, 6, size=(300, 1340))
    X[:, 777] = 0  # an item without interactions: G_ff + l2 == 0 when l2 == 0
    G = gram(X)
    for j in (0, 511, 512, 777, 1023, 1024, 1339):
        a = slim_column_plain(G, j, l2, l1, n_iter, tol, positive_only)
        for chunk in (64, 256, 512, 1024):
            b = slim_column(G, j, l2, l1, n_iter, tol, positive_only, chunk=chunk, dense_fraction=2.0)
            assert a.tobytes() == b.tobytes(), (j, chunk)
        assert np.isfinite(a).all() and a[j] == 0 and a[777] == 0
        assert a.any() or j == 777, j


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("positive_only", [True, False])
@pytest.mark.parametrize("l2, l1", [(5.0, 0.5), (5.0, 0.0), (0.0, 0.5), (0.0, 0.0)])
def test_embedding_into_a_wider_catalogue_changes_nothing(dtype, positive_only, l2, l1):
    """Embedding lemma (tests/test_gpu_slim_wide.py rests on it): a matrix embedded into a wider one whose
    extra items have no interactions - every touched column keeps its coefficients bit for bit at the
    touched coordinates, every other coefficient is zero, a column of an extra item is all zero.  An extra
    coordinate f has G[f, :] = 0: its candidate is (-0 -+ l1) / (0 + l2), never > 0 as plus and never < 0 as
    minus (0 / 0 and -l1 / 0 fail both tests), so it never changes and never enters the running product; the
    touched coordinates then see the operations of the small problem in the same order.  400 touched of
    1,500 items, 3 sweeps (unconverged)."""
    n_small, n_big, n_iter = 400, 1500, 3
    rng = np.random.default_rng(11)
    small = (rng.random((200, n_small)) < 0.06) * rng.integers(1, 6, size=(200, n_small))
    assert (small != 0).sum(axis=0).min() > 0
    touched = np.sort(rng.choice(n_big, size=n_small, replace=False))
    extra = np.setdiff1d(np.arange(n_big), touched)
    big = np.zeros((200, n_big), dtype=small.dtype)
    big[:, touched] = small
    G_small, G_big = gram(small, dtype), gram(big, dtype)
    assert G_big.dtype == dtype and not G_big[extra].any() and not G_big[:, extra].any()
    for c in (0, 1, 199, 398, 399):
        w_small = slim_column(G_small, c, l2, l1, n_iter, 0.0, positive_only)
        w_big = slim_column(G_big, int(touched[c]), l2, l1, n_iter, 0.0, positive_only, chunk=1024)
        assert w_small.dtype == dtype and w_small.any()
        assert w_big[touched].tobytes() == w_small.tobytes(), c
        assert not w_big[extra].any(), c
    for j in (int(extra[0]), int(extra[-1])):
        assert not slim_column(G_big, j, l2, l1, n_iter, 0.0, positive_only, chunk=1024).any(), j
