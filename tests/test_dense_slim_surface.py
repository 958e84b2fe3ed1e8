"""EASE / EDLAE without a GPU: the Python surface is the reference's (``recommenders/dense_slim.py:34-37``,
``recommenders/edlae.py:41-47``), the C ABI declares and exports ``irs_dense_slim_fit``, its matrix checks
come before any device work, and the float64 numpy restatement that arbitrates the GPU tests satisfies
EASE's optimality conditions."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import scipy.sparse as sps

from _dense_slim_restatement import ease_weights, optimality_residual, regularised_gram

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _positional(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()
            if p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]


def test_recommenders_have_the_reference_signature():
    from irspack_amd import recommenders
    from irspack_amd.recommenders import BaseSimilarityRecommender, DenseSLIMRecommender, EDLAERecommender

    empty = inspect.Parameter.empty
    assert "DenseSLIMRecommender" in recommenders.__all__ and "EDLAERecommender" in recommenders.__all__
    assert issubclass(DenseSLIMRecommender, BaseSimilarityRecommender)
    assert issubclass(EDLAERecommender, BaseSimilarityRecommender)
    assert _positional(DenseSLIMRecommender.__init__) == [("self", empty), ("X_train_all", empty), ("reg", 1)]
    assert _positional(EDLAERecommender.__init__) == [("self", empty), ("X_train_all", empty), ("reg", 1.0),
                                                      ("dropout_p", 0.1)]
    X = sps.csr_matrix(np.eye(3))
    ease, edlae = DenseSLIMRecommender(X), EDLAERecommender(X)
    assert ease.reg == 1 and (edlae.reg, edlae.dropout_p) == (1.0, 0.1)
    for rec in (ease, edlae):
        with pytest.raises(RuntimeError):
            rec.W  # noqa: B018 (fetched before fit)


def test_dense_slim_weight_signature():
    from irspack_amd import utils

    empty = inspect.Parameter.empty
    sig = inspect.signature(utils.dense_slim_weight)
    assert _positional(utils.dense_slim_weight) == [("X", empty), ("reg", empty), ("diag_scale", 0.0)]
    assert [p.name for p in sig.parameters.values() if p.kind is inspect.Parameter.KEYWORD_ONLY] == \
        ["device", "stats"]


def test_symbol_declared_and_exported():
    from irspack_amd import _lib

    header = open(os.path.join(ROOT, "include", "irspack_amd.h")).read()
    declared = set(re.findall(r"\b(irs_[a-z0-9_]+)\s*\(", header))
    s = "irs_dense_slim_fit"
    assert s in declared and s in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), s)
    assert _lib.lib().irs_abi_version() == 4  # an additive change


def test_c_abi_checks_come_before_device_work():
    """The matrix validation of the bare C call (the cases of test_slim_c_abi_checks_come_before_device_work)
    is status 1 (invalid argument), raised before the device is touched: a status 2 where no device is
    visible would mean the device was asked first.  The output array stays as it was."""
    from irspack_amd import _lib

    lib = _lib.lib()
    indptr = np.array([0, 2, 3], dtype=np.int64)
    indices = np.array([0, 2, 1], dtype=np.int32)
    data = np.ones(3, dtype=np.float32)

    def call(indptr=indptr, indices=indices, cols=3):
        W = np.full((cols, cols), 7.0, dtype=np.float32)
        st = lib.irs_dense_slim_fit(len(indptr) - 1, cols, _lib.ptr(indptr, C.c_int64), _lib.ptr(indices, C.c_int32),
                                    _lib.ptr(data, C.c_float), 1.0, 0.0, 0, _lib.ptr(W, C.c_float), None)
        assert (W == 7.0).all()
        return st, lib.irs_last_error().decode()

    assert call(indptr=np.array([0, 3, 2], dtype=np.int64)) == (1, "malformed indptr.")
    assert call(indptr=np.array([1, 2, 3], dtype=np.int64))[0] == 1
    assert call(cols=2) == (1, "column index out of range.")
    assert call(indices=np.array([0, -1, 1], dtype=np.int32)) == (1, "column index out of range.")
    st, msg = call(indices=np.array([2, 2, 1], dtype=np.int32))
    assert st == 1 and "duplicate column index" in msg
    st, msg = call(indices=np.array([2, 0, 1], dtype=np.int32))
    assert st == 1 and "sorted" in msg


def test_empty_matrix_needs_no_device():
    """nnz == 0: P = reg I, every off-diagonal weight is 0 - answered on the host; reg = 0 is singular"""
    from irspack_amd.utils import dense_slim_weight

    stats = {}
    W = dense_slim_weight(sps.csr_matrix((4, 6)), 2.0, stats=stats)
    assert W.shape == (6, 6) and W.dtype == np.float32 and W.flags.c_contiguous and not W.any()
    assert stats["n_pad"] == 64
    assert dense_slim_weight(sps.csr_matrix((3, 0)), 1.0).shape == (0, 0)
    with pytest.raises(np.linalg.LinAlgError, match="not positive definite"):
        dense_slim_weight(sps.csr_matrix((4, 6)), 0.0)


def test_edlae_dropout_one_divides_by_zero():
    from irspack_amd.recommenders import EDLAERecommender

    with pytest.raises(ZeroDivisionError):
        EDLAERecommender(sps.csr_matrix(np.eye(3)), dropout_p=1.0).learn()


@pytest.mark.parametrize("reg, diag_scale", [(1.0, 0.0), (10.0, 0.0), (1.0, 1.0 / 9.0)])
def test_float64_restatement_satisfies_the_optimality_conditions(reg, diag_scale):
    """diag(W) == 0 and (P W)_ij == P_ij for i != j, to 1e-12 of max|P| (measured 1.5e-16 .. 3.3e-16)"""
    rng = np.random.default_rng(5)
    X = (rng.random((60, 37)) < 0.25) * rng.integers(1, 6, size=(60, 37))
    W = ease_weights(X, reg, diag_scale, np.float64)
    P = regularised_gram(X, reg, diag_scale, np.float64)
    assert W.dtype == np.float64 and W.shape == (37, 37)
    assert (np.diag(W) == 0).all()
    res = optimality_residual(P, W)
    print("optimality residual", reg, diag_scale, res)
    assert res <= 1e-12
    assert ease_weights(X, reg, diag_scale, np.float32).dtype == np.float32
