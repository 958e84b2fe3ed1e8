"""The evaluator's device paths for SLIM, DenseSLIM / EDLAE, truncated SVD and NMF without a GPU: the two C
entries are declared, listed and exported, ``EvaluatorCore`` has the two methods, and ``Evaluator._device_path``
- the decision ``_evaluate_model`` acts on - names the path for every recommender class and falls back to the
block loop for what the device cannot read as it is.  The models are stubs carrying the fitted attributes: no
fit, no device work."""
import inspect
import os
import re

import numpy as np
import pytest
import scipy.sparse as sps

from irspack_amd.evaluation import Evaluator
from irspack_amd.evaluation._core_evaluator import EvaluatorCore
from irspack_amd.recommenders import (DenseSLIMRecommender, EDLAERecommender, NMFRecommender, SLIMRecommender,
                                      TruncatedSVDRecommender)
from irspack_amd.recommenders.truncsvd import TruncatedSVDDecomposer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = inspect.Parameter.empty
U, I, K = 40, 30, 6


def test_symbols_declared_listed_and_exported():
    from irspack_amd import _lib

    header = open(os.path.join(ROOT, "include", "irspack_amd.h")).read()
    declared = set(re.findall(r"\b(irs_[a-z0-9_]+)\s*\(", header))
    for s in ("irs_eval_get_metrics_dense_similarity", "irs_eval_get_metrics_factors"):
        assert s in declared and s in _lib.EXPORTED_SYMBOLS and s in _lib.ARGTYPES and hasattr(_lib.lib(), s), s
    assert _lib.lib().irs_abi_version() == 4  # an additive change
    # the helper that reaches the MFMA score tiles stays inside the library
    assert not hasattr(_lib.lib(), "irs_gk_scores_device_")


def test_core_methods_have_the_signatures():
    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]

    tail = [("begin", EMPTY), ("end", EMPTY), ("mask", EMPTY), ("mask_begin", EMPTY), ("cutoffs", EMPTY),
            ("offset", EMPTY), ("recall_with_cutoff", False)]
    assert params(EvaluatorCore.get_metrics_dense_similarity) == [("self", EMPTY), ("X", EMPTY), ("W", EMPTY)] + tail
    assert params(EvaluatorCore.get_metrics_factors) == \
        [("self", EMPTY), ("user_factors", EMPTY), ("item_factors", EMPTY)] + tail


@pytest.fixture(scope="module")
def problem():
    rns = np.random.RandomState(0)
    X = sps.csr_matrix((rns.rand(U, I) > 0.8).astype(np.float64))
    gt = sps.csr_matrix((rns.rand(U, I) > 0.9).astype(np.float64))
    return X, gt, rns


def _evaluator(fused=True):
    """an ``Evaluator`` as far as the decision needs it (the constructor puts the ground truth on the device)"""
    ev = Evaluator.__new__(Evaluator)
    ev.fused = fused
    return ev


def _stub(kind, X, rns):
    """a recommender of the class with the attributes a fit leaves (dtypes and layouts of the real fits)"""
    if kind == "slim":
        m = SLIMRecommender(X)
        m._W = sps.random(I, I, density=0.2, format="csc", random_state=rns, dtype=np.float32)
    elif kind in ("dense_slim", "edlae"):
        m = (DenseSLIMRecommender if kind == "dense_slim" else EDLAERecommender)(X)
        m._W = rns.randn(I, I).astype(np.float32)
    elif kind == "truncsvd":
        m = TruncatedSVDRecommender(X, n_components=K)
        m.z_ = rns.randn(U, K).astype(np.float32)
        m.decomposer_ = TruncatedSVDDecomposer(rns.randn(K, I).astype(np.float32), np.ones(K, dtype=np.float32))
    else:
        m = NMFRecommender(X, n_components=K)
        m.W, m.H = rns.rand(U, K).astype(np.float32), rns.rand(K, I).astype(np.float32)
    return m


@pytest.mark.parametrize("kind, path", [("slim", "similarity"), ("dense_slim", "dense_similarity"),
                                        ("edlae", "dense_similarity"), ("truncsvd", "factors"), ("nmf", "factors")])
def test_dispatcher_names_the_path_of_every_recommender(problem, kind, path):
    X, gt, rns = problem
    model = _stub(kind, X, rns)
    assert _evaluator()._device_path(model) == path
    assert _evaluator(fused=False)._device_path(model) == "blocks"
    # a subclass with its own block scores is scored by them
    sub = type("Own" + type(model).__name__, (type(model),), {"get_score_block": lambda self, b, e: None})
    model.__class__ = sub
    assert _evaluator()._device_path(model) == "blocks"


def test_dispatcher_operands(problem):
    X, gt, rns = problem
    ev = _evaluator()
    slim = _stub("slim", X, rns)
    W_before = slim._W.copy()
    profiles, Wr = ev._similarity_weights(slim)
    assert sps.isspmatrix_csr(Wr) and Wr.dtype == np.float64 and Wr.has_sorted_indices
    assert (Wr != slim._W.astype(np.float64).tocsr()).nnz == 0  # the exact cast
    assert slim._W.dtype == np.float32 and sps.isspmatrix_csc(slim._W)  # the model's matrix is as it was
    assert np.array_equal(slim._W.indices, W_before.indices) and np.array_equal(slim._W.data, W_before.data)
    assert ev._similarity_weights(slim)[1] is Wr  # kept while the model's W is the same object
    dense = _stub("dense_slim", X, rns)
    profiles, W = ev._dense_similarity_weights(dense)
    assert W is dense._W and profiles is dense.X_train_all
    svd = _stub("truncsvd", X, rns)
    users, items = ev._factor_operands(svd)
    assert users is svd.z_ and items.shape == (I, K) and items.flags.c_contiguous
    assert np.array_equal(items, svd.decomposer_.components_.T)
    nmf = _stub("nmf", X, rns)
    users, items = ev._factor_operands(nmf)
    assert users is nmf.W and np.array_equal(items, nmf.H.T) and items.flags.c_contiguous


def test_what_the_device_cannot_read_goes_through_the_block_loop(problem):
    X, gt, rns = problem
    ev = _evaluator()
    dense = _stub("dense_slim", X, rns)
    for W in (np.asfortranarray(dense._W), dense._W.astype(np.float16), dense._W[:, :-1].copy(), None):
        dense._W = W
        assert ev._device_path(dense) == "blocks"
    dense._W = rns.randn(I, I)  # float64, C order
    assert ev._device_path(dense) == "dense_similarity"
    svd = _stub("truncsvd", X, rns)
    svd.z_ = svd.z_.astype(np.float64)  # the host product would be float64: not what the device computes
    assert ev._device_path(svd) == "blocks"
    nmf = _stub("nmf", X, rns)
    nmf.W, nmf.H = np.zeros((U, 577), dtype=np.float32), np.zeros((577, I), dtype=np.float32)
    assert ev._device_path(nmf) == "blocks"
    del nmf.W  # not fitted
    assert ev._device_path(nmf) == "blocks"
