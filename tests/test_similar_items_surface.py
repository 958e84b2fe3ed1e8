"""The public surface of the neighbour calls (no GPU): ``irs_serve_neighbors`` in the header, the loader and the
library; ``DeviceRecommender.similar_items`` / ``similar_users`` and the ``ItemIDMapper`` / ``IDMapper`` methods with
their defaults; ``serving.embedding_width`` on hand-built models; ``TypeError`` for a model the device cannot serve.
"""
import inspect
import os
import re

import numpy as np
import pytest
import scipy.sparse as sps

from irspack_amd import _lib, serving
from irspack_amd.utils import IDMapper, ItemIDMapper

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def X():
    rng = np.random.default_rng(0)
    return sps.csr_matrix((rng.random((30, 20)) < 0.2).astype(np.float64))


def test_symbol_is_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "irspack_amd.h")).read()
    assert re.search(r"\birs_status\s+irs_serve_neighbors\s*\(\s*irs_server\s*\*", header)
    for name, value in (("WEIGHT", 0), ("COSINE", 1), ("DOT", 2)):
        assert re.search(rf"#define\s+IRS_NEIGHBOR_{name}\s+{value}\b", header), name
        assert getattr(_lib, f"NEIGHBOR_{name}") == value
    assert "irs_serve_neighbors" in _lib.EXPORTED_SYMBOLS
    assert len(_lib.ARGTYPES["irs_serve_neighbors"]) == 14
    lib = _lib.lib()
    assert hasattr(lib, "irs_serve_neighbors")
    assert lib.irs_abi_version() == 4 == _lib.ABI_VERSION
    assert re.search(r"#define\s+IRS_ABI_VERSION\s+4\b", header)


def defaults(fn):
    return {name: p.default for name, p in inspect.signature(fn).parameters.items()
            if p.default is not inspect.Parameter.empty}


def names(fn):
    return list(inspect.signature(fn).parameters)


def test_device_recommender_methods_and_defaults():
    D = serving.DeviceRecommender
    for fn in (D.similar_items_arrays, D.similar_items):
        assert names(fn) == ["self", "item_indices", "cutoff", "allowed", "per_item_allowed", "forbidden", "metric"]
        assert defaults(fn) == dict(allowed=None, per_item_allowed=None, forbidden=None, metric=None)
    for fn in (D.similar_users_arrays, D.similar_users):
        assert names(fn) == ["self", "user_indices", "cutoff", "allowed", "per_user_allowed", "forbidden", "metric"]
        assert defaults(fn) == dict(allowed=None, per_user_allowed=None, forbidden=None, metric=None)


def test_id_mapper_methods_and_defaults():
    assert names(ItemIDMapper.similar_items) == [
        "self", "recommender", "item_id", "cutoff", "allowed_item_ids", "forbidden_item_ids", "metric"]
    assert defaults(ItemIDMapper.similar_items) == dict(
        cutoff=20, allowed_item_ids=None, forbidden_item_ids=None, metric=None)
    assert names(ItemIDMapper.similar_items_batch) == [
        "self", "recommender", "item_ids", "cutoff", "allowed_item_ids", "per_item_allowed_item_ids",
        "forbidden_item_ids", "metric"]
    assert defaults(ItemIDMapper.similar_items_batch) == dict(
        cutoff=20, allowed_item_ids=None, per_item_allowed_item_ids=None, forbidden_item_ids=None, metric=None)
    assert IDMapper.similar_items is ItemIDMapper.similar_items
    assert names(IDMapper.similar_users) == [
        "self", "recommender", "user_id", "cutoff", "allowed_user_ids", "forbidden_user_ids", "metric"]
    assert defaults(IDMapper.similar_users) == dict(
        cutoff=20, allowed_user_ids=None, forbidden_user_ids=None, metric=None)
    assert names(IDMapper.similar_users_batch) == [
        "self", "recommender", "user_ids", "cutoff", "allowed_user_ids", "per_user_allowed_user_ids",
        "forbidden_user_ids", "metric"]
    assert defaults(IDMapper.similar_users_batch) == dict(
        cutoff=20, allowed_user_ids=None, per_user_allowed_user_ids=None, forbidden_user_ids=None, metric=None)


def test_embedding_width_of_each_model_class(X):
    from irspack_amd.recommenders.bpr import BPRFMRecommender, WARPFMRecommender
    from irspack_amd.recommenders.ials import IALSRecommender
    from irspack_amd.recommenders.multvae import MultVAERecommender
    from irspack_amd.recommenders.nmf import NMFRecommender
    from irspack_amd.recommenders.truncsvd import TruncatedSVDRecommender

    width = serving.embedding_width
    assert width(BPRFMRecommender(X, n_components=7)) == 7  # (not the bias column of [V | b])
    assert width(WARPFMRecommender(X, n_components=9)) == 9
    assert width(IALSRecommender(X, n_components=5)) == 5
    assert width(MultVAERecommender(X, dim_z=4, enc_hidden_dims=48)) == 48  # (the decoder's width defaults to it)
    assert width(MultVAERecommender(X, dim_z=4, enc_hidden_dims=48, dec_hidden_dims=32)) == 32
    assert width(TruncatedSVDRecommender(X, n_components=6)) == 6
    nmf = NMFRecommender(X, n_components=8)
    assert width(nmf) == 8
    nmf.W = np.zeros((30, 11), dtype=np.float32)  # hand-made tables: their width counts
    nmf.H = np.zeros((11, 20), dtype=np.float32)
    assert width(nmf) == 11


def test_unrecognised_models_raise_type_error(X):
    from irspack_amd.recommenders.base import BaseRecommender

    class Fixed(BaseRecommender):
        def get_score(self, user_indices):
            return np.zeros((len(user_indices), self.n_items))

    model = Fixed(X)
    with pytest.raises(TypeError):
        serving.embedding_width(model)
    with pytest.raises(TypeError, match="not a model the device can serve"):
        serving.DeviceRecommender(model)
    mapper = IDMapper(list(range(30)), [f"i{i}" for i in range(20)])
    with pytest.raises(TypeError, match="not a model the device can serve"):
        mapper.similar_items(model, "i3")
    with pytest.raises(TypeError, match="not a model the device can serve"):
        mapper.similar_items_batch(model, ["i3", "i4"])
    with pytest.raises(TypeError, match="not a model the device can serve"):
        mapper.similar_users(model, 3)
    with pytest.raises(RuntimeError, match="not found"):
        mapper.similar_items(model, "nope")
    with pytest.raises(RuntimeError, match="not found"):
        mapper.similar_users_batch(model, [3, 99])
