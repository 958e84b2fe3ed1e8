"""CPU-only checks of ``irspack_amd.utils.id_mapping`` (the reference's ``irspack/utils/id_mapping.py:51-453``)
and of what ``irspack_amd.serving`` does before it touches a device: the public signatures against the hand-written
``tests/golden/id_mapping_surface.json`` (names, argument order, defaults), the constructor errors, the profile
matrix, the single-user host logic on a mock recommender with fixed scores, and the ``TypeError`` for a model the
device cannot serve."""
import inspect
import json
import os

import numpy as np
import pytest
import scipy.sparse as sps

from irspack_amd import serving
from irspack_amd.recommenders.base import BaseRecommender
from irspack_amd.utils import IDMapper, ItemIDMapper, id_mapping

HERE = os.path.dirname(os.path.abspath(__file__))
SURFACE = json.load(open(os.path.join(HERE, "golden", "id_mapping_surface.json")))

N_USERS, N_ITEMS = 31, 42


class FixedScores(BaseRecommender):
    """scores fixed in advance; nothing the device recognises"""

    def __init__(self, X, scores):
        super().__init__(X)
        self.scores = scores
        self.item_item = np.random.default_rng(5).standard_normal((N_ITEMS, N_ITEMS))

    def get_score(self, user_indices):
        return self.scores[user_indices].copy()

    def get_score_cold_user(self, X):
        return np.asarray(sps.csr_matrix(X).dot(self.item_item))


@pytest.fixture(scope="module")
def world():
    rng = np.random.default_rng(3)
    X = sps.csr_matrix((rng.random((N_USERS, N_ITEMS)) < 0.2).astype(np.float64))
    scores = rng.standard_normal((N_USERS, N_ITEMS))
    scores[4, 5:9] = np.inf
    scores[4, 20] = -np.inf
    user_ids = [f"u{u}" for u in range(N_USERS)]
    item_ids = [f"i{i}" for i in range(N_ITEMS)]
    return X, scores, FixedScores(X, scores), IDMapper(user_ids, item_ids), user_ids, item_ids


def _check(where, fn, ref):
    ps = [p for p in inspect.signature(fn).parameters.values() if p.name != "self"]
    names = [p.name for p in ps]
    assert names[:len(ref["args"])] == ref["args"], (where, names)
    for p in ps[len(ref["args"]):]:
        assert p.default is not inspect.Parameter.empty, (where, p.name)
    for p in ps[:len(ref["args"])]:
        if p.name in ref["defaults"]:
            assert p.default == ref["defaults"][p.name] and (p.default is None) == (ref["defaults"][p.name] is None), \
                (where, p.name, p.default)
        # (an argument the reference requires may be optional here: utils.retrieve_recommend_from_score's n_threads)


def test_signatures_match_the_reference():
    for fname, ref in SURFACE["functions"].items():
        _check(fname, getattr(id_mapping, fname), ref)
    for cname, methods in SURFACE["classes"].items():
        cls = getattr(id_mapping, cname)
        for mname, ref in methods.items():
            _check(f"{cname}.{mname}", getattr(cls, mname), ref)
    assert issubclass(IDMapper, ItemIDMapper)
    import irspack_amd.utils as U

    assert U.IDMapper is id_mapping.IDMapper and U.ItemIDMapper is id_mapping.ItemIDMapper
    assert id_mapping.retrieve_recommend_from_score is U.retrieve_recommend_from_score


def test_constructor_errors(world):
    X, scores, model, mapper, user_ids, item_ids = world
    with pytest.raises(ValueError, match="Duplicates in item_ids"):
        ItemIDMapper(["a", "b", "a"])
    with pytest.raises(ValueError, match="Duplicates in user_ids"):
        IDMapper([1, 2, 1], ["a", "b"])
    with pytest.raises(ValueError, match="Duplicates in item_ids"):
        IDMapper([1, 2], ["a", "a"])
    short = IDMapper(user_ids[:-1], item_ids)
    with pytest.raises(ValueError):
        short.recommend_for_known_user_id(model, "u0")
    with pytest.raises(ValueError):
        short.recommend_for_known_user_batch(model, ["u0"])
    narrow = IDMapper(user_ids, item_ids[:-1])
    with pytest.raises(ValueError, match="n_items"):
        narrow.recommend_for_new_user(model, ["i0"])
    with pytest.raises(ValueError, match="n_items"):
        narrow.recommend_for_new_user_batch(model, [["i0"]])
    with pytest.raises(ValueError, match="score.shape"):
        narrow.score_to_recommended_items(scores[0], 3)
    with pytest.raises(RuntimeError, match="not found"):
        mapper.recommend_for_known_user_id(model, "nobody")


def test_list_of_user_profile_to_matrix():
    m = ItemIDMapper(["a", "b", "c", "d", "e"])
    X = m.list_of_user_profile_to_matrix([["c", "zz", "a"], {"b": 0.0, "e": 2.5, "yy": 9.0}, [], {}])
    assert sps.isspmatrix_csr(X) and X.shape == (4, 5)
    assert X.indptr.tolist() == [0, 2, 4, 4, 4]
    assert X.indices.tolist() == [2, 0, 1, 4]  # list order kept, unknown ids dropped
    assert X.data.tolist() == [1.0, 1.0, 0.0, 2.5]  # the rating 0.0 stays a stored zero
    assert X.nnz == 4
    assert np.array_equal(X.toarray(), [[1, 0, 1, 0, 0], [0, 0, 0, 0, 2.5], [0] * 5, [0] * 5])


def _expected_row(score, cutoff, allowed=None, forbidden=()):
    cand = list(range(len(score))) if allowed is None else list(allowed)
    keep = [i for i in cand if not np.isinf(score[i]) and i not in forbidden]
    keep.sort(key=lambda i: -score[i])
    return keep[:cutoff]


def test_single_user_methods(world):
    X, scores, model, mapper, user_ids, item_ids = world
    dense = X.toarray()
    for u in (0, 4, 17, 30):
        masked = scores[u].copy()
        masked[dense[u] != 0] = -np.inf
        for cutoff in (1, 5, N_ITEMS + 3):
            got = mapper.recommend_for_known_user_id(model, user_ids[u], cutoff=cutoff)
            want = _expected_row(masked, cutoff)
            assert [i for i, _ in got] == [item_ids[i] for i in want]
            assert [s for _, s in got] == [float(masked[i]) for i in want]
            assert len(got) <= cutoff
            assert all(np.isfinite(s) for _, s in got)  # +inf and -inf are both skipped
            assert all(dense[u, int(i[1:])] == 0 for i, _ in got)  # nothing seen
            assert [s for _, s in got] == sorted((s for _, s in got), reverse=True)
        allowed = [item_ids[i] for i in (7, 3, 20, 11, 40, 2)] + ["unknown"]
        forbidden = [item_ids[i] for i in (3, 40)] + ["nobody"]
        got = mapper.recommend_for_known_user_id(model, user_ids[u], cutoff=4, allowed_item_ids=allowed,
                                                 forbidden_item_ids=forbidden)
        want = _expected_row(masked, 4, allowed=[7, 3, 20, 11, 40, 2], forbidden=(3, 40))
        assert [i for i, _ in got] == [item_ids[i] for i in want]  # best first (no equal finite scores here)
        assert [s for _, s in got] == [float(masked[i]) for i in want]
        assert set(i for i, _ in got) <= set(allowed) - set(forbidden)
    # defaults: cutoff 20
    assert len(mapper.recommend_for_known_user_id(model, "u1")) == 20


def test_new_user_and_score_to_recommended_items(world):
    X, scores, model, mapper, user_ids, item_ids = world
    profile = {"i3": 2.0, "i9": 1.0, "nope": 5.0}
    row = 2.0 * model.item_item[3] + 1.0 * model.item_item[9]
    want_scores = row.copy()
    want_scores[[3, 9]] = -np.inf
    got = mapper.recommend_for_new_user(model, profile, cutoff=6, forbidden_item_ids=["i0"])
    want = _expected_row(want_scores, 6, forbidden=(0,))
    assert [i for i, _ in got] == [item_ids[i] for i in want]
    assert all("i3" != i and "i9" != i and "i0" != i for i, _ in got)
    s = np.array([0.5, np.inf, -np.inf, 2.0, 1.0] + [0.0] * (N_ITEMS - 5))
    assert mapper.score_to_recommended_items(s, 3) == [("i3", 2.0), ("i4", 1.0), ("i0", 0.5)]
    assert mapper.score_to_recommended_items(s, 2, allowed_item_ids=["i4", "i1", "i0", "i2"]) == \
        [("i4", 1.0), ("i0", 0.5)]


def test_device_recommender_refuses_unknown_models_before_any_device_use(world, monkeypatch):
    X, scores, model, mapper, user_ids, item_ids = world

    def no_library():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(serving, "lib", no_library)
    assert serving.model_operands(model) is None
    with pytest.raises(TypeError, match="FixedScores"):
        serving.DeviceRecommender(model)
    with pytest.raises(TypeError):
        serving.DeviceRecommender(object())

    # a recognised class whose get_score_block is overridden scores some other way: not recognised either
    from irspack_amd.recommenders.base import BaseSimilarityRecommender

    class Odd(BaseSimilarityRecommender):
        def get_score_block(self, begin, end):
            return super().get_score_block(begin, end) * 2

    odd = Odd(X)
    odd._W = sps.identity(N_ITEMS, format="csr")
    with pytest.raises(TypeError):
        serving.DeviceRecommender(odd)
    plain = BaseSimilarityRecommender(X)
    plain._W = sps.identity(N_ITEMS, format="csr")
    assert serving.model_operands(plain)[0] == "similarity"


class _StubServed:
    """stands in for serving.DeviceRecommender: no device, counts what the cache does with it"""
    made = []

    def __init__(self, model, device=None, weak_model=False):
        assert weak_model, "the cache must not make its copy hold the model"
        self.kind, self.closed = "similarity", 0
        _StubServed.made.append(self)

    def close(self):
        self.closed += 1


def _stub_the_device(monkeypatch, keys):
    from irspack_amd.recommenders.base import BaseSimilarityRecommender

    _StubServed.made = []
    monkeypatch.setattr(serving, "DeviceRecommender", _StubServed)
    monkeypatch.setattr(id_mapping, "_operand_key", lambda kind, operands: (kind, keys[0]))
    return BaseSimilarityRecommender


def test_the_cache_lets_go_of_a_model_that_is_dropped(world, monkeypatch):
    """the per-model cache must not keep a model alive: when the model goes, its entry goes and the device copy is
    closed (once); a copy that was replaced earlier is let go of without the finalizer closing it later"""
    import gc
    import weakref

    X = world[0]
    keys = ["first"]
    Plain = _stub_the_device(monkeypatch, keys)
    before = len(id_mapping._recommenders)
    model = Plain(X)
    model._W = sps.identity(N_ITEMS, format="csr")
    a = id_mapping._device_recommender(model, 3)
    assert isinstance(a, _StubServed) and id_mapping._device_recommender(model, 1) is a  # kept
    assert len(id_mapping._recommenders) == before + 1
    keys[0] = "second"  # the operands changed: a new copy, the old one is only released
    b = id_mapping._device_recommender(model, 3)
    assert b is not a and _StubServed.made == [a, b] and id_mapping._recommenders[model].served is b
    gone = weakref.ref(model)
    del model
    gc.collect()
    assert gone() is None, "something still holds the model"
    assert len(id_mapping._recommenders) == before
    assert (a.closed, b.closed) == (0, 1)


def test_device_recommender_can_hold_its_model_weakly(world, monkeypatch):
    """DeviceRecommender(weak_model=True) keeps neither the model nor its operand tuple; a call after the model is
    gone raises ReferenceError.  (The constructor's device calls are stubbed: no device here.)"""
    import gc
    import weakref

    from irspack_amd.recommenders.base import BaseSimilarityRecommender

    class NoLibrary:
        def __getattr__(self, name):
            return lambda *args: 0

    monkeypatch.setattr(serving, "lib", lambda: NoLibrary())
    monkeypatch.setattr(serving._lib, "default_device", lambda: 0)
    for weak in (True, False):
        model = BaseSimilarityRecommender(world[0])
        model._W = sps.identity(N_ITEMS, format="csr")
        dev = serving.DeviceRecommender(model, weak_model=weak)
        assert dev.model is model and not hasattr(dev, "operands")
        gone = weakref.ref(model)
        del model
        gc.collect()
        assert (gone() is None) == weak
        if weak:
            with pytest.raises(ReferenceError):
                dev.recommend_known_arrays([0], 3)


def test_batches_below_the_threshold_take_the_two_step_path(world, monkeypatch):
    Plain = _stub_the_device(monkeypatch, ["k"])
    model = Plain(world[0])
    model._W = sps.identity(N_ITEMS, format="csr")
    monkeypatch.setitem(id_mapping.DEVICE_MIN_BATCH, "similarity", 8)
    assert id_mapping._device_recommender(model, 7) is None and _StubServed.made == []
    assert isinstance(id_mapping._device_recommender(model, 8), _StubServed)
    assert id_mapping._device_recommender(world[2], 100) is None  # FixedScores: not recognised
