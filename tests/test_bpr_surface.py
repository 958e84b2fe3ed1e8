"""BPRFMRecommender and TopPopRecommender without a GPU: the Python surface against the reference's
(``recommenders/bpr.py:107-128``, ``toppop.py:14-50``), the C ABI's declarations and its argument checks (all before
any device work), the numpy restatement that arbitrates the GPU tests (``tests/_bpr_restatement.py``) on the planted
data, the operand rules of the evaluator and the serving layer, and ``bpr_host_prep.hpp`` under the sanitizers."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sps

from _bpr_restatement import TABLES, bpr_fit, bpr_step, ndcg_at, planted_split, scores, unseen_by_rank
from irspack_amd.recommenders import BPRFMRecommender, TopPopRecommender  # (the parent commit fails here)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = inspect.Parameter.empty
BPR_SYMBOLS = ["irs_bpr_create", "irs_bpr_run_epochs", "irs_bpr_sample", "irs_bpr_step_triples", "irs_bpr_get_state",
               "irs_bpr_set_state", "irs_bpr_stats", "irs_bpr_destroy"]


def _params(fn, kind):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values() if p.kind is kind]


def test_bpr_recommender_has_the_reference_surface(X_small):
    from irspack_amd import recommenders
    from irspack_amd.recommenders import BaseRecommender, BaseRecommenderWithEarlyStopping, IALSRecommender

    assert "BPRFMRecommender" in recommenders.__all__ and "TopPopRecommender" in recommenders.__all__
    assert issubclass(BPRFMRecommender, BaseRecommenderWithEarlyStopping)
    assert issubclass(IALSRecommender, BaseRecommenderWithEarlyStopping)
    assert issubclass(BaseRecommenderWithEarlyStopping, BaseRecommender)
    # the reference's arguments in the reference's order; the extensions are keyword-only
    assert _params(BPRFMRecommender.__init__, inspect.Parameter.POSITIONAL_OR_KEYWORD) == [
        ("self", EMPTY), ("X_train_all", EMPTY), ("n_components", 128), ("item_alpha", 1e-9), ("user_alpha", 1e-9),
        ("loss", "bpr"), ("n_threads", None), ("train_epochs", 128)]
    assert _params(BPRFMRecommender.__init__, inspect.Parameter.KEYWORD_ONLY) == [
        ("learning_rate", 0.05), ("batch_size", 4096), ("random_seed", 42), ("device", None)]
    rec = BPRFMRecommender(X_small)
    assert (rec.n_components, rec.item_alpha, rec.user_alpha, rec.loss, rec.train_epochs) == (128, 1e-9, 1e-9, "bpr", 128)
    assert rec.trainer is None and rec.best_state is None and rec.n_threads >= 1
    for name in ("get_score", "get_score_block", "get_user_embedding", "get_item_embedding",
                 "get_score_from_user_embedding", "get_score_from_item_embedding", "item_biases", "_create_trainer"):
        assert name in vars(BPRFMRecommender), name
    for name in ("start_learning", "run_epoch", "save_state", "load_state", "learn_with_evaluator", "_learn"):
        assert hasattr(BaseRecommenderWithEarlyStopping, name), name
    assert not hasattr(BPRFMRecommender, "fm")
    with pytest.raises(NotImplementedError, match="warp"):
        BPRFMRecommender(X_small, loss="warp")
    with pytest.raises(ValueError, match='BPRFM loss must be either "bpr" or "warp".'):
        BPRFMRecommender(X_small, loss="x")
    with pytest.raises(RuntimeError):
        rec.get_score(np.arange(2))
    with pytest.raises(RuntimeError, match="before initializing the trainer"):
        rec.run_epoch()
    with pytest.raises(NotImplementedError):
        rec.get_score_cold_user(X_small)


def test_toppop_is_the_reference(X_small):
    assert _params(TopPopRecommender.__init__, inspect.Parameter.POSITIONAL_OR_KEYWORD) == [
        ("self", EMPTY), ("X_train", EMPTY)]
    rec = TopPopRecommender(X_small)
    with pytest.raises(RuntimeError, match="before ``learn``"):
        rec.score
    assert rec.learn() is rec
    want = np.asarray(X_small.sum(axis=0), dtype=np.float64)
    assert rec.score.shape == (1, 5) and rec.score.dtype == np.float64
    for got in (rec.get_score(np.array([3, 0, 1])), rec.get_score_cold_user(X_small[:3])):
        assert got.shape == (3, 5) and got.dtype == np.float64
        np.testing.assert_array_equal(got, np.repeat(want, 3, axis=0))
    removed = rec.get_score_remove_seen(np.array([1]))
    assert np.isneginf(removed[0, [1, 3]]).all() and np.isfinite(removed[0, [0, 2, 4]]).all()
    X_train, X_test = planted_split()
    pop = TopPopRecommender(X_train).learn()
    got = ndcg_at(pop.get_score(np.arange(X_train.shape[0])), X_train, X_test)
    print("TopPop nDCG@20 on the planted split:", got)
    assert got == pytest.approx(0.0335, abs=5e-5)


def test_symbols_declared_listed_and_exported():
    from irspack_amd import _lib

    header = open(os.path.join(ROOT, "include", "irspack_amd.h")).read()
    declared = set(re.findall(r"\b(irs_[a-z0-9_]+)\s*\(", header))
    for s in BPR_SYMBOLS:
        assert s in declared and s in _lib.EXPORTED_SYMBOLS and s in _lib.ARGTYPES and hasattr(_lib.lib(), s), s
    assert _lib.lib().irs_abi_version() == 4 and _lib.ABI_VERSION == 4  # an additive change
    assert C.sizeof(_lib.BprStatsStruct) == 72
    assert "typedef struct irs_bpr irs_bpr;" in header and "} irs_bpr_stats_t;" in header


# ---- the C ABI's argument checks ----------------------------------------------------------------------------------
BASE = dict(indptr=np.array([0, 2, 3, 3], dtype=np.int64), indices=np.array([0, 2, 1], dtype=np.int32),
            data=np.ones(3, dtype=np.float32), cols=4, k=2, user_alpha=0.0, item_alpha=0.0, lr=0.05, batch=8,
            user_init=None, item_init=None)


def _create(**kw):
    from irspack_amd import _lib

    a = dict(BASE, **kw)
    h = C.c_void_p()
    rows = len(a["indptr"]) - 1
    inits = [None if t is None else _lib.ptr(t, C.c_float) for t in (a["user_init"], a["item_init"])]
    st = _lib.lib().irs_bpr_create(rows, a["cols"], _lib.ptr(a["indptr"], C.c_int64), _lib.ptr(a["indices"], C.c_int32),
                                   _lib.ptr(a["data"], C.c_float), a["k"], a["user_alpha"], a["item_alpha"], a["lr"],
                                   a["batch"], 42, *inits, 0, C.byref(h))
    return st, _lib.lib().irs_last_error().decode(), h


def test_create_checks_come_before_device_work():
    """Status 1 (invalid argument) with its message from every check where no device is visible too (a status 2
    there would mean the device was asked first), and no handle comes back."""
    def call(**kw):
        st, msg, h = _create(**kw)
        assert st == 0 or not h.value
        return st, msg

    # the matrix checks, in the words of irs_truncsvd_create
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
    assert call(k=0) == (1, "k must be >= 1.")
    assert call(k=513) == (1, "k must be <= 512.")
    assert call(batch=0) == (1, "batch_size must be >= 1.")
    for bad in (-1e-9, np.nan, np.inf):
        assert call(user_alpha=bad) == (1, "the alphas must be finite and >= 0.")
        assert call(item_alpha=bad) == (1, "the alphas must be finite and >= 0.")
        assert call(lr=bad) == (1, "learning_rate must be finite and >= 0.")
    assert call(lr=0.0) == (1, "learning_rate must not be 0.")
    for bad in (np.nan, -np.inf):
        t = np.full((3, 2), 0.1, dtype=np.float32)
        t[2, 1] = bad
        assert call(user_init=t) == (1, "the initial user table holds a non-finite value.")
        t = np.full((4, 2), 0.1, dtype=np.float32)
        t[0, 0] = bad
        assert call(item_init=t) == (1, "the initial item table holds a non-finite value.")
    st, msg = call(item_init=np.full((4, 2), 300.0, dtype=np.float32))
    assert st == 1 and "magnitude" in msg


def test_state_and_triple_checks_come_before_device_work():
    """a handle is made without a device (entries <= 0 are dropped there and then); what it is handed is checked
    before the device is asked for"""
    from irspack_amd import _lib

    lib = _lib.lib()
    st, msg, h = _create(data=np.array([1.0, -2.0, 0.5], dtype=np.float32), k=512)
    assert st == 0 and h.value, msg
    try:
        stats = _lib.BprStatsStruct()
        assert lib.irs_bpr_stats(h, C.byref(stats)) == 0
        assert (stats.n_positives, stats.n_skipped_full_rows, stats.n_skipped_positives) == (2, 0, 0)
        assert (stats.batches_per_epoch, stats.lanes_per_triple, stats.scale_log2) == (1, 64, 44)
        # the initial state is readable without a device: LightFM's start
        k = 512
        tabs = {n: np.full(s, 7.0, dtype=np.float32) for n, s in
                (("U", (3, k)), ("V", (4, k)), ("b", 4), ("GU", (3, k)), ("GV", (4, k)), ("Gb", 4))}
        epoch = C.c_int64(-1)
        assert lib.irs_bpr_get_state(h, *(_lib.ptr(tabs[n], C.c_float) for n in TABLES), C.byref(epoch)) == 0
        assert epoch.value == 0 and not tabs["b"].any() and all((tabs[n] == 1.0).all() for n in ("GU", "GV", "Gb"))
        for n in ("U", "V"):
            assert (np.abs(tabs[n]) < 0.5 / k).all() and np.unique(tabs[n]).size > tabs[n].size // 2
            assert abs(float(tabs[n].mean())) < 0.05 / k

        def set_state(epoch=3, **kw):
            t = {n: (np.ones_like(tabs[n]) if n.startswith("G") else np.zeros_like(tabs[n])) for n in TABLES}
            for n, (at, v) in kw.items():
                t[n][at] = v
            return (lib.irs_bpr_set_state(h, *(_lib.ptr(t[n], C.c_float) for n in TABLES), epoch),
                    lib.irs_last_error().decode())

        for n, at in (("U", (2, 511)), ("V", (0, 0)), ("b", 3)):
            for bad in (np.nan, np.inf):
                assert set_state(**{n: (at, bad)}) == (1, "the state holds a non-finite value.")
            assert set_state(**{n: (at, -256.0)}) == (1, "the state holds a value of magnitude >= 2^8.")
        for n, at in (("GU", (0, 5)), ("GV", (3, 511)), ("Gb", 0)):
            for bad in (0.0, -1.0, np.nan):
                assert set_state(**{n: (at, bad)}) == (1, "the Adagrad accumulators must be finite and > 0.")
        assert set_state(epoch=-1) == (1, "epoch must be >= 0.")
        # (nothing of the refused states was kept)
        assert lib.irs_bpr_get_state(h, *(_lib.ptr(tabs[n], C.c_float) for n in TABLES), C.byref(epoch)) == 0
        assert epoch.value == 0 and (tabs["GU"] == 1.0).all()

        def step(u, i, j):
            arrays = [np.array(a, dtype=np.int32) for a in (u, i, j)]
            return (lib.irs_bpr_step_triples(h, len(u), *(_lib.ptr(a, C.c_int32) for a in arrays)),
                    lib.irs_last_error().decode())

        assert step([0, 3], [0, 0], [1, 1]) == (1, "a triple's user is out of range.")
        assert step([-1], [0], [1]) == (1, "a triple's user is out of range.")
        assert step([0], [4], [1]) == (1, "a triple's item is out of range.")
        assert step([0], [0], [-1]) == (1, "a triple's item is out of range.")
        assert step([], [], [])[0] == 0
        assert lib.irs_bpr_sample(h, 0, 1, 2, None, None, None) == 1  # (2 positions in an epoch)
        assert lib.irs_bpr_sample(h, -1, 0, 0, None, None, None) == 1
        assert lib.irs_bpr_run_epochs(h, -1) == 1
    finally:
        assert lib.irs_bpr_destroy(h) == 0


# ---- the restatement ----------------------------------------------------------------------------------------------
_fits = {}


def restatement_fit():
    """K = 16, batch 1024, 20 epochs, seed 42 on the planted split (once)"""
    if "f" not in _fits:
        X_train, _ = planted_split()
        _fits["f"] = bpr_fit(X_train, 16, batch_size=1024, epochs=20, seed=42)
    return _fits["f"]


def test_restatement_learns_the_planted_groups():
    X_train, X_test = planted_split()
    assert X_train.shape == (600, 400)
    state = restatement_fit()
    bpr = ndcg_at(scores(state), X_train, X_test)
    pop = ndcg_at(np.repeat(np.asarray(X_train.sum(axis=0)), 600, axis=0), X_train, X_test)
    print("nDCG@20 on the planted split: restatement", bpr, "TopPop", pop)
    assert bpr >= 0.25 and pop <= 0.05
    assert state["epoch"] == 20 and all(np.isfinite(state[n]).all() for n in TABLES)


def test_restatement_step_by_hand():
    """one batch of two triples on one user, K = 1, written out: the shared row gets both contributions, its L2
    term once, and G is read before it is updated; the untouched rows keep their values"""
    state = dict(U=np.array([[0.5], [9.0]]), V=np.array([[1.0], [-1.0], [0.25], [3.0]]), b=np.array([0.1, 0.0, -0.1, 7.0]),
                 GU=np.array([[4.0], [2.0]]), GV=np.full((4, 1), 1.0), Gb=np.array([1.0, 1.0, 4.0, 5.0]))
    lr, ua, ia = 0.5, 0.1, 0.2
    new = bpr_step(state, [0, 0], [0, 2], [1, 1], ua, ia, lr)
    w0 = 1 / (1 + np.exp(0.5 * 2.0 + 0.1))
    w1 = 1 / (1 + np.exp(0.5 * 1.25 - 0.1))
    gU = -w0 * 2.0 - w1 * 1.25 + ua * 0.5
    assert new["U"][0, 0] == pytest.approx(0.5 - lr * gU / 2.0, rel=1e-15) and new["GU"][0, 0] == pytest.approx(4 + gU * gU)
    g1 = (w0 + w1) * 0.5 + ia * -1.0  # item 1: the negative of both
    assert new["V"][1, 0] == pytest.approx(-1.0 - lr * g1, rel=1e-15) and new["GV"][1, 0] == pytest.approx(1 + g1 * g1)
    gb2 = -w1 + ia * -0.1
    assert new["b"][2] == pytest.approx(-0.1 - lr * gb2 / 2.0, rel=1e-15) and new["Gb"][2] == pytest.approx(4 + gb2 * gb2)
    for n, row in (("U", 1), ("V", 3), ("b", 3), ("GU", 1), ("GV", 3), ("Gb", 3)):
        assert new[n][row] == state[n][row]
    assert state["U"][0, 0] == 0.5  # (the input is not changed)
    # float32 runs in float32
    assert bpr_step(state, [0], [0], [1], ua, ia, lr, np.float32)["U"].dtype == np.float32
    assert [unseen_by_rank([1, 2, 5], r) for r in range(4)] == [0, 3, 4, 6] and unseen_by_rank([], 3) == 3


def test_operand_rules_recognise_a_bpr_model():
    """a model whose trainer holds the restatement's fit is a "factors" model of K + 1 columns to the evaluator and
    to the serving layer (no device needed: the handle has not been uploaded)"""
    from irspack_amd.evaluation import Evaluator
    from irspack_amd.serving import copied_operands, model_operands

    X_train, X_test = planted_split()
    state = restatement_fit()
    model = BPRFMRecommender(X_train, n_components=16, batch_size=1024, train_epochs=20)
    assert model_operands(model) is None  # (not trained)
    model.start_learning()
    model.trainer.set_state(state)
    U32, V32, b32 = (state[n].astype(np.float32) for n in ("U", "V", "b"))
    assert model.get_user_embedding().tobytes() == U32.tobytes() and model.item_biases.tobytes() == b32.tobytes()
    kind, (users, items) = model_operands(model)
    assert kind == "factors" and users.shape == (600, 17) and items.shape == (17, 400)
    assert users.dtype == items.dtype == np.float32 and users.flags.c_contiguous and items.flags.c_contiguous
    np.testing.assert_array_equal(users, np.concatenate([U32, np.ones((600, 1), np.float32)], axis=1))
    np.testing.assert_array_equal(items, np.concatenate([V32, b32[:, None]], axis=1).T)
    assert copied_operands(kind, (users, items))[-1] is items
    assert model_operands(model)[1][0] is users  # (held per state)
    ev = Evaluator.__new__(Evaluator)
    ev.fused = True
    fu, fi = ev._factor_operands(model)
    assert fu is users and fi.shape == (400, 17) and fi.flags.c_contiguous
    np.testing.assert_array_equal(fi, items.T)
    ev.fused = False
    assert ev._factor_operands(model) is None
    # the host scores are U V^T + b, the product of the two tables up to the order of the sum
    block = model.get_score_block(10, 30)
    np.testing.assert_allclose(block, (users @ items)[10:30], rtol=0, atol=1e-5)
    np.testing.assert_array_equal(block, model.get_score(np.arange(10, 30)))
    np.testing.assert_array_equal(block, model.get_score_from_user_embedding(U32[10:30]))
    np.testing.assert_array_equal(model.get_score_from_item_embedding(np.arange(3), V32[:5]), U32[:3] @ V32[:5].T)
    # a subclass that scores differently is left to the block loop; a new state hands out new tables
    Other = type("Other", (BPRFMRecommender,), {"get_score_block": lambda self, b, e: None})
    other = Other(X_train, n_components=16)
    other.trainer = model.trainer
    assert model_operands(other) is None and ev._factor_operands(other) is None
    state2 = dict(state, b=state["b"] + 1.0)
    model.trainer.set_state(state2)
    assert model_operands(model)[1][1][16, 0] == np.float32(state["b"][0] + 1.0)


_HOST_CXX = shutil.which("g++") or shutil.which("clang++")


@pytest.mark.skipif(_HOST_CXX is None, reason="needs a host C++ compiler")
def test_bpr_host_preparation_under_address_and_ub_sanitizers(tmp_path):
    """irspack_amd/csrc/bpr_host_prep.hpp - the filter of the positives, the argument checks, the permutation as a
    bijection at many sizes, the unseen-rank mapping against a scan, whole epochs sampled on the host, the scale
    bound, the lane layout - in a program of its own (tests/host/bpr_host_prep_main.cpp), every report fatal."""
    exe = str(tmp_path / "bpr_host_prep_main")
    src = os.path.join(ROOT, "tests", "host", "bpr_host_prep_main.cpp")
    subprocess.check_call([_HOST_CXX, "-std=c++17", "-O1", "-g", "-pthread", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "bpr_host_prep ok" in r.stdout
