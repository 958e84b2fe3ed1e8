"""WARPFMRecommender and ``BPRFMTrainer(loss="warp")`` without a GPU: the Python surface, the C ABI's declarations and
its argument checks (all before any device work), the numpy restatement that arbitrates the GPU tests
(``tests/_warp_restatement.py``) by hand and on the planted data, the operand rules of the evaluator and the serving
layer, what the inputs of the GPU tests promise (``tests/_warp_cases.py``), and the WARP part of ``bpr_host_prep.hpp``
under the sanitizers."""
import ctypes as C
import inspect
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from _bpr_restatement import TABLES, ndcg_at, planted_split, scores
from _warp_cases import (K_LIST, LR, SEARCH_SIZES, five_item_case, many_item_case, random_state, search_batch,
                         step_cases)
from _warp_restatement import warp_fit, warp_search, warp_step, warp_weights
from irspack_amd.recommenders import BPRFMRecommender, WARPFMRecommender  # (the parent commit fails here)
from irspack_amd.recommenders.bpr import BPRFMTrainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = inspect.Parameter.empty
WARP_SYMBOLS = ["irs_bpr_create_warp", "irs_bpr_warp_candidates", "irs_bpr_warp_search", "irs_bpr_warp_step",
                "irs_bpr_warp_stats"]


def _params(fn, kind):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values() if p.kind is kind]


def test_warp_recommender_surface(X_small):
    from irspack_amd import recommenders
    from irspack_amd.recommenders import BaseRecommenderWithEarlyStopping

    assert "WARPFMRecommender" in recommenders.__all__ and "BPRFMRecommender" in recommenders.__all__
    assert issubclass(WARPFMRecommender, BPRFMRecommender)
    assert issubclass(WARPFMRecommender, BaseRecommenderWithEarlyStopping)
    assert _params(WARPFMRecommender.__init__, inspect.Parameter.POSITIONAL_OR_KEYWORD) == [
        ("self", EMPTY), ("X_train_all", EMPTY), ("n_components", 128), ("item_alpha", 1e-9), ("user_alpha", 1e-9),
        ("n_threads", None), ("train_epochs", 128)]
    assert _params(WARPFMRecommender.__init__, inspect.Parameter.KEYWORD_ONLY) == [
        ("max_sampled", 10), ("learning_rate", 0.05), ("batch_size", 4096), ("random_seed", 42), ("device", None)]
    rec = WARPFMRecommender(X_small)
    assert (rec.n_components, rec.item_alpha, rec.user_alpha, rec.loss, rec.max_sampled, rec.train_epochs) == \
        (128, 1e-9, 1e-9, "warp", 10, 128)
    assert rec.trainer is None and rec.n_threads >= 1
    # scoring is the parent's, so the evaluator and the serving layer see a K + 1 factor model
    for name in ("get_score", "get_score_block", "factor_tables", "get_user_embedding", "get_item_embedding"):
        assert name not in vars(WARPFMRecommender), name
    assert "_create_trainer" in vars(WARPFMRecommender)
    # the pinned constructor still refuses, in the same words
    with pytest.raises(NotImplementedError, match='BPRFM loss "warp" is not implemented on the device'):
        BPRFMRecommender(X_small, loss="warp")
    # the trainer has learnt the loss
    sig = inspect.signature(BPRFMTrainer.__init__).parameters
    assert sig["loss"].default == "bpr" and sig["max_sampled"].default == 10
    for name in ("candidates", "search", "step_candidates", "warp_stats"):
        assert callable(getattr(BPRFMTrainer, name)), name
    with pytest.raises(ValueError, match='BPRFM loss must be either "bpr" or "warp".'):
        BPRFMTrainer(X_small, 4, 0.0, 0.0, loss="x")
    rec.start_learning()  # (a handle is made without a device)
    assert rec.trainer.hyper["loss"] == "warp" and rec.trainer.hyper["max_sampled"] == 10
    st = rec.trainer.warp_stats()
    assert (st["max_sampled"], st["scale_log2"], st["epoch_positions"], st["call_tries"]) == (10, 40, 0, 0)
    assert st["in_flight"] in (1, 2, 4) and "reserved" not in st
    bpr = BPRFMTrainer(X_small, 4, 0.0, 0.0, max_sampled=7)
    assert bpr.hyper["loss"] == "bpr" and bpr.hyper["max_sampled"] == 0  # (max_sampled is WARP's alone)
    with pytest.raises(ValueError, match="irs_bpr_create_warp"):
        bpr.warp_stats()
    for bad in (0, 257, -1):
        with pytest.raises(ValueError, match="max_sampled must be"):
            BPRFMTrainer(X_small, 4, 0.0, 0.0, loss="warp", max_sampled=bad)
    with pytest.raises(ValueError, match="shape"):
        rec.trainer.search([0], [0], np.zeros((1, 9), dtype=np.int32))


def test_symbols_declared_listed_and_exported():
    from irspack_amd import _lib

    header = open(os.path.join(ROOT, "include", "irspack_amd.h")).read()
    declared = set(re.findall(r"\b(irs_[a-z0-9_]+)\s*\(", header))
    for s in WARP_SYMBOLS:
        assert s in declared and s in _lib.EXPORTED_SYMBOLS and s in _lib.ARGTYPES and hasattr(_lib.lib(), s), s
    assert _lib.lib().irs_abi_version() == 4 and _lib.ABI_VERSION == 4  # an additive change
    assert C.sizeof(_lib.BprStatsStruct) == 72 and C.sizeof(_lib.BprWarpStatsStruct) == 88
    assert "} irs_bpr_warp_stats_t;" in header
    # irs_bpr_create_warp: irs_bpr_create's arguments and max_sampled before the handle
    assert _lib.ARGTYPES["irs_bpr_create_warp"] == \
        _lib.ARGTYPES["irs_bpr_create"][:-1] + [C.c_int32] + _lib.ARGTYPES["irs_bpr_create"][-1:]
    # the struct's fields in the header's order
    body = header[header.index("typedef struct {\n  int32_t max_sampled;"):header.index("} irs_bpr_warp_stats_t;")]
    assert re.findall(r"^\s+(?:int32_t|int64_t|double)\s+(\w+);", body, flags=re.M) == \
        [name for name, _ in _lib.BprWarpStatsStruct._fields_]


# ---- the C ABI's argument checks ----------------------------------------------------------------------------------
BASE = dict(indptr=np.array([0, 2, 3, 3], dtype=np.int64), indices=np.array([0, 2, 1], dtype=np.int32),
            data=np.ones(3, dtype=np.float32), cols=4, k=2, max_sampled=3)


def _create(warp=True, **kw):
    from irspack_amd import _lib

    a = dict(BASE, **kw)
    h = C.c_void_p()
    args = [len(a["indptr"]) - 1, a["cols"], _lib.ptr(a["indptr"], C.c_int64), _lib.ptr(a["indices"], C.c_int32),
            _lib.ptr(a["data"], C.c_float), a["k"], 0.0, 0.0, 0.05, 8, 42, None, None, 0]
    if warp:
        st = _lib.lib().irs_bpr_create_warp(*args, a["max_sampled"], C.byref(h))
    else:
        st = _lib.lib().irs_bpr_create(*args, C.byref(h))
    return st, _lib.lib().irs_last_error().decode(), h


def test_every_check_comes_before_device_work():
    """status 1 (invalid argument) with its message from every check where no device is visible too (a status 2 there
    would mean the device was asked first)"""
    from irspack_amd import _lib

    lib = _lib.lib()
    for bad, msg in ((0, "max_sampled must be >= 1."), (-5, "max_sampled must be >= 1."),
                     (257, "max_sampled must be <= 256.")):
        st, got, h = _create(max_sampled=bad)
        assert (st, got) == (1, msg) and not h.value
    assert _create(k=513)[:2] == (1, "k must be <= 512.")  # (irs_bpr_create's checks)
    assert _create(cols=2)[:2] == (1, "column index out of range.")
    st, msg, h = _create(max_sampled=256)
    assert st == 0 and h.value, msg
    assert lib.irs_bpr_destroy(h) == 0
    st, msg, h = _create()
    assert st == 0 and h.value, msg
    st, msg, plain = _create(warp=False)
    assert st == 0 and plain.value, msg
    i32 = lambda *v: np.array(v, dtype=np.int32)  # noqa: E731
    p = lambda a: _lib.ptr(a, C.c_int32)  # noqa: E731
    err = lambda: lib.irs_last_error().decode()  # noqa: E731
    try:
        ws = _lib.BprWarpStatsStruct()
        assert lib.irs_bpr_warp_stats(h, C.byref(ws)) == 0
        assert (ws.max_sampled, ws.scale_log2, ws.epoch_positions, ws.call_positions) == (3, 40, 0, 0)
        stats = _lib.BprStatsStruct()
        assert lib.irs_bpr_stats(h, C.byref(stats)) == 0 and stats.n_positives == 3  # (the BPR call works on it)
        assert lib.irs_bpr_warp_stats(h, None) == 1 and err() == "null argument."
        out = [np.zeros(4, dtype=np.int32) for _ in range(2)] + [np.zeros(12, dtype=np.int32)]

        def candidates(epoch, first, count, arrays=out):
            return lib.irs_bpr_warp_candidates(h, epoch, first, count, *(None if a is None else p(a) for a in arrays)), err()

        window = "first and count must describe positions of the epoch."
        assert candidates(-1, 0, 1) == (1, "epoch must be >= 0.")
        assert candidates(0, 2, 2) == (1, window) and candidates(0, -1, 1) == (1, window)  # (3 positions)
        assert candidates(0, 0, -1) == (1, window) and candidates(0, 4, 0) == (1, window)
        assert candidates(0, 0, 3, [None] + out[1:])[0] == 1 and candidates(0, 0, 3, out[:2] + [None])[0] == 1
        assert candidates(0, 3, 0, [None, None, None])[0] == 0  # (an empty window needs no array and no device)

        def batch(call, users, pos, cand, n=None, outs=True):
            arrays = [None if a is None else p(a) for a in (users, pos, cand)]
            n = len(users) if n is None else n
            if call == "search":
                neg, tries = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
                return lib.irs_bpr_warp_search(h, n, *arrays, *((p(neg), p(tries)) if outs else (None, None))), err()
            return lib.irs_bpr_warp_step(h, n, *arrays), err()

        good = (i32(0, 2), i32(3, 0), i32(1, 2, 3, 0, 0, 1))
        for call in ("search", "step"):
            assert batch(call, *good, n=-1) == (1, "n must be >= 0.")
            assert batch(call, *good, n=(1 << 31) // 3 + 1) == (1, "n * max_sampled must be below 2^31.")
            for k in range(3):
                arrays = list(good)
                arrays[k] = None
                assert batch(call, *arrays, n=2) == (1, "the position and candidate arrays must not be null.")
            assert batch(call, i32(0, 3), *good[1:]) == (1, "a position's user is out of range.")
            assert batch(call, i32(-1, 0), *good[1:]) == (1, "a position's user is out of range.")
            assert batch(call, good[0], i32(4, 0), good[2]) == (1, "a position's item is out of range.")
            assert batch(call, good[0], i32(0, -1), good[2]) == (1, "a position's item is out of range.")
            assert batch(call, *good[:2], i32(1, 2, 3, 0, 0, 4)) == (1, "a candidate is out of range.")
            assert batch(call, *good[:2], i32(-1, 2, 3, 0, 0, 1)) == (1, "a candidate is out of range.")
            assert batch(call, i32(), i32(), i32())[0] == 0  # (an empty batch needs no device)
        assert batch("search", *good, outs=False) == (1, "the output arrays must not be null.")
        # a WARP handle has no triples, a BPR handle no candidates
        three = [np.zeros(3, dtype=np.int32) for _ in range(3)]
        assert lib.irs_bpr_sample(h, 0, 0, 3, *(p(a) for a in three)) == 1 and "irs_bpr_warp_candidates" in err()
        assert lib.irs_bpr_step_triples(h, 1, p(i32(0)), p(i32(0)), p(i32(1))) == 1 and "irs_bpr_warp_step" in err()
        needs = "this call needs a handle made by irs_bpr_create_warp."
        assert lib.irs_bpr_warp_stats(plain, C.byref(ws)) == 1 and err() == needs
        assert lib.irs_bpr_warp_candidates(plain, 0, 0, 0, None, None, None) == 1 and err() == needs
        assert lib.irs_bpr_warp_step(plain, 0, None, None, None) == 1 and err() == needs
        assert lib.irs_bpr_warp_search(plain, 0, None, None, None, None, None) == 1 and err() == needs
        assert lib.irs_bpr_warp_stats(None, C.byref(ws)) == 1 and err() == "null handle."
        # the state calls work on the handle without a device
        k = 2
        tabs = {n: np.zeros(s, dtype=np.float32) for n, s in
                (("U", (3, k)), ("V", (4, k)), ("b", 4), ("GU", (3, k)), ("GV", (4, k)), ("Gb", 4))}
        epoch = C.c_int64(-1)
        assert lib.irs_bpr_get_state(h, *(_lib.ptr(tabs[n], C.c_float) for n in TABLES), C.byref(epoch)) == 0
        assert epoch.value == 0 and (tabs["GU"] == 1.0).all()
        assert lib.irs_bpr_set_state(h, *(_lib.ptr(tabs[n], C.c_float) for n in TABLES), 5) == 0
        assert lib.irs_bpr_run_epochs(h, -1) == 1
    finally:
        assert lib.irs_bpr_destroy(h) == 0 and lib.irs_bpr_destroy(plain) == 0


def test_load_state_refuses_another_loss_or_max_sampled(X_small):
    import io
    import pickle

    warp10 = BPRFMTrainer(X_small, 4, 0.0, 0.0, loss="warp", max_sampled=10)
    buf = io.BytesIO()
    warp10.save_state(buf)
    BPRFMTrainer(X_small, 4, 0.0, 0.0, loss="warp", max_sampled=10).load_state(io.BytesIO(buf.getvalue()))
    for other in (dict(loss="warp", max_sampled=9), dict(loss="bpr")):
        with pytest.raises(ValueError, match="trained with"):
            BPRFMTrainer(X_small, 4, 0.0, 0.0, **other).load_state(io.BytesIO(buf.getvalue()))
    bpr = BPRFMTrainer(X_small, 4, 0.0, 0.0)
    buf = io.BytesIO()
    bpr.save_state(buf)
    with pytest.raises(ValueError, match="trained with"):
        warp10.load_state(io.BytesIO(buf.getvalue()))
    # a state pickled before the trainer knew a loss is a BPR state
    old = pickle.loads(buf.getvalue())
    for key in ("loss", "max_sampled"):
        del old["hyper"][key]
    bpr.load_state(io.BytesIO(pickle.dumps(old)))
    with pytest.raises(ValueError, match="trained with"):
        warp10.load_state(io.BytesIO(pickle.dumps(old)))


# ---- the restatement ----------------------------------------------------------------------------------------------
def test_restatement_step_by_hand():
    """two positions on one user at K = 1, 3 candidates: the first finds its violation at t = 2, the second none.
    Written out: only the first position's three rows move, with the weight of t = 2; G is read before it is updated"""
    state = dict(U=np.array([[0.5], [9.0]]), V=np.array([[1.0], [-3.0], [2.0], [4.0]]), b=np.array([0.1, 0.0, -0.2, 7.0]),
                 GU=np.array([[4.0], [2.0]]), GV=np.full((4, 1), 1.0), Gb=np.array([1.0, 1.0, 4.0, 5.0]))
    # position 0: u = 0, i = 0: x+ = 0.6; candidates 1 (x- = -1.5: no), 2 (x- = 0.8 > -0.4: yes), 3 (not examined)
    # position 1: u = 0, i = 3: x+ = 9.0; candidates 1, 2, 0: x- = -1.5, 0.8, 0.6, none above 8
    users, pos, cand = [0, 0], [0, 3], [[1, 2, 3], [1, 2, 0]]
    neg, tries, margins = warp_search(state, users, pos, cand)
    assert neg.tolist() == [2, -1] and tries.tolist() == [2, 3]
    np.testing.assert_allclose(margins[0, :2], [-1.5 - (0.6 - 1), 0.8 - (0.6 - 1)], rtol=1e-15)
    assert np.isnan(margins[0, 2]) and not np.isnan(margins[1]).any() and (margins[1] < 0).all()
    n_items = 4
    w = math.log(3 // 2)  # floor((4 - 1) / 2) = 1: weight 0 - so take 9 items' weights below
    assert w == 0.0 and warp_weights(n_items, 3).tolist() == [math.log(3), 0.0, 0.0]
    lr, ua, ia = 0.5, 0.1, 0.2
    new = warp_step(state, users, pos, cand, ua, ia, lr, n_items=9)
    w = math.log(4)  # floor((9 - 1) / 2)
    assert warp_weights(9, 3).tolist() == [math.log(8), math.log(4), math.log(2)]
    gU = -w * (1.0 - 2.0) + ua * 0.5
    assert new["U"][0, 0] == pytest.approx(0.5 - lr * gU / 2.0, rel=1e-15) and new["GU"][0, 0] == pytest.approx(4 + gU * gU)
    g0 = -w * 0.5 + ia * 1.0  # item 0: the positive
    assert new["V"][0, 0] == pytest.approx(1.0 - lr * g0, rel=1e-15) and new["GV"][0, 0] == pytest.approx(1 + g0 * g0)
    g2 = w * 0.5 + ia * 2.0  # item 2: the violating candidate
    assert new["V"][2, 0] == pytest.approx(2.0 - lr * g2, rel=1e-15)
    gb2 = w + ia * -0.2
    assert new["b"][2] == pytest.approx(-0.2 - lr * gb2 / 2.0, rel=1e-15) and new["Gb"][2] == pytest.approx(4 + gb2 * gb2)
    gb0 = -w + ia * 0.1
    assert new["b"][0] == pytest.approx(0.1 - lr * gb0, rel=1e-15)
    # the examined but not chosen item 1, the second position's positive 3 and the other user keep their values: a
    # position without a violation touches no row (no L2 term either)
    for n, row in (("U", 1), ("V", 1), ("V", 3), ("b", 1), ("b", 3), ("GU", 1), ("GV", 1), ("GV", 3), ("Gb", 3)):
        assert new[n][row] == state[n][row], (n, row)
    assert state["U"][0, 0] == 0.5  # (the input is not changed)
    # float32 takes (j, t) from the float64 search and runs the update in float32
    new32 = warp_step(state, users, pos, cand, ua, ia, lr, np.float32, n_items=9)
    assert new32["U"].dtype == np.float32 and new32["U"][0, 0] == pytest.approx(new["U"][0, 0], rel=1e-6)
    # a batch in which nothing violates changes nothing
    same = warp_step(state, [0], [3], [[1, 2, 0]], ua, ia, lr)
    assert all((same[n] == state[n]).all() for n in TABLES)


_fits = {}


def restatement_fit():
    """K = 16, batch 1024, 20 epochs, seed 42, max_sampled = 10 on the planted split (once)"""
    if "f" not in _fits:
        X_train, _ = planted_split()
        stats = []
        _fits["f"] = (warp_fit(X_train, 16, batch_size=1024, epochs=20, seed=42, max_sampled=10, stats=stats), stats)
    return _fits["f"]


def test_restatement_learns_the_planted_groups():
    X_train, X_test = planted_split()
    state, stats = restatement_fit()
    warp = ndcg_at(scores(state), X_train, X_test)
    pop = ndcg_at(np.repeat(np.asarray(X_train.sum(axis=0)), 600, axis=0), X_train, X_test)
    print("nDCG@20 on the planted split: WARP restatement", warp, "TopPop", pop)
    print("mean tries, share without a violation, max |theta| per epoch:", [tuple(round(v, 3) for v in s) for s in stats])
    assert warp >= 0.25 and pop <= 0.05 and warp >= 3.0 * pop
    assert state["epoch"] == 20 and all(np.isfinite(state[n]).all() for n in TABLES)
    assert stats[-1][0] > stats[0][0] >= 1.0  # the search gets longer as the fit learns
    assert max(s[2] for s in stats) < 16.0  # (far inside the cap of 2^8)


def test_operand_rules_recognise_a_warp_model():
    """a WARPFMRecommender whose trainer holds the restatement's fit is a "factors" model of K + 1 columns to the
    evaluator and to the serving layer (no device needed: the handle has not been uploaded)"""
    from irspack_amd.evaluation import Evaluator
    from irspack_amd.serving import model_operands

    X_train, _ = planted_split()
    state, _ = restatement_fit()
    model = WARPFMRecommender(X_train, n_components=16, batch_size=1024, train_epochs=20)
    assert model_operands(model) is None  # (not trained)
    model.start_learning()
    assert model.trainer.hyper["loss"] == "warp"
    model.trainer.set_state(state)
    U32, V32, b32 = (state[n].astype(np.float32) for n in ("U", "V", "b"))
    kind, (users, items) = model_operands(model)
    assert kind == "factors" and users.shape == (600, 17) and items.shape == (17, 400)
    np.testing.assert_array_equal(users, np.concatenate([U32, np.ones((600, 1), np.float32)], axis=1))
    np.testing.assert_array_equal(items, np.concatenate([V32, b32[:, None]], axis=1).T)
    ev = Evaluator.__new__(Evaluator)
    ev.fused = True
    fu, fi = ev._factor_operands(model)
    assert fu is users and fi.shape == (400, 17) and fi.flags.c_contiguous
    np.testing.assert_allclose(model.get_score_block(10, 30), (users @ items)[10:30], rtol=0, atol=1e-5)


# ---- what the inputs of the GPU tests promise -------------------------------------------------------------------------
def test_inputs_of_the_gpu_search_test():
    """in the float64 restatement no examined candidate's margin is within 1e-9 of zero, and at max_sampled = 10 first
    violations at t = 1, at t >= 2 and no violation each make up at least 5 % of the positions, for every K"""
    users, pos, cand = search_batch()
    assert SEARCH_SIZES == [1, 63, 64, 65, 1000] and (cand[:20] == cand[:20, :1]).all()
    for k in K_LIST:
        state = random_state(k, 200 + k)
        for n in ("U", "V", "b"):
            assert np.abs(state[n]).max() < 256 and state[n].dtype == np.float32
        for max_sampled in (1, 3, 10):
            neg, tries, margins = warp_search(state, users, pos, cand[:, :max_sampled])
            assert np.nanmin(np.abs(margins)) > 1e-9, (k, max_sampled)
            assert ((neg >= 0) | (tries == max_sampled)).all()
        shares = [float(((neg >= 0) & (tries == 1)).mean()), float(((neg >= 0) & (tries >= 2)).mean()),
                  float((neg < 0).mean())]
        print(f"K={k}: first violation at t = 1 / t >= 2 / none: {shares}")
        assert min(shares) >= 0.05, (k, shares)
        assert len(set(tries[neg >= 0].tolist())) >= 6  # (many trip counts in one wave)


def test_inputs_of_the_gpu_batch_test():
    """every batch's margins are away from zero - by 1e-9 where the batch starts from the given state, by 1e-5 where
    it starts from a state the device computed itself (the second and third batch of a row) -, no parameter comes
    near the cap, and the special cases are what their names say"""
    for k in K_LIST:
        cases = step_cases(k)
        assert len(cases) == 10
        for name, (start, runs) in cases.items():
            s64 = start
            for nth, (users, pos, cand) in enumerate(runs):
                assert cand.shape == (users.size, 10) and pos.shape == users.shape
                neg, tries, margins = warp_search(s64, users, pos, cand)
                assert np.nanmin(np.abs(margins)) > (1e-9 if nth == 0 else 1e-5), (k, name, nth)
                assert (neg >= 0).any() == (name != "no violation"), (k, name)
                s64 = warp_step(s64, users, pos, cand, 0.1, 0.1, LR)
            assert max(float(np.abs(s64[n]).max()) for n in ("U", "V", "b")) < 128.0, (k, name)
        assert [r[0].size for r in cases["three batches in a row"][1]] == [65, 257, 9]
        u, i, c = cases["one item as positive and as the only candidate"][1][0]
        assert (i[:60] == 11).all() and (c[60:] == 11).all() and not (i[60:] == 11).any()
        u, i, c = cases["identical positions"][1][0]
        assert u.size == 300 and len(set(u.tolist())) == len(set(i.tolist())) == 1 and (c == c[0]).all()
        state, (users, pos, cand) = five_item_case(k)
        neg, tries, margins = warp_search(state, users, pos, cand)
        assert (neg == 4).all() and (tries == 3).all() and np.nanmin(np.abs(margins)) > 1.0
    state, (users, pos, cand) = many_item_case()
    neg, tries, margins = warp_search(state, users, pos, cand)
    assert (tries == 1).all() and (neg == cand[:, 0]).all() and np.nanmin(np.abs(margins)) > 1.0
    assert state["V"].shape == (30000, 4) and warp_weights(30000, 10)[0] == 10.0


_HOST_CXX = shutil.which("g++") or shutil.which("clang++")


@pytest.mark.skipif(_HOST_CXX is None, reason="needs a host C++ compiler")
def test_warp_host_preparation_under_address_and_ub_sanitizers(tmp_path):
    """the WARP part of irspack_amd/csrc/bpr_host_prep.hpp - the candidate stream on the host against a scan, its
    prefix property and key, the scale bound, the weight table, the checks - in a program of its own
    (tests/host/warp_host_prep_main.cpp), every report fatal"""
    exe = str(tmp_path / "warp_host_prep_main")
    src = os.path.join(ROOT, "tests", "host", "warp_host_prep_main.cpp")
    subprocess.check_call([_HOST_CXX, "-std=c++17", "-O1", "-g", "-pthread", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "warp_host_prep ok" in r.stdout
