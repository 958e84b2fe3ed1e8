"""MultVAERecommender without a GPU: the Python surface against the reference's (``recommenders/multvae.py:329-342``),
the C ABI's declarations and its argument checks (all before any device work), the numpy restatement that arbitrates
the GPU tests (``tests/_multvae_restatement.py``) against finite differences and on the planted data, the operand
rule of the serving layer and the evaluator, and ``multvae_host_prep.hpp`` under the sanitizers."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sps

import _multvae_restatement as R
from _bpr_restatement import ndcg_at, planted_split
from irspack_amd.recommenders import MultVAERecommender  # (the parent commit fails here)
from irspack_amd.recommenders.multvae import STATE_TABLES, TABLES, MultVAETrainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = inspect.Parameter.empty
SYMBOLS = ["irs_multvae_create", "irs_multvae_run_epochs", "irs_multvae_order", "irs_multvae_noise",
           "irs_multvae_step_batch", "irs_multvae_gradients", "irs_multvae_get_state", "irs_multvae_set_state",
           "irs_multvae_encode", "irs_multvae_score", "irs_multvae_stats", "irs_multvae_destroy"]


def _params(fn, kind):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values() if p.kind is kind]


def test_recommender_has_the_reference_surface(X_small):
    from irspack_amd import recommenders
    from irspack_amd.recommenders import BaseRecommenderWithEarlyStopping

    assert "MultVAERecommender" in recommenders.__all__
    assert issubclass(MultVAERecommender, BaseRecommenderWithEarlyStopping)
    # the reference's arguments in the reference's order with its defaults; the extensions are keyword-only
    assert _params(MultVAERecommender.__init__, inspect.Parameter.POSITIONAL_OR_KEYWORD) == [
        ("self", EMPTY), ("X_train_all", EMPTY), ("dim_z", 16), ("enc_hidden_dims", 256), ("dec_hidden_dims", None),
        ("dropout_p", 0.5), ("l2_regularizer", 0), ("kl_anneal_goal", 0.2), ("anneal_end_epoch", 50),
        ("minibatch_size", 512), ("train_epochs", 300), ("learning_rate", 1e-3)]
    assert _params(MultVAERecommender.__init__, inspect.Parameter.KEYWORD_ONLY) == [("random_seed", 42), ("device", None)]
    rec = MultVAERecommender(X_small)
    assert (rec.dim_z, rec.enc_hidden_dims, rec.dec_hidden_dims, rec.dropout_p, rec.l2_regularizer, rec.kl_anneal_goal,
            rec.anneal_end_epoch, rec.minibatch_size, rec.train_epochs, rec.learning_rate) == \
        (16, 256, None, 0.5, 0, 0.2, 50, 512, 300, 1e-3)
    assert rec.trainer is None and rec.best_state is None
    for name in ("get_score", "get_score_block", "get_score_cold_user", "factor_tables", "_create_trainer"):
        assert name in vars(MultVAERecommender), name
    for call in (lambda: rec.get_score(np.arange(2)), lambda: rec.get_score_block(0, 2),
                 lambda: rec.get_score_cold_user(X_small), lambda: rec.factor_tables()):
        with pytest.raises(RuntimeError, match="encoder called before training."):
            call()
    with pytest.raises(RuntimeError, match="before initializing the trainer"):
        rec.run_epoch()
    assert "no effect" in MultVAERecommender.__doc__ and "no effect" in MultVAETrainer.__doc__  # (l2_regularizer)


def test_symbols_declared_listed_and_exported():
    from irspack_amd import _lib

    header = open(os.path.join(ROOT, "include", "irspack_amd.h")).read()
    declared = set(re.findall(r"\b(irs_[a-z0-9_]+)\s*\(", header))
    for s in SYMBOLS:
        assert s in declared and s in _lib.EXPORTED_SYMBOLS and s in _lib.ARGTYPES and hasattr(_lib.lib(), s), s
    assert _lib.lib().irs_abi_version() == 4 and _lib.ABI_VERSION == 4  # an additive change
    assert C.sizeof(_lib.MultVaeStatsStruct) == 144
    assert "typedef struct irs_multvae irs_multvae;" in header and "} irs_multvae_stats_t;" in header


# ---- the C ABI's argument checks ----------------------------------------------------------------------------------
BASE = dict(indptr=np.array([0, 2, 3, 3], dtype=np.int64), indices=np.array([0, 2, 1], dtype=np.int32),
            data=np.array([1.0, 0.0, 2.5], dtype=np.float32), cols=4, L=2, H=3, Hd=5, p=0.5, l2=0.0, goal=0.2, end=50,
            mb=2, lr=1e-3, init=None)
SHAPES = R.shapes(4, 3, 2, 5)


def _create(**kw):
    from irspack_amd import _lib

    a = dict(BASE, **kw)
    h = C.c_void_p()
    rows = len(a["indptr"]) - 1
    init = None if a["init"] is None else _lib.ptr_array(a["init"], C.c_float)
    st = _lib.lib().irs_multvae_create(
        rows, a["cols"], _lib.ptr(a["indptr"], C.c_int64), _lib.ptr(a["indices"], C.c_int32),
        _lib.ptr(a["data"], C.c_float), a["L"], a["H"], a["Hd"], a["p"], a["l2"], a["goal"], a["end"], a["mb"], a["lr"],
        42, init, 0, C.byref(h))
    return st, _lib.lib().irs_last_error().decode(), h


def test_create_checks_come_before_device_work():
    """Status 1 (invalid argument) with its message from every check where no device is visible too (a status 2
    there would mean the device was asked first), and no handle comes back."""
    def call(**kw):
        st, msg, h = _create(**kw)
        assert st == 0 or not h.value
        return st, msg

    assert call(indptr=np.array([0, 3, 2, 3], dtype=np.int64)) == (1, "malformed indptr.")
    assert call(cols=2) == (1, "column index out of range.")
    st, msg = call(indices=np.array([2, 2, 1], dtype=np.int32))
    assert st == 1 and "duplicate column index" in msg
    st, msg = call(indices=np.array([2, 0, 1], dtype=np.int32))
    assert st == 1 and "sorted" in msg
    for bad in (np.nan, np.inf):
        st, msg = call(data=np.array([1.0, bad, 1.0], dtype=np.float32))
        assert st == 1 and "non-finite" in msg
    assert call(L=0) == (1, "dim_z must be >= 1.")
    for kw in (dict(H=0), dict(Hd=0)):
        assert call(**kw) == (1, "enc_hidden_dims and dec_hidden_dims must be >= 1.")
    for kw in (dict(H=575), dict(Hd=575)):
        assert call(**kw) == (1, "enc_hidden_dims and dec_hidden_dims must be <= 574.")
    for bad in (-0.1, 1.0, np.nan):
        assert call(p=bad) == (1, "dropout_p must be in [0, 1).")
    assert call(l2=np.inf) == (1, "l2_regularizer must be finite.")
    for bad in (-0.1, np.nan):
        assert call(goal=bad) == (1, "kl_anneal_goal must be finite and >= 0.")
    assert call(end=-1) == (1, "anneal_end_epoch must be >= 0.")
    assert call(mb=0) == (1, "minibatch_size must be >= 1.")
    for bad in (0.0, -1e-3, np.nan, np.inf):
        assert call(lr=bad) == (1, "learning_rate must be finite and > 0.")
    init = [np.full(SHAPES[n], 0.1, dtype=np.float32) for n in TABLES]
    init[6][4, 3] = np.nan
    assert call(init=init) == (1, "an initial table holds a non-finite value.")
    init[6][4, 3] = 0.0
    assert call(init=init[:7] + [None]) == (1, "the initial tables must not be null.")
    st, msg, h = _create(H=574, Hd=574, p=0.0, l2=3.0)  # (the limits themselves are accepted)
    assert st == 0 and h.value, msg
    from irspack_amd import _lib
    assert _lib.lib().irs_multvae_destroy(h) == 0


def test_state_batch_and_row_checks_come_before_device_work():
    """a handle is made without a device; what it is handed is checked before the device is asked for"""
    from irspack_amd import _lib

    lib = _lib.lib()
    st, msg, h = _create()
    assert st == 0 and h.value, msg
    try:
        stats = _lib.MultVaeStatsStruct()
        assert lib.irs_multvae_stats(h, C.byref(stats)) == 0
        assert (stats.n_updates, stats.epoch, stats.batches_per_epoch, stats.scale_log2) == (0, 0, 2, 44)
        assert stats.dh2_slab >= 16 and stats.dw4_slab >= 16 and stats.klc_next == 0.0
        # the initial state is readable without a device: zero biases and moments, truncated-normal weights
        tabs = {n: np.full(SHAPES[n[-2:]], 7.0, dtype=np.float32) for n in STATE_TABLES}
        updates, epoch = C.c_int64(-1), C.c_int64(-1)

        def get():
            return lib.irs_multvae_get_state(h, _lib.ptr_array([tabs[n] for n in STATE_TABLES], C.c_float),
                                             C.byref(updates), C.byref(epoch))

        assert get() == 0 and (updates.value, epoch.value) == (0, 0)
        for n in TABLES:
            assert not tabs["m" + n].any() and not tabs["v" + n].any()
            if n.startswith("b"):
                assert not tabs[n].any()
            else:
                bound = 2.0 / np.sqrt(SHAPES[n][0])
                assert (np.abs(tabs[n]) <= bound * (1 + 1e-6)).all() and np.unique(tabs[n]).size == tabs[n].size

        def set_state(updates=3, epoch=1, drop=None, **kw):
            t = {n: np.zeros(SHAPES[n[-2:]], dtype=np.float32) for n in STATE_TABLES}
            for n, (at, v) in kw.items():
                t[n][at] = v
            arrays = [None if n == drop else t[n] for n in STATE_TABLES]
            return (lib.irs_multvae_set_state(h, _lib.ptr_array(arrays, C.c_float), updates, epoch),
                    lib.irs_last_error().decode())

        for n, at in (("W1", (3, 2)), ("b4", 3), ("mW2", (0, 0)), ("vb3", 4)):
            for bad in (np.nan, np.inf):
                assert set_state(**{n: (at, bad)}) == (1, "the state holds a non-finite value.")
        assert set_state(vW4=((4, 3), -1e-9)) == (1, "the second moments of the state must be >= 0.")
        assert set_state(drop="mb2") == (1, "the state arrays must not be null.")
        assert set_state(updates=-1) == (1, "n_updates must be >= 0.")
        assert set_state(epoch=-1) == (1, "epoch must be >= 0.")
        # (nothing of the refused states was kept)
        assert get() == 0 and (updates.value, epoch.value) == (0, 0) and tabs["W1"].any()
        assert set_state(updates=5, epoch=2, W1=((0, 0), 1.5))[0] == 0
        assert get() == 0 and (updates.value, epoch.value) == (5, 2) and tabs["W1"][0, 0] == 1.5
        assert lib.irs_multvae_stats(h, C.byref(stats)) == 0
        assert stats.klc_next == pytest.approx(0.2 * 5 / (50 * 3 / 2), rel=1e-12)

        def step(users, keep=None, eps=None, klc=0.1):
            u = np.array(users, dtype=np.int32)
            return (lib.irs_multvae_step_batch(
                h, len(users), _lib.ptr(u, C.c_int32), None if keep is None else _lib.ptr(np.array(keep, np.uint8), C.c_uint8),
                None if eps is None else _lib.ptr(np.array(eps, np.float32), C.c_float), klc, None, None),
                lib.irs_last_error().decode())

        assert step([]) == (1, "a batch must have at least one row.")
        assert step([0, 3]) == (1, "a batch row's user is out of range.")
        assert step([-1]) == (1, "a batch row's user is out of range.")
        assert step([0], klc=-1.0) == (1, "klc must be finite and >= 0.")
        assert step([0], klc=np.nan) == (1, "klc must be finite and >= 0.")
        assert step([0, 1], keep=[1, 0, 2]) == (1, "keep must hold 0 or 1.")
        assert step([0], eps=[0.0, np.inf]) == (1, "eps holds a non-finite value.")

        def rows(call, indptr, indices, data):
            out = np.zeros(64, dtype=np.float32)
            args = (h, len(indptr) - 1, _lib.ptr(np.array(indptr, np.int64), C.c_int64),
                    _lib.ptr(np.array(indices, np.int32), C.c_int32), _lib.ptr(np.array(data, np.float32), C.c_float))
            st = call(*args, _lib.ptr(out, C.c_float), _lib.ptr(out, C.c_float)) if call is lib.irs_multvae_encode \
                else call(*args, _lib.ptr(out, C.c_float))
            return st, lib.irs_last_error().decode()

        for call in (lib.irs_multvae_encode, lib.irs_multvae_score):
            assert rows(call, [0, 2], [0, 4], [1, 1]) == (1, "column index out of range.")
            assert rows(call, [0, 2, 1], [0, 1], [1, 1]) == (1, "malformed indptr.")
            assert "duplicate" in rows(call, [0, 2], [1, 1], [1, 1])[1]
            assert "non-finite" in rows(call, [0, 1], [1], [np.nan])[1]
            assert rows(call, [0], [], [])[0] == 0  # (no rows: nothing to do)
        assert lib.irs_multvae_order(h, 0, 2, 2, None) == 1  # (3 positions in an epoch)
        assert lib.irs_multvae_order(h, -1, 0, 0, None) == 1
        users = np.zeros(3, dtype=np.int32)
        assert lib.irs_multvae_order(h, 0, 0, 3, _lib.ptr(users, C.c_int32)) == 0 and sorted(users.tolist()) == [0, 1, 2]
        assert lib.irs_multvae_run_epochs(h, -1) == 1
        assert lib.irs_multvae_noise(h, -1, 0, None, None, None) == 1
        assert lib.irs_multvae_gradients(h, None) == 1
    finally:
        assert lib.irs_multvae_destroy(h) == 0


# ---- the restatement ----------------------------------------------------------------------------------------------
def test_restatement_gradients_against_central_differences():
    """the yardstick checking itself: float64 gradients of a tiny model against (loss(+h) - loss(-h)) / 2 h on every
    element of every table, with dropout, non-binary values, an empty row and klc > 0"""
    rng = np.random.RandomState(0)
    I, H, L, Hd, n, p, klc = 7, 4, 2, 3, 5, 0.5, 0.2
    state = R.initial_state(I, H, L, Hd, rng)
    for name in TABLES:
        if name.startswith("b"):
            state[name] = 0.1 * rng.standard_normal(state[name].shape)
    x = (rng.random_sample((n, I)) < 0.5) * rng.choice([1.0, 2.0, 0.5], (n, I))
    x[1] = 0
    keep = rng.random_sample((n, I)) >= p
    eps = rng.standard_normal((n, L))
    grads, f = R.gradients(state, x, keep, eps, p, klc)
    assert float(f["nll"] + klc * f["kl"]) == pytest.approx(float(R.loss(state, x, keep, eps, p, klc)), rel=1e-15)
    h = 1e-6
    for name in TABLES:
        num = np.zeros_like(state[name])
        for at in np.ndindex(*state[name].shape):
            up, down = dict(state), dict(state)
            up[name], down[name] = state[name].copy(), state[name].copy()
            up[name][at] += h
            down[name][at] -= h
            num[at] = (R.loss(up, x, keep, eps, p, klc) - R.loss(down, x, keep, eps, p, klc)) / (2 * h)
        np.testing.assert_allclose(grads[name], num, rtol=1e-6, atol=1e-9, err_msg=name)
    # Adam by hand on one element, first and second update
    one = R.adam_step(state, grads, 0.01)
    g = grads["W2"][1, 2]
    assert one["mW2"][1, 2] == pytest.approx(0.1 * g) and one["vW2"][1, 2] == pytest.approx(0.001 * g * g)
    assert one["W2"][1, 2] == pytest.approx(state["W2"][1, 2] - 0.01 * g / (abs(g) + 1e-8), rel=1e-12)
    two = R.adam_step(one, grads, 0.01)
    m, v = 0.9 * 0.1 * g + 0.1 * g, 0.999 * 0.001 * g * g + 0.001 * g * g
    assert two["W2"][1, 2] == pytest.approx(one["W2"][1, 2] - 0.01 * (m / 0.19) / (np.sqrt(v / (1 - 0.999 ** 2)) + 1e-8), rel=1e-12)
    assert two["n_updates"] == 2 and state["n_updates"] == 0
    assert R.step(state, x, keep, eps, p, klc, 0.01, np.float32)[0]["W1"].dtype == np.float32
    # evaluation: log-softmax rows, no noise
    s = R.eval_scores(state, x)
    np.testing.assert_allclose(np.exp(s).sum(axis=1), 1.0, rtol=1e-12)


_fits = {}


def restatement_fit():
    if "f" not in _fits:
        _fits["f"] = R.fit(planted_split()[0], dim_z=16, enc_hidden=64, minibatch_size=100, learning_rate=1e-2, epochs=10)
    return _fits["f"]


def test_restatement_learns_the_planted_groups():
    X_train, X_test = planted_split()
    state = restatement_fit()
    vae = ndcg_at(R.eval_scores(state, np.asarray(X_train.todense())), X_train, X_test)
    pop = ndcg_at(np.repeat(np.asarray(X_train.sum(axis=0)), 600, axis=0), X_train, X_test)
    print("nDCG@20 on the planted split: restatement", vae, "TopPop", pop)
    assert vae >= 3.0 * pop and vae >= 0.25 and pop == pytest.approx(0.0335, abs=5e-5)
    assert (state["epoch"], state["n_updates"]) == (10, 60) and all(np.isfinite(state[n]).all() for n in STATE_TABLES)


def test_operand_rules_recognise_a_multvae_model():
    """a model whose trainer holds the restatement's fit is a "factors" model of Hd + 2 columns to the serving layer
    and to the evaluator (the encoder is the restatement's here: no device)"""
    from irspack_amd.evaluation import Evaluator
    from irspack_amd.serving import model_operands

    X_train, _ = planted_split()
    state = restatement_fit()
    model = MultVAERecommender(X_train, enc_hidden_dims=64, dim_z=16, minibatch_size=100, learning_rate=1e-2)
    assert model_operands(model) is None  # (not trained)
    model.start_learning()
    model.trainer.set_state(state)
    assert model.trainer.get_state()["W4"].tobytes() == state["W4"].astype(np.float32).tobytes()
    calls = []

    def encode(X):
        calls.append(X.shape)
        h2, logit = R.eval_hidden(state, np.asarray(sps.csr_matrix(X).todense()))
        mx = logit.max(axis=1)
        return h2.astype(np.float32), (mx + np.log(np.exp(logit - mx[:, None]).sum(axis=1))).astype(np.float32)

    model.trainer.encode = encode
    kind, (users, items) = model_operands(model)
    assert kind == "factors" and users.shape == (600, 66) and items.shape == (66, 400)
    assert users.dtype == items.dtype == np.float32 and users.flags.c_contiguous and items.flags.c_contiguous
    assert (users[:, 64] == 1).all() and (items[65] == 1).all()
    np.testing.assert_array_equal(items[:64], state["W4"].astype(np.float32))
    np.testing.assert_array_equal(items[64], state["b4"].astype(np.float32))
    # the product of the two tables is the log-softmax of the rows
    want = R.eval_scores(state, np.asarray(X_train.todense()))
    np.testing.assert_allclose(users.astype(np.float64) @ items.astype(np.float64), want, rtol=0, atol=2e-5)
    assert model_operands(model)[1][0] is users and calls == [(600, 400)]  # (held per state)
    ev = Evaluator.__new__(Evaluator)
    ev.fused = True
    fu, fi = ev._factor_operands(model)
    assert fu is users and fi.shape == (400, 66) and fi.flags.c_contiguous
    ev.fused = False
    assert ev._factor_operands(model) is None
    # a subclass that scores differently is left to the block loop; a new state hands out new tables
    Other = type("Other", (MultVAERecommender,), {"get_score_block": lambda self, b, e: None})
    other = Other(X_train, enc_hidden_dims=64)
    other.trainer = model.trainer
    ev.fused = True
    assert model_operands(other) is None and ev._factor_operands(other) is None
    model.trainer.set_state(dict(state, b4=state["b4"] + 1.0))
    assert model_operands(model)[1][1][64, 0] == np.float32(state["b4"][0] + 1.0) and len(calls) == 2


_HOST_CXX = shutil.which("g++") or shutil.which("clang++")


@pytest.mark.skipif(_HOST_CXX is None, reason="needs a host C++ compiler")
def test_multvae_host_preparation_under_address_and_ub_sanitizers(tmp_path):
    """irspack_amd/csrc/multvae_host_prep.hpp - the arena's layout and packing, the argument checks, the schedule,
    the order as a bijection, the noise's statistics, the initial tables, the scale bound, the slabs - in a program
    of its own (tests/host/multvae_host_prep_main.cpp), every report fatal."""
    exe = str(tmp_path / "multvae_host_prep_main")
    src = os.path.join(ROOT, "tests", "host", "multvae_host_prep_main.cpp")
    subprocess.check_call([_HOST_CXX, "-std=c++17", "-O1", "-g", "-pthread", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "multvae_host_prep ok" in r.stdout
