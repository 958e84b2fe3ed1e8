"""MultVAERecommender on the device: single updates and runs of updates against the numpy restatement
(``tests/_multvae_restatement.py``) judged by float64 (the inputs: ``tests/_multvae_cases.py``), a batch larger than
the handle was sized for and a smaller one after it, the divergence flag, byte-identical reruns and restores, the
order and the noise, the annealing schedule, scoring (in ragged chunks, at large logits), quality on the planted data,
early stopping, and the fitted model through the fused evaluator and the serving layer."""
import io

import numpy as np
import pytest
import scipy.sparse as sps

import _multvae_cases as K
import _multvae_restatement as R
from _bpr_restatement import ndcg_at, planted_split
from _multvae_cases import LR, batch_matrix, explicit_noise, random_start
from conftest import assert_float64_bar
from irspack_amd.recommenders import MultVAERecommender, TopPopRecommender
from irspack_amd.recommenders.multvae import STATE_TABLES, TABLES, MultVAETrainer

pytestmark = pytest.mark.gpu


def same_bytes(a, b):
    return (a["epoch"], a["n_updates"]) == (b["epoch"], b["n_updates"]) and \
        all(a[n].tobytes() == b[n].tobytes() for n in STATE_TABLES)


def make_trainer(X, H, Hd, L, p, **kw):
    args = dict(l2_regularizer=0.0, kl_anneal_goal=0.2, anneal_end_epoch=2, minibatch_size=max(X.shape[0], 1),
                learning_rate=LR)
    args.update(kw)
    return MultVAETrainer(X, L, H, Hd, p, **args)


def compare_update(trainer, X, start, users, keep, eps, p, klc, what):
    """one update from ``start`` on the device and in the restatement (float32, float64); every gradient table and
    every table and moment of the new state, row by row, under the project's float64 bar"""
    trainer.set_state(start)
    nll, kl = trainer.step_batch(users, keep if p > 0 else None, eps, klc)
    x = np.asarray(X[users].todense())
    dense = R.dense_keep(X, users, keep)
    new64, g64, f64 = R.step(start, x, dense, eps, p, klc, LR, np.float64)
    new32, g32, _ = R.step(start, x, dense, eps, p, klc, LR, np.float32)
    assert np.isfinite([nll, kl]).all()
    assert nll == pytest.approx(float(f64["nll"]), rel=1e-4, abs=1e-6) and kl == pytest.approx(float(f64["kl"]), rel=1e-4, abs=1e-6)
    got_g, got = trainer.gradients(), trainer.get_state()
    assert got["n_updates"] == start["n_updates"] + 1
    for n in TABLES:
        rows = (1, -1) if n.startswith("b") else (g64[n].shape[0], -1)
        assert got_g[n].dtype == np.float32 and np.isfinite(got_g[n]).all(), (what, n)
        assert_float64_bar(got_g[n].reshape(rows), g32[n].reshape(rows), g64[n].reshape(rows), f"{what} d{n}",
                           test="multvae_update")
        for pre in ("", "m", "v"):
            assert_float64_bar(got[pre + n].reshape(rows), new32[pre + n].reshape(rows), new64[pre + n].reshape(rows),
                               f"{what} {pre}{n}", test="multvae_update")
    return got, new64


def slabs():
    probe = make_trainer(sps.csr_matrix(np.ones((2, 70), dtype=np.float32)), 4, 4, 2, 0.0)
    st = probe.stats()
    probe.close()
    return int(st["dh2_slab"]), int(st["dw4_slab"])


def update_cases():
    """``_multvae_cases.update_cases`` at the slab sizes that stats report"""
    return K.update_cases(*slabs())


@pytest.mark.parametrize("case", range(20))
def test_one_update_against_the_restatement(case):
    I, H, Hd, L, n, p, klc = update_cases()[case]
    dh2, dw4 = slabs()
    X, users, keep, eps, start = K.case_inputs(update_cases()[case], case, wide=False)
    trainer = make_trainer(X, H, Hd, L, p)
    st = trainer.stats()
    assert (st["dh2_slab"], st["dw4_slab"]) == (dh2, dw4)
    got, _ = compare_update(trainer, X, start, users, keep, eps, p, klc, f"case {case} {update_cases()[case]}")
    assert got["W1"][3].tobytes() != start["W1"][3].tobytes()  # (Adam moves a row with a zero gradient by its momentum)
    trainer.close()


@pytest.mark.parametrize("case", range(12))
def test_wide_update_against_the_restatement(case):
    """``_multvae_cases.wide_cases``: two and three passes of the sparse kernels, two of the latent kernel, five tiles
    of 2 L and of Hd + 1, n and I at a slab, a tile and a BK step and one past, 64 dh2 slabs and the doubled slab"""
    dh2, dw4 = slabs()
    shape = K.wide_cases(dh2, dw4)[case]
    I, H, Hd, L, n, p, klc = shape
    X, users, keep, eps, start = K.case_inputs(shape, case, wide=True)
    trainer = make_trainer(X, H, Hd, L, p)
    st = trainer.stats()
    assert (st["dh2_slab"], st["dw4_slab"]) == (K.dh2_slab(I), dw4) and dh2 == K.dh2_slab(70)
    assert (-(-I // st["dh2_slab"]), -(-n // st["dw4_slab"])) == K.WIDE_SLABS[case][::2]
    got, _ = compare_update(trainer, X, start, users, keep, eps, p, klc, f"wide case {case} {shape}")
    assert got["W1"][3].tobytes() != start["W1"][3].tobytes()  # (Adam moves a row with a zero gradient by its momentum)
    trainer.close()


def test_a_small_batch_after_a_larger_one():
    """a handle sized for 8 rows takes 300 (the work buffers regrow; two dW4 slabs and 44 rows), then 5, the empty and
    the full row among them, with rows 5 .. 299 of every work buffer left over from before: both against the
    restatement, and both byte for byte what a handle sized for 300 rows from the start gives - the bytes of a step
    depend on the tiling, and the tiling on n, I and the widths, not on the capacity"""
    c = K.REGROW
    X, batches = K.regrowth_inputs()
    grown = make_trainer(X, c["H"], c["Hd"], c["L"], c["p"], minibatch_size=c["first_capacity"])
    sized = make_trainer(X, c["H"], c["Hd"], c["L"], c["p"], minibatch_size=c["rows"])
    for users, keep, eps, start in batches:
        got, _ = compare_update(grown, X, start, users, keep, eps, c["p"], c["klc"], f"regrown, {users.size} rows")
        grads = grown.gradients()
        sized.set_state(start)
        sized.step_batch(users, keep, eps, c["klc"])
        assert same_bytes(got, sized.get_state())
        other = sized.gradients()
        assert all(grads[n].tobytes() == other[n].tobytes() for n in TABLES)
    grown.close()
    sized.close()


def test_softmax_at_large_logits():
    """[W4; b4] scaled so that the logits span about +-80: the loss and the gradients are finite and inside the bar"""
    I, H, Hd, L, n, p, klc = 257, 33, 33, 3, 40, 0.5, 0.2
    X = batch_matrix(n, I, 7)
    start = random_start(I, H, L, Hd, 8)
    users = np.arange(n, dtype=np.int32)
    keep, eps = explicit_noise(X, users, L, p, 9)
    logit = R.forward(start, np.asarray(X.todense()), R.dense_keep(X, users, keep), eps, p)
    span = float(np.abs(logit["h2"] @ start["W4"].astype(np.float64) + start["b4"]).max())
    start["W4"] = (start["W4"] * (80.0 / span)).astype(np.float32)
    start["b4"] = (start["b4"] * (80.0 / span)).astype(np.float32)
    f = R.forward(start, np.asarray(X.todense()), R.dense_keep(X, users, keep), eps, p)
    lg = f["h2"] @ start["W4"].astype(np.float64) + start["b4"]
    print("logits span", float(lg.min()), float(lg.max()))
    assert lg.max() > 60 and lg.min() < -60
    trainer = make_trainer(X, H, Hd, L, p)
    compare_update(trainer, X, start, users, keep, eps, p, klc, "large logits")
    trainer.close()


def test_five_consecutive_updates():
    """from zero moments and update 0 with the device's own noise and the schedule's klc growing from 0: bias
    corrections, moments and the annealing"""
    I, H, Hd, L, n, p = 257, 33, 64, 16, 60, 0.5
    X = batch_matrix(n, I, 17)
    trainer = make_trainer(X, H, Hd, L, p, minibatch_size=20, anneal_end_epoch=1)
    start = random_start(I, H, L, Hd, 18, moments=False)
    trainer.set_state(start)
    ref64, ref32 = start, start
    for t in range(5):
        users = trainer.order(t // 3, 20 * (t % 3), 20)
        keep, eps = trainer.noise(t, users)
        klc = trainer.stats()["klc_next"]
        assert klc == pytest.approx(0.2 * min(1.0, t / 3.0), rel=1e-12)
        trainer.step_batch(users, keep, eps, klc)
        x, dense = np.asarray(X[users].todense()), R.dense_keep(X, users, keep)
        ref64 = R.step(ref64, x, dense, eps, p, klc, LR, np.float64)[0]
        ref32 = R.step(ref32, x, dense, eps, p, klc, LR, np.float32)[0]
    got = trainer.get_state()
    assert got["n_updates"] == 5
    for n in STATE_TABLES:
        rows = (1, -1) if n[-2] == "b" else (got[n].shape[0], -1)
        assert_float64_bar(got[n].reshape(rows), ref32[n].reshape(rows), ref64[n].reshape(rows), f"five updates {n}",
                           test="multvae_five_updates")
    trainer.close()


def test_divergence_is_reported_and_set_state_recovers():
    """One batch row, p = 0, klc = 0: the gradients are linear in the row's stored values, and the largest
    contribution to the fixed-point sums of W1 is max |db1| (``_multvae_cases.divergence_inputs``).  User 0 is the
    row scaled to bring that into (64, 128]: a legal step, summed correctly at scale 2^44.  User 1 is the row scaled
    to [512, 1024): past the cap of 2^8, a reported error with every value finite.  ``set_state`` clears the flag and
    the sums: the next legal step gives the bytes of a fresh handle."""
    c, d = K.DIVERGENCE, K.divergence_inputs()
    X, start, keep, eps = d["X"], d["start"], d["keep"], d["eps"]
    legal, diverging = np.array([0], dtype=np.int32), np.array([1], dtype=np.int32)
    fresh = make_trainer(X, c["H"], c["Hd"], c["L"], c["p"])
    assert fresh.stats()["scale_log2"] == 44
    want, _ = compare_update(fresh, X, start, legal, keep, eps, c["p"], c["klc"], "a contribution of 2^6 .. 2^7")
    want_g = fresh.gradients()
    top = float(np.abs(want_g["b1"]).max())
    print("max |db1| of the legal step on the device:", top)
    assert 64.0 < top <= 128.0
    trainer = make_trainer(X, c["H"], c["Hd"], c["L"], c["p"])
    trainer.set_state(start)
    with pytest.raises(RuntimeError, match="diverged"):
        trainer.step_batch(diverging, None, eps, c["klc"])
    with pytest.raises(RuntimeError, match="diverged"):  # (the flag stays up: the state is no longer usable)
        trainer.step_batch(legal, None, eps, c["klc"])
    trainer.set_state(start)
    trainer.step_batch(legal, None, eps, c["klc"])
    assert same_bytes(want, trainer.get_state())
    got_g = trainer.gradients()
    assert all(got_g[n].tobytes() == want_g[n].tobytes() for n in TABLES)
    fresh.close()
    trainer.close()


# ---- reproducibility ----------------------------------------------------------------------------------------------
def planted_trainer(**kw):
    X_train, _ = planted_split()
    args = dict(dim_z=16, enc_hidden_dim=64, dec_hidden_dim=None, dropout_p=0.5, l2_regularizer=0.0, kl_anneal_goal=0.2,
                anneal_end_epoch=3, minibatch_size=128, learning_rate=1e-2, random_seed=3)
    args.update(kw)
    return MultVAETrainer(X_train, **args)


def test_same_seed_same_bytes_and_restores_continue_identically():
    a, b = planted_trainer(), planted_trainer()
    assert a.n_users % 128 != 0  # (the last batch is short)
    a.run_epochs(4)
    for _ in range(4):
        b.run_epoch()
    want = a.get_state()
    assert (want["epoch"], want["n_updates"]) == (4, 4 * 5) and same_bytes(want, b.get_state())
    assert all(np.isfinite(want[n]).all() for n in STATE_TABLES)
    other = planted_trainer(random_seed=4)
    assert other.get_state()["W1"].tobytes() != planted_trainer().get_state()["W1"].tobytes()
    other.run_epochs(4)
    assert not (other.get_state()["W4"] == want["W4"]).all()
    # save after two epochs -> restore into a fresh trainer -> two more
    c = planted_trainer()
    c.run_epochs(2)
    buf = io.BytesIO()
    c.save_state(buf)
    d = planted_trainer()
    d.load_state(io.BytesIO(buf.getvalue()))
    d.run_epochs(2)
    assert same_bytes(want, d.get_state())
    e = planted_trainer()
    e.set_state(c.get_state())
    e.run_epochs(2)
    assert same_bytes(want, e.get_state())
    with pytest.raises(ValueError, match="trained with"):
        planted_trainer(minibatch_size=127).load_state(io.BytesIO(buf.getvalue()))


# ---- order and noise ------------------------------------------------------------------------------------------------
def test_order_and_noise():
    X_train, _ = planted_split()
    p = 0.3
    trainer = planted_trainer(dropout_p=p, minibatch_size=128)
    n = trainer.n_users
    st = trainer.stats()
    assert st["batches_per_epoch"] == -(-n // 128) and n % 128 != 0
    orders = [trainer.order(e) for e in range(3)]
    for o in orders:
        assert sorted(o.tolist()) == list(range(n))  # a bijection
    assert orders[0].tolist() != orders[1].tolist() != orders[2].tolist()
    cuts = [0, 1, 128, 129, 500, n]
    np.testing.assert_array_equal(np.concatenate([trainer.order(1, a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]), orders[1])
    assert trainer.order(0, 128 * (st["batches_per_epoch"] - 1)).size == n % 128  # the last batch is short
    with pytest.raises(ValueError):
        trainer.order(0, n - 1, 2)
    # the same keys give the same noise from any window
    users = orders[0]
    keep, eps = trainer.noise(5, users)
    deg = np.diff(X_train.indptr)[users]
    assert keep.size == deg.sum() and eps.shape == (n, 16) and set(np.unique(keep)) <= {0, 1}
    k2, e2 = trainer.noise(5, users[100:150])
    at = int(deg[:100].sum())
    np.testing.assert_array_equal(k2, keep[at:at + int(deg[100:150].sum())])
    np.testing.assert_array_equal(e2, eps[100:150])
    k3, e3 = trainer.noise(6, users)
    assert (k3 != keep).any() and (e3 != eps).any()
    # the kept share and the moments of eps, pooled over 8 updates
    keeps, epss = zip(*(trainer.noise(t, users) for t in range(8)))
    kept, N = np.concatenate(keeps), sum(k.size for k in keeps)
    print("kept share", kept.mean(), "of", N)
    assert abs(kept.mean() - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / N)
    e = np.concatenate(epss).astype(np.float64).ravel()
    print("eps mean", e.mean(), "variance", e.var(), "of", e.size)
    assert abs(e.mean()) <= 5 / np.sqrt(e.size) and abs(e.var() - 1) <= 5 * np.sqrt(2.0 / e.size)
    trainer.close()


@pytest.mark.parametrize("H", [5, 300])
def test_an_epoch_is_its_batches(H):
    """run_epochs(1) against the same state fed ``order`` / ``noise`` batch by batch through ``step_batch`` with the
    schedule's klc (H = 5: two lanes per entry, one tile; 300: a whole wave with two passes, three tiles)"""
    X_train, _ = planted_split()
    kw = dict(enc_hidden_dim=H, dec_hidden_dim=H + 3, minibatch_size=128, anneal_end_epoch=2)
    a, b = planted_trainer(**kw), planted_trainer(**kw)
    a.run_epochs(1)  # (so that the compared epoch is not the first)
    b.set_state(a.get_state())
    a.run_epochs(1)
    n, t = a.n_users, b.get_state()["n_updates"]
    for first in range(0, n, 128):
        users = b.order(1, first, min(128, n - first))
        keep, eps = b.noise(t, users)
        klc = R.kl_coefficient(0.2, t, 2, n, 128)
        assert b.stats()["klc_next"] == pytest.approx(klc, rel=1e-12)
        b.step_batch(users, keep, eps, klc)
        t += 1
    got, want = b.get_state(), a.get_state()
    assert want["epoch"] == 2 and got["epoch"] == 1
    assert same_bytes(dict(got, epoch=2), want)
    # and without handing the noise over: drawn at the current update count
    c = planted_trainer(**kw)
    c.run_epochs(1)
    t = c.get_state()["n_updates"]
    for first in range(0, n, 128):
        c.step_batch(c.order(1, first, min(128, n - first)), None, None, R.kl_coefficient(0.2, t, 2, n, 128))
        t += 1
    assert same_bytes(dict(c.get_state(), epoch=2), want)


def test_annealing_schedule():
    """klc of every update of two epochs as stats report it, against the formula; anneal_end_epoch = 1 saturates at
    the goal after the first epoch"""
    for end in (1, 50):
        trainer = planted_trainer(anneal_end_epoch=end, minibatch_size=128, kl_anneal_goal=0.4)
        n, batches = trainer.n_users, trainer.stats()["batches_per_epoch"]
        seen = []
        for epoch in range(2):
            for first in range(0, n, 128):
                st = trainer.stats()
                seen.append(st["klc_next"])
                trainer.step_batch(trainer.order(epoch, first, min(128, n - first)), None, None, st["klc_next"])
                assert trainer.stats()["klc_last"] == seen[-1]
        want = [0.4 * min(1.0, t / (end * n / 128)) for t in range(2 * batches)]
        np.testing.assert_allclose(seen, want, rtol=1e-12, atol=0)
        assert seen[0] == 0.0 and (seen[-1] == pytest.approx(0.4) if end == 1 else seen[-1] < 0.4)
        # run_epochs follows the same schedule
        other = planted_trainer(anneal_end_epoch=end, minibatch_size=128, kl_anneal_goal=0.4)
        other.run_epochs(2)
        st = other.stats()
        assert st["n_updates"] == 2 * batches and st["klc_last"] == pytest.approx(want[-1], rel=1e-12)
        assert same_bytes(dict(trainer.get_state(), epoch=2), other.get_state())


# ---- scoring, quality, early stopping --------------------------------------------------------------------------------
_fits = {}
CONFIG = dict(enc_hidden_dims=64, dim_z=16, minibatch_size=100, learning_rate=1e-2)


def device_fit():
    if "device" not in _fits:
        _fits["device"] = MultVAERecommender(planted_split()[0], train_epochs=10, **CONFIG).learn()
    return _fits["device"]


def restatement_fit():
    if "ref" not in _fits:
        _fits["ref"] = R.fit(planted_split()[0], dim_z=16, enc_hidden=64, minibatch_size=100, learning_rate=1e-2, epochs=10)
    return _fits["ref"]


def test_scoring():
    X_train, _ = planted_split()
    model = device_fit()
    state = model.trainer.get_state()
    rng = np.random.default_rng(1)
    cold = sps.csr_matrix(((rng.random((70, 400)) < 0.06) * rng.choice([1.0, 2.0], (70, 400))).astype(np.float64))
    cold = sps.vstack([cold, sps.csr_matrix((1, 400))]).tocsr()  # (and a row without entries)
    got = model.get_score_cold_user(cold)
    assert got.dtype == np.float64 and got.shape == (71, 400)
    want64 = R.eval_scores(state, np.asarray(cold.todense()), np.float64)
    want32 = R.eval_scores(state, np.asarray(cold.todense()), np.float32)
    assert_float64_bar(got, want32, want64, "cold-user log-softmax", test="multvae_scoring")
    users = np.array([5, 0, 599, 17, 17])
    np.testing.assert_array_equal(model.get_score(users), model.get_score_cold_user(X_train[users]))
    np.testing.assert_array_equal(model.get_score_block(100, 130), model.get_score(np.arange(100, 130)))
    total = np.exp(model.get_score_block(0, 600)).sum(axis=1)
    assert np.abs(total - 1).max() <= 400 * 2.0 ** -24 * 4  # float32 rounding of I terms
    removed = model.get_score_remove_seen(np.array([3]))
    assert np.isneginf(removed[0, X_train[3].indices]).all()


def test_scores_and_factors_in_ragged_chunks():
    """21 cold rows through a handle of 8 rows (chunks of 8, 8 and 5; empty rows first, at the head of a chunk and
    last; the full row before a chunk's head, so that the next chunk's entries begin far into the arrays): scores,
    h2 and lse against the restatement, the factor product against the scores, and every row the same bytes
    whichever chunk and position it is computed at"""
    c = K.SCORING
    I, H, Hd, L, cap = c["I"], c["H"], c["Hd"], c["L"], c["capacity"]
    X = batch_matrix(c["users"], I, 42)
    state = random_start(I, H, L, Hd, 43)
    cold = K.ragged_cold_rows()
    dense = np.asarray(cold.todense())
    chunked, whole = make_trainer(X, H, Hd, L, 0.5, minibatch_size=cap), make_trainer(X, H, Hd, L, 0.5)
    for t in (chunked, whole):
        t.set_state(state)
    got = chunked.score(cold)
    assert got.dtype == np.float32 and got.shape == (21, I) and np.isfinite(got).all()
    assert_float64_bar(got, R.eval_scores(state, dense, np.float32), R.eval_scores(state, dense, np.float64),
                       "ragged chunks: log-softmax", test="multvae_scoring")
    h2, lse = chunked.encode(cold)
    assert h2.shape == (21, Hd) and lse.shape == (21,) and h2.dtype == lse.dtype == np.float32
    (h32, l32), (h64, l64) = (R.eval_hidden(state, dense, d) for d in (np.float32, np.float64))
    assert_float64_bar(h2, h32, h64, "ragged chunks: h2", test="multvae_scoring")
    assert_float64_bar(lse[:, None], K.log_sum_exp(l32)[:, None], K.log_sum_exp(l64)[:, None], "ragged chunks: lse",
                       test="multvae_scoring")
    # the two factor tables multiply to the scores
    k = Hd + 2
    Z = np.concatenate([h2, np.ones((21, 1), np.float32), -lse[:, None]], axis=1).astype(np.float64)
    Ct = np.concatenate([state["W4"], state["b4"][None, :], np.ones((1, I), np.float32)], axis=0).astype(np.float64)
    bound = 4.0 * k * 2.0 ** -24 * (np.abs(Z) @ np.abs(Ct)).max(axis=1)
    assert (np.abs(Z @ Ct - got).max(axis=1) <= bound).all()
    # one chunk of 21 rows, and three rows alone: the same bytes
    w_h2, w_lse = whole.encode(cold)
    assert whole.score(cold).tobytes() == got.tobytes() and w_h2.tobytes() == h2.tobytes() and w_lse.tobytes() == lse.tobytes()
    alone = [c["full"], 8, 20]
    for t in (chunked, whole):
        a_h2, a_lse = t.encode(cold[alone])
        assert t.score(cold[alone]).tobytes() == got[alone].tobytes()
        assert a_h2.tobytes() == h2[alone].tobytes() and a_lse.tobytes() == lse[alone].tobytes()
    none = chunked.score(sps.csr_matrix((0, I), dtype=np.float32))
    assert none.shape == (0, I) and none.dtype == np.float32
    chunked.close()
    whole.close()


def test_log_softmax_scores_at_large_logits():
    """the state of ``test_softmax_at_large_logits`` with [W4; b4] scaled until the evaluation logits of the scored
    rows span beyond +-60: SM_LOG_SOFTMAX is finite everywhere and inside the bar"""
    I, H, Hd, L, n = 257, 33, 33, 3, 40
    X = batch_matrix(n, I, 7)
    state = random_start(I, H, L, Hd, 8)
    dense = np.asarray(X.todense())
    span = float(np.abs(R.eval_hidden(state, dense)[1]).max())
    state["W4"] = (state["W4"] * (80.0 / span)).astype(np.float32)
    state["b4"] = (state["b4"] * (80.0 / span)).astype(np.float32)
    lg = R.eval_hidden(state, dense)[1]
    print("logits span", float(lg.min()), float(lg.max()))
    assert lg.max() > 60 and lg.min() < -60
    trainer = make_trainer(X, H, Hd, L, 0.5, minibatch_size=16)  # (chunks of 16, 16 and 8)
    trainer.set_state(state)
    got = trainer.score(X)
    assert got.shape == (n, I) and np.isfinite(got).all()
    assert_float64_bar(got, R.eval_scores(state, dense, np.float32), R.eval_scores(state, dense, np.float64),
                       "large logits: log-softmax", test="multvae_scoring")
    trainer.close()


def test_quality_on_the_planted_split():
    X_train, X_test = planted_split()
    model = device_fit()
    got = ndcg_at(model.get_score_block(0, 600), X_train, X_test)
    ref = ndcg_at(R.eval_scores(restatement_fit(), np.asarray(X_train.todense())), X_train, X_test)
    pop = ndcg_at(TopPopRecommender(X_train).learn().get_score(np.arange(600)), X_train, X_test)
    print(f"nDCG@20 on the planted split: device {got:.4f}, restatement {ref:.4f}, TopPop {pop:.4f}")
    assert got >= 0.9 * ref and got >= 3.0 * pop
    st = model.trainer.get_state()
    assert (st["epoch"], st["n_updates"]) == (10, 60)


class ScriptedEvaluator:
    """the real evaluator's score is computed (the model must be scorable mid-fit), a scripted one is returned: the
    best validation is the second"""

    def __init__(self, evaluator, script):
        self.evaluator, self.script, self.real = evaluator, list(script), []

    def get_target_score(self, model):
        self.real.append(self.evaluator.get_target_score(model))
        return self.script[len(self.real) - 1]


def test_early_stopping_restores_the_best_state():
    from irspack_amd.evaluation import Evaluator

    X_train, X_test = planted_split()
    ev = ScriptedEvaluator(Evaluator(X_test, cutoff=20, target_metric="ndcg"), [0.1, 0.3, 0.2, 0.25, 0.9, 0.9])
    model = MultVAERecommender(X_train, train_epochs=10, **CONFIG)
    model.learn_with_evaluator(ev, max_epoch=30, validate_epoch=2, score_degradation_max=2)
    assert len(ev.real) == 4  # validated after epochs 2, 4, 6, 8; stopped after two misses
    assert model.learnt_config["train_epochs"] == 4
    assert all(np.isfinite(v) and v > 0 for v in ev.real)  # (the model can be scored mid-fit)
    plain = MultVAERecommender(X_train, train_epochs=4, **CONFIG).learn()
    assert same_bytes(model.trainer.get_state(), plain.trainer.get_state())
    np.testing.assert_array_equal(model.get_score_block(0, 50), plain.get_score_block(0, 50))


# ---- evaluator and serving -----------------------------------------------------------------------------------------
def test_fitted_model_through_the_fused_evaluator_and_the_serving_layer():
    from irspack_amd.serving import DeviceRecommender
    from test_gpu_evaluator_models import check_model_on_device, without_near_ties

    # (a narrow decoder: the near-tie bound of the factor product grows with its Hd + 2 terms, and with 64 of them
    # it takes 14 % of this data's users out of the comparison)
    X_train, X_test = planted_split()
    model = MultVAERecommender(X_train, train_epochs=10, dec_hidden_dims=8, **CONFIG).learn()
    users, items = model.factor_tables()
    k = 8 + 2
    assert users.shape == (600, k) and items.shape == (k, 400) and users.dtype == items.dtype == np.float32
    assert model.factor_tables()[0] is users  # (held per state)
    # the product of the two tables is the log-softmax: scores match, not only ranks
    Z, Ct = users.astype(np.float64), items.astype(np.float64)
    bound = 4.0 * k * 2.0 ** -24 * (np.abs(Z) @ np.abs(Ct)).max(axis=1)
    assert (np.abs(Z @ Ct - model.get_score_block(0, 600)).max(axis=1) <= bound).all()
    gt, share = without_near_ties(users, items, model.X_train_all, X_test, k)
    print(f"near-tied users removed: {share:.4f}")
    assert share <= 0.05
    dev = DeviceRecommender(model)
    assert dev.kind == "factors"
    who = np.arange(0, 600, 3)
    idx, score, length = dev.recommend_known_arrays(who, 10)
    h_idx, h_score, h_length = dev._two_step(model.get_score_remove_seen(who), [], None, 10)
    np.testing.assert_array_equal(length, h_length)
    s64 = Z[who] @ Ct
    differ = idx != h_idx
    print("rows whose lists differ from the host's:", int(differ.any(axis=1).sum()), "of", who.size)
    for r, p in zip(*np.nonzero(differ)):
        assert abs(s64[r, idx[r, p]] - s64[r, h_idx[r, p]]) < bound[who][r], (r, p)
    np.testing.assert_allclose(score, np.take_along_axis(s64, idx.astype(np.int64), axis=1), rtol=0, atol=float(bound.max()))
    # new users: their factors come from the encoder
    rng = np.random.default_rng(3)
    cold = sps.csr_matrix((rng.random((40, 400)) < 0.05).astype(np.float64))
    c_idx, c_score, c_length = dev.recommend_profiles_arrays(cold, 10)
    w_idx, w_score, w_length = dev._two_step(model.get_score_cold_user_remove_seen(cold), [], None, 10)
    np.testing.assert_array_equal(c_length, w_length)
    F = model.profile_factors(cold).astype(np.float64)
    c64 = F @ Ct
    c_bound = 4.0 * k * 2.0 ** -24 * (np.abs(F) @ np.abs(Ct)).max(axis=1)
    for r, p in zip(*np.nonzero(c_idx != w_idx)):
        assert abs(c64[r, c_idx[r, p]] - c64[r, w_idx[r, p]]) < c_bound[r], (r, p)
    np.testing.assert_allclose(c_score, np.take_along_axis(c64, c_idx.astype(np.int64), axis=1), rtol=0, atol=float(c_bound.max()))
    assert len(dev.recommend_profiles(cold[:3], 5)) == 3
    dev.close()
    # the fused evaluator takes the "factors" path and equals the block loop
    check_model_on_device(model, gt, "factors")
