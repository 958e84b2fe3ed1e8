"""The WARP loss on the device (``BPRFMTrainer(loss="warp")``, ``WARPFMRecommender``): the search exact against the
numpy restatement (``tests/_warp_restatement.py``), one batch judged by float64, the candidate stream's properties,
an epoch as its candidate batches, byte-identical reruns and restores, quality on the planted data, early stopping,
the fitted model through the fused evaluator and the serving layer, and the divergence flag.  The inputs come from
``tests/_warp_cases.py``; what they promise is checked without a device in ``tests/test_warp_surface.py``."""
import io

import numpy as np
import pytest
import scipy.sparse as sps

from _bpr_restatement import TABLES, ndcg_at, planted_split, scores
from _warp_cases import (ALPHAS, K_LIST, LR, MAX_SAMPLED_LIST, N_USERS, SEARCH_SIZES, X_ANY, five_item_case,
                         many_item_case, random_state, search_batch, step_cases)
from _warp_restatement import touched_rows, warp_fit, warp_search, warp_step, warp_weights
from conftest import assert_float64_bar
from irspack_amd.recommenders import TopPopRecommender, WARPFMRecommender
from irspack_amd.recommenders.bpr import BPRFMTrainer

pytestmark = pytest.mark.gpu


def same_bytes(a, b):
    return a["epoch"] == b["epoch"] and all(a[n].tobytes() == b[n].tobytes() for n in TABLES)


def warp_trainer(X, k, alpha=0.0, max_sampled=10, **kw):
    return BPRFMTrainer(X, k, alpha, alpha, loss="warp", max_sampled=max_sampled, **kw)


# ---- the search, exact ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_sampled", MAX_SAMPLED_LIST)
@pytest.mark.parametrize("k", K_LIST)
def test_search_is_the_restatements(k, max_sampled):
    users, pos, cand = search_batch()
    cand = np.ascontiguousarray(cand[:, :max_sampled])
    state = random_state(k, 200 + k)
    trainer = warp_trainer(X_ANY, k, max_sampled=max_sampled, batch_size=64)
    trainer.set_state(state)
    for n in SEARCH_SIZES:
        want_neg, want_tries, _ = warp_search(state, users[:n], pos[:n], cand[:n])
        neg, tries = trainer.search(users[:n], pos[:n], cand[:n])
        np.testing.assert_array_equal(neg, want_neg, err_msg=f"K={k} max_sampled={max_sampled} n={n}")
        np.testing.assert_array_equal(tries, want_tries, err_msg=f"K={k} max_sampled={max_sampled} n={n}")
        st = trainer.warp_stats()
        assert (st["call_positions"], st["call_updates"], st["call_tries"]) == \
            (n, int((want_neg >= 0).sum()), int(want_tries.sum()))
    assert same_bytes(trainer.get_state(), state)  # (the search updates nothing)
    assert st["max_sampled"] == max_sampled and st["in_flight"] in (1, 2, 4)
    trainer.close()


# ---- one batch against the restatement ---------------------------------------------------------------------------
def run_case(trainer, start, runs, alpha, what):
    """the batches on the device and in the restatement (float64 the arbiter, float32 with float64's choices what a
    plain float32 update loses); the touched rows meet the float64 bar, the others keep their bytes"""
    trainer.set_state(start)
    ref64, ref32 = start, start
    touched_u, touched_i = set(), set()
    for users, pos, cand in runs:
        choice = warp_search(ref64, users, pos, cand)[:2]
        trainer.step_candidates(users, pos, cand)
        st = trainer.warp_stats()
        assert (st["call_positions"], st["call_updates"], st["call_tries"]) == \
            (users.size, int((choice[0] >= 0).sum()), int(choice[1].sum())), what
        ref32 = warp_step(ref32, users, pos, cand, alpha, alpha, LR, np.float32, choice=choice)
        ref64 = warp_step(ref64, users, pos, cand, alpha, alpha, LR, np.float64, choice=choice)
        tu, ti = touched_rows(users, pos, choice[0])
        touched_u |= tu
        touched_i |= ti
    got = trainer.get_state()
    assert got["epoch"] == 0
    for n in TABLES:
        rows = sorted(touched_u if n in ("U", "GU") else touched_i)
        rest = np.setdiff1d(np.arange(start[n].shape[0]), rows)
        assert got[n].dtype == np.float32 and np.isfinite(got[n]).all()
        assert got[n][rest].tobytes() == start[n][rest].tobytes(), (what, n)
        if not rows:  # (a batch without a violation)
            continue
        shape = (len(rows), -1)
        assert_float64_bar(got[n][rows].reshape(shape), ref32[n][rows].reshape(shape), ref64[n][rows].reshape(shape),
                           f"{what} {n}", test="warp_one_batch")
    return got, ref64, (touched_u, touched_i)


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("k", K_LIST)
def test_one_batch_against_the_restatement(k, alpha):
    trainer = warp_trainer(X_ANY, k, alpha, learning_rate=LR, batch_size=64)
    assert trainer.warp_stats()["scale_log2"] == 40
    for name, (start, runs) in step_cases(k).items():
        got, _, (tu, ti) = run_case(trainer, start, runs, alpha, f"{name} K={k} alpha={alpha}")
        if name == "no violation":
            # every byte of every table, accumulators included
            assert not tu and not ti and same_bytes(got, start)
        else:
            assert tu and ti
            for n in TABLES:
                rows = sorted(tu if n in ("U", "GU") else ti)
                assert not (got[n][rows] == start[n][rows]).all(), (name, n)
    trainer.close()
    # n_items = 5: every violation is found at t = 3, where the weight is 0 - still a triple that touches its rows
    start, (users, pos, cand) = five_item_case(k)
    X5 = sps.csr_matrix(np.ones((N_USERS, 5), dtype=np.float32))
    trainer = warp_trainer(X5, k, alpha, learning_rate=LR, batch_size=64)
    trainer.set_state(start)
    neg, tries = trainer.search(users, pos, cand)
    assert (neg == 4).all() and (tries == 3).all() and warp_weights(5, 10)[2] == 0.0
    got, ref64, (tu, ti) = run_case(trainer, start, [(users, pos, cand)], alpha, f"five items K={k} alpha={alpha}")
    assert ti == {0, 4} and tu == set(users.tolist())
    if alpha == 0.0:
        assert same_bytes(got, start)  # a zero gradient moves nothing
    else:
        for n, G in (("U", "GU"), ("V", "GV"), ("b", "Gb")):  # the L2 term alone
            rows = sorted(tu if n == "U" else ti)
            th, g2 = start[n][rows].astype(np.float64), start[G][rows].astype(np.float64)
            np.testing.assert_allclose(ref64[n][rows], th - LR * alpha * th / np.sqrt(g2), rtol=1e-14)
            assert not (got[n][rows] == start[n][rows]).all()
    trainer.close()


def test_weight_is_capped_at_ten_with_many_items():
    """n_items = 30,000: ln 29,999 = 10.31 enters as 10 (every position's first candidate violates)"""
    start, (users, pos, cand) = many_item_case()
    n_items = start["V"].shape[0]
    assert warp_weights(n_items, 10)[0] == 10.0 and np.log(n_items - 1) > 10.3
    X = sps.csr_matrix(np.ones((8, 1), dtype=np.float32)) @ sps.csr_matrix(np.ones((1, n_items), dtype=np.float32))
    trainer = warp_trainer(X, 4, 0.0, learning_rate=LR, batch_size=64)
    trainer.set_state(start)
    neg, tries = trainer.search(users, pos, cand)
    np.testing.assert_array_equal(neg, cand[:, 0])
    assert (tries == 1).all()
    run_case(trainer, start, [(users, pos, cand)], 0.0, "30,000 items K=4")
    # (a weight of 10.31 would miss the bar by far: the steps scale with it)
    trainer.close()


# ---- the candidates -------------------------------------------------------------------------------------------------
def sampler_matrix():
    """40 x 23 with an empty row (2), a full row (5: skipped and counted), a row with all items but one (9: its
    candidates are all item 4), a row with 10 unseen items (12) and an entry that is not positive"""
    rng = np.random.default_rng(11)
    D = (rng.random((40, 23)) < 0.3).astype(np.float32)
    D[2] = 0
    D[5] = 1
    D[9] = 1
    D[9, 4] = 0
    D[12] = 0
    D[12, rng.choice(23, 13, replace=False)] = 1
    X = sps.csr_matrix(D)
    X.data[3] = -1.0  # (a stored entry <= 0 is no positive, and its item stays unseen)
    return X


def test_candidate_properties():
    X = sampler_matrix()
    positives = X.multiply(X > 0).tocsr()
    positives.eliminate_zeros()
    seen = positives.toarray() > 0
    t10 = warp_trainer(X, 8, max_sampled=10, batch_size=16, random_seed=9)
    t3 = warp_trainer(X, 8, max_sampled=3, batch_size=5, random_seed=9)
    bpr = BPRFMTrainer(X, 8, 0.0, 0.0, batch_size=16, random_seed=9)
    st = t10.stats()
    assert (st["n_positives"], st["n_skipped_full_rows"], st["n_skipped_positives"]) == (positives.nnz, 1, 23)
    n = t10.epoch_length
    assert n == positives.nnz - 23 == bpr.epoch_length
    drawn_by_12 = set()
    for epoch in range(40):
        u, i, c = t10.candidates(epoch)
        assert c.shape == (n, 10) and c.dtype == np.int32
        assert ((c >= 0) & (c < 23)).all() and not seen[u[:, None], c].any()  # all unseen by their user
        assert (c[u == 9] == 4).all() and (u == 9).sum() == 22 and not (u == 5).any() and not (u == 2).any()
        drawn_by_12 |= set(c[u == 12].ravel().tolist())
        if epoch < 3:
            # the positions of the BPR trainer at the same seed and epoch
            bu, bi, bj = bpr.sample(epoch)
            np.testing.assert_array_equal(u, bu)
            np.testing.assert_array_equal(i, bi)
            assert not (c[:, 0] == bj).all()  # (a stream of its own)
            # the prefix property: candidate t does not depend on max_sampled (nor on the batch size)
            u3, i3, c3 = t3.candidates(epoch)
            np.testing.assert_array_equal(u3, u)
            np.testing.assert_array_equal(i3, i)
            np.testing.assert_array_equal(c3, c[:, :3])
            # any window is the same slice of the whole epoch
            cuts = [0, 1, 16, 17, 100, n]
            for a, b in zip(cuts[:-1], cuts[1:]):
                for whole, part in zip((u, i, c), t10.candidates(epoch, a, b - a)):
                    np.testing.assert_array_equal(part, whole[a:b])
    assert drawn_by_12 == set(np.flatnonzero(~seen[12]).tolist()) and len(drawn_by_12) == 10
    assert not (t10.candidates(0)[2] == t10.candidates(1)[2]).all()
    assert t10.candidates(0, n, 0)[0].size == 0
    with pytest.raises(ValueError):
        t10.candidates(0, n - 1, 2)
    with pytest.raises(ValueError, match="irs_bpr_warp_candidates"):
        t10.sample(0)
    with pytest.raises(ValueError, match="irs_bpr_warp_step"):
        t10.step_triples([0], [0], [1])
    with pytest.raises(ValueError, match="irs_bpr_create_warp"):
        bpr.warp_stats()


@pytest.mark.parametrize("k", [8, 70])
def test_an_epoch_is_its_candidate_batches(k):
    """run_epochs(1) against the same state fed irs_bpr_warp_candidates' windows batch by batch through
    step_candidates, byte for byte; the epoch's counters equal those of search calls made before each step"""
    X = sampler_matrix()
    args = dict(learning_rate=0.1, batch_size=16, random_seed=9)
    a = BPRFMTrainer(X, k, 1e-2, 1e-3, loss="warp", max_sampled=10, **args)
    b = BPRFMTrainer(X, k, 1e-2, 1e-3, loss="warp", max_sampled=10, **args)
    a.run_epochs(2)  # (so that the compared epoch is not the first)
    b.set_state(a.get_state())
    a.run_epochs(1)
    u, i, c = b.candidates(2)
    positions = updates = tries = 0
    for first in range(0, u.size, 16):
        sl = slice(first, first + 16)
        neg, t = b.search(u[sl], i[sl], c[sl])
        positions, updates, tries = positions + neg.size, updates + int((neg >= 0).sum()), tries + int(t.sum())
        b.step_candidates(u[sl], i[sl], c[sl])
    got, want = b.get_state(), a.get_state()
    assert want["epoch"] == 3 and got["epoch"] == 2
    assert same_bytes(dict(got, epoch=3), want)
    st = a.warp_stats()
    assert (st["epoch_positions"], st["epoch_updates"], st["epoch_tries"]) == (positions, updates, tries)
    assert positions == u.size and 0 < updates <= positions and positions <= tries <= 10 * positions
    assert st["epoch_ms"] > 0
    start = BPRFMTrainer(X, k, 1e-2, 1e-3, loss="warp", max_sampled=10, **args).get_state()
    for n in TABLES:  # the empty row and the full row were never touched
        rows = [2, 5] if n in ("U", "GU") else []
        assert want[n][rows].tobytes() == start[n][rows].tobytes()
    assert not (want["U"][[0, 9, 12]] == start["U"][[0, 9, 12]]).all()


# ---- state and reproducibility --------------------------------------------------------------------------------------
def planted_trainer(**kw):
    X_train, _ = planted_split()
    args = dict(n_components=18, item_alpha=1e-4, user_alpha=1e-4, learning_rate=0.05, batch_size=1000, random_seed=3,
                loss="warp", max_sampled=10)
    args.update(kw)
    return BPRFMTrainer(X_train, **args)


def test_same_seed_same_bytes_and_restores_continue_identically():
    a, b = planted_trainer(), planted_trainer()
    assert a.epoch_length == 11920
    a.run_epochs(3)
    for _ in range(3):
        b.run_epoch()
    want = a.get_state()
    assert want["epoch"] == 3 and same_bytes(want, b.get_state())
    other = planted_trainer(random_seed=4)
    other.run_epochs(3)
    assert not (other.get_state()["U"] == want["U"]).all()
    fewer = planted_trainer(max_sampled=3)
    fewer.run_epochs(3)
    assert not same_bytes(fewer.get_state(), want)
    # get_state -> set_state into a fresh trainer -> continue
    c = planted_trainer()
    c.run_epochs(1)
    d = planted_trainer()
    d.set_state(c.get_state())
    d.run_epochs(2)
    assert same_bytes(want, d.get_state())
    # save_state / load_state
    buf = io.BytesIO()
    c.save_state(buf)
    e = planted_trainer()
    e.load_state(io.BytesIO(buf.getvalue()))
    e.run_epochs(2)
    assert same_bytes(want, e.get_state())
    # a state saved under another loss or max_sampled is refused, both ways
    with pytest.raises(ValueError, match="trained with"):
        planted_trainer(max_sampled=9).load_state(io.BytesIO(buf.getvalue()))
    with pytest.raises(ValueError, match="trained with"):
        planted_trainer(loss="bpr").load_state(io.BytesIO(buf.getvalue()))
    bpr_buf = io.BytesIO()
    planted_trainer(loss="bpr").save_state(bpr_buf)
    with pytest.raises(ValueError, match="trained with"):
        planted_trainer().load_state(io.BytesIO(bpr_buf.getvalue()))


# ---- quality, early stopping ---------------------------------------------------------------------------------------
_fits = {}


def restatement_fit():
    if "f" not in _fits:
        _fits["f"] = warp_fit(planted_split()[0], 16, batch_size=1024, epochs=20, seed=42, max_sampled=10)
    return _fits["f"]


def test_quality_on_the_planted_split():
    X_train, X_test = planted_split()
    model = WARPFMRecommender(X_train, n_components=16, batch_size=1024, train_epochs=20, max_sampled=10).learn()
    got = ndcg_at(model.get_score_block(0, 600), X_train, X_test)
    ref = ndcg_at(scores(restatement_fit()), X_train, X_test)
    pop = ndcg_at(TopPopRecommender(X_train).learn().get_score(np.arange(600)), X_train, X_test)
    st = model.trainer.warp_stats()
    print(f"nDCG@20 on the planted split: device {got:.4f}, restatement {ref:.4f}, TopPop {pop:.4f}; last epoch: "
          f"mean tries {st['epoch_tries'] / st['epoch_positions']:.3f}, "
          f"no violation {1 - st['epoch_updates'] / st['epoch_positions']:.3f}")
    assert got >= 0.9 * ref and got >= 3.0 * pop
    assert model.trainer.get_state()["epoch"] == 20


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
    model = WARPFMRecommender(X_train, n_components=16, batch_size=1024, train_epochs=20)
    model.learn_with_evaluator(ev, max_epoch=30, validate_epoch=2, score_degradation_max=2)
    assert len(ev.real) == 4  # validated after epochs 2, 4, 6, 8; stopped after two misses
    assert model.learnt_config["train_epochs"] == 4
    assert all(np.isfinite(v) and v > 0 for v in ev.real)  # (the model can be scored mid-fit)
    plain = WARPFMRecommender(X_train, n_components=16, batch_size=1024, train_epochs=4).learn()
    assert same_bytes(model.trainer.get_state(), plain.trainer.get_state())
    np.testing.assert_array_equal(model.get_score_block(0, 50), plain.get_score_block(0, 50))


# ---- evaluator and serving -----------------------------------------------------------------------------------------
def test_fitted_model_through_the_fused_evaluator_and_the_serving_layer():
    from irspack_amd.serving import DeviceRecommender
    from test_gpu_evaluator_models import check_model_on_device, without_near_ties

    X_train, X_test = planted_split()
    model = WARPFMRecommender(X_train, n_components=16, batch_size=1024, train_epochs=20)
    model.start_learning()
    model.trainer.set_state(restatement_fit())
    users, items = model.factor_tables()  # (600, 17), (17, 400)
    gt, share = without_near_ties(users, items, model.X_train_all, X_test, 17)
    print(f"near-tied users removed: {share:.4f}")
    assert share <= 0.05
    dev = DeviceRecommender(model)
    assert dev.kind == "factors"
    who = np.arange(0, 600, 3)
    idx, score, length = dev.recommend_known_arrays(who, 10)
    h_idx, h_score, h_length = dev._two_step(model.get_score_remove_seen(who), [], None, 10)
    np.testing.assert_array_equal(length, h_length)
    Z, Ct = users.astype(np.float64), items.astype(np.float64)
    s64 = Z[who] @ Ct
    bound = 4.0 * 17 * 2.0 ** -24 * (np.abs(Z[who]) @ np.abs(Ct)).max(axis=1)
    differ = idx != h_idx
    print("rows whose lists differ from the host's:", int(differ.any(axis=1).sum()), "of", who.size)
    for r, p in zip(*np.nonzero(differ)):
        assert abs(s64[r, idx[r, p]] - s64[r, h_idx[r, p]]) < bound[r], (r, p)
    np.testing.assert_allclose(score, np.take_along_axis(s64, idx.astype(np.int64), axis=1), rtol=0, atol=float(bound.max()))
    dev.close()
    check_model_on_device(model, gt, "factors")


# ---- divergence ------------------------------------------------------------------------------------------------------
def test_a_diverged_fit_is_the_librarys_runtime_error():
    """a learning rate that drives a parameter past 2^8 ends in the library's error from the flag, and nothing else"""
    start, runs = step_cases(5)["identical positions"]
    trainer = warp_trainer(X_ANY, 5, learning_rate=64.0, batch_size=64)
    trainer.set_state(start)
    with pytest.raises(RuntimeError, match="diverged"):
        trainer.step_candidates(*runs[0])
    trainer.close()
