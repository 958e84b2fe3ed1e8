"""BPRFMRecommender on the device: one batch against the numpy restatement (``tests/_bpr_restatement.py``) judged by
float64, byte-identical reruns and restores, the sampler's properties, quality on the planted data, early stopping,
and the fitted model through the fused evaluator and the serving layer."""
import io

import numpy as np
import pytest
import scipy.sparse as sps

from _bpr_restatement import TABLES, bpr_fit, bpr_step, ndcg_at, planted_split, scores
from conftest import assert_float64_bar
from irspack_amd.recommenders import BPRFMRecommender, TopPopRecommender
from irspack_amd.recommenders.bpr import BPRFMTrainer

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS = 50, 37


def same_bytes(a, b):
    return a["epoch"] == b["epoch"] and all(a[n].tobytes() == b[n].tobytes() for n in TABLES)


# ---- one batch against the restatement ---------------------------------------------------------------------------
def random_state(k, seed):
    """float32 tables of scale 0.3 (so w is not always 1/2) and accumulators in [1, 4]"""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    return dict(U=(0.3 * rng.standard_normal((N_USERS, k))).astype(f32), V=(0.3 * rng.standard_normal((N_ITEMS, k))).astype(f32),
                b=(0.3 * rng.standard_normal(N_ITEMS)).astype(f32), GU=rng.uniform(1, 4, (N_USERS, k)).astype(f32),
                GV=rng.uniform(1, 4, (N_ITEMS, k)).astype(f32), Gb=rng.uniform(1, 4, N_ITEMS).astype(f32), epoch=0)


def batches():
    """name -> list of batches (users, pos, neg), run in a row from one state"""
    rng = np.random.default_rng(5)

    def rand(n):
        return (rng.integers(0, N_USERS, n), rng.integers(0, N_ITEMS, n), rng.integers(0, N_ITEMS, n))

    out = {f"random {n}": [rand(n)] for n in (1, 63, 64, 65, 1000)}
    u, i, j = rand(200)
    out["one user in every triple"] = [(np.full(200, 7), i, j)]
    u, i, j = rand(120)
    i[:60], j[60:] = 11, 11  # item 11: the positive of 60 triples and the negative of 60 others
    out["one item as positive and as negative"] = [(u, i, j)]
    out["identical triples"] = [(np.full(300, 3), np.full(300, 5), np.full(300, 8))]
    out["three batches in a row"] = [rand(65), rand(257), rand(9)]
    return out


BATCHES = batches()
_X_ANY = sps.csr_matrix(np.ones((N_USERS, N_ITEMS), dtype=np.float32))  # (step_triples does not look at it)
LR = 0.25  # (a step that is large against the parameters: an error in the update shows in the rows; a float32 value)


@pytest.mark.parametrize("alpha", [0.0, 0.1])
@pytest.mark.parametrize("k", [1, 5, 64, 65, 128, 130, 256, 512])
def test_one_batch_against_the_restatement(k, alpha):
    trainer = BPRFMTrainer(_X_ANY, k, alpha, alpha, learning_rate=LR, batch_size=64)
    for case, (name, runs) in enumerate(BATCHES.items()):
        start = random_state(k, 100 + case)
        trainer.set_state(start)
        ref64, ref32 = start, start
        touched_u, touched_i = set(), set()
        for users, pos, neg in runs:
            trainer.step_triples(users, pos, neg)
            ref64 = bpr_step(ref64, users, pos, neg, alpha, alpha, LR, np.float64)
            ref32 = bpr_step(ref32, users, pos, neg, alpha, alpha, LR, np.float32)
            touched_u |= set(users.tolist())
            touched_i |= set(pos.tolist()) | set(neg.tolist())
        got = trainer.get_state()
        assert got["epoch"] == 0
        for n in TABLES:
            rows = sorted(touched_u if n in ("U", "GU") else touched_i)
            rest = np.setdiff1d(np.arange(start[n].shape[0]), rows)
            assert got[n].dtype == np.float32 and np.isfinite(got[n]).all()
            # untouched rows keep their bytes, accumulators included
            assert got[n][rest].tobytes() == start[n][rest].tobytes(), (name, n)
            assert not (got[n][rows] == start[n][rows]).all(), (name, n)
            shape = (len(rows), -1)
            assert_float64_bar(got[n][rows].reshape(shape), ref32[n][rows].reshape(shape),
                               ref64[n][rows].reshape(shape), f"{name} K={k} alpha={alpha} {n}",
                               test="bpr_one_batch")
    trainer.close()


# ---- reproducibility ----------------------------------------------------------------------------------------------
def planted_trainer(**kw):
    X_train, _ = planted_split()
    args = dict(n_components=18, item_alpha=1e-4, user_alpha=1e-4, learning_rate=0.05, batch_size=1000, random_seed=3)
    args.update(kw)
    return BPRFMTrainer(X_train, **args)


def test_same_seed_same_bytes_and_restores_continue_identically():
    a, b = planted_trainer(), planted_trainer()
    assert a.epoch_length == 11920 and a.epoch_length % 1000 != 0  # (the last batch is partial)
    a.run_epochs(3)
    for _ in range(3):
        b.run_epoch()
    want = a.get_state()
    assert want["epoch"] == 3 and same_bytes(want, b.get_state())
    assert not same_bytes(want, dict(planted_trainer(random_seed=4).get_state(), epoch=3))
    other = planted_trainer(random_seed=4)
    other.run_epochs(3)
    assert not (other.get_state()["U"] == want["U"]).all()
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
    with pytest.raises(ValueError, match="trained with"):
        planted_trainer(batch_size=999).load_state(io.BytesIO(buf.getvalue()))


# ---- the sampler ----------------------------------------------------------------------------------------------------
def sampler_matrix():
    """40 x 23 with an empty row (2), a full row (5: skipped and counted), a row with all items but one (9: its
    negative is always item 4), a row with 10 unseen items (12) and an entry that is not positive"""
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


def test_sampler_properties():
    X = sampler_matrix()
    pos = X.multiply(X > 0).tocsr()
    pos.eliminate_zeros()
    deg = np.diff(pos.indptr)
    trainer = BPRFMTrainer(X, 8, 0.0, 0.0, batch_size=16, random_seed=9)
    st = trainer.stats()
    assert (st["n_positives"], st["n_skipped_full_rows"], st["n_skipped_positives"]) == (pos.nnz, 1, 23)
    n = trainer.epoch_length
    assert n == pos.nnz - 23 and n % 16 != 0 and st["batches_per_epoch"] == -(-n // 16)
    rows = np.repeat(np.arange(40), deg)
    want = sorted((int(u), int(i)) for u, i in zip(rows, pos.indices) if u != 5)
    seen = pos.toarray() > 0
    orders, negatives_of_12 = [], set()
    for epoch in range(200):
        u, i, j = trainer.sample(epoch)
        if epoch < 3:
            assert sorted(zip(u.tolist(), i.tolist())) == want  # every positive of a row with a negative, once
            orders.append((u.tolist(), i.tolist()))
            # windows concatenate to the whole epoch
            cuts = [0, 1, 16, 17, 100, n]
            parts = [trainer.sample(epoch, a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
            for whole, k in zip((u, i, j), range(3)):
                np.testing.assert_array_equal(np.concatenate([p[k] for p in parts]), whole)
        assert ((j >= 0) & (j < 23)).all() and not seen[u, j].any()
        assert (j[u == 9] == 4).all() and (u == 9).sum() == 22 and not (u == 5).any() and not (u == 2).any()
        negatives_of_12 |= set(j[u == 12].tolist())
    assert orders[0] != orders[1] and orders[1] != orders[2]
    assert negatives_of_12 == set(np.flatnonzero(~seen[12]).tolist()) and len(negatives_of_12) == 10
    np.testing.assert_array_equal(trainer.sample(1)[2], BPRFMTrainer(X, 8, 0.0, 0.0, batch_size=5, random_seed=9).sample(1)[2])
    assert trainer.sample(0, n, 0)[0].size == 0
    with pytest.raises(ValueError):
        trainer.sample(0, n - 1, 2)


@pytest.mark.parametrize("k", [8, 70])
def test_an_epoch_is_its_sampled_batches(k):
    """run_epochs(1) against the same state fed irs_bpr_sample's triples batch by batch through step_triples"""
    X = sampler_matrix()
    a = BPRFMTrainer(X, k, 1e-3, 1e-2, learning_rate=0.1, batch_size=16, random_seed=9)
    b = BPRFMTrainer(X, k, 1e-3, 1e-2, learning_rate=0.1, batch_size=16, random_seed=9)
    a.run_epochs(2)  # (so that the compared epoch is not the first)
    b.set_state(a.get_state())
    a.run_epochs(1)
    u, i, j = b.sample(2)
    for first in range(0, u.size, 16):
        b.step_triples(u[first:first + 16], i[first:first + 16], j[first:first + 16])
    got, want = b.get_state(), a.get_state()
    assert want["epoch"] == 3 and got["epoch"] == 2
    assert same_bytes(dict(got, epoch=3), want)
    start = BPRFMTrainer(X, k, 1e-3, 1e-2, learning_rate=0.1, batch_size=16, random_seed=9).get_state()
    for n in TABLES:  # the empty row and the full row were never touched
        rows = [2, 5] if n in ("U", "GU") else []
        assert want[n][rows].tobytes() == start[n][rows].tobytes()
    assert not (want["U"][[0, 9, 12]] == start["U"][[0, 9, 12]]).all()


# ---- quality, early stopping ---------------------------------------------------------------------------------------
_fits = {}


def restatement_fit():
    if "f" not in _fits:
        _fits["f"] = bpr_fit(planted_split()[0], 16, batch_size=1024, epochs=20, seed=42)
    return _fits["f"]


def test_quality_on_the_planted_split():
    X_train, X_test = planted_split()
    model = BPRFMRecommender(X_train, n_components=16, batch_size=1024, train_epochs=20).learn()
    got = ndcg_at(model.get_score_block(0, 600), X_train, X_test)
    ref = ndcg_at(scores(restatement_fit()), X_train, X_test)
    pop = ndcg_at(TopPopRecommender(X_train).learn().get_score(np.arange(600)), X_train, X_test)
    print(f"nDCG@20 on the planted split: device {got:.4f}, restatement {ref:.4f}, TopPop {pop:.4f}")
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
    model = BPRFMRecommender(X_train, n_components=16, batch_size=1024, train_epochs=20)
    model.learn_with_evaluator(ev, max_epoch=30, validate_epoch=2, score_degradation_max=2)
    assert len(ev.real) == 4  # validated after epochs 2, 4, 6, 8; stopped after two misses
    assert model.learnt_config["train_epochs"] == 4
    assert all(np.isfinite(v) and v > 0 for v in ev.real)  # (the model can be scored mid-fit)
    plain = BPRFMRecommender(X_train, n_components=16, batch_size=1024, train_epochs=4).learn()
    assert same_bytes(model.trainer.get_state(), plain.trainer.get_state())
    np.testing.assert_array_equal(model.get_score_block(0, 50), plain.get_score_block(0, 50))


# ---- evaluator and serving -----------------------------------------------------------------------------------------
def test_fitted_model_through_the_fused_evaluator_and_the_serving_layer():
    from irspack_amd.serving import DeviceRecommender
    from test_gpu_evaluator_models import check_model_on_device, without_near_ties

    X_train, X_test = planted_split()
    model = BPRFMRecommender(X_train, n_components=16, batch_size=1024, train_epochs=20)
    model.start_learning()
    model.trainer.set_state(restatement_fit())
    users, items = model.factor_tables()  # (600, 17), (17, 400)
    gt, share = without_near_ties(users, items, model.X_train_all, X_test, 17)
    print(f"near-tied users removed: {share:.4f}")
    assert share <= 0.05
    # serving: the device's lists against the two-step host ranking; where they differ, the two items' float64
    # scores lie within the bound of that rule
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
    with pytest.raises(NotImplementedError):
        dev.recommend_profiles(X_train[:3], 10)
    dev.close()
    # the fused evaluator takes the "factors" path and equals the block loop
    check_model_on_device(model, gt, "factors")
