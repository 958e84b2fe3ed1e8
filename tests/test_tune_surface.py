"""The tuning surface of the recommenders without a device: every class's ``default_tune_range`` against the
reference's (``tests/golden/tune_ranges.json``), ``tune`` end to end on a host-only recommender and evaluator, the
early-stopping loop's conversation with a trial, and ``IALSRecommender.tune_doubling_dimension``."""
import enum
import json
import math
import os
import pickle

import numpy as np
import pytest
import scipy.sparse as sps

import irspack_amd.recommenders as R
from irspack_amd.optimization import (CategoricalRange, LogUniformFloatRange, LogUniformIntegerRange, MedianPruner,
                                      Optimizer, RandomSampler, TPESampler, TrialPruned, UniformFloatRange,
                                      UniformIntegerRange, create_study, study_to_dataframe)
from irspack_amd.optimization import study as study_module
from irspack_amd.recommenders import knn as knn_module
from irspack_amd.recommenders.base import BaseRecommender
from irspack_amd.recommenders.base_earlystop import BaseRecommenderWithEarlyStopping, TrainerBase

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tune_ranges.json")
KINDS = {UniformFloatRange: "uniform_float", LogUniformFloatRange: "log_uniform_float",
         UniformIntegerRange: "uniform_int", LogUniformIntegerRange: "log_uniform_int",
         CategoricalRange: "categorical"}
X = sps.csr_matrix(np.eye(4))


# ---- default ranges ----------------------------------------------------------------------------------------------
def as_data(ranges):
    return [dict(name=r.name, kind=KINDS[type(r)], low=getattr(r, "low", None), high=getattr(r, "high", None),
                 step=getattr(r, "step", None), choices=getattr(r, "choices", None)) for r in ranges]


def expected_ranges():
    with open(GOLDEN) as f:
        golden = json.load(f)
    # the two stated differences: no ``loss`` choice for BPR (loss="warp" raises here), and the library's own
    # WARPFMRecommender with the same three ranges
    golden["BPRFMRecommender"] = [r for r in golden["BPRFMRecommender"] if r["name"] != "loss"]
    assert len(golden["BPRFMRecommender"]) == 3
    golden["WARPFMRecommender"] = golden["BPRFMRecommender"]
    return golden


EXPECTED = expected_ranges()


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_default_tune_range(name):
    cls = getattr(R, name, None) or getattr(knn_module, name)
    assert as_data(cls.default_tune_range) == EXPECTED[name]


def test_every_exported_class_has_its_range_checked():
    concrete = {n for n in R.__all__ if not n.startswith("Base")}
    assert concrete <= set(EXPECTED), concrete - set(EXPECTED)
    assert BaseRecommender.default_tune_range == [] and R.TopPopRecommender.default_tune_range == []


# ---- tune end to end on the host ---------------------------------------------------------------------------------
class Metric(enum.Enum):
    ndcg = 0


class FakeEvaluator:
    """scores a recommender by ``recommender.quality()``, a number in (0, 1]"""
    target_metric = Metric.ndcg
    cutoff = 7
    target_metric_name = "ndcg@7"

    def __init__(self):
        self.scored = []

    def get_score(self, model):
        q = model.quality()
        self.scored.append(model)
        return {"ndcg": q, "recall": q / 2}

    def get_target_score(self, model):
        return self.get_score(model)["ndcg"]


class HostRecommender(BaseRecommender):
    default_tune_range = [LogUniformFloatRange("reg", 1e-4, 1.0), UniformIntegerRange("k", 1, 9),
                          CategoricalRange("mode", ["x", "y"])]
    built = []

    def __init__(self, X_train_all, reg=0.5, k=1, mode="x", offset=0.0):
        super().__init__(X_train_all)
        self.reg, self.k, self.mode, self.offset = reg, k, mode, offset
        self.learnt = False
        type(self).built.append(self)

    def _learn(self):
        self.learnt = True

    def quality(self):
        assert self.learnt
        return 1.0 / (1.0 + (math.log10(self.reg) + 2) ** 2 + abs(self.k - 4) + (self.mode != "y") + self.offset)


@pytest.fixture
def built():
    HostRecommender.built = []
    return HostRecommender.built


def test_tune_end_to_end(built):
    evaluator = FakeEvaluator()
    best, frame = HostRecommender.tune(X, evaluator, n_trials=30, tuning_random_seed=0, offset=0.25)
    assert len(built) == 30 and len(frame) == 30 and frame.index.name == "number"
    assert frame.index.tolist() == list(range(30))
    assert all(r.offset == 0.25 for r in built) and all(r.X_train_all.shape == (4, 4) for r in built)
    # one row per trial: the suggested parameters, value == -score, and the metric columns
    for number, r in enumerate(built):
        row = frame.loc[number]
        assert (row["reg"], row["k"], row["mode"]) == (r.reg, r.k, r.mode)
        assert row["value"] == -r.quality() and row["ndcg@7"] == r.quality() and row["recall@7"] == r.quality() / 2
        assert row["state"] == "COMPLETE"
    assert "offset" not in frame.columns
    # the best parameters are the best row's, without the fixed one
    winner = built[int(np.argmin(frame["value"].to_numpy()))]
    assert best == dict(reg=winner.reg, k=winner.k, mode=winner.mode)
    assert type(best["k"]) is int and type(best["reg"]) is float
    assert winner.quality() == max(r.quality() for r in built)
    # the same seed, the same search
    again, frame_again = HostRecommender.tune(X, FakeEvaluator(), n_trials=30, tuning_random_seed=0, offset=0.25)
    assert again == best and frame_again["value"].equals(frame["value"])


def test_a_fixed_parameter_is_not_searched(built):
    best, frame = HostRecommender.tune(X, FakeEvaluator(), n_trials=5, tuning_random_seed=1, k=4, mode="y")
    assert all((r.k, r.mode) == (4, "y") for r in built)
    assert set(best) == {"reg"} and "k" not in frame.columns and "mode" not in frame.columns


def test_tune_needs_data(built):
    with pytest.raises(ValueError):
        HostRecommender.tune(None, FakeEvaluator(), n_trials=2)
    assert built == []


def test_the_callers_suggest_functions_are_used(built):
    matrices = {n: sps.csr_matrix(np.eye(n)) for n in (2, 3)}

    def data_of(trial):
        return matrices[trial.suggest_categorical("n", [2, 3])]

    def params_of(trial):
        return dict(reg=trial.suggest_float("reg", 1e-3, 1e-1, log=True), k=4)

    best, frame = HostRecommender.tune(None, FakeEvaluator(), n_trials=12, tuning_random_seed=0,
                                       data_suggest_function=data_of, parameter_suggest_function=params_of, mode="y")
    assert len(built) == 12
    for number, r in enumerate(built):
        assert r.n_users == frame.loc[number, "n"] and r.k == 4 and r.mode == "y" and 1e-3 <= r.reg <= 1e-1
    assert {r.n_users for r in built} == {2, 3}
    assert set(best) == {"n", "reg"}  # (k was not suggested through the trial, so it is the caller's to keep)


def test_tune_on_a_given_study(built):
    study = create_study(sampler=RandomSampler(seed=5), pruner=MedianPruner())
    best, frame = HostRecommender.tune(X, FakeEvaluator(), study=study, n_trials=4)
    assert len(study.trials) == 4 and best == study.best_params
    assert [entry[0] for entry in study.user_attrs["scores"]] == [0, 1, 2, 3]
    assert study_to_dataframe(study).equals(frame)
    # the same through an Optimizer of one's own
    optimizer = Optimizer(lambda trial: X, lambda trial: dict(k=trial.suggest_int("k", 1, 9)), dict(mode="y"),
                          FakeEvaluator())
    assert optimizer.logger.name == "IRSPACK"
    best, frame = optimizer.optimize_with_study(create_study(sampler=RandomSampler(seed=5)), HostRecommender,
                                                n_trials=3)
    assert set(best) == {"k"} and len(frame) == 3


# ---- early stopping with a trial ---------------------------------------------------------------------------------
class CountingTrainer(TrainerBase):
    def __init__(self):
        self.epochs = 0

    def run_epoch(self):
        self.epochs += 1

    def save_state(self, ofs):
        pickle.dump(self.epochs, ofs)

    def load_state(self, ifs):
        self.epochs = pickle.load(ifs)


class EpochRecommender(BaseRecommenderWithEarlyStopping):
    """its quality is ``curve[epochs - 1]``: scripted validation scores"""
    default_tune_range = [UniformIntegerRange("shift", 0, 3)]
    curve = []

    def __init__(self, X_train_all, shift=0, train_epochs=128):
        super().__init__(X_train_all, train_epochs=train_epochs)
        self.shift = shift

    def _create_trainer(self):
        return CountingTrainer()

    def quality(self):
        return type(self).curve[self.trainer.epochs - 1]


class ScriptedTrial:
    def __init__(self, prune_at=None):
        self.reports, self.asked, self.prune_at = [], 0, prune_at

    def report(self, value, step):
        self.reports.append((value, step))

    def should_prune(self):
        self.asked += 1
        return self.prune_at is not None and self.reports[-1][1] >= self.prune_at


def test_reports_at_the_validated_epochs_only():
    #                        epoch 1    2    3    4    5    6    7    8    9   10   11   12
    EpochRecommender.curve = [.9, .1, .9, .3, .9, .5, .9, .4, .9, .45, .9, .2, .9, .9]
    rec, trial, evaluator = EpochRecommender(X), ScriptedTrial(), FakeEvaluator()
    rec.learn_with_optimizer(evaluator, trial, max_epoch=14, validate_epoch=2, score_degradation_max=3)
    # validated after epochs 2, 4, 6 (best), 8, 10, 12: the third miss in a row ends the fit and is not reported
    assert trial.reports == [(-.1, 1), (-.3, 3), (-.5, 5), (-.4, 7), (-.45, 9)]
    assert trial.asked == 5
    assert rec.learnt_config == {"train_epochs": 6} and rec.trainer.epochs == 6  # (the best state is back)
    assert len(evaluator.scored) == 6
    # without a trial the same fit, through either method
    for fit in (lambda r: r.learn_with_optimizer(FakeEvaluator(), None, max_epoch=14, validate_epoch=2,
                                                 score_degradation_max=3),
                lambda r: r.learn_with_evaluator(FakeEvaluator(), max_epoch=14, validate_epoch=2,
                                                 score_degradation_max=3)):
        other = EpochRecommender(X)
        fit(other)
        assert other.learnt_config == {"train_epochs": 6} and other.trainer.epochs == 6
    # no evaluator: max_epoch epochs, nothing reported, nothing learnt
    plain, trial = EpochRecommender(X, train_epochs=5), ScriptedTrial()
    plain.learn_with_optimizer(None, trial, max_epoch=5)
    assert plain.trainer.epochs == 5 and trial.reports == [] and plain.learnt_config == {}
    assert EpochRecommender(X, train_epochs=3).learn().trainer.epochs == 3


def test_a_trial_that_says_prune_ends_the_fit():
    EpochRecommender.curve = [.1, .2, .3, .4, .5, .6]
    rec, trial = EpochRecommender(X), ScriptedTrial(prune_at=2)
    with pytest.raises(TrialPruned):
        rec.learn_with_optimizer(FakeEvaluator(), trial, max_epoch=6, validate_epoch=1)
    assert trial.reports == [(-.1, 0), (-.2, 1), (-.3, 2)] and rec.trainer.epochs == 3


def test_the_study_records_pruned_fits():
    # every fit climbs to its third epoch; from the second trial on the pruner compares with the first
    curves = [[.5, .6, .7, .1], [.1, .1, .1, .1], [.5, .6, .8, .1], [.4, .9, .1, .1]]

    class ByTrial(EpochRecommender):
        def quality(self):
            return curves[len(study.trials) - 1][self.trainer.epochs - 1]

    study = create_study(sampler=TPESampler(seed=0), pruner=MedianPruner(n_startup_trials=1))
    best, frame = ByTrial.tune(X, FakeEvaluator(), study=study, n_trials=4, max_epoch=4, validate_epoch=1,
                               score_degradation_max=1)
    # trial 1: -0.1 > -0.5 at step 0: pruned there.  trial 3: -0.4 > median(-0.5, -0.5) at step 0: pruned.
    assert frame["state"].tolist() == ["COMPLETE", "PRUNED", "COMPLETE", "PRUNED"]
    assert frame["value"].tolist() == [-.7, -.1, -.8, -.4]
    assert frame["train_epochs"].tolist()[::2] == [3, 3] and np.isnan(frame["ndcg@7"][1])
    assert frame["ndcg@7"].tolist()[::2] == [.7, .8]
    assert best == dict(shift=study.trials[2].params["shift"], train_epochs=3)


# ---- tune_doubling_dimension -------------------------------------------------------------------------------------
class HostIALS(R.IALSRecommender):
    """``IALSRecommender``'s tuning entry points over a fit that stays on the host: its quality peaks at
    ``alpha0 = 0.1 * n_components / 4``, ``reg = 1e-2`` and after 3 epochs"""
    built = []

    def __init__(self, X_train_all, n_components=20, alpha0=0.0, reg=1e-3, train_epochs=16):
        BaseRecommenderWithEarlyStopping.__init__(self, X_train_all, train_epochs=train_epochs)
        self.n_components, self.alpha0, self.reg = n_components, alpha0, reg
        type(self).built.append(self)

    def _create_trainer(self):
        return CountingTrainer()

    def quality(self):
        miss = (math.log10(self.alpha0 / (0.025 * self.n_components)) ** 2 + (math.log10(self.reg) + 2) ** 2
                + 0.1 * abs(self.trainer.epochs - 3))
        return (1.0 - 2.0 / self.n_components) / (1.0 + miss)


def test_tune_doubling_dimension(monkeypatch):
    made = dict(seeds=[], startups=[], names=[])

    class SeenSampler(TPESampler):
        def __init__(self, seed=None, **kw):
            made["seeds"].append(seed)
            super().__init__(seed=seed, **kw)

    class SeenPruner(MedianPruner):
        def __init__(self, n_startup_trials=5, **kw):
            made["startups"].append(n_startup_trials)
            super().__init__(n_startup_trials=n_startup_trials, **kw)

    def seen_create_study(**kw):
        made["names"].append(kw.get("study_name"))
        return create_study(**kw)

    monkeypatch.setattr(study_module, "TPESampler", SeenSampler)
    monkeypatch.setattr(study_module, "MedianPruner", SeenPruner)
    monkeypatch.setattr(study_module, "create_study", seen_create_study)
    HostIALS.built = []
    scale = 2.0
    best, frame = HostIALS.tune_doubling_dimension(
        X, FakeEvaluator(), 4, 20, study_name_prefix="run", n_trials_initial=14, n_trials_following=6,
        n_startup_trials_initial=7, n_startup_trials_following=2, neighborhood_scale=scale, random_seed=10)
    # 4, 8, 16: 32 is past the maximum
    assert made == dict(seeds=[11, 12, 13], startups=[7, 2, 2], names=["run_4", "run_8", "run_16"])
    assert frame["n_components"].tolist() == [4] * 14 + [8] * 6 + [16] * 6
    assert frame.index.tolist() == list(range(14)) + list(range(6)) * 2
    assert [r.n_components for r in HostIALS.built] == frame["n_components"].tolist()
    # the first study searches the class's range, without n_components
    first = HostIALS.built[:14]
    assert all(3e-3 <= r.alpha0 <= 1 and 1e-4 <= r.reg <= 1e-1 for r in first)
    # every later study searches around the best of the study before it
    centre = frame[frame["n_components"] == 4].sort_values("value", kind="stable").iloc[0]
    for d, rows in ((8, HostIALS.built[14:20]), (16, HostIALS.built[20:])):
        for r in rows:
            for name in ("alpha0", "reg"):
                assert centre[name] / scale <= getattr(r, name) <= centre[name] * scale, (d, name)
        assert "train_epochs" in centre.index  # (an int: learnt, not searched)
        assert len({r.alpha0 for r in rows}) == len(rows)  # (searched, not copied)
        centre = frame[frame["n_components"] == d].sort_values("value", kind="stable").iloc[0]
    # the best over all dimensions
    winner = frame.sort_values("value", kind="stable").iloc[0]
    assert best == dict(n_components=int(winner["n_components"]), alpha0=winner["alpha0"], reg=winner["reg"],
                        train_epochs=int(winner["train_epochs"]))
    assert best["n_components"] == 16 and best["train_epochs"] == 3
    # iALS's own loop defaults reached the fits: validated every epoch, given up after 3 misses
    assert all(r.trainer.epochs == r.learnt_config["train_epochs"] for r in HostIALS.built if r.learnt_config)

    with pytest.raises(ValueError):
        HostIALS.tune_doubling_dimension(X, FakeEvaluator(), 4, 8, storage="sqlite:///x.db")


def test_ials_tune_defaults():
    import inspect

    own = inspect.signature(R.IALSRecommender.tune).parameters
    base = inspect.signature(BaseRecommender.tune).parameters
    assert list(own) == list(base)
    assert (own["max_epoch"].default, own["validate_epoch"].default, own["score_degradation_max"].default) == (16, 1, 3)
    assert (base["max_epoch"].default, base["validate_epoch"].default, base["score_degradation_max"].default) == (
        128, 5, 5)
    assert base["prunning_n_startup_trials"].default == 10 and base["n_trials"].default == 20
    for name in own:
        if name not in ("max_epoch", "validate_epoch", "score_degradation_max"):
            assert own[name].default == base[name].default and own[name].kind == base[name].kind, name
