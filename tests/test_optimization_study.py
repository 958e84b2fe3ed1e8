"""``irspack_amd.optimization``: the parameter ranges, the built-in ``Study`` / ``Trial``, the two samplers and the
median pruner, on the host alone."""
import collections
import math

import numpy as np
import pytest

from irspack_amd.optimization import (CategoricalRange, LogUniformFloatRange, LogUniformIntegerRange, MedianPruner,
                                      ParameterRange, RandomSampler, TPESampler, TrialPruned, UniformFloatRange,
                                      UniformIntegerRange, create_study, default_tune_range_knn,
                                      default_tune_range_knn_with_weighting, is_valid_param_name)


# ---- ranges ------------------------------------------------------------------------------------------------------
def test_parameter_names():
    for good in ("alpha", "top_k", "n_components", "a1", "kl-anneal_goal", "x_"):
        assert is_valid_param_name(good), good
    for bad in ("", "_x", "ndcg@10", "a b", "a.b", "-x"):
        assert not is_valid_param_name(bad), bad
    with pytest.raises(ValueError):
        UniformFloatRange("ndcg@10", 0, 1)
    with pytest.raises(ValueError):
        CategoricalRange("", [1])


@pytest.mark.parametrize("cls", [UniformFloatRange, LogUniformFloatRange, UniformIntegerRange,
                                 LogUniformIntegerRange])
def test_low_above_high(cls):
    with pytest.raises(ValueError, match="Got low > high."):
        cls("x", 3, 2)
    r = cls("x", 2, 2)  # (equal bounds are a range)
    assert isinstance(r, ParameterRange) and (r.low, r.high) == (2, 2)


class RecordingTrial:
    def __init__(self):
        self.calls = []

    def suggest_float(self, name, low, high, **kw):
        self.calls.append(("float", name, low, high, kw))
        return "f"

    def suggest_int(self, name, low, high, **kw):
        self.calls.append(("int", name, low, high, kw))
        return "i"

    def suggest_categorical(self, name, choices):
        self.calls.append(("categorical", name, choices))
        return "c"


def test_suggest_forwards_to_the_trial():
    t = RecordingTrial()
    assert UniformFloatRange("a", 0.5, 2).suggest(t) == "f"
    assert LogUniformFloatRange("b", 1e-3, 1).suggest(t, prefix="p_") == "f"
    assert UniformIntegerRange("c", 1, 9).suggest(t) == "i"
    assert UniformIntegerRange("d", 1, 9, step=4).suggest(t, "q_") == "i"
    assert LogUniformIntegerRange("e", 1, 64).suggest(t) == "i"
    assert CategoricalRange("f", ["x", "y"]).suggest(t, prefix="r_") == "c"
    floats, ints = t.calls[:2], t.calls[2:5]
    assert [c[:4] for c in floats] == [("float", "a", 0.5, 2), ("float", "p_b", 1e-3, 1)]
    assert not floats[0][4].get("log", False) and floats[1][4] == {"log": True}
    assert [c[:4] for c in ints] == [("int", "c", 1, 9), ("int", "q_d", 1, 9), ("int", "e", 1, 64)]
    assert ints[0][4] == {"step": 1} and ints[1][4] == {"step": 4} and ints[2][4] == {"log": True}
    assert t.calls[5] == ("categorical", "r_f", ["x", "y"])


def test_shared_knn_ranges():
    assert [(r.name, type(r), r.low, r.high) for r in default_tune_range_knn] == [
        ("top_k", UniformIntegerRange, 4, 1000), ("shrinkage", UniformFloatRange, 0, 1000)]
    assert [r.name for r in default_tune_range_knn_with_weighting] == ["top_k", "shrinkage", "feature_weighting"]
    assert default_tune_range_knn_with_weighting[2].choices == ["NONE", "TF_IDF", "BM_25"]


# ---- Trial -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler, n_trials", [(RandomSampler, 1000), (TPESampler, 150)])  # (7 draws per trial)
def test_suggestions_stay_inside_their_ranges(sampler, n_trials):
    seen = collections.defaultdict(set)

    def objective(trial):
        x = trial.suggest_float("x", -2.0, 3.0)
        lx = trial.suggest_float("lx", 1e-5, 1e-1, log=True)
        sx = trial.suggest_float("sx", 0.0, 1.0, step=0.25)
        i = trial.suggest_int("i", -3, 4)
        si = trial.suggest_int("si", 2, 12, step=3)  # (12 is off the grid 2, 5, 8, 11)
        li = trial.suggest_int("li", 1, 40, log=True)
        c = trial.suggest_categorical("c", ["a", None, 3])
        assert -2.0 <= x <= 3.0 and 1e-5 <= lx <= 1e-1
        assert type(x) is float and type(lx) is float and type(sx) is float
        assert sx in (0.0, 0.25, 0.5, 0.75, 1.0)
        assert type(i) is int and type(si) is int and type(li) is int
        assert -3 <= i <= 4 and si in (2, 5, 8, 11) and 1 <= li <= 40
        assert c in ("a", None, 3)
        for name, value in (("sx", sx), ("i", i), ("si", si), ("c", c)):
            seen[name].add(value)
        # asked again, a name keeps its value
        assert trial.suggest_float("x", -2.0, 3.0) == x and trial.suggest_int("si", 2, 12, step=3) == si
        assert trial.suggest_categorical("c", ["a", None, 3]) is c
        assert trial.params == dict(x=x, lx=lx, sx=sx, i=i, si=si, li=li, c=c)
        return x * x + lx + i

    study = create_study(sampler=sampler(seed=0))
    study.optimize(objective, n_trials=n_trials)
    assert len(study.trials) == n_trials
    if sampler is TPESampler:  # (it concentrates where the objective is low)
        return
    # every grid point and choice is reachable, the ends included
    assert seen["sx"] == {0.0, 0.25, 0.5, 0.75, 1.0} and seen["i"] == set(range(-3, 5))
    assert seen["si"] == {2, 5, 8, 11} and seen["c"] == {"a", None, 3}


def test_invalid_suggestions():
    def attempt(call):
        def objective(trial):
            call(trial)
            return 0.0

        with pytest.raises(ValueError):
            create_study(sampler=RandomSampler(seed=0)).optimize(objective, n_trials=1)

    attempt(lambda t: t.suggest_float("x", 0.0, 1.0, log=True))
    attempt(lambda t: t.suggest_float("x", -1.0, 1.0, log=True))
    attempt(lambda t: t.suggest_float("x", 2.0, 1.0))
    attempt(lambda t: t.suggest_int("x", 0, 8, log=True))
    attempt(lambda t: t.suggest_int("x", 1, 8, step=2, log=True))
    attempt(lambda t: t.suggest_int("x", 3, 2))


def test_equal_bounds_return_the_bound():
    def objective(trial):
        assert trial.suggest_float("a", 0.7, 0.7) == 0.7
        assert trial.suggest_float("b", 0.7, 0.7, log=True) == 0.7
        assert trial.suggest_int("c", 5, 5) == 5 and type(trial.params["c"]) is int
        return 0.0

    create_study(sampler=TPESampler(seed=0, n_startup_trials=2)).optimize(objective, n_trials=5)


# ---- samplers ----------------------------------------------------------------------------------------------------
def bowl(trial):
    x = trial.suggest_float("x", 1e-4, 1.0, log=True)
    y = trial.suggest_float("y", 0.0, 1.0)
    return (math.log10(x) + 2) ** 2 + (y - 0.3) ** 2


def mixed(trial):
    k = trial.suggest_int("k", 4, 300)
    c = trial.suggest_categorical("c", ["p", "q", "r"])
    return bowl(trial) + abs(k - 100) / 100 + (c != "q")


def test_a_seed_fixes_the_suggestions():
    def params(seed):
        study = create_study(sampler=TPESampler(seed=seed))
        study.optimize(mixed, n_trials=30)
        frame = study.trials_dataframe()
        return frame[[c for c in frame.columns if c.startswith("params_")]]

    a, b, other = params(3), params(3), params(4)
    assert sorted(a.columns) == ["params_c", "params_k", "params_x", "params_y"]
    assert a.equals(b)
    assert not a.equals(other)
    # past the start-up trials too
    assert not a.iloc[10:].reset_index(drop=True).equals(other.iloc[10:].reset_index(drop=True))


def test_tpe_beats_random_search():
    """the mean best value of 60 trials over seeds 0..19: TPE at most half of plain random search"""
    tpe, baseline = [], []
    for seed in range(20):
        study = create_study(sampler=TPESampler(seed=seed))
        study.optimize(bowl, n_trials=60)
        tpe.append(study.best_value)
        rng = np.random.RandomState(seed)
        best = np.inf
        for _ in range(60):
            x = 10 ** rng.uniform(-4, 0)
            y = rng.uniform(0, 1)
            best = min(best, (math.log10(x) + 2) ** 2 + (y - 0.3) ** 2)
        baseline.append(best)
    print(f"TPE {np.mean(tpe):.4f}  random search {np.mean(baseline):.4f}")
    assert np.mean(tpe) <= 0.5 * np.mean(baseline)


@pytest.mark.parametrize("seed", range(5))
def test_tpe_finds_the_good_category(seed):
    def objective(trial):
        choice = trial.suggest_categorical("choice", ["a", "b", "c", "d"])
        trial.suggest_float("nuisance", 0.0, 1.0)
        return 0.0 if choice == "b" else 1.0

    study = create_study(sampler=TPESampler(seed=seed))
    study.optimize(objective, n_trials=40)
    counts = collections.Counter(t.params["choice"] for t in study.trials[20:40])
    assert all(counts["b"] > n for c, n in counts.items() if c != "b"), counts


def test_tpe_counts_only_trials_with_the_same_range():
    """a parameter whose range changes from trial to trial never has ``n_startup_trials`` comparable trials, so
    the sampler stays uniform: it draws what RandomSampler draws from the same seed"""
    def objective(trial):
        return trial.suggest_float("x", 0.0, 1.0 + trial.number)

    a, b = create_study(sampler=TPESampler(seed=1, n_startup_trials=3)), create_study(sampler=RandomSampler(seed=1))
    a.optimize(objective, n_trials=12)
    b.optimize(objective, n_trials=12)
    assert [t.params for t in a.trials] == [t.params for t in b.trials]


# ---- MedianPruner ------------------------------------------------------------------------------------------------
def run_scripted(pruner, scripts):
    """One trial per script, a list of ``(step, value)`` reports; a trial ends at its first ``should_prune()``.
    Returns the study and, per trial, the answers of ``should_prune()``."""
    answers = []

    def objective(trial):
        mine = []
        answers.append(mine)
        for step, value in scripts[trial.number]:
            trial.report(value, step)
            mine.append(trial.should_prune())
            if mine[-1]:
                raise TrialPruned()
        return scripts[trial.number][-1][1]

    study = create_study(sampler=RandomSampler(seed=0), pruner=pruner)
    study.optimize(objective, n_trials=len(scripts))
    return study, answers


def test_median_pruner_waits_for_its_startup_trials():
    flat = [(0, 1.0), (1, 1.0)]
    worse = [(0, 9.0), (1, 9.0)]
    study, answers = run_scripted(MedianPruner(n_startup_trials=3), [flat, worse, flat, worse, worse])
    # trials 1 ran with 1 complete trial and trial 3 with 3: only the latter is pruned, at its first report
    assert answers == [[False, False], [False, False], [False, False], [True], [True]]
    assert [t.state.name for t in study.trials] == ["COMPLETE", "COMPLETE", "COMPLETE", "PRUNED", "PRUNED"]
    # one complete trial short, nothing is pruned
    _, answers = run_scripted(MedianPruner(n_startup_trials=4), [flat, worse, flat, worse])
    assert all(not any(a) for a in answers)


def test_median_pruner_rule():
    done = [[(0, 1.0), (1, 0.5), (3, 0.2)], [(0, 3.0), (1, 2.5), (3, 0.1)], [(0, 2.0), (1, 0.7)]]
    # medians of the complete trials: step 0: 2.0; step 1: 0.7; step 3: 0.15 (two trials); step 2: nobody

    def answers_of(script, **kw):
        _, answers = run_scripted(MedianPruner(n_startup_trials=3, **kw), done + [script])
        return answers[3]

    assert answers_of([(0, 2.0)]) == [False]  # equal to the median
    assert answers_of([(0, 2.0 + 1e-9)]) == [True]
    assert answers_of([(0, 1.9), (1, 0.8)]) == [False, True]
    # the best value so far is what counts, not the last: 0.6 at step 0 keeps the trial alive at step 1
    assert answers_of([(0, 0.6), (1, 5.0)]) == [False, False]
    # a step that no complete trial reported
    assert answers_of([(2, 100.0)]) == [False]
    assert answers_of([(7, 100.0)]) == [False]
    # the median over those complete trials that reported the step
    assert answers_of([(3, 0.15)]) == [False] and answers_of([(3, 0.16)]) == [True]
    # warm-up steps
    assert answers_of([(0, 100.0), (1, 100.0)], n_warmup_steps=1) == [False, True]
    assert answers_of([(0, 100.0), (1, 100.0)], n_warmup_steps=2) == [False, False]


def test_should_prune_before_any_report():
    def objective(trial):
        assert trial.should_prune() is False
        return 0.0

    create_study(pruner=MedianPruner(n_startup_trials=0)).optimize(objective, n_trials=3)


# ---- Study -------------------------------------------------------------------------------------------------------
class Boom(Exception):
    pass


def test_study_states_and_best_trial():
    values = {0: 3.0, 2: 1.0, 4: 1.0, 5: 2.0}

    def objective(trial):
        trial.suggest_float("x", 0.0, 1.0)
        trial.set_user_attr("twice", 2 * trial.number)
        if trial.number == 1:
            trial.report(0.5, 0)
            trial.report(0.25, 4)
            raise TrialPruned()
        if trial.number == 3:
            raise Boom("no")
        return values[trial.number]

    study = create_study(sampler=RandomSampler(seed=0), study_name="s")
    study.optimize(objective, n_trials=3)
    with pytest.raises(Boom):
        study.optimize(objective, n_trials=3)
    assert len(study.trials) == 4  # (the failure ended that call)
    study.optimize(objective, n_trials=2)
    assert [t.state.name for t in study.trials] == ["COMPLETE", "PRUNED", "COMPLETE", "FAIL", "COMPLETE", "COMPLETE"]
    assert [t.number for t in study.trials] == list(range(6))
    assert study.trials[1].value == 0.25 and study.trials[3].value is None
    # the pruned trial's 0.25 is the lowest value and does not count; of the two 1.0 the lower number wins
    assert study.best_trial is study.trials[2]
    assert study.best_value == 1.0 and study.best_params == study.trials[2].params
    assert study.trials[2].user_attrs == {"twice": 4} and study.trials[2].study is study
    study.set_user_attr("note", [1])
    assert study.user_attrs == {"note": [1]}

    frame = study.trials_dataframe()
    assert list(frame.columns) == ["number", "value", "datetime_start", "datetime_complete", "duration", "params_x",
                                   "user_attrs_twice", "state"]
    assert frame["number"].tolist() == list(range(6))
    assert frame["state"].tolist() == [t.state.name for t in study.trials]
    assert frame["value"].tolist()[:3] == [3.0, 0.25, 1.0] and np.isnan(frame["value"][3])
    assert (frame["datetime_complete"] >= frame["datetime_start"]).all()
    assert (frame["duration"] == frame["datetime_complete"] - frame["datetime_start"]).all()
    assert frame["params_x"].tolist() == [t.params["x"] for t in study.trials]


def test_no_complete_trial():
    study = create_study()
    for attribute in ("best_trial", "best_params", "best_value"):
        with pytest.raises(ValueError):
            getattr(study, attribute)

    def pruned(trial):
        raise TrialPruned()

    study.optimize(pruned, n_trials=2)
    assert [t.state.name for t in study.trials] == ["PRUNED", "PRUNED"] and study.trials[0].value is None
    with pytest.raises(ValueError):
        study.best_trial
    with pytest.raises(Boom):
        study.optimize(lambda trial: (_ for _ in ()).throw(Boom()), n_trials=1)
    with pytest.raises(ValueError):
        study.best_trial
    assert study.trials_dataframe()["state"].tolist() == ["PRUNED", "PRUNED", "FAIL"]


def test_timeout_is_checked_between_trials():
    study = create_study(sampler=RandomSampler(seed=0))
    study.optimize(lambda trial: trial.suggest_float("x", 0, 1), n_trials=5, timeout=0)
    assert len(study.trials) == 1 and study.trials[0].state.name == "COMPLETE"
    study.optimize(lambda trial: trial.suggest_float("x", 0, 1), timeout=0)  # (no n_trials: the timeout alone ends it)
    assert len(study.trials) == 2
    study.optimize(lambda trial: trial.suggest_float("x", 0, 1), n_trials=3, timeout=3600)
    assert len(study.trials) == 5


def test_trial_pruned_is_optunas_where_optuna_is():
    try:
        from optuna.exceptions import TrialPruned as theirs
    except ImportError:
        assert TrialPruned.__bases__ == (Exception,)
    else:
        assert issubclass(TrialPruned, theirs)
