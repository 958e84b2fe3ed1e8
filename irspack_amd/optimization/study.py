"""The built-in study: the part of Optuna's ``Study`` / ``Trial`` protocol that ``Optimizer`` and the recommenders'
``tune`` use, under Optuna's names, with a random sampler, an independent tree-structured Parzen estimator and a
median pruner.  Studies always minimise and live in memory; there is no storage back end and no parallel trials.

The samplers are this library's own statement of the published algorithms (Bergstra et al., "Algorithms for
Hyper-Parameter Optimization", NeurIPS 2011): nothing here claims to draw the same numbers as Optuna does.
"""

import datetime
import enum
import math
import time
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
from scipy.special import ndtr, ndtri

try:
    from optuna.exceptions import TrialPruned as _TrialPrunedBase
except ImportError:
    _TrialPrunedBase = Exception


class TrialPruned(_TrialPrunedBase):
    """Raised inside an objective to end a trial that the pruner gave up on.  Where Optuna is installed this is a
    subclass of its exception of the same name, so that either study recognises it."""


class TrialState(enum.Enum):
    RUNNING = 0
    COMPLETE = 1
    PRUNED = 2
    FAIL = 3


class _Numeric:
    """The range of a float or integer parameter"""

    def __init__(self, kind: str, low: Any, high: Any, step: Any, log: bool) -> None:
        self.kind, self.low, self.high, self.step, self.log = kind, low, high, step, log

    def _key(self) -> Tuple:
        return (self.kind, self.low, self.high, self.step, self.log)

    def __eq__(self, other: Any) -> bool:
        return isinstance(other, _Numeric) and self._key() == other._key()

    def n_grid(self) -> int:
        """how many values ``low + k * step <= high`` there are (a stepped range only)"""
        return int(math.floor((self.high - self.low) / self.step + 1e-9)) + 1

    def interval(self) -> Tuple[float, float]:
        """the continuous interval the samplers work in: the log of a log range, and a grid widened by half a step
        on either side, so that rounding gives every grid point the same share"""
        if self.step is None:
            low, high = float(self.low), float(self.high)
        else:
            half = 0.5 * self.step
            low, high = self.low - half, self.low + (self.n_grid() - 1) * self.step + half
        return (math.log(low), math.log(high)) if self.log else (low, high)

    def to_internal(self, value: Any) -> float:
        return math.log(value) if self.log else float(value)

    def from_internal(self, x: float) -> Any:
        value = math.exp(x) if self.log else x
        if self.step is not None:
            k = min(max(int(round((value - self.low) / self.step)), 0), self.n_grid() - 1)
            value = self.low + k * self.step
        value = min(max(value, self.low), self.high)
        return int(value) if self.kind == "int" else float(value)


class _Categorical:
    def __init__(self, choices: Sequence[Any]) -> None:
        self.choices = list(choices)

    def __eq__(self, other: Any) -> bool:
        return isinstance(other, _Categorical) and self.choices == other.choices


class RandomSampler:
    """Every parameter uniformly over its range (over its logarithm for a log range)"""

    def __init__(self, seed: Optional[int] = None) -> None:
        self._rng = np.random.RandomState(seed)

    def sample(self, study: "Study", trial: "Trial", name: str, dist: Any) -> Any:
        if isinstance(dist, _Categorical):
            return dist.choices[int(self._rng.randint(len(dist.choices)))]
        low, high = dist.interval()
        return dist.from_internal(float(self._rng.uniform(low, high)))


class _ParzenEstimator:
    """A mixture of Gaussians truncated to ``[low, high]``: one per observation and one wide prior at the centre,
    equally weighted.  An observation's width is the larger distance to its neighbours (the ends of the interval
    count as neighbours), kept inside ``[(high - low) / min(100, 1 + n), high - low]``."""

    def __init__(self, observations: np.ndarray, low: float, high: float) -> None:
        width = high - low
        order = np.argsort(np.append(observations, 0.5 * (low + high)), kind="stable")
        mus = np.append(observations, 0.5 * (low + high))[order]
        prior_at = int(np.nonzero(order == len(observations))[0][0])
        edges = np.concatenate([[low], mus, [high]])
        sigmas = np.maximum(edges[1:-1] - edges[:-2], edges[2:] - edges[1:-1])
        sigmas = np.clip(sigmas, width / min(100.0, 1.0 + len(mus)), width)
        sigmas[prior_at] = width
        self.low, self.high, self.mus, self.sigmas = low, high, mus, sigmas
        self._cdf_low = ndtr((low - mus) / sigmas)
        self._cdf_high = ndtr((high - mus) / sigmas)

    def sample(self, rng: np.random.RandomState, n: int) -> np.ndarray:
        which = rng.randint(len(self.mus), size=n)
        u = rng.uniform(size=n)
        p = self._cdf_low[which] + u * (self._cdf_high[which] - self._cdf_low[which])
        return np.clip(self.mus[which] + self.sigmas[which] * ndtri(p), self.low, self.high)

    def log_pdf(self, x: np.ndarray) -> np.ndarray:
        z = (x[:, None] - self.mus[None, :]) / self.sigmas[None, :]
        log_terms = (-0.5 * z * z - np.log(self.sigmas * math.sqrt(2.0 * math.pi) * len(self.mus)
                                          * (self._cdf_high - self._cdf_low))[None, :])
        top = log_terms.max(axis=1)
        return top + np.log(np.exp(log_terms - top[:, None]).sum(axis=1))


class TPESampler(RandomSampler):
    """The independent tree-structured Parzen estimator: every parameter on its own.

    Of the finished trials that hold the parameter with the same range, ordered by ``(state != COMPLETE, value)``,
    the best ``min(ceil(0.1 n), 25)`` make the density ``l`` and the rest make ``g``; ``n_ei_candidates`` values are
    drawn from ``l`` and the one with the largest ``l / g`` is suggested.  Numbers are modelled in the interval of
    ``_Numeric.interval``; a categorical parameter by its counts in the two groups plus one per choice.  With fewer
    than ``n_startup_trials`` such trials the value is drawn as by ``RandomSampler``.  All draws come from one
    generator, so with a seed the suggestions depend on the seed and the reported values alone."""

    def __init__(self, seed: Optional[int] = None, n_startup_trials: int = 10, n_ei_candidates: int = 24) -> None:
        super().__init__(seed)
        self.n_startup_trials = n_startup_trials
        self.n_ei_candidates = n_ei_candidates

    def sample(self, study: "Study", trial: "Trial", name: str, dist: Any) -> Any:
        seen = [t for t in study.trials
                if t.state in (TrialState.COMPLETE, TrialState.PRUNED) and t.value is not None
                and name in t.params and t.distributions[name] == dist]
        if len(seen) < self.n_startup_trials:
            return super().sample(study, trial, name, dist)
        seen.sort(key=lambda t: (t.state is not TrialState.COMPLETE, t.value))  # (stable: ties by number)
        n_below = min(int(math.ceil(0.1 * len(seen))), 25)
        below = [t.params[name] for t in seen[:n_below]]
        above = [t.params[name] for t in seen[n_below:]]
        if isinstance(dist, _Categorical):
            return self._sample_categorical(dist, below, above)
        low, high = dist.interval()
        l, g = (_ParzenEstimator(np.array([dist.to_internal(v) for v in values], dtype=np.float64), low, high)
                for values in (below, above))
        candidates = l.sample(self._rng, self.n_ei_candidates)
        return dist.from_internal(float(candidates[int(np.argmax(l.log_pdf(candidates) - g.log_pdf(candidates)))]))

    def _sample_categorical(self, dist: _Categorical, below: List[Any], above: List[Any]) -> Any:
        def weights(values: List[Any]) -> np.ndarray:
            counts = np.ones(len(dist.choices), dtype=np.float64)
            for v in values:
                counts[dist.choices.index(v)] += 1.0
            return counts / counts.sum()

        l, g = weights(below), weights(above)
        candidates = self._rng.choice(len(dist.choices), size=self.n_ei_candidates, p=l)
        return dist.choices[int(candidates[int(np.argmax(l[candidates] / g[candidates]))])]


class MedianPruner:
    """Gives up on a trial whose best reported value so far is worse than the median of what the complete trials
    reported at the same step.  It never prunes while fewer than ``n_startup_trials`` trials are complete, before
    step ``n_warmup_steps``, or at a step that no complete trial reported."""

    def __init__(self, n_startup_trials: int = 5, n_warmup_steps: int = 0) -> None:
        self.n_startup_trials = n_startup_trials
        self.n_warmup_steps = n_warmup_steps

    def prune(self, study: "Study", trial: "Trial") -> bool:
        if not trial.intermediate_values:
            return False
        step = trial.last_step
        complete = [t for t in study.trials if t.state is TrialState.COMPLETE]
        if len(complete) < self.n_startup_trials or step < self.n_warmup_steps:
            return False
        others = [t.intermediate_values[step] for t in complete if step in t.intermediate_values]
        if not others:
            return False
        return bool(min(trial.intermediate_values.values()) > float(np.median(others)))


class Trial:
    """One evaluation of the objective: the parameters it was given, what it reported, and how it ended"""

    def __init__(self, study: "Study", number: int) -> None:
        self.study = study
        self.number = number
        self.params: Dict[str, Any] = {}
        self.distributions: Dict[str, Any] = {}
        self.user_attrs: Dict[str, Any] = {}
        self.intermediate_values: Dict[int, float] = {}
        self.last_step: Optional[int] = None
        self.state = TrialState.RUNNING
        self.value: Optional[float] = None
        self.datetime_start = datetime.datetime.now()
        self.datetime_complete: Optional[datetime.datetime] = None

    def _suggest(self, name: str, dist: Any) -> Any:
        if name not in self.params:  # (asked twice, a name keeps its value)
            self.distributions[name] = dist
            if isinstance(dist, _Numeric) and dist.low == dist.high:
                self.params[name] = dist.low
            else:
                self.params[name] = self.study.sampler.sample(self.study, self, name, dist)
        return self.params[name]

    def suggest_float(self, name: str, low: float, high: float, *, step: Optional[float] = None,
                      log: bool = False) -> float:
        if low > high:
            raise ValueError(f"'{name}': got low > high.")
        if log and (low <= 0 or step is not None):
            raise ValueError(f"'{name}': a log range needs low > 0 and no step.")
        if step is not None and step <= 0:
            raise ValueError(f"'{name}': step must be positive.")
        return self._suggest(name, _Numeric("float", float(low), float(high), step, log))

    def suggest_int(self, name: str, low: int, high: int, *, step: int = 1, log: bool = False) -> int:
        if low > high:
            raise ValueError(f"'{name}': got low > high.")
        if log and (low < 1 or step != 1):
            raise ValueError(f"'{name}': a log range needs low >= 1 and step == 1.")
        if step < 1:
            raise ValueError(f"'{name}': step must be a positive integer.")
        return self._suggest(name, _Numeric("int", int(low), int(high), int(step), log))

    def suggest_categorical(self, name: str, choices: Sequence[Any]) -> Any:
        if len(choices) == 0:
            raise ValueError(f"'{name}': no choices.")
        return self._suggest(name, _Categorical(choices))

    def set_user_attr(self, key: str, value: Any) -> None:
        self.user_attrs[key] = value

    def report(self, value: float, step: int) -> None:
        self.intermediate_values[int(step)] = float(value)
        self.last_step = int(step)

    def should_prune(self) -> bool:
        return self.study.pruner.prune(self.study, self)

    @property
    def duration(self) -> Optional[datetime.timedelta]:
        return None if self.datetime_complete is None else self.datetime_complete - self.datetime_start


class Study:
    def __init__(self, sampler: Any, pruner: Any, study_name: Optional[str] = None) -> None:
        self.sampler = sampler
        self.pruner = pruner
        self.study_name = study_name
        self.direction = "minimize"
        self.trials: List[Trial] = []
        self.user_attrs: Dict[str, Any] = {}

    def set_user_attr(self, key: str, value: Any) -> None:
        self.user_attrs[key] = value

    def optimize(self, func: Callable[[Trial], float], n_trials: Optional[int] = None,
                 timeout: Optional[float] = None) -> None:
        """Runs ``func`` on new trials until ``n_trials`` have run or, looked at between trials only, ``timeout``
        seconds have passed: the first trial always runs and a running trial is never interrupted.  ``TrialPruned``
        ends a trial as ``PRUNED`` with its last reported value; any other exception marks it ``FAIL`` and goes on
        to the caller.  A value that is not a number marks the trial ``FAIL`` and the study goes on."""
        began = time.monotonic()
        done = 0
        while n_trials is None or done < n_trials:
            trial = Trial(self, len(self.trials))
            self.trials.append(trial)
            try:
                value = float(func(trial))
                trial.value = value
                trial.state = TrialState.FAIL if math.isnan(value) else TrialState.COMPLETE
            except TrialPruned:
                trial.state = TrialState.PRUNED
                if trial.last_step is not None:
                    trial.value = trial.intermediate_values[trial.last_step]
            except BaseException:
                trial.state = TrialState.FAIL
                raise
            finally:
                trial.datetime_complete = datetime.datetime.now()
            done += 1
            if timeout is not None and time.monotonic() - began >= timeout:
                break

    @property
    def best_trial(self) -> Trial:
        complete = [t for t in self.trials if t.state is TrialState.COMPLETE]
        if not complete:
            raise ValueError("No trials are completed yet.")
        return min(complete, key=lambda t: (t.value, t.number))

    @property
    def best_params(self) -> Dict[str, Any]:
        return self.best_trial.params

    @property
    def best_value(self) -> float:
        return self.best_trial.value

    def trials_dataframe(self) -> Any:
        """One row per trial: ``number``, ``value``, ``datetime_start``, ``datetime_complete``, ``duration``, one
        ``params_<name>`` and one ``user_attrs_<name>`` column per name that any trial holds, and ``state``"""
        import pandas as pd

        def names(of: Callable[[Trial], Dict[str, Any]]) -> List[str]:
            return list(dict.fromkeys(key for t in self.trials for key in of(t)))

        param_names, attr_names = names(lambda t: t.params), names(lambda t: t.user_attrs)
        columns = (["number", "value", "datetime_start", "datetime_complete", "duration"]
                   + [f"params_{n}" for n in param_names] + [f"user_attrs_{n}" for n in attr_names] + ["state"])
        rows = []
        for t in self.trials:
            row = dict(number=t.number, value=t.value, datetime_start=t.datetime_start,
                       datetime_complete=t.datetime_complete, duration=t.duration, state=t.state.name)
            row.update({f"params_{n}": t.params[n] for n in param_names if n in t.params})
            row.update({f"user_attrs_{n}": t.user_attrs[n] for n in attr_names if n in t.user_attrs})
            rows.append(row)
        frame = pd.DataFrame(rows, columns=columns)
        frame["value"] = frame["value"].astype(float)
        return frame


def create_study(sampler: Any = None, pruner: Any = None, study_name: Optional[str] = None) -> Study:
    """A new in-memory study that minimises.  The defaults are ``TPESampler()`` and ``MedianPruner()``."""
    return Study(TPESampler() if sampler is None else sampler, MedianPruner() if pruner is None else pruner,
                 study_name)
