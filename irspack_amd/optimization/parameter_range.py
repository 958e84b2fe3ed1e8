"""Search ranges of tunable parameters (``irspack/optimization/parameter_range.py``): a range knows its parameter's
name and bounds and asks a trial for a value through the ``suggest_float`` / ``suggest_int`` / ``suggest_categorical``
calls of Optuna's ``Trial`` protocol, which ``irspack_amd.optimization.study.Trial`` implements."""

import re
from typing import Any, List

_PARAM_NAME = re.compile(r"^([a-zA-Z\d]+[\-_]*)+$")


def is_valid_param_name(name: str) -> bool:
    """True for names made of alphanumeric runs, each optionally followed by ``-`` / ``_``"""
    return _PARAM_NAME.match(name) is not None


class ParameterRange:
    """The range one parameter is searched in.  ``suggest(trial, prefix)`` asks ``trial`` for a value under the
    name ``prefix + name``."""

    def __init__(self, name: str) -> None:
        if not is_valid_param_name(name):
            raise ValueError(f'"{name}" is not a valid parameter name: it has to match {_PARAM_NAME.pattern!r}.')
        self.name = name

    def suggest(self, trial: Any, prefix: str = "") -> Any:
        raise NotImplementedError('"suggest" must be implemented.')


class _Interval(ParameterRange):
    def __init__(self, name: str, low: Any, high: Any) -> None:
        super().__init__(name)
        if low > high:
            raise ValueError("Got low > high.")
        self.low = low
        self.high = high


class UniformFloatRange(_Interval):
    def __init__(self, name: str, low: float, high: float) -> None:
        super().__init__(name, low, high)

    def suggest(self, trial: Any, prefix: str = "") -> Any:
        return trial.suggest_float(prefix + self.name, self.low, self.high)


class LogUniformFloatRange(_Interval):
    def __init__(self, name: str, low: float, high: float) -> None:
        super().__init__(name, low, high)

    def suggest(self, trial: Any, prefix: str = "") -> Any:
        return trial.suggest_float(prefix + self.name, self.low, self.high, log=True)


class UniformIntegerRange(_Interval):
    def __init__(self, name: str, low: int, high: int, step: int = 1) -> None:
        super().__init__(name, low, high)
        self.step = step

    def suggest(self, trial: Any, prefix: str = "") -> Any:
        return trial.suggest_int(prefix + self.name, self.low, self.high, step=self.step)


class LogUniformIntegerRange(_Interval):
    def __init__(self, name: str, low: int, high: int) -> None:
        super().__init__(name, low, high)

    def suggest(self, trial: Any, prefix: str = "") -> Any:
        return trial.suggest_int(prefix + self.name, self.low, self.high, log=True)


class CategoricalRange(ParameterRange):
    def __init__(self, name: str, choices: List[Any]) -> None:
        super().__init__(name)
        self.choices = choices

    def suggest(self, trial: Any, prefix: str = "") -> Any:
        return trial.suggest_categorical(prefix + self.name, self.choices)


default_tune_range_knn: List[ParameterRange] = [
    UniformIntegerRange("top_k", 4, 1000),
    UniformFloatRange("shrinkage", 0, 1000),
]

default_tune_range_knn_with_weighting: List[ParameterRange] = default_tune_range_knn + [
    CategoricalRange("feature_weighting", ["NONE", "TF_IDF", "BM_25"]),
]
