"""Hyper-parameter tuning (``irspack.optimization``): parameter ranges, the ``Optimizer`` that turns a recommender
class and a validation evaluator into an objective, and the built-in study that runs it where Optuna is absent."""

from .optimizer import Optimizer, add_score_to_trial, study_to_dataframe
from .parameter_range import (CategoricalRange, LogUniformFloatRange, LogUniformIntegerRange, ParameterRange,
                              UniformFloatRange, UniformIntegerRange, default_tune_range_knn,
                              default_tune_range_knn_with_weighting, is_valid_param_name)
from .study import (MedianPruner, RandomSampler, Study, TPESampler, Trial, TrialPruned, TrialState,
                    create_study)

__all__ = ["Optimizer", "add_score_to_trial", "study_to_dataframe", "ParameterRange", "UniformFloatRange",
           "LogUniformFloatRange", "UniformIntegerRange", "LogUniformIntegerRange", "CategoricalRange",
           "default_tune_range_knn", "default_tune_range_knn_with_weighting", "is_valid_param_name",
           "create_study", "Study", "Trial", "TrialState", "TrialPruned", "RandomSampler", "TPESampler",
           "MedianPruner"]
