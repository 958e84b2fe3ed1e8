"""``Optimizer`` (``irspack/optimization/optimizer.py:21-203``): the objective of a tuning study.  One trial suggests
the training data and the parameters, fits the recommender against the validation evaluator (with early stopping and
pruning where the class trains by epochs), scores it, and returns minus the target metric.

Only the ``Study`` / ``Trial`` protocol of ``irspack_amd.optimization.study`` is used on ``study`` and ``trial``, and
that protocol is Optuna's by name, so an ``optuna.Study`` can be passed in its place.  The project's test machines
have no Optuna, so that path has never been run here.
"""

import logging
import re
import time
from typing import Any, Callable, Dict, List, Optional, Tuple

from .parameter_range import is_valid_param_name


def add_score_to_trial(trial: Any, score: Dict[str, float], cutoff: int) -> None:
    """Appends ``(trial number, {"<metric>@<cutoff>": value})`` to the study's ``"scores"`` attribute"""
    history: List[Tuple[int, Dict[str, float]]] = trial.study.user_attrs.get("scores", [])
    history.append((trial.number, {f"{name}@{cutoff}": value for name, value in score.items()}))
    trial.study.set_user_attr("scores", history)


def study_to_dataframe(study: Any) -> Any:
    """The study's trials indexed by ``number``, the ``params_`` / ``user_attrs_`` prefixes dropped from the column
    names, left-joined with the ``<metric>@<cutoff>`` columns that ``add_score_to_trial`` recorded"""
    import pandas as pd

    frame = study.trials_dataframe().set_index("number")
    frame.columns = [re.sub(r"^(user_attrs|params)_", "", column) for column in frame.columns]
    history = study.user_attrs.get("scores", [])
    scores = pd.DataFrame([entry[1] for entry in history], index=[entry[0] for entry in history])
    scores.index.name = "number"
    return frame.join(scores, how="left")


class Optimizer:
    """``data_suggest_function(trial)`` gives a trial's training matrix and ``parameter_suggest_function(trial)`` its
    tuned constructor arguments; ``recommender_params`` are fixed arguments laid over them.  ``max_epoch``,
    ``validate_epoch`` and ``score_degradation_max`` go to ``learn_with_optimizer`` and matter only to classes that
    train by epochs.  ``logger=None`` is ``logging.getLogger("IRSPACK")``."""

    def __init__(self, data_suggest_function: Callable[[Any], Any],
                 parameter_suggest_function: Callable[[Any], Dict[str, Any]], recommender_params: Dict[str, Any],
                 val_evaluator: Any, logger: Optional[logging.Logger] = None, max_epoch: int = 128,
                 validate_epoch: int = 5, score_degradation_max: int = 5) -> None:
        self.logger = logging.getLogger("IRSPACK") if logger is None else logger
        self._data_suggest_function = data_suggest_function
        self._parameter_suggest_function = parameter_suggest_function
        self.recommender_params = recommender_params
        self.val_evaluator = val_evaluator
        self.max_epoch = max_epoch
        self.validate_epoch = validate_epoch
        self.score_degradation_max = score_degradation_max

    def objective_function(self, recommender_class: Any) -> Callable[[Any], float]:
        """The callable to hand to ``study.optimize``: it takes a trial and returns minus the target metric"""

        def objective(trial: Any) -> float:
            began = time.time()
            data = self._data_suggest_function(trial)
            params = self._parameter_suggest_function(trial)
            params.update(self.recommender_params)
            self.logger.info("Trial %s:", trial.number)
            self.logger.info("parameter = %s", params)
            recommender = recommender_class(data, **params)
            recommender.learn_with_optimizer(self.val_evaluator, trial, max_epoch=self.max_epoch,
                                             validate_epoch=self.validate_epoch,
                                             score_degradation_max=self.score_degradation_max)
            score = self.val_evaluator.get_score(recommender)
            self.logger.info("Config %d obtained the following scores: %s within %f seconds.", trial.number, score,
                             time.time() - began)
            # what the fit itself settled, the best epoch above all, is kept with the trial
            for name, value in recommender.learnt_config.items():
                trial.set_user_attr(name, value)
            add_score_to_trial(trial, score, self.val_evaluator.cutoff)
            return -score[self.val_evaluator.target_metric.name]

        return objective

    def optimize_with_study(self, study: Any, recommender_class: Any, n_trials: int = 20,
                            timeout: Optional[float] = None) -> Tuple[Dict[str, Any], Any]:
        """Runs ``n_trials`` trials (pruned ones included) on ``study``.  Returns the best trial's parameters, joined
        by those of its user attributes whose names are valid parameter names (``train_epochs``), which can be passed
        to the recommender as keywords, and the frame of ``study_to_dataframe``."""
        self.logger.info("Start parameter search for %s", recommender_class.__name__)
        study.optimize(self.objective_function(recommender_class), n_trials=n_trials, timeout=timeout)
        best = study.best_trial
        best_params = dict(best.params)
        best_params.update({name: value for name, value in best.user_attrs.items() if is_valid_param_name(name)})
        return best_params, study_to_dataframe(study)
