"""Minimal recommender base: the caller contract of the reference's
``irspack/recommenders/base.py:79-126, 290-337, 406-429`` that the hot path relies on
(matrix normalisation, ``learn``, seen-item masking, similarity scoring), and its tuning entry
points (``base.py:132-282``: ``default_tune_range``, ``learn_with_optimizer``, ``tune``) on top of
``irspack_amd.optimization``.  The registry metaclass and config classes are out of scope.
"""

import logging
from typing import Any, Callable, Dict, List, Optional, Tuple, Union

import numpy as np
import scipy.sparse as sps

from ..optimization.parameter_range import ParameterRange


def _sparse_to_array(U: Any) -> np.ndarray:
    if sps.issparse(U):
        return np.asarray(U.toarray())
    return np.asarray(U)


class BaseRecommender:
    # the ranges that ``tune`` searches when the caller gives no ``parameter_suggest_function``
    default_tune_range: List[ParameterRange] = []

    def __init__(self, X_train_all: Any, **kwargs: Any) -> None:
        # base.py:94-101
        self.X_train_all: sps.csr_matrix = sps.csr_matrix(X_train_all).astype(np.float64)
        self.n_users: int = self.X_train_all.shape[0]
        self.n_items: int = self.X_train_all.shape[1]
        self.X_train_all.sort_indices()
        # what the fit itself settles, e.g. the epoch with the best validation score (base.py:103-105)
        self.learnt_config: Dict[str, Any] = {}

    def learn(self):
        self._learn()
        return self

    def learn_with_optimizer(self, evaluator: Any, trial: Any, max_epoch: int = 128, validate_epoch: int = 5,
                             score_degradation_max: int = 5) -> None:
        """base.py:132-163: the fit of one tuning trial.  A class that does not train by epochs has nothing to
        stop early or prune, so the evaluator, the trial and the three numbers play no part."""
        self.learn()

    @classmethod
    def default_suggest_parameter(cls, trial: Any, recommender_params: Dict[str, Any]) -> Dict[str, Any]:
        # base.py:165-173: a fixed parameter is not searched
        return {r.name: r.suggest(trial) for r in cls.default_tune_range if r.name not in recommender_params}

    @classmethod
    def tune(cls, data: Any, evaluator: Any, study: Any = None, n_trials: int = 20,
             timeout: Optional[int] = None, data_suggest_function: Optional[Callable[[Any], Any]] = None,
             parameter_suggest_function: Optional[Callable[[Any], Dict[str, Any]]] = None,
             tuning_random_seed: Optional[int] = None, prunning_n_startup_trials: int = 10, max_epoch: int = 128,
             validate_epoch: int = 5, score_degradation_max: int = 5, logger: Optional[logging.Logger] = None,
             **recommender_params: Any) -> Tuple[Dict[str, Any], Any]:
        """base.py:176-282: searches the constructor arguments of ``cls`` for the best score of ``evaluator``.

        ``data`` is the training matrix; a ``data_suggest_function(trial)`` can give one per trial instead, with
        ``data=None``.  ``parameter_suggest_function(trial)`` replaces ``default_tune_range`` as the source of the
        searched arguments.  ``recommender_params`` are fixed arguments of every trial's constructor: they win over
        a suggested argument of the same name and are not part of the returned parameters.  ``study`` may be a
        study of ``irspack_amd.optimization`` or an ``optuna.Study``; ``None`` creates an in-memory study with
        ``TPESampler(seed=tuning_random_seed)`` and ``MedianPruner(n_startup_trials=prunning_n_startup_trials)``.
        ``n_trials`` counts pruned trials too, ``timeout`` (seconds) is looked at between trials, and
        ``max_epoch``, ``validate_epoch`` and ``score_degradation_max`` go to ``learn_with_optimizer``.

        Returns the best trial's parameters (searched and learnt, such as ``train_epochs``) and a pandas frame
        with one row per trial."""
        from ..optimization.optimizer import Optimizer

        if study is None:
            from ..optimization.study import MedianPruner, TPESampler, create_study

            study = create_study(sampler=TPESampler(seed=tuning_random_seed),
                                 pruner=MedianPruner(n_startup_trials=prunning_n_startup_trials))
        if data is None and data_suggest_function is None:
            raise ValueError("Either `data` or `data_suggest_function` must be provided.")
        if data is not None:
            def data_suggest_function(trial: Any) -> Any:
                return data
        if parameter_suggest_function is None:
            def parameter_suggest_function(trial: Any) -> Dict[str, Any]:
                return cls.default_suggest_parameter(trial, recommender_params)
        optimizer = Optimizer(data_suggest_function, parameter_suggest_function, recommender_params, evaluator,
                              logger=logger, max_epoch=max_epoch, validate_epoch=validate_epoch,
                              score_degradation_max=score_degradation_max)
        return optimizer.optimize_with_study(study, cls, n_trials=n_trials, timeout=timeout)

    def _learn(self) -> None:
        raise NotImplementedError("_learn must be implemented.")

    def get_score(self, user_indices: np.ndarray) -> np.ndarray:
        raise NotImplementedError("get_score must be implemented")

    def get_score_block(self, begin: int, end: int) -> np.ndarray:
        raise NotImplementedError("get_score_block not implemented!")

    def get_score_remove_seen(self, user_indices: np.ndarray) -> np.ndarray:
        # base.py:308-322
        scores = _sparse_to_array(self.get_score(user_indices))
        m = self.X_train_all[user_indices].tocsr()
        scores[m.nonzero()] = -np.inf
        return scores

    def get_score_remove_seen_block(self, begin: int, end: int) -> np.ndarray:
        # base.py:324-337
        scores = _sparse_to_array(self.get_score_block(begin, end))
        m = self.X_train_all[begin:end]
        scores[m.nonzero()] = -np.inf
        return scores

    def get_score_cold_user(self, X: Any) -> np.ndarray:
        raise NotImplementedError(
            f"get_score_cold_user is not implemented for {self.__class__.__name__}!")

    def _create_cold_user_with_item_features_scorer(self, item_features: Any) -> Callable[[Any], np.ndarray]:
        """base.py:353-362: lets an evaluator prepare feature-derived item state once and score
        many user blocks against it."""
        return lambda X: self.get_score_cold_user_with_item_features(X, item_features)

    def get_score_cold_user_with_item_features(self, X: Any, item_features: Any) -> np.ndarray:
        # base.py:364-389
        raise NotImplementedError("Scoring additional items from features is not implemented for "
                                  f"{self.__class__.__name__}.")

    def get_score_cold_user_remove_seen(self, X: Any) -> np.ndarray:
        score = self.get_score_cold_user(X)
        score[sps.csr_matrix(X).nonzero()] = -np.inf
        return score


class BaseSimilarityRecommender(BaseRecommender):
    """base.py:406-429: score = X[u] @ W with the learnt item-item weights."""

    def __init__(self, *args: Any, **kwargs: Any) -> None:
        super().__init__(*args, **kwargs)
        self._W: Optional[Union[sps.csr_matrix, sps.csc_matrix, np.ndarray]] = None

    @property
    def W(self):
        if self._W is None:
            raise RuntimeError("W fetched before fit.")
        return self._W

    def get_score(self, user_indices: np.ndarray) -> np.ndarray:
        return _sparse_to_array(self.X_train_all[user_indices].dot(self.W))

    def get_score_cold_user(self, X: Any) -> np.ndarray:
        return _sparse_to_array(sps.csr_matrix(X).dot(self.W))

    def get_score_block(self, begin: int, end: int) -> np.ndarray:
        return _sparse_to_array(self.X_train_all[begin:end].dot(self.W))


class BaseUserSimilarityRecommender(BaseRecommender):
    """base.py:432-453: score = U[u] @ X with the learnt user-user weights."""

    def __init__(self, *args: Any, **kwargs: Any) -> None:
        super().__init__(*args, **kwargs)
        self._X_csc: sps.csc_matrix = self.X_train_all.tocsc()
        self.U_: Optional[Union[sps.csr_matrix, sps.csc_matrix, np.ndarray]] = None

    @property
    def U(self):
        if self.U_ is None:
            raise RuntimeError("W fetched before fit.")  # (the reference's wording, base.py:446)
        return self.U_

    def get_score(self, user_indices: np.ndarray) -> np.ndarray:
        return _sparse_to_array(self.U[user_indices].dot(self._X_csc).toarray())

    def get_score_block(self, begin: int, end: int) -> np.ndarray:
        return _sparse_to_array(self.U[begin:end].dot(self._X_csc))
