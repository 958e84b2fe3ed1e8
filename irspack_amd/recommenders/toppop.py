"""``TopPopRecommender`` (irspack/recommenders/toppop.py:14-50): every user is recommended the most popular items of
the training set.  Host only; it is the baseline the personalised models are read against."""
from typing import Any, Optional

import numpy as np

from .base import BaseRecommender


class TopPopRecommender(BaseRecommender):
    def __init__(self, X_train: Any) -> None:
        super().__init__(X_train)
        self.score_: Optional[np.ndarray] = None

    def _learn(self) -> None:
        self.score_ = np.asarray(self.X_train_all.sum(axis=0), dtype=np.float64).reshape(1, -1)

    @property
    def score(self) -> np.ndarray:
        if self.score_ is None:
            raise RuntimeError("The method called before ``learn``.")
        return self.score_

    def get_score(self, user_indices: np.ndarray) -> np.ndarray:
        return np.repeat(self.score, user_indices.shape[0], axis=0)

    def get_score_cold_user(self, X: Any) -> np.ndarray:
        return np.repeat(self.score, X.shape[0], axis=0)
