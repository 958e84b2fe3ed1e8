"""``NMFRecommender`` (irspack/recommenders/nmf.py): non-negative matrix factorisation of the interaction
matrix.  The reference fits ``sklearn.decomposition.NMF`` (coordinate descent, Frobenius loss); here the fit is
``irspack_amd.utils.nmf_fit`` and the cold-user transform ``irspack_amd.utils.nmf_transform`` (``irs_nmf_fit``:
sparse x block products, Gram matrices and the coordinate sweeps on the device).  Scoring is the reference's:
dense products on the host."""
from typing import Any, Optional

import numpy as np

from ..optimization.parameter_range import LogUniformFloatRange, UniformFloatRange, UniformIntegerRange
from ..utils import NMF_INITS, nmf_fit, nmf_transform
from .base import BaseRecommender


class NMFModel:
    """What the recommender uses of a fitted ``sklearn.decomposition.NMF``: ``components_`` ``(k, I)``,
    ``n_components_``, ``n_iter_`` and ``transform``."""

    def __init__(self, components: np.ndarray, n_iter: int, alpha: float, l1_ratio: float) -> None:
        self.components_ = components
        self.n_components_ = components.shape[0]
        self.n_iter_ = n_iter
        self.alpha_W = alpha
        self.l1_ratio = l1_ratio

    def transform(self, X: Any) -> np.ndarray:
        return nmf_transform(X, self.components_, self.alpha_W, self.l1_ratio)


class NMFRecommender(BaseRecommender):
    default_tune_range = [UniformIntegerRange("n_components", 4, 512), LogUniformFloatRange("alpha", 1e-10, 1e-1),
                          UniformFloatRange("l1_ratio", 0, 1)]

    def __init__(self, X_train_all: Any, n_components: int = 64, alpha: float = 1e-2, l1_ratio: float = 1e-2,
                 beta_loss: str = "frobenius", init: Optional[str] = None) -> None:
        super().__init__(X_train_all)
        self.n_components = n_components
        self.alpha = alpha
        self.l1_ratio = l1_ratio
        self.beta_loss = beta_loss
        self.init = init

    def _learn(self) -> None:
        # what sklearn's "cd" solver accepts
        if self.beta_loss not in (2, "frobenius"):
            raise ValueError(f"Invalid beta_loss parameter: solver 'cd' does not handle beta_loss = {self.beta_loss!r}")
        if self.init not in NMF_INITS:
            raise ValueError(f"Invalid init parameter: got {self.init!r} instead of one of {NMF_INITS!r}")
        W, H, n_iter = nmf_fit(self.X_train_all, self.n_components, self.alpha, self.l1_ratio, init=self.init,
                               random_state=42)
        self.nmf_model = NMFModel(H, n_iter, self.alpha, self.l1_ratio)
        self.W = W
        self.H = H

    def get_score(self, user_indices: np.ndarray) -> np.ndarray:
        return self.W[user_indices].dot(self.H)

    def get_score_block(self, begin: int, end: int) -> np.ndarray:
        return self.W[begin:end].dot(self.H)

    def get_score_cold_user(self, X: Any) -> np.ndarray:
        return self.nmf_model.transform(X).dot(self.H)
