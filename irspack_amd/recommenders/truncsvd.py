"""``TruncatedSVDRecommender`` (irspack/recommenders/truncsvd.py): the rank-``n_components`` randomized SVD of
the interaction matrix.  The reference fits ``sklearn.decomposition.TruncatedSVD``; here the fit is
``irspack_amd.utils.truncated_svd`` (``irs_truncsvd_*``: sparse x block products, Gram matrices and block
rotations on the device).  Scoring is the reference's: dense products on the host."""
import warnings
from typing import Any, Optional

import numpy as np
import scipy.sparse as sps

from ..optimization.parameter_range import UniformIntegerRange
from ..utils import truncated_svd
from .base import BaseRecommender


class TruncatedSVDDecomposer:
    """What the recommender uses of a fitted ``sklearn.decomposition.TruncatedSVD``: ``components_`` ``(k, I)``,
    ``singular_values_`` ``(k,)`` and ``transform``."""

    def __init__(self, components: np.ndarray, singular_values: np.ndarray) -> None:
        self.components_ = components
        self.singular_values_ = singular_values
        self.n_components = components.shape[0]

    def transform(self, X: Any) -> np.ndarray:
        if sps.issparse(X):
            return np.asarray(X.dot(self.components_.T))
        return np.asarray(X).dot(self.components_.T)


class TruncatedSVDRecommender(BaseRecommender):
    default_tune_range = [UniformIntegerRange("n_components", 4, 512)]

    def __init__(self, X_train_all: Any, n_components: int = 4, random_seed: int = 0) -> None:
        assert X_train_all.shape[1] > 1
        super().__init__(X_train_all)
        if n_components >= self.X_train_all.shape[1]:
            warnings.warn("n_components >= than X_train_all.shape[1]. Set it to X_train_all.shape[1] - 1.")
            n_components = self.X_train_all.shape[1] - 1
        self.n_components = n_components
        self.decomposer_: Optional[TruncatedSVDDecomposer] = None
        self.z_: Optional[np.ndarray] = None
        self.random_seed = random_seed

    @property
    def z(self) -> np.ndarray:
        if self.z_ is None:
            raise RuntimeError("z fetched before fit")
        return self.z_

    @property
    def decomposer(self) -> TruncatedSVDDecomposer:
        if self.decomposer_ is None:
            raise RuntimeError("decomposer fetched before fit.")
        return self.decomposer_

    def _learn(self) -> None:
        z, sigma, components = truncated_svd(self.X_train_all, self.n_components, self.random_seed)
        self.decomposer_ = TruncatedSVDDecomposer(components, sigma)
        self.z_ = z

    def get_score(self, user_indices: np.ndarray) -> np.ndarray:
        return self.z[user_indices].dot(self.decomposer.components_)

    def get_score_block(self, begin: int, end: int) -> np.ndarray:
        return self.z[begin:end].dot(self.decomposer.components_)

    def get_score_cold_user(self, X: Any) -> np.ndarray:
        return self.decomposer.transform(X).dot(self.decomposer.components_)

    def get_user_embedding(self) -> np.ndarray:
        return self.z

    def get_score_from_user_embedding(self, user_embedding: np.ndarray) -> np.ndarray:
        return user_embedding.dot(self.decomposer.components_)

    def get_item_embedding(self) -> np.ndarray:
        return self.decomposer.components_.T

    def get_score_from_item_embedding(self, user_indices: np.ndarray, item_embedding: np.ndarray) -> np.ndarray:
        return self.z[user_indices].dot(item_embedding.T)
