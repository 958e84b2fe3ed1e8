"""``SLIMRecommender`` (irspack/recommenders/slim.py): elastic-net item-item weights, learnt on the
device by ``irspack_amd.utils.slim_weight_*`` (``irs_slim_fit``)."""

from typing import Any, Optional

from .._threading import get_n_threads
from ..optimization.parameter_range import LogUniformFloatRange, UniformFloatRange
from ..utils import slim_weight_allow_negative, slim_weight_positive_only
from .base import BaseSimilarityRecommender


class SLIMRecommender(BaseSimilarityRecommender):
    r"""SLIM with the elastic-net loss of the reference (slim.py:21-87)

    .. math ::

        \frac{1}{2} ||X - XB||^2_F + \frac{\alpha (1 - l_1) U}{2} ||B||^2_F + \alpha l_1 U |B|

    minimised column by column by cyclic coordinate descent.  Unlike the reference's, the descent visits
    the coordinates in ascending order in every sweep and each column stops on its own ``tol`` test, so
    ``W`` is a function of the arguments alone (``n_threads`` does not change it; see
    :func:`irspack_amd.utils.slim_weight_allow_negative`).  ``W`` is a float32 ``csc_matrix``."""

    default_tune_range = [LogUniformFloatRange("alpha", 1e-5, 1), UniformFloatRange("l1_ratio", 0, 1)]

    def __init__(self, X_train_all: Any, alpha: float = 0.05, l1_ratio: float = 0.01,
                 positive_only: bool = True, n_iter: int = 100, tol: float = 1e-4,
                 top_k: Optional[int] = None, n_threads: Optional[int] = None) -> None:
        super().__init__(X_train_all)
        self.alpha = alpha
        self.l1_ratio = l1_ratio
        self.positive_only = positive_only
        self.n_threads = get_n_threads(n_threads)
        self.n_iter = n_iter
        self.tol = tol
        self.top_k = top_k

    def _learn(self) -> None:
        # slim.py:89-113
        l2_coeff = self.n_users * self.alpha * (1 - self.l1_ratio)
        l1_coeff = self.n_users * self.alpha * self.l1_ratio
        fit = slim_weight_positive_only if self.positive_only else slim_weight_allow_negative
        self._W = fit(self.X_train_all, n_threads=self.n_threads, n_iter=self.n_iter, l2_coeff=l2_coeff,
                      l1_coeff=l1_coeff, tol=self.tol, top_k=-1 if self.top_k is None else self.top_k)
