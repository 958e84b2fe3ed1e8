"""``DenseSLIMRecommender`` (irspack/recommenders/dense_slim.py): EASE, the closed-form dense item-item
weights, computed on the device by ``irspack_amd.utils.dense_slim_weight`` (``irs_dense_slim_fit``)."""

from typing import Any

from ..optimization.parameter_range import LogUniformFloatRange
from ..utils import dense_slim_weight
from .base import BaseSimilarityRecommender


class DenseSLIMRecommender(BaseSimilarityRecommender):
    r"""EASE (`Embarrassingly Shallow Autoencoders for Sparse Data <https://arxiv.org/abs/1905.03375>`_),
    the reference's dense_slim.py:39-53:

    .. math ::

        B = (X^T X + \mathrm{reg} \cdot I)^{-1}, \qquad W_{ij} = -B_{ij} / B_{jj} \; (i \ne j), \quad W_{jj} = 0

    in float32.  ``W`` is a dense float32 ``ndarray``.  The inverse comes from a Cholesky factor, so a
    system that is not positive definite (``reg <= 0`` with an item nobody touched) raises
    ``numpy.linalg.LinAlgError``."""

    default_tune_range = [LogUniformFloatRange("reg", 1, 1e4)]

    def __init__(self, X_train_all: Any, reg: float = 1) -> None:
        super().__init__(X_train_all)
        self.reg = reg

    def _learn(self) -> None:
        self._W = dense_slim_weight(self.X_train_all, self.reg)
