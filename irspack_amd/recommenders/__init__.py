"""Mirror of ``irspack.recommenders`` for the hot path (irspack/recommenders/__init__.py):
the recommenders whose compiled core is rebuilt here."""

from .base import BaseRecommender, BaseSimilarityRecommender, BaseUserSimilarityRecommender
from .base_earlystop import BaseRecommenderWithEarlyStopping
from .bpr import BPRFMRecommender, WARPFMRecommender
from .dense_slim import DenseSLIMRecommender
from .edlae import EDLAERecommender
from .ials import IALSRecommender
from .multvae import MultVAERecommender
from .knn import (AsymmetricCosineKNNRecommender, CosineKNNRecommender, JaccardKNNRecommender,
                  P3alphaRecommender, RP3betaRecommender, TverskyIndexKNNRecommender)
from .nmf import NMFRecommender
from .slim import SLIMRecommender
from .toppop import TopPopRecommender
from .truncsvd import TruncatedSVDRecommender
from .user_knn import AsymmetricCosineUserKNNRecommender, CosineUserKNNRecommender

__all__ = ["BaseRecommender", "BaseSimilarityRecommender", "IALSRecommender",
           "CosineKNNRecommender", "AsymmetricCosineKNNRecommender", "JaccardKNNRecommender",
           "TverskyIndexKNNRecommender", "P3alphaRecommender", "RP3betaRecommender",
           "BaseUserSimilarityRecommender", "CosineUserKNNRecommender",
           "AsymmetricCosineUserKNNRecommender", "SLIMRecommender", "DenseSLIMRecommender",
           "EDLAERecommender", "TruncatedSVDRecommender", "NMFRecommender",
           "BaseRecommenderWithEarlyStopping", "BPRFMRecommender", "TopPopRecommender",
           "MultVAERecommender", "WARPFMRecommender"]
