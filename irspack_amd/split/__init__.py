"""Train / validation / test splits of interaction data (the reference's ``irspack.split``).  The random row-wise
hold-out runs on the device; everything around it is pandas and scipy on the host."""

from ..utils import rowwise_train_test_split
from .specified import holdout_specific_interactions
from .time import split_last_n_interaction_df
from .userwise import (UserTrainTestInteractionPair, split_dataframe_partial_user_holdout,
                       split_train_test_userwise_random, split_train_test_userwise_time)

__all__ = [
    "UserTrainTestInteractionPair",
    "split_dataframe_partial_user_holdout",
    "split_train_test_userwise_random",
    "split_train_test_userwise_time",
    "holdout_specific_interactions",
    "rowwise_train_test_split",
    "split_last_n_interaction_df",
]
