"""Hold-out of interactions the caller points at (the reference's ``irspack/split/specified.py``): pandas and scipy
on the host, no random choice of entries - only of users."""

from typing import Dict, Tuple

import numpy as np
from scipy import sparse as sps

from ..utils import convert_randomstate
from .userwise import UserTrainTestInteractionPair, _split_list


def holdout_specific_interactions(df, user_column: str, item_column: str, interaction_indicator: np.ndarray,
                                  validatable_user_ratio_val: float = 0.2, validatable_user_ratio_test: float = 0.2,
                                  random_state=None) -> Tuple[np.ndarray, Dict[str, UserTrainTestInteractionPair]]:
    """Holds out the interactions ``interaction_indicator`` marks (a boolean mask or positions into ``df``), for a
    part of the users who have such interactions.

    A user with at least one marked interaction is "validatable".  The validatable users are split at random into
    train, validation and test users by the two ratios; of the validation and test users the marked interactions
    become ``X_test`` and the others ``X_train``.  Every interaction of the other users - marked or not - is
    train data.  Useful to evaluate on a part of the catalogue only, or to split a log at a point in time without
    later information leaking into the training set.

    Raises:
        ValueError: the two ratios sum to more than 1.

    Returns:
        ``(item_ids, {"train": pair, "val": pair, "test": pair})``; ``item_ids`` (sorted) are the columns of every
        matrix, all values are 1 (float64)."""
    ratio_train = 1 - validatable_user_ratio_val - validatable_user_ratio_test
    if ratio_train < -1e-10:
        raise ValueError("validatable_use_ratio_val + validatable_user_ratio_test exceeds 1.")

    users = np.asarray(df[user_column])
    item_ids, item_index = np.unique(np.asarray(df[item_column]), return_inverse=True)
    item_index = np.asarray(item_index).ravel()
    marked = np.zeros(users.shape[0], dtype=bool)
    marked[interaction_indicator] = True

    validatable = np.unique(users[marked])
    ratio_val_test = 1 - ratio_train
    rns = convert_randomstate(random_state)
    if ratio_val_test >= 1.0:
        v_train, v_val_test = [], validatable.tolist()
    else:
        v_val_test, v_train = _split_list(validatable.tolist(), int(ratio_train * validatable.shape[0]), rns)
    v_test, v_val = _split_list(v_val_test, int(len(v_val_test) * validatable_user_ratio_val / ratio_val_test), rns)

    def dataset(rows: np.ndarray, train: bool) -> UserTrainTestInteractionPair:
        uid_unique, uindex = np.unique(users[rows], return_inverse=True)
        uindex = np.asarray(uindex).ravel()
        shape = (len(uid_unique), len(item_ids))

        def matrix(sel: np.ndarray) -> sps.csr_matrix:
            return sps.csr_matrix((np.ones(int(sel.sum()), dtype=np.float64), (uindex[sel], item_index[rows][sel])),
                                  shape=shape)

        if train:
            return UserTrainTestInteractionPair(uid_unique, X_train=matrix(np.ones(rows.shape[0], dtype=bool)),
                                                X_test=None)
        held = marked[rows]
        return UserTrainTestInteractionPair(uid_unique, X_train=matrix(~held), X_test=matrix(held))

    is_train = np.isin(users, v_train) | ~np.isin(users, validatable)
    return item_ids, {
        "train": dataset(np.flatnonzero(is_train), True),
        "val": dataset(np.flatnonzero(np.isin(users, v_val)), False),
        "test": dataset(np.flatnonzero(np.isin(users, v_test)), False),
    }
