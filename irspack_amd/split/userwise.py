"""User-wise hold-outs on a data frame (the reference's ``irspack/split/userwise.py``).  The random hold-out goes
through the device split (:func:`irspack_amd.utils.rowwise_train_test_split`); the time-ordered one is pandas on the
host."""

from typing import Any, Dict, List, Optional, Tuple, Union

import numpy as np
from scipy import sparse as sps

from ..utils import convert_randomstate, df_to_sparse, rowwise_train_test_split
from .time import split_last_n_interaction_df


def _split_list(ids, test_size: int, rns: np.random.RandomState) -> Tuple[Any, Any]:
    """shuffles ``ids`` in place (one ``rns.shuffle``); returns (all but the first ``test_size``, the first
    ``test_size``)"""
    rns.shuffle(ids)
    return ids[test_size:], ids[:test_size]


class UserTrainTestInteractionPair:
    """The train and (if any) test interactions of a set of users, with their ids.

    Args:
        user_ids: the user of every row of ``X_train``.
        X_train: the train part of the interactions.
        X_test: the held-out part; ``None`` stands for an empty matrix of ``X_train``'s shape.
        item_ids: the item of every column (needed by ``df_train`` / ``df_test`` only).

    Raises:
        ValueError: ``user_ids`` and the rows of ``X_train`` differ in number; ``X_train`` and ``X_test`` differ in
            shape; ``item_ids`` and the columns differ in number.

    Attributes: ``X_train``, ``X_test`` (CSR), ``X_all = X_train + X_test``, ``n_users``, ``n_items``, ``user_ids``
    (a list), ``item_ids``.
    """

    X_train: sps.csr_matrix
    X_test: sps.csr_matrix
    n_users: int
    n_items: int
    X_all: sps.csr_matrix

    def __init__(self, user_ids: Union[List[Any], np.ndarray], X_train, X_test,
                 item_ids: Optional[Union[List[Any], np.ndarray]] = None):
        if len(user_ids) != X_train.shape[0]:
            raise ValueError("user_ids and X_train have different shapes.")
        if X_test is None:
            X_test = sps.csr_matrix(X_train.shape, dtype=X_train.dtype)
        elif X_train.shape != X_test.shape:
            raise ValueError("X_train and X_test have different shapes.")
        self.user_ids = list(user_ids)
        self.X_train = sps.csr_matrix(X_train)
        self.X_test = sps.csr_matrix(X_test)
        self.n_users, self.n_items = self.X_train.shape
        self.X_all = sps.csr_matrix(self.X_train + self.X_test)
        if item_ids is not None and len(item_ids) != self.n_items:
            raise ValueError("X_train.shape[1] != len(item_ids)")
        self.item_ids = item_ids

    def _X_to_df(self, X: sps.csr_matrix, user_ids: List[Any]):
        import pandas as pd

        if self.item_ids is None:
            raise RuntimeError("Setting item_ids is required to use this method.")
        X.sort_indices()
        entries = X.tocoo()
        keep = entries.data != 0  # (stored zeros are no interactions)
        return pd.DataFrame(dict(user_id=[user_ids[r] for r in entries.row[keep]],
                                 item_id=[self.item_ids[c] for c in entries.col[keep]], rating=entries.data[keep]))

    def df_train(self):
        """the train interactions as a frame with the columns ``user_id, item_id, rating``"""
        return self._X_to_df(self.X_train, self.user_ids)

    def df_test(self):
        """the held-out interactions as a frame with the columns ``user_id, item_id, rating``"""
        return self._X_to_df(self.X_test, self.user_ids)

    def concat(self, other: "UserTrainTestInteractionPair") -> "UserTrainTestInteractionPair":
        """The users of ``self`` followed by the users of ``other`` (``item_ids`` are not carried over).

        Raises:
            ValueError: the two have different ``n_items``."""
        if self.n_items != other.n_items:
            raise ValueError("inconsistent n_items.")
        return UserTrainTestInteractionPair(
            self.user_ids + other.user_ids,
            sps.vstack([self.X_train, other.X_train], format="csr"),
            sps.vstack([self.X_test, other.X_test], format="csr"),
        )


def split_train_test_userwise_random(df_, user_column: str, item_column: str, item_ids: Union[List[Any], np.ndarray],
                                     heldout_ratio: float, n_heldout: Optional[int], rns: np.random.RandomState,
                                     rating_column: Optional[str] = None,
                                     ceil_n_heldout: bool = False) -> UserTrainTestInteractionPair:
    """The interactions of ``df_`` as a matrix over ``item_ids`` whose rows are split at random, on the device:
    ``n_heldout`` entries per user when it is given, else ``floor(N_u * heldout_ratio)`` (``ceil`` with
    ``ceil_n_heldout``).  One draw is taken from ``rns``."""
    X_all, user_ids, _ = df_to_sparse(df_, user_column=user_column, item_column=item_column, item_ids=item_ids,
                                      rating_column=rating_column)
    X_learn, X_predict = rowwise_train_test_split(X_all, heldout_ratio, n_heldout, random_state=rns,
                                                  ceil_n_heldout=ceil_n_heldout)
    return UserTrainTestInteractionPair(user_ids, X_learn, X_predict, item_ids)


def split_train_test_userwise_time(df_, user_column: str, item_column: str, time_column: str, item_ids: List[Any],
                                   heldout_ratio: float, n_heldout: Optional[int],
                                   rating_column: Optional[str] = None,
                                   ceil_n_heldout: bool = False) -> UserTrainTestInteractionPair:
    """As :func:`split_train_test_userwise_random` with the LAST interactions of every user (by ``time_column``) held
    out (:func:`split_last_n_interaction_df`).  The rating column, when given, travels through the time split with
    the three other columns (the reference selects those three alone and then does not find the ratings)."""
    unique_user_ids = np.asarray(list(set(df_[user_column])))
    columns = [user_column, item_column, time_column]
    if rating_column is not None and rating_column not in columns:
        columns.append(rating_column)
    df_train, df_test = split_last_n_interaction_df(df_[columns], user_column, time_column, n_heldout=n_heldout,
                                                    heldout_ratio=heldout_ratio, ceil_n_heldout=ceil_n_heldout)
    X_train, _, __ = df_to_sparse(df_train, user_column, item_column, user_ids=unique_user_ids, item_ids=item_ids,
                                  rating_column=rating_column)
    X_test, _, __ = df_to_sparse(df_test, user_column, item_column, user_ids=unique_user_ids, item_ids=item_ids,
                                 rating_column=rating_column)
    return UserTrainTestInteractionPair(unique_user_ids, X_train, X_test, item_ids)


def split_dataframe_partial_user_holdout(
    df_all,
    user_column: str,
    item_column: str,
    time_column: Optional[str] = None,
    rating_column: Optional[str] = None,
    n_val_user: Optional[int] = None,
    n_test_user: Optional[int] = None,
    val_user_ratio: float = 0.1,
    test_user_ratio: float = 0.1,
    heldout_ratio_val: float = 0.5,
    n_heldout_val: Optional[int] = None,
    heldout_ratio_test: float = 0.5,
    n_heldout_test: Optional[int] = None,
    ceil_n_heldout: bool = False,
    random_state=None,
) -> Tuple[Dict[str, UserTrainTestInteractionPair], List[Any]]:
    """Splits the users of an interaction log into train, validation and test users and holds out a part of the
    interactions of the validation and test users.

    Args:
        df_all: the interaction log.
        user_column, item_column: its user and item columns.
        time_column: when set, the most recent interactions of a user are held out, else random ones (on the device).
        rating_column: the values of the matrices (1 when ``None``).
        n_val_user, n_test_user: the numbers of validation and test users; when ``None``,
            ``int(n_users * val_user_ratio)`` and ``int(n_users * test_user_ratio)``.
        heldout_ratio_val, n_heldout_val, heldout_ratio_test, n_heldout_test: how much of a validation / test user's
            interactions is held out: ``n_heldout_*`` when given, else the ratio.
        ceil_n_heldout: round the ratio's share up, not down.
        random_state: ``None``, a seed or a ``numpy.random.RandomState``.

    Raises:
        ValueError: ``n_val_user``, or ``n_val_user + n_test_user``, exceeds the number of users.

    Returns:
        ``({"train": pair, "val": pair, "test": pair}, item_ids)``; ``item_ids`` are the columns of every matrix.  The
        train pair has an empty ``X_test``."""
    assert (test_user_ratio <= 1) and (test_user_ratio >= 0)
    assert (val_user_ratio <= 1) and (val_user_ratio >= 0)

    uids = df_all[user_column].unique()
    n_users_all = len(uids)
    if n_val_user is None:
        n_val_user = int(n_users_all * val_user_ratio)
        val_user_ratio = n_val_user / n_users_all
    elif n_val_user > n_users_all:
        raise ValueError("n_val_user exceeds the number of total users.")
    if n_test_user is None:
        n_test_user = int(n_users_all * test_user_ratio)
        test_user_ratio = n_test_user / n_users_all
    elif (n_test_user + n_val_user) > n_users_all:
        raise ValueError("n_val_user + n_test_users exceeds the number of total users.")

    df_all = df_all.drop_duplicates([user_column, item_column])
    rns = convert_randomstate(random_state)
    train_uids, val_test_uids = _split_list(uids, n_val_user + n_test_user, rns)
    if (test_user_ratio * len(uids)) >= 1:
        val_uids, test_uids = _split_list(val_test_uids, n_test_user, rns)
    else:
        val_uids, test_uids = val_test_uids, []
    item_all: List[Any] = list(set(df_all[item_column]))

    who = df_all[user_column]
    X_train_users, _, __ = df_to_sparse(df_all[who.isin(train_uids)], user_column, item_column, user_ids=train_uids,
                                        item_ids=item_all)
    result: Dict[str, UserTrainTestInteractionPair] = dict(
        train=UserTrainTestInteractionPair(train_uids, X_train_users, None))
    for name, ids, heldout_ratio, n_heldout in (("val", val_uids, heldout_ratio_val, n_heldout_val),
                                                ("test", test_uids, heldout_ratio_test, n_heldout_test)):
        df_part = df_all[who.isin(ids)].copy()
        if time_column is None:
            result[name] = split_train_test_userwise_random(df_part, user_column, item_column, item_all,
                                                            heldout_ratio, n_heldout, rns,
                                                            rating_column=rating_column,
                                                            ceil_n_heldout=ceil_n_heldout)
        else:
            result[name] = split_train_test_userwise_time(df_part, user_column, item_column, time_column, item_all,
                                                          heldout_ratio, n_heldout, rating_column=rating_column,
                                                          ceil_n_heldout=ceil_n_heldout)
    return result, item_all
