"""Time-ordered hold-out on a data frame (the reference's ``irspack/split/time.py``): pandas on the host."""

from typing import Optional, Tuple

import numpy as np


def split_last_n_interaction_df(df, user_column: str, timestamp_column: str, n_heldout: Optional[int] = None,
                                heldout_ratio: float = 0.1, ceil_n_heldout: bool = False) -> Tuple:
    """Holds out the last interactions of every user.

    The frame is sorted by user, then by ``timestamp_column`` (any sortable column); rows of one user with equal
    timestamps keep the order they have in ``df``.  Of a user with ``N`` rows the last ``n_heldout`` (all of them
    when there are fewer) are held out, or, when ``n_heldout`` is ``None``, the last ``floor(N * heldout_ratio)`` -
    ``ceil`` with ``ceil_n_heldout``.

    Returns ``(df_first, df_heldout)``, both in the sorted order."""
    ordered = df.sort_values([user_column, timestamp_column], kind="stable")
    per_user = ordered.groupby(user_column, sort=False)
    from_end = per_user.cumcount(ascending=False).to_numpy()
    if n_heldout is not None:
        held = from_end < n_heldout
    else:
        n_rows = per_user[user_column].transform("size").to_numpy().astype(np.float64)
        n_held = np.ceil(n_rows * heldout_ratio) if ceil_n_heldout else np.floor(n_rows * heldout_ratio)
        held = from_end < n_held
    return ordered.iloc[np.flatnonzero(~held)], ordered.iloc[np.flatnonzero(held)]
