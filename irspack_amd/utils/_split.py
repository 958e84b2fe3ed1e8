"""The row-wise hold-out split of the reference's ``irspack.utils`` on the device (``irs_split_rowwise``), and the
two helpers its callers go through: ``convert_randomstate`` (``irspack/utils/random.py``) and ``df_to_sparse``
(``irspack/utils/__init__.py:72-130``).

``rowwise_train_test_split_by_ratio`` / ``_by_fixed_n`` are the reference's ``_util_cpp`` functions of those names
(``cpp_source/util.hpp:72-156``).  Which entries of a row are held out follows this package's own counter-based rule
(``irspack_amd/csrc/split_host_plan.hpp``), not libstdc++'s ``std::shuffle`` of one
``std::mt19937`` stream: the same arguments give the same split on every machine, but not the reference's split.
How MANY entries of a row are held out is the reference's number exactly.

pandas is imported inside the functions that need it.
"""

import ctypes as C
from typing import Any, List, Optional, Tuple, Union

import numpy as np
import scipy.sparse as sps

from .. import _lib
from .._lib import check, lib, ptr


def convert_randomstate(arg) -> np.random.RandomState:
    """``None`` or an ``int`` make a new ``RandomState``; a ``RandomState`` is returned as it is."""
    if arg is None or isinstance(arg, int):
        return np.random.RandomState(arg)
    elif isinstance(arg, np.random.RandomState):
        return arg
    else:
        raise ValueError(f"{arg} cannot be interpreted as a random state.")


def _canonical_csr(X) -> sps.csr_matrix:
    """CSR with sorted columns and duplicates summed; the caller's matrix is never modified (what has to change
    changes on a copy), the dtype stays"""
    Xc = sps.csr_matrix(X)
    if not Xc.has_canonical_format:
        Xc = Xc.copy()
        Xc.sum_duplicates()
    return Xc


def _split(X, random_seed: int, mode: int, ratio: float, ceil: bool, n_held_out: int, device: Optional[int],
           stats: Optional[dict]) -> Tuple[sps.csr_matrix, sps.csr_matrix]:
    Xc = _canonical_csr(X)
    dtype = Xc.dtype
    rows, cols = Xc.shape
    indptr = np.ascontiguousarray(Xc.indptr, dtype=np.int64)
    indices = np.ascontiguousarray(Xc.indices, dtype=np.int32)
    data = np.ascontiguousarray(Xc.data)
    if data.size == 0:
        indices, data = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=dtype)
    vptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    handle = C.c_void_p()
    check(lib().irs_split_rowwise(
        rows, cols, ptr(indptr, C.c_int64), ptr(indices, C.c_int32), vptr(data), int(dtype.itemsize), int(random_seed),
        int(mode), float(ratio), 1 if ceil else 0, int(n_held_out),
        _lib.default_device() if device is None else device, C.byref(handle)))
    try:
        n_train, n_test = C.c_int64(), C.c_int64()
        check(lib().irs_split_nnz(handle, C.byref(n_train), C.byref(n_test)))
        out = []
        for n in (n_train.value, n_test.value):
            out.append((np.empty(rows + 1, dtype=np.int64), np.empty(max(n, 1), dtype=np.int32),
                        np.empty(max(n, 1), dtype=dtype), n))
        (tr_p, tr_i, tr_d, _), (te_p, te_i, te_d, _) = out
        check(lib().irs_split_fetch(handle, ptr(tr_p, C.c_int64), ptr(tr_i, C.c_int32), vptr(tr_d),
                                    ptr(te_p, C.c_int64), ptr(te_i, C.c_int32), vptr(te_d)))
        if stats is not None:
            st = _lib.SplitStatsStruct()
            check(lib().irs_split_last_stats(handle, C.cast(C.byref(st), C.c_void_p)))
            stats.update({name: getattr(st, name) for name, _ in _lib.SplitStatsStruct._fields_})
    finally:
        lib().irs_split_destroy(handle)
    result = []
    for p, i, d, n in out:
        M = sps.csr_matrix((d[:n], i[:n], p), shape=(rows, cols))
        M.has_sorted_indices = True
        result.append(M)
    return result[0], result[1]


def rowwise_train_test_split_by_ratio(X, random_seed: int, heldout_ratio: float, n_test_ceil: bool, *,
                                      device: Optional[int] = None,
                                      stats: Optional[dict] = None) -> Tuple[sps.csr_matrix, sps.csr_matrix]:
    """util.hpp:117-141: of a row with ``m`` stored entries, ``floor(m * heldout_ratio)`` (``ceil`` with
    ``n_test_ceil``; the product in double, so ``100 * 0.07`` gives 8 with ``ceil``) go to the second matrix, the others to the
    first; ``heldout_ratio`` outside ``[0, 1]`` is a ``ValueError``.  Returns ``(X_train, X_test)``: the shape and
    dtype of ``X``, sorted indices, ``X_train + X_test == X``.

    Every stored entry takes part, explicit zeros too.  A matrix that is not canonical is sorted and its duplicates
    are summed first, on a copy (the reference splits the duplicates one by one and sums them afterwards).  Values
    are moved as they are - any dtype of 1, 2, 4 or 8 bytes, no round trip through float64.  The split depends on
    the arguments alone; two calls give identical bytes.

    ``stats`` (measurement only) receives the HIP-event phase times ``upload_ms, select_ms, scan_ms, scatter_ms,
    d2h_ms`` and the rows per kernel class ``rows_empty, rows_wave, rows_lds, rows_stream``."""
    return _split(X, random_seed, _lib.SPLIT_BY_RATIO, heldout_ratio, bool(n_test_ceil), 0, device, stats)


def rowwise_train_test_split_by_fixed_n(X, random_seed: int, n_held_out: int, *, device: Optional[int] = None,
                                        stats: Optional[dict] = None) -> Tuple[sps.csr_matrix, sps.csr_matrix]:
    """util.hpp:143-156: ``min(m, n_held_out)`` entries of every row go to the second matrix.  Otherwise as
    :func:`rowwise_train_test_split_by_ratio`; a negative ``n_held_out`` is a ``ValueError``."""
    return _split(X, random_seed, _lib.SPLIT_BY_FIXED_N, 0.0, False, n_held_out, device, stats)


def rowwise_train_test_split(X, test_ratio: float = 0.5, n_test: Optional[int] = None, ceil_n_heldout: bool = False,
                             random_state=None, *, device: Optional[int] = None,
                             stats: Optional[dict] = None) -> Tuple[sps.csr_matrix, sps.csr_matrix]:
    """Splits the stored entries of every row of ``X`` into train and test interactions, which sum back to ``X``
    (the reference's ``irspack.utils.rowwise_train_test_split``).  ``n_test`` entries per row (at most the row)
    when it is given, else ``floor(test_ratio * m)`` - ``ceil`` with ``ceil_n_heldout``.

    The seed of the split is one ``int32`` drawn from ``random_state`` the way the reference draws it, so a
    ``RandomState`` shared with other calls advances as it does there.  The outputs have the dtype of ``X``."""
    rns = convert_randomstate(random_state)
    random_seed = int(rns.randint(0, np.iinfo(np.int32).max, dtype=np.int32))
    if n_test is None:
        return rowwise_train_test_split_by_ratio(X, random_seed, test_ratio, ceil_n_heldout, device=device,
                                                 stats=stats)
    return rowwise_train_test_split_by_fixed_n(X, random_seed, n_test, device=device, stats=stats)


def df_to_sparse(df, user_column: str, item_column: str, user_ids: Optional[Union[List[Any], np.ndarray]] = None,
                 item_ids: Optional[Union[List[Any], np.ndarray]] = None,
                 rating_column: Optional[str] = None) -> Tuple[sps.csr_matrix, np.ndarray, np.ndarray]:
    """A pandas data frame of interactions as a sparse matrix (float64; an interaction that occurs twice is summed).

    ``user_ids`` / ``item_ids``: when given, the rows / columns of the matrix are exactly these, in this order, and
    the interactions of other users / items are dropped; when ``None`` they are the sorted distinct values of the
    column.  ``rating_column``: the values (all 1 when ``None``).

    Returns the matrix, the user ids of its rows and the item ids of its columns."""
    import pandas as pd

    if user_ids is not None:
        df = df[df[user_column].isin(user_ids)]
    if item_ids is not None:
        df = df[df[item_column].isin(item_ids)]
    users = pd.Categorical(df[user_column], categories=user_ids)
    items = pd.Categorical(df[item_column], categories=item_ids)
    if rating_column is None:
        data = np.ones(df.shape[0])
    else:
        data = np.asarray(df[rating_column].values, dtype=float)
    X = sps.csr_matrix((data, (users.codes, items.codes)), shape=(len(users.categories), len(items.categories)))
    return X, users.categories, items.categories
