"""The rule of the row-wise hold-out split, restated in numpy from its text (it calls nothing of the library):

* every stored entry of a canonical row takes part, explicit zeros included; ``j`` is the position of an entry in
  its row, ``m`` the row's length;
* ``n_test(m)``: ``floor(double(m) * ratio)`` or ``ceil(double(m) * ratio)`` in double, or ``min(m, n_held_out)``;
* ``row_key = mix64(mix64(seed) ^ mix64(row + 0x53504C4954))``, ``key(j) = mix64(row_key ^ mix64(j))``, ``mix64``
  the finaliser of splitmix64 on 64-bit words;
* held out are the ``n_test`` smallest pairs ``(key(j), j)`` of the row in lexicographic order;
* both outputs keep the column order, the values are moved as they are.
"""
import numpy as np
import scipy.sparse as sps

U64 = np.uint64
ROW_SALT = 0x53504C4954


def mix64(z):
    z = np.asarray(z, dtype=U64).copy()
    with np.errstate(over="ignore"):
        z += U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def n_test_of(m, ratio=None, ceil=False, n_held_out=None):
    """held-out count of rows of length ``m`` (an int64 array)"""
    m = np.asarray(m, dtype=np.int64)
    if n_held_out is not None:
        return np.minimum(m, np.int64(n_held_out))
    x = m.astype(np.float64) * np.float64(ratio)
    return (np.ceil(x) if ceil else np.floor(x)).astype(np.int64)


def entry_keys(seed, rows_of_entries, j):
    """key of the entry at position ``j`` of row ``rows_of_entries`` (arrays of equal length)"""
    seed = U64(int(seed) & 0xFFFFFFFFFFFFFFFF)
    with np.errstate(over="ignore"):
        row_key = mix64(mix64(np.array([seed]))[0] ^ mix64(np.asarray(rows_of_entries).astype(U64) + U64(ROW_SALT)))
    return mix64(row_key ^ mix64(np.asarray(j).astype(U64)))


def held_out_mask(indptr, seed, ratio=None, ceil=False, n_held_out=None, keys=None):
    """one bool per stored entry of a CSR with row pointer ``indptr``; ``keys`` replaces the rule's keys (tests of the
    tie-break)"""
    indptr = np.asarray(indptr, dtype=np.int64)
    m = np.diff(indptr)
    nnz = int(indptr[-1])
    row = np.repeat(np.arange(m.shape[0], dtype=np.int64), m)
    j = np.arange(nnz, dtype=np.int64) - indptr[:-1][row]
    if keys is None:
        keys = entry_keys(seed, row, j)
    order = np.lexsort((j, keys, row))  # by row, then key, then j
    rank = np.empty(nnz, dtype=np.int64)
    rank[order] = np.arange(nnz, dtype=np.int64) - indptr[:-1][row]  # (row[order] == row: entries stay in their row)
    return rank < n_test_of(m, ratio, ceil, n_held_out)[row]


def split(X, seed, ratio=None, ceil=False, n_held_out=None):
    """(X_train, X_test) of a canonical CSR matrix by the rule"""
    X = sps.csr_matrix(X)
    assert X.has_canonical_format
    held = held_out_mask(X.indptr, seed, ratio, ceil, n_held_out)
    m = np.diff(X.indptr).astype(np.int64)
    row = np.repeat(np.arange(X.shape[0], dtype=np.int64), m)
    out = []
    for sel in (~held, held):
        counts = np.bincount(row[sel], minlength=X.shape[0]).astype(np.int64)
        indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        out.append(sps.csr_matrix((X.data[sel].copy(), X.indices[sel].astype(np.int32), indptr), shape=X.shape))
    return out[0], out[1]
