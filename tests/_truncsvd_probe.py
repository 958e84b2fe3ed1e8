"""Integer-valued inputs and the float64 reference chain of the truncated SVD's stage probes
(``tests/test_truncsvd_probe_inputs.py`` on the CPU, ``tests/test_gpu_truncsvd_stages.py`` on the GPU).

Every input is seeded, integer-valued and stored as float32.  A float32 sum of integer terms is exact in any
order while the sum of the terms' magnitudes stays within 2^24, so a stage whose ``bounds`` entry is at most 2^24
is compared with the device for equality: no tolerance, and no dependence on the order in which a kernel adds.

``probe_matrix`` plants rows and columns at the edges of the sparse product's segment rule (a row of more than
``SEG`` = 1024 stored entries is cut into segments of 1024): rows of exactly 1024 and 1025 entries, a row with
every live item, columns of 1024, 1025 and 2049 = 1024 + 1024 + 1 entries, an empty row and an empty column.
3,000 rows at ``l_pad`` = 576 are 47 chunks of 64 rows for 45 slabs of a Gram pass: slabs of two chunks, the last
one of a single chunk with 56 live rows."""
import numpy as np
import scipy.sparse as sps

SEG = 1024
EXACT = 2 ** 24
N_USERS, N_ITEMS = 3000, 1100
WIDTHS = (1, 63, 64, 65, 128, 129, 192, 256, 257, 320, 384, 448, 512, 513, 576)
TALL_WIDTHS = (1, 5, 64, 70)
G3_NOT_EXACT = ("probe", "tall")  # matrices whose Gram of Q = A^T Y2 sums more than 2^24: a derived bound there

# positions in the 3000 x 1100 orientation: the last user row (in the last, partly filled chunk of 64) is split
FULL_USER, USER_1024, USER_1025, EMPTY_USER = 7, 1500, 2999, 2970
ITEM_2049, ITEM_1024, ITEM_1025, EMPTY_ITEM = 3, 640, 1099, 64
USER_COUNTS = {FULL_USER: N_ITEMS - 1, USER_1024: 1024, USER_1025: 1025, EMPTY_USER: 0}
ITEM_COUNTS = {ITEM_2049: 2049, ITEM_1024: 1024, ITEM_1025: 1025, EMPTY_ITEM: 0}

_CACHE = {}


def widths_of(l):
    """``(l, l2, k)`` of a probe at sketch width ``l``"""
    l2 = max(1, l - 3)
    return l, l2, max(1, l2 - 2)


def _finish(mask, rng):
    X = sps.csr_matrix(mask.astype(np.float32))
    X.sort_indices()
    X.data = rng.integers(1, 3, size=X.nnz).astype(np.float32)
    return X


def _background(rng):
    mask = rng.random((N_USERS, N_ITEMS)) < 0.01
    mask[EMPTY_USER, :] = False
    mask[:, EMPTY_ITEM] = False
    return mask


def _build(planted):
    rng = np.random.default_rng(20240611)
    mask = _background(rng)
    if planted:
        special_users = np.array([FULL_USER, USER_1024, USER_1025, EMPTY_USER])
        special_items = np.array([ITEM_2049, ITEM_1024, ITEM_1025, EMPTY_ITEM])
        plain_users = np.setdiff1d(np.arange(N_USERS), special_users)
        plain_items = np.setdiff1d(np.arange(N_ITEMS), special_items)
        # the planted columns first: the full user and count - 1 plain users, no other planted user
        for item in (ITEM_2049, ITEM_1024, ITEM_1025):
            mask[:, item] = False
            mask[rng.choice(plain_users, ITEM_COUNTS[item] - 1, replace=False), item] = True
            mask[FULL_USER, item] = True
        # then the planted rows, which touch plain columns only (the full row: every column but the empty one,
        # the planted ones already hold it)
        mask[FULL_USER, :] = True
        mask[FULL_USER, EMPTY_ITEM] = False
        for user in (USER_1024, USER_1025):
            mask[user, :] = False
            mask[user, rng.choice(plain_items, USER_COUNTS[user], replace=False)] = True
    return _finish(mask, rng)


def _oriented(name, transposed):
    key = (name, bool(transposed))
    if key not in _CACHE:
        if (name, False) not in _CACHE:
            _CACHE[(name, False)] = _build(name == "probe")
        if transposed:
            Xt = _CACHE[(name, False)].T.tocsr()
            Xt.sort_indices()
            _CACHE[key] = Xt
    return _CACHE[key]


def probe_matrix(transposed=False):
    """3000 x 1100 (``transposed``: its transpose, 1100 x 3000), values in {1, 2}, 1 % background plus the
    planted rows and columns of the module docstring"""
    return _oriented("probe", transposed)


def light_matrix(transposed=False):
    """the same shape and background with the empty row and column but no planted dense row or column"""
    return _oriented("light", transposed)


def tall_matrix(transposed=False):
    """20,000 x 70 with about three entries per row (``transposed``: 70 x 20,000): 313 chunks of 64 rows for the
    256 slabs a Gram pass has at most, at ``l_pad`` = 64 and 128"""
    key = ("tall", bool(transposed))
    if key not in _CACHE:
        rng = np.random.default_rng(20240612)
        X = _finish(rng.random((20000, 70)) < 3.0 / 70.0, rng)
        if transposed:
            X = X.T.tocsr()
            X.sort_indices()
        _CACHE[key] = X
    return _CACHE[key]


def empties(transposed=False):
    """``(empty user row, empty item column)`` of ``probe_matrix`` / ``light_matrix`` in that orientation"""
    return (EMPTY_ITEM, EMPTY_USER) if transposed else (EMPTY_USER, EMPTY_ITEM)


def expected_segments(transposed=False):
    """``(per user row, per item column)`` of ``probe_matrix``: ``{index: segments}`` of every row that is not a
    single segment (an empty row is 0 by ``ceil(len / 1024)``)"""
    users = {FULL_USER: 2, USER_1025: 2, EMPTY_USER: 0}
    items = {ITEM_2049: 3, ITEM_1025: 2, EMPTY_ITEM: 0}
    return (items, users) if transposed else (users, items)


def segments(indptr):
    """``ceil(len / 1024)`` of every row"""
    return -(-np.diff(np.asarray(indptr, dtype=np.int64)) // SEG)


def omega(n, l):
    """``n x l``, entries in {-1, 0, 1} at density 0.25"""
    rng = np.random.default_rng([11, n, l])
    signs = rng.integers(0, 2, size=(n, l)) * 2 - 1
    return np.ascontiguousarray(np.where(rng.random((n, l)) < 0.25, signs, 0), dtype=np.float32)


def small(rows, cols):
    """``rows x cols`` with two entries of +/-1 per column (one where there is a single row)"""
    rng = np.random.default_rng([13, rows, cols])
    M = np.zeros((rows, cols), dtype=np.float32)
    for j in range(cols):
        at = rng.choice(rows, size=min(2, rows), replace=False)
        M[at, j] = rng.integers(0, 2, size=at.size) * 2.0 - 1.0
    return M


def inputs(X, l):
    """``(omega, M, rot)`` of the probe at width ``l`` on the user-item matrix ``X``"""
    l, l2, k = widths_of(l)
    return omega(min(X.shape), l), small(l, l2), small(l2, k)


def _gram(B):
    return B.T @ B, float((B * B).sum(axis=0).max()) if B.size else 0.0


def stages(X, omega, M, rot):
    """The chain of ``irs_truncsvd_range(n_iter=0)``, ``_apply``, ``_project`` and ``_finish`` in float64 (exact
    for these integers): a dict of ``Y, G1, Y2, G2, Q, G3, V, z, components`` as float64 arrays and ``bounds``,
    the largest sum of the magnitudes of the terms of one output element per stage (for a Gram matrix that is
    its largest diagonal entry: ``(|B|^T |B|)_ij <= sqrt((B^T B)_ii (B^T B)_jj)``).

    ``A = X`` when ``n_users >= n_items``, else ``X^T``.  The sign rule is ``finish``'s: per component, the entry
    of largest magnitude (the first among equals) is made positive, a zero component keeps +1, and ``z`` takes
    the same signs."""
    X = sps.csr_matrix(X, dtype=np.float64)
    transposed = X.shape[0] < X.shape[1]
    A = X.T.tocsr() if transposed else X
    At = A.T.tocsr()
    omega, M, rot = (np.asarray(a, dtype=np.float64) for a in (omega, M, rot))
    absA, absAt, absX = abs(A), abs(At), abs(X)
    out, bounds = {}, {}
    Y = np.asarray(A @ omega)
    bounds["Y"] = float(np.asarray(absA @ np.abs(omega)).max())
    out["G1"], bounds["G1"] = _gram(Y)
    Y2 = Y @ M
    bounds["Y2"] = float((np.abs(Y) @ np.abs(M)).max())
    out["G2"], bounds["G2"] = _gram(Y2)
    Q = np.asarray(At @ Y2)
    bounds["Q"] = float(np.asarray(absAt @ np.abs(Y2)).max())
    out["G3"], bounds["G3"] = _gram(Q)
    basis = Y2 if transposed else Q  # the n_items x l2 side
    V = basis @ rot
    bounds["V"] = float((np.abs(basis) @ np.abs(rot)).max())
    z = np.asarray(X @ V)
    bounds["z"] = float(np.asarray(absX @ np.abs(V)).max())
    top = V[np.abs(V).argmax(axis=0), np.arange(V.shape[1])]
    signs = np.where(top < 0, -1.0, 1.0)
    out.update(Y=Y, Y2=Y2, Q=Q, V=V, z=z * signs, components=np.ascontiguousarray((V * signs).T), bounds=bounds)
    return out
