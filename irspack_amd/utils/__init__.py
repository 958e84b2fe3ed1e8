"""The pieces of the reference's ``irspack.utils._util_cpp`` that the kNN path calls
(/root/reference/cpp_source/util.hpp:158-226, util.cpp:14,29-32) and the SLIM coordinate descent
(util.hpp:228-424, util.cpp:31-40); and the closed-form EASE / EDLAE weights (``dense_slim_weight``), which the
reference computes with scipy inside ``recommenders/dense_slim.py`` and ``recommenders/edlae.py``; and the
randomized truncated SVD (``truncated_svd``), which the reference takes from scikit-learn inside
``recommenders/truncsvd.py``.

Everything goes through the C ABI: ``remove_diagonal``, the serving top-k
``retrieve_recommend_from_score`` and the two feature weightings (``irs_knn_weight``; the kNN
recommenders do not call them - they hand the weighting to the computer's constructor, which
applies it on the device without a host copy of the weighted matrix).
"""

from typing import List, Optional, Sequence, Tuple

import ctypes as C

import numpy as np
import scipy.sparse as sps

from .. import _lib
from .._lib import check, lib, ptr


def remove_diagonal(X) -> sps.csr_matrix:
    """util.hpp:211-226: stored diagonal entries are set to 0.0 and kept (explicit zeros)."""
    Xc, indptr, indices, data = _lib.csr_arrays(X, np.float64)
    data = data.copy()
    if data.size == 0:
        data_arg = np.zeros(1, dtype=np.float64)
        idx_arg = np.zeros(1, dtype=np.int32)
    else:
        data_arg, idx_arg = data, indices
    check(lib().irs_remove_diagonal(C.c_int64(Xc.shape[0]), C.c_int64(Xc.shape[1]),
                                    ptr(indptr, C.c_int64), ptr(idx_arg, C.c_int32),
                                    ptr(data_arg, C.c_double)))
    out = sps.csr_matrix((data, indices.copy(), indptr.copy()), shape=Xc.shape)
    out.has_sorted_indices = True
    return out


def _weight(X, scheme: int, k1: float, b: float, smooth: bool, device: Optional[int]) -> sps.csr_matrix:
    """X's pattern with the weighted values: column counts, row sums and the idf table on host threads,
    the per-entry pass on the device (``irs_knn_weight``; the values are the host loop's bit for bit)."""
    Xc, indptr, indices, data = _lib.csr_arrays(X, np.float64)
    out = np.empty(data.shape[0], dtype=np.float64)
    if data.shape[0]:
        check(lib().irs_knn_weight(
            C.c_int32(scheme), C.c_int64(Xc.shape[0]), C.c_int64(Xc.shape[1]), ptr(indptr, C.c_int64),
            ptr(indices, C.c_int32), ptr(data, C.c_double), C.c_double(k1), C.c_double(b),
            C.c_int32(1 if smooth else 0), C.c_int32(_lib.default_device() if device is None else device),
            ptr(out, C.c_double)))
    res = sps.csr_matrix((out, Xc.indices.copy(), Xc.indptr.copy()), shape=Xc.shape)
    res.has_sorted_indices = True
    return res


def tf_idf_weight(X, smooth: bool = True, *, device: Optional[int] = None) -> sps.csr_matrix:
    """util.hpp:190-209 (bound at util.cpp:29-32): ``x * log(N / (df + smooth))``."""
    return _weight(X, _lib.WEIGHT_TF_IDF, 0.0, 0.0, bool(smooth), device)


def okapi_BM_25_weight(X, k1: float = 1.2, b: float = 0.75, *, device: Optional[int] = None) -> sps.csr_matrix:
    """util.hpp:158-188: ``idf * x (k1 + 1) / (x + k1 (1 - b + b dl / avgdl))``."""
    return _weight(X, _lib.WEIGHT_BM25, float(k1), float(b), True, device)


def _retrieve(score: np.ndarray, allowed_item_indices: Sequence[Sequence[int]], cutoff: int,
              n_threads: int, device: Optional[int]) -> List[List[Tuple[int, float]]]:
    if cutoff < 0 or n_threads < 0:
        raise TypeError("cutoff and n_threads must be non-negative (size_t).")
    score = np.ascontiguousarray(score)
    if score.ndim != 2:
        raise ValueError("score must be a 2-d array.")
    rows, n_items = score.shape
    lptr = np.zeros(len(allowed_item_indices) + 1, dtype=np.int64)
    for i, l in enumerate(allowed_item_indices):
        lptr[i + 1] = lptr[i] + len(l)
    litems = np.zeros(max(int(lptr[-1]), 1), dtype=np.int64)
    for i, l in enumerate(allowed_item_indices):
        litems[lptr[i]:lptr[i + 1]] = np.asarray(l, dtype=np.int64)
    # the reference clamps the list length to the candidate count (util.hpp:476-481): a cutoff
    # of n_items ("rank everything") needs n_items slots at most (above 2048 the device keeps
    # the selected lists in global scratch instead of LDS: rank_rows_kernel<..., BIG>)
    width = max(min(int(cutoff), int(n_items)), 0)
    out = np.full((rows, max(width, 1)), -1, dtype=np.int32)
    check(lib().irs_retrieve_recommend(
        C.c_int32(1 if score.dtype == np.float64 else 0), score.ctypes.data_as(C.c_void_p),
        C.c_int64(rows), C.c_int64(n_items), C.c_int64(len(allowed_item_indices)),
        ptr(lptr, C.c_int64), ptr(litems, C.c_int64), C.c_int64(width), C.c_int64(n_threads),
        C.c_int32(_lib.default_device() if device is None else device), ptr(out, C.c_int32)))
    result: List[List[Tuple[int, float]]] = []
    for r in range(rows):
        idx = out[r][out[r] >= 0] if width > 0 else out[r][:0]
        # the reference returns std::pair<int64_t, float>: scores are narrowed to float32
        vals = score[r, idx].astype(np.float32)
        result.append([(int(i), float(v)) for i, v in zip(idx, vals)])
    return result


def retrieve_recommend_from_score_f32(score, allowed_indices, cutoff: int, n_threads: int = 1,
                                      *, device: Optional[int] = None):
    """util.hpp:426-504 for float32 scores (bound as ``retrieve_recommend_from_score_f32``)."""
    return _retrieve(np.asarray(score, dtype=np.float32), allowed_indices, cutoff, n_threads,
                     device)


def retrieve_recommend_from_score_f64(score, allowed_indices, cutoff: int, n_threads: int = 1,
                                      *, device: Optional[int] = None):
    """util.hpp:426-504 for float64 scores (bound as ``retrieve_recommend_from_score_f64``)."""
    return _retrieve(np.asarray(score, dtype=np.float64), allowed_indices, cutoff, n_threads,
                     device)


def retrieve_recommend_from_score(score, allowed_item_indices, cutoff: int, n_threads: int = 1,
                                  *, device: Optional[int] = None):
    """irspack/utils/id_mapping.py:29-44: dispatch on the score dtype."""
    score = np.asarray(score)
    if score.dtype == np.float32:
        return retrieve_recommend_from_score_f32(score, allowed_item_indices, cutoff, n_threads,
                                                 device=device)
    if score.dtype == np.float64:
        return retrieve_recommend_from_score_f64(score, allowed_item_indices, cutoff, n_threads,
                                                 device=device)
    raise ValueError("Only float32 or float64 are allowed.")


def _slim(X, positive_only: bool, n_threads: int, n_iter: int, l2_coeff: float, l1_coeff: float,
          tol: float, top_k: int, device: Optional[int], stats: Optional[dict] = None) -> sps.csc_matrix:
    # util.hpp:233-236, before any device work (the C call repeats the last three)
    if n_threads <= 0:
        raise ValueError("n_threads must be > 0.")
    if n_iter <= 0:
        raise ValueError("n_iter must be > 0.")
    if l2_coeff < 0:
        raise ValueError("l2_coeff must be > 0.")
    if l1_coeff < 0:
        raise ValueError("l1_coeff must be > 0.")
    Xc = sps.csr_matrix(X, dtype=np.float32)
    if not Xc.has_canonical_format:
        Xc = Xc.copy()
        Xc.sum_duplicates()  # (the C call rejects duplicate column indices within a row)
    n_items = Xc.shape[1]
    indptr = np.ascontiguousarray(Xc.indptr, dtype=np.int64)
    indices = np.ascontiguousarray(Xc.indices, dtype=np.int32)
    data = np.ascontiguousarray(Xc.data, dtype=np.float32)
    if data.size == 0:
        indices, data = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.float32)
    handle = C.c_void_p()
    check(lib().irs_slim_fit(
        Xc.shape[0], n_items, ptr(indptr, C.c_int64), ptr(indices, C.c_int32), ptr(data, C.c_float),
        1 if positive_only else 0, int(n_iter), float(l2_coeff), float(l1_coeff), float(tol), int(top_k),
        _lib.default_device() if device is None else device, C.byref(handle)))
    try:
        nnz = C.c_int64()
        check(lib().irs_slim_nnz(handle, C.byref(nnz)))
        col_ptr = np.zeros(n_items + 1, dtype=np.int64)
        rows = np.zeros(max(nnz.value, 1), dtype=np.int32)
        vals = np.zeros(max(nnz.value, 1), dtype=np.float32)
        check(lib().irs_slim_fetch(handle, ptr(col_ptr, C.c_int64), ptr(rows, C.c_int32), ptr(vals, C.c_float)))
        if stats is not None:
            g, d, e = C.c_double(), C.c_double(), C.c_double()
            sw, up = C.c_int64(), C.c_int64()
            check(lib().irs_slim_last_stats(handle, C.byref(g), C.byref(d), C.byref(e), C.byref(sw), C.byref(up)))
            stats.update(gram_ms=g.value, descent_ms=d.value, emit_ms=e.value, sweeps_total=sw.value,
                         updates_total=up.value)
    finally:
        lib().irs_slim_destroy(handle)
    W = sps.csc_matrix((vals[:nnz.value], rows[:nnz.value], col_ptr), shape=(n_items, n_items))
    W.has_sorted_indices = True
    return W


def slim_weight_allow_negative(X, n_threads: int, n_iter: int, l2_coeff: float, l1_coeff: float,
                               tol: float, top_k: int = -1, *, device: Optional[int] = None) -> sps.csc_matrix:
    """util.hpp:228-424 with ``positive_only = false`` (bound at util.cpp:31-35): for every item ``j`` the
    elastic-net fit of column ``j`` on the other columns, ``min 1/2 |x_j - X w|^2 + l2/2 |w|^2 + l1 |w|_1``,
    by cyclic coordinate descent from 0 on the device (``irs_slim_fit``).  Returns the ``I x I`` float32
    ``csc_matrix`` with ``W[f, j] = w_f`` of target ``j``: sorted indices, no stored zeros, empty diagonal.

    Where the reference's output depends on more than its arguments, this one does not:

    * the coordinate order is the ascending one in every sweep (the reference shuffles with a per-thread
      generator, so its unconverged output depends on ``n_threads`` and scheduling); the update is exact
      Gauss-Seidel and the result is bit-identical from call to call.  ``n_threads`` is validated
      (``> 0``) and otherwise ignored;
    * every column stops on its own: after the first sweep whose largest coefficient change is ``< tol``
      (the reference stops a SIMD-packet-sized block of columns together);
    * a coordinate with ``G_ff + l2 == 0`` (an item without interactions, ``l2_coeff = 0``) gets 0.

    ``top_k >= 0`` keeps the ``top_k`` largest values (not magnitudes) of a column that has more
    non-zeros; ``-1`` keeps everything.  Duplicate entries of ``X`` are summed first."""
    return _slim(X, False, n_threads, n_iter, l2_coeff, l1_coeff, tol, top_k, device)


def slim_weight_positive_only(X, n_threads: int, n_iter: int, l2_coeff: float, l1_coeff: float,
                              tol: float, top_k: int = -1, *, device: Optional[int] = None) -> sps.csc_matrix:
    """:func:`slim_weight_allow_negative` under the constraint ``w >= 0`` (util.cpp:36-40)."""
    return _slim(X, True, n_threads, n_iter, l2_coeff, l1_coeff, tol, top_k, device)


def dense_slim_weight(X, reg: float, diag_scale: float = 0.0, *, device: Optional[int] = None,
                      stats: Optional[dict] = None) -> np.ndarray:
    """The EASE / EDLAE item-item weights (dense_slim.py:39-53, edlae.py:49-66) on the device
    (``irs_dense_slim_fit``), float32 throughout::

        G = X^T X,  P = G + diag(diag_scale * diag(G) + reg),  B = P^-1,
        W[i, j] = -B[i, j] / B[j, j]  (i != j),  W[j, j] = 0

    Returns the C-contiguous float32 ``(I, I)`` array; two calls give identical bytes.  Duplicate entries
    of ``X`` are summed first.  ``P`` is inverted from its Cholesky factor: a ``P`` that is not positive
    definite raises ``numpy.linalg.LinAlgError`` (the reference's scipy LU inverse raises it for a singular
    ``P`` only; an indefinite but non-singular ``P`` - ``dropout_p > 1``, a negative ``reg`` - is an error
    here).  ``stats`` receives the phase times ``gram_ms, factor_ms, invert_ms, finalize_ms, d2h_ms`` (HIP
    events) and the padded order ``n_pad``."""
    Xc = sps.csr_matrix(X, dtype=np.float32)
    if not Xc.has_canonical_format:
        Xc = Xc.copy()
        Xc.sum_duplicates()  # (the C call rejects duplicate column indices within a row)
    n_items = Xc.shape[1]
    indptr = np.ascontiguousarray(Xc.indptr, dtype=np.int64)
    indices = np.ascontiguousarray(Xc.indices, dtype=np.int32)
    data = np.ascontiguousarray(Xc.data, dtype=np.float32)
    if data.size == 0:
        indices, data = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.float32)
    W = np.empty((n_items, n_items), dtype=np.float32)
    st = _lib.DenseSlimStatsStruct()
    status = lib().irs_dense_slim_fit(
        Xc.shape[0], n_items, ptr(indptr, C.c_int64), ptr(indices, C.c_int32), ptr(data, C.c_float),
        float(reg), float(diag_scale), _lib.default_device() if device is None else device,
        W.ctypes.data_as(C.POINTER(C.c_float)), C.cast(C.byref(st), C.c_void_p))
    if status == 2:
        msg = lib().irs_last_error().decode("utf-8", "replace")
        if "not positive definite" in msg:
            raise np.linalg.LinAlgError(msg)
    check(status)
    if stats is not None:
        stats.update({name: getattr(st, name) for name, _ in _lib.DenseSlimStatsStruct._fields_})
    return W


def _descending_eigh(G: np.ndarray):
    """eigenvalues (descending) and eigenvectors of a symmetric matrix, float64"""
    w, V = np.linalg.eigh(np.asarray(G, dtype=np.float64))
    return w[::-1], V[:, ::-1]


def truncated_svd(X, n_components: int, random_seed: int = 0, *, n_iter: int = 5, n_oversamples: int = 10,
                  device: Optional[int] = None, stats: Optional[dict] = None):
    """The randomized truncated SVD of ``sklearn.decomposition.TruncatedSVD(n_components, random_state=random_seed)``
    (what truncsvd.py:79-83 of the reference fits) with the sparse and the tall dense products on the device
    (``irs_truncsvd_*``), float32.  Returns ``(z, singular_values, components)``: ``(U, k)``, ``(k,)`` and
    ``(k, I)`` float32, C-contiguous; ``z = X @ components.T``; in each row of ``components`` the entry of
    largest magnitude is positive.  Two calls give identical bytes.

    The Gaussian test matrix is sklearn's (``RandomState(random_seed).normal(size=(n, k + n_oversamples))``,
    ``n = n_items`` when ``n_users >= n_items``, else ``n_users`` with ``X^T`` in the place of ``X``), cast to
    float32 and clipped to its leading ``min(l, n_users, n_items)`` columns; the power iterations are
    normalised by a shifted Cholesky factor instead of sklearn's LU, which spans the same subspace.  The
    final basis is orthonormalised twice through the eigen-decomposition of its Gram matrix (float64, on the
    host, eigenvalues ``<= 1e-6 * max`` dropped: rank revealing), the singular values and the rotation come
    from the eigen-decomposition of ``B B^T``, ``B = Y^T A``.  A component past the numerical rank (the
    basis has fewer columns than ``n_components``, or its eigenvalue of ``B B^T`` is not positive) is a zero
    row with singular value 0.

    ``stats`` receives the device phase times ``setup_ms, spmm_ms, gram_ms, chol_ms, apply_ms, d2h_ms`` (HIP
    events), ``n_spmm``, ``l_pad``, the host times ``host_ms`` (signs and the transpose of the components inside the
    last call), ``eigh_ms`` (the eigenproblems) and ``omega_ms`` (the test matrix)."""
    import time

    Xc = sps.csr_matrix(X, dtype=np.float32)
    if not Xc.has_canonical_format:
        Xc = Xc.copy()
        Xc.sum_duplicates()  # (the C call rejects duplicate column indices within a row)
    n_users, n_items = Xc.shape
    k = int(n_components)
    if k < 1:
        raise ValueError("n_components must be >= 1.")
    if k > n_items:
        raise ValueError(f"n_components({k}) must be <= n_features({n_items}).")  # (sklearn's check)
    if n_iter < 0 or n_oversamples < 0:
        raise ValueError("n_iter and n_oversamples must be >= 0.")
    z = np.zeros((n_users, k), dtype=np.float32)
    sigma = np.zeros(k, dtype=np.float32)
    comps = np.zeros((k, n_items), dtype=np.float32)
    if stats is not None:
        stats.update({name: 0 for name, _ in _lib.TruncSvdStatsStruct._fields_}, eigh_ms=0.0, omega_ms=0.0)
    if n_users == 0 or not Xc.data.any():
        return z, sigma, comps
    t0 = time.perf_counter()
    n = n_items if n_users >= n_items else n_users
    l_full = k + int(n_oversamples)
    l = min(l_full, n_users, n_items)
    omega = np.random.RandomState(random_seed).normal(size=(n, l_full))
    omega = np.ascontiguousarray(omega[:, :l], dtype=np.float32)
    omega_ms = (time.perf_counter() - t0) * 1e3
    indptr = np.ascontiguousarray(Xc.indptr, dtype=np.int64)
    indices = np.ascontiguousarray(Xc.indices, dtype=np.int32)
    data = np.ascontiguousarray(Xc.data, dtype=np.float32)
    fptr = lambda a: ptr(a, C.c_float)  # noqa: E731
    eigh_s = 0.0
    handle = C.c_void_p()
    check(lib().irs_truncsvd_create(n_users, n_items, ptr(indptr, C.c_int64), ptr(indices, C.c_int32), fptr(data),
                                    _lib.default_device() if device is None else device, C.byref(handle)))
    try:
        G = np.empty((l, l), dtype=np.float32)
        check(lib().irs_truncsvd_range(handle, fptr(omega), n, l, int(n_iter), fptr(G)))
        for _ in range(2):  # Y <- Y V diag(w)^-1/2 over the eigenvalues that count
            t = time.perf_counter()
            w, V = _descending_eigh(G)
            keep = w > 1e-6 * w[0]
            M = np.ascontiguousarray(V[:, keep] / np.sqrt(w[keep]), dtype=np.float32)
            eigh_s += time.perf_counter() - t
            if M.shape[1] == 0:
                return z, sigma, comps
            G = np.empty((M.shape[1], M.shape[1]), dtype=np.float32)
            check(lib().irs_truncsvd_apply(handle, fptr(M), M.shape[1], fptr(G)))
        l2 = G.shape[0]
        check(lib().irs_truncsvd_project(handle, fptr(G)))
        t = time.perf_counter()
        w, R = _descending_eigh(G)
        kk = min(k, l2)
        s = np.sqrt(np.maximum(w[:kk], 0.0))
        live = s > 0
        s = np.where(live, s, 0.0)
        # A = X: V = B^T R / sigma;  A = X^T: the components are the rotated basis Y R itself
        scale = np.where(live, 1.0 / np.where(live, s, 1.0), 0.0) if n_users >= n_items else live.astype(np.float64)
        rot = np.ascontiguousarray(R[:, :kk] * scale, dtype=np.float32)
        eigh_s += time.perf_counter() - t
        zk = np.empty((n_users, kk), dtype=np.float32)
        ck = np.empty((kk, n_items), dtype=np.float32)
        check(lib().irs_truncsvd_finish(handle, fptr(rot), kk, fptr(zk), fptr(ck)))
        z[:, :kk], comps[:kk], sigma[:kk] = zk, ck, s
        if stats is not None:
            st = _lib.TruncSvdStatsStruct()
            check(lib().irs_truncsvd_stats(handle, C.cast(C.byref(st), C.c_void_p)))
            stats.update({name: getattr(st, name) for name, _ in _lib.TruncSvdStatsStruct._fields_},
                         eigh_ms=eigh_s * 1e3, omega_ms=omega_ms)
    finally:
        lib().irs_truncsvd_destroy(handle)
    return z, sigma, comps
