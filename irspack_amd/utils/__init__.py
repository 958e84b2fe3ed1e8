"""The pieces of the reference's ``irspack.utils._util_cpp`` that the kNN path calls
(/root/reference/cpp_source/util.hpp:158-226, util.cpp:14,29-32) and the SLIM coordinate descent
(util.hpp:228-424, util.cpp:31-40); and the closed-form EASE / EDLAE weights (``dense_slim_weight``), which the
reference computes with scipy inside ``recommenders/dense_slim.py`` and ``recommenders/edlae.py``; and the
randomized truncated SVD (``truncated_svd``), which the reference takes from scikit-learn inside
``recommenders/truncsvd.py``; and the coordinate-descent NMF (``nmf_fit``, ``nmf_transform``), which the reference takes
from scikit-learn inside ``recommenders/nmf.py``; and the row-wise hold-out split (util.hpp:72-156, ``_split.py``).

Everything goes through the C ABI: ``remove_diagonal``, the serving top-k
``retrieve_recommend_from_score`` and the two feature weightings (``irs_knn_weight``; the kNN
recommenders do not call them - they hand the weighting to the computer's constructor, which
applies it on the device without a host copy of the weighted matrix).
"""

import warnings
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
            la = [C.c_int32() for _ in range(5)]
            limit = C.c_int64()
            check(lib().irs_slim_last_launch(handle, *[C.byref(v) for v in la], C.byref(limit)))
            stats.update(lds_r=bool(la[0].value), lds_bytes=la[1].value, threads=la[2].value, n_wg=la[3].value,
                         raise_dynamic_lds=bool(la[4].value), lds_per_block=limit.value)
    finally:
        lib().irs_slim_destroy(handle)
    W = sps.csc_matrix((vals[:nnz.value], rows[:nnz.value], col_ptr), shape=(n_items, n_items))
    W.has_sorted_indices = True
    return W


def slim_weight_allow_negative(X, n_threads: int, n_iter: int, l2_coeff: float, l1_coeff: float,
                               tol: float, top_k: int = -1, *, device: Optional[int] = None,
                               stats: Optional[dict] = None) -> sps.csc_matrix:
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
    non-zeros; ``-1`` keeps everything.  Duplicate entries of ``X`` are summed first.

    ``stats`` (measurement only) receives the phase times ``gram_ms, descent_ms, emit_ms`` (HIP events), the
    counters ``sweeps_total, updates_total`` and the launch of the descent kernel: ``lds_r`` (the running vector
    in LDS), ``lds_bytes``, ``threads``, ``n_wg``, ``raise_dynamic_lds`` and the per-block LDS limit the device
    reported, ``lds_per_block`` (``irs_slim_last_stats``, ``irs_slim_last_launch``)."""
    return _slim(X, False, n_threads, n_iter, l2_coeff, l1_coeff, tol, top_k, device, stats)


def slim_weight_positive_only(X, n_threads: int, n_iter: int, l2_coeff: float, l1_coeff: float,
                              tol: float, top_k: int = -1, *, device: Optional[int] = None,
                              stats: Optional[dict] = None) -> sps.csc_matrix:
    """:func:`slim_weight_allow_negative` under the constraint ``w >= 0`` (util.cpp:36-40)."""
    return _slim(X, True, n_threads, n_iter, l2_coeff, l1_coeff, tol, top_k, device, stats)


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


def truncated_svd_transform(X, components: np.ndarray, *, device: Optional[int] = None) -> np.ndarray:
    """The fold-in of the truncated SVD for rows the fit has not seen, ``X @ components.T`` (what
    ``TruncatedSVD.transform`` computes), on the device (``irs_truncsvd_transform``): ``components`` is ``(k, I)``
    float32 with ``1 <= k <= 576``, the result ``(rows, k)`` float32.  The values of ``X`` are read as float32 and
    the entries of a row are taken in column order with duplicates summed; every row sum is kept in double and
    rounded to float32 once, so an element differs from the float64 product by one float32 rounding plus the
    error of a double sum.  The result depends on the arguments alone: two calls give identical bytes."""
    C_ = np.asarray(components)
    if C_.ndim != 2 or C_.dtype != np.float32:
        raise ValueError("components must be a 2-D float32 array (k, n_items).")
    k, n_items = C_.shape
    if not 1 <= k <= 576:
        raise ValueError("the number of components must lie in 1 .. 576.")
    Xc = sps.csr_matrix(X, dtype=np.float32)
    if Xc.shape[1] != n_items:
        raise ValueError(f"X has {Xc.shape[1]} columns, components has {n_items}.")
    if not Xc.has_canonical_format:
        Xc = Xc.copy()
        Xc.sum_duplicates()  # (the C call wants sorted rows without duplicates)
    out = np.zeros((Xc.shape[0], k), dtype=np.float32)
    if Xc.shape[0] == 0:
        return out
    table = np.ascontiguousarray(C_.T)  # (I, k): a gathered row is contiguous
    indptr = np.ascontiguousarray(Xc.indptr, dtype=np.int64)
    indices = np.ascontiguousarray(Xc.indices, dtype=np.int32)
    data = np.ascontiguousarray(Xc.data, dtype=np.float32)
    if data.size == 0:
        indices, data = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.float32)
    check(lib().irs_truncsvd_transform(Xc.shape[0], n_items, ptr(indptr, C.c_int64), ptr(indices, C.c_int32),
                                       ptr(data, C.c_float), k, ptr(table, C.c_float),
                                       _lib.default_device() if device is None else device, ptr(out, C.c_float)))
    return out


class ConvergenceWarning(UserWarning):
    """scikit-learn's ``sklearn.exceptions.ConvergenceWarning`` by name (this package does not import scikit-learn)"""


NMF_INITS = (None, "random", "nndsvd", "nndsvda", "nndsvdar")


def nndsvd_init(U: np.ndarray, S: np.ndarray, Vt: np.ndarray, mean: float, variant: str = "nndsvda",
                rng: Optional[np.random.RandomState] = None, eps: float = 1e-6) -> Tuple[np.ndarray, np.ndarray]:
    """The NNDSVD arithmetic of scikit-learn's ``_initialize_nmf`` (Boutsidis & Gallopoulos 2008) on the host, in
    the dtype of ``U``: from the singular triplets ``U (n, k)``, ``S (k,)``, ``Vt (k, m)`` to the non-negative
    ``(W0 (n, k), H0 (k, m))``.  Every triplet past the first is split into its positive and negative parts and
    the pair with the larger product of norms is kept, entries below ``eps`` become 0; ``variant``:
    ``"nndsvd"`` leaves the zeros, ``"nndsvda"`` fills them with ``mean``, ``"nndsvdar"`` with
    ``|mean * rng.standard_normal() / 100|`` (``W`` first).  The result does not depend on the sign of a triplet.
    A triplet whose kept parts have norm 0 (a zero singular vector) gives a zero column and row, where
    scikit-learn divides 0 by 0."""
    if variant not in ("nndsvd", "nndsvda", "nndsvdar"):
        raise ValueError(f"Invalid init parameter: got {variant!r} instead of one of {NMF_INITS!r}")
    norm = lambda v: np.sqrt(np.dot(v, v))  # noqa: E731  (sklearn.utils.extmath.norm)
    W, H = np.zeros_like(U), np.zeros_like(Vt)
    W[:, 0] = np.sqrt(S[0]) * np.abs(U[:, 0])
    H[0, :] = np.sqrt(S[0]) * np.abs(Vt[0, :])
    for j in range(1, U.shape[1]):
        x, y = U[:, j], Vt[j, :]
        x_p, y_p = np.maximum(x, 0), np.maximum(y, 0)
        x_n, y_n = np.abs(np.minimum(x, 0)), np.abs(np.minimum(y, 0))
        x_p_nrm, y_p_nrm = norm(x_p), norm(y_p)
        x_n_nrm, y_n_nrm = norm(x_n), norm(y_n)
        m_p, m_n = x_p_nrm * y_p_nrm, x_n_nrm * y_n_nrm
        if m_p > m_n:
            u, v, sigma = x_p / x_p_nrm, y_p / y_p_nrm, m_p
        elif m_n > 0:
            u, v, sigma = x_n / x_n_nrm, y_n / y_n_nrm, m_n
        else:
            continue
        lbd = np.sqrt(S[j] * sigma)
        W[:, j] = lbd * u
        H[j, :] = lbd * v
    W[W < eps] = 0
    H[H < eps] = 0
    if variant == "nndsvda":
        W[W == 0] = mean
        H[H == 0] = mean
    elif variant == "nndsvdar":
        if rng is None:
            raise ValueError("nndsvdar needs a random generator.")
        W[W == 0] = abs(mean * rng.standard_normal(size=len(W[W == 0])) / 100)
        H[H == 0] = abs(mean * rng.standard_normal(size=len(H[H == 0])) / 100)
    return W, H


def _nmf_matrix(X) -> sps.csr_matrix:
    Xc = sps.csr_matrix(X, dtype=np.float32)
    if not Xc.has_canonical_format:
        Xc = Xc.copy()
        Xc.sum_duplicates()  # (the C call rejects duplicate column indices within a row)
    if Xc.nnz and Xc.data.min() < 0:
        raise ValueError("Negative values in data passed to NMF (input X).")
    return Xc


def _nmf_call(Xc, W: np.ndarray, H: np.ndarray, alpha: float, l1_ratio: float, tol: float, max_iter: int,
              update_H: bool, device: Optional[int], stats: Optional[dict]) -> int:
    """``irs_nmf_fit`` on the float32 arrays ``W`` and ``H`` in place; sklearn's scaling of the regularisers
    (``_compute_regularization`` with ``alpha_H = "same"``) and its convergence warning"""
    n_users, n_items = Xc.shape
    indptr = np.ascontiguousarray(Xc.indptr, dtype=np.int64)
    indices = np.ascontiguousarray(Xc.indices, dtype=np.int32)
    data = np.ascontiguousarray(Xc.data, dtype=np.float32)
    if data.size == 0:
        indices, data = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.float32)
    n_iter = C.c_int64(0)
    violations = np.zeros(max(int(max_iter), 1), dtype=np.float64)
    st = _lib.NmfStatsStruct()
    check(lib().irs_nmf_fit(
        n_users, n_items, ptr(indptr, C.c_int64), ptr(indices, C.c_int32), ptr(data, C.c_float), W.shape[1],
        ptr(W, C.c_float), ptr(H, C.c_float), n_items * alpha * l1_ratio, n_items * alpha * (1.0 - l1_ratio),
        n_users * alpha * l1_ratio, n_users * alpha * (1.0 - l1_ratio), float(tol), int(max_iter),
        1 if update_H else 0, _lib.default_device() if device is None else device, C.byref(n_iter),
        ptr(violations, C.c_double), C.cast(C.byref(st), C.c_void_p) if stats is not None else None))
    if stats is not None:
        stats.update({name: getattr(st, name) for name, _ in _lib.NmfStatsStruct._fields_},
                     violations=violations[:n_iter.value].copy())
    if n_iter.value == max_iter and tol > 0:
        warnings.warn("Maximum number of iterations %d reached. Increase it to improve convergence." % max_iter,
                      ConvergenceWarning)
    return int(n_iter.value)


def _check_nmf_params(alpha: float, l1_ratio: float, tol: float, max_iter: int) -> None:
    if not alpha >= 0:
        raise ValueError("alpha must be >= 0.")
    if not 0 <= l1_ratio <= 1:
        raise ValueError("l1_ratio must be in [0, 1].")
    if not tol >= 0:
        raise ValueError("tol must be >= 0.")
    if max_iter < 1:
        raise ValueError("max_iter must be >= 1.")


def nmf_fit(X, n_components: int, alpha: float = 0.0, l1_ratio: float = 0.0, *, init: Optional[str] = None,
            random_state: int = 42, tol: float = 1e-4, max_iter: int = 200, W0: Optional[np.ndarray] = None,
            H0: Optional[np.ndarray] = None, device: Optional[int] = None, stats: Optional[dict] = None):
    """The fit of ``sklearn.decomposition.NMF(n_components, init=init, solver="cd", beta_loss="frobenius",
    alpha_W=alpha, alpha_H="same", l1_ratio=l1_ratio, random_state=random_state, tol=tol, max_iter=max_iter)``
    (what nmf.py:48-64 of the reference fits) on the device (``irs_nmf_fit``), float32: alternating exact
    Gauss-Seidel coordinate sweeps over the rows of ``W`` and the columns of ``H``, coordinates ascending,
    stopped by sklearn's projected-gradient test.  Returns ``(W (U, k), H (k, I), n_iter)``, the factors float32
    and C-contiguous.  Two calls give identical bytes.  Duplicate entries of ``X`` are summed first.

    ``init``: ``None`` is ``"nndsvda"`` when ``n_components <= min(X.shape)``, else ``"random"``;
    ``"random"`` is sklearn's draw (``H`` first); the NNDSVD variants (:func:`nndsvd_init`) start from
    :func:`truncated_svd` with sklearn's automatic iteration count (7 when ``n_components < 0.1 min(X.shape)``,
    else 4) - the float32 device SVD in the place of sklearn's float64 one, so the start differs from sklearn's
    by rounding.  ``W0`` and ``H0`` (both or neither) are sklearn's ``init="custom"``.  An all-zero ``X`` without
    custom factors gives zero factors and ``n_iter = 1``, as sklearn does.

    When ``max_iter`` is reached and ``tol > 0``, sklearn's ``ConvergenceWarning`` is raised (a ``UserWarning``
    subclass of that name).  ``stats`` receives the device phase times ``setup_ms, spmm_ms, gram_ms, sweep_ms,
    d2h_ms`` (HIP events) and ``violations``, the per-iteration violation sums."""
    Xc = _nmf_matrix(X)
    n_users, n_items = Xc.shape
    k = int(n_components)
    if k < 1:
        raise ValueError("n_components must be >= 1.")
    _check_nmf_params(alpha, l1_ratio, tol, max_iter)
    if (W0 is None) != (H0 is None):
        raise ValueError("W0 and H0 go together: both or neither.")
    if init not in NMF_INITS:
        raise ValueError(f"Invalid init parameter: got {init!r} instead of one of {NMF_INITS!r}")
    if init not in (None, "random") and W0 is None and k > min(n_users, n_items):
        raise ValueError(f"init = '{init}' can only be used when n_components <= min(n_samples, n_features)")
    if n_users == 0 or n_items == 0:
        raise ValueError("the matrix must have at least one row and one column.")
    if W0 is not None:
        W = np.array(W0, dtype=np.float32, order="C")
        H = np.array(H0, dtype=np.float32, order="C")
        if W.shape != (n_users, k) or H.shape != (k, n_items):
            raise ValueError(f"W0 must be {(n_users, k)} and H0 {(k, n_items)}.")
    elif not Xc.data.any():
        if stats is not None:
            stats.update({name: 0.0 for name, _ in _lib.NmfStatsStruct._fields_}, violations=np.zeros(1))
        return np.zeros((n_users, k), dtype=np.float32), np.zeros((k, n_items), dtype=np.float32), 1
    else:
        mean = float(Xc.data.sum(dtype=np.float64)) / (float(n_users) * float(n_items))
        if init is None:
            init = "nndsvda" if k <= min(n_users, n_items) else "random"
        if init == "random":
            avg = np.sqrt(mean / k)
            rng = np.random.RandomState(random_state)
            H64 = np.abs(avg * rng.standard_normal(size=(k, n_items)))
            W64 = np.abs(avg * rng.standard_normal(size=(n_users, k)))
        else:
            auto_iter = 7 if k < 0.1 * min(n_users, n_items) else 4
            z, sigma, comps = truncated_svd(Xc, k, random_state, n_iter=auto_iter, device=device)
            S = sigma.astype(np.float64)
            U = np.where(S > 0, z.astype(np.float64) / np.where(S > 0, S, 1.0), 0.0)
            W64, H64 = nndsvd_init(U, S, comps.astype(np.float64), mean, init, np.random.RandomState(random_state))
        W = np.ascontiguousarray(W64, dtype=np.float32)
        H = np.ascontiguousarray(H64, dtype=np.float32)
    n_iter = _nmf_call(Xc, W, H, float(alpha), float(l1_ratio), float(tol), int(max_iter), True, device, stats)
    return W, H, n_iter


def nmf_transform(X, H: np.ndarray, alpha: float = 0.0, l1_ratio: float = 0.0, *, tol: float = 1e-4,
                  max_iter: int = 200, device: Optional[int] = None, stats: Optional[dict] = None) -> np.ndarray:
    """``NMF.transform`` of a model with ``components_ = H`` (what ``get_score_cold_user`` of the reference calls):
    the same loop with ``H`` fixed and only ``W`` swept, from ``W = 0`` as scikit-learn 1.x starts its ``cd``
    solver there, the regularisers scaled by the shape of ``X``.  Returns ``W (rows of X, k)`` float32."""
    Xc = _nmf_matrix(X)
    Hc = np.array(H, dtype=np.float32, order="C")
    if Hc.ndim != 2 or Hc.shape[1] != Xc.shape[1]:
        raise ValueError(f"H must be (k, {Xc.shape[1]}).")
    _check_nmf_params(alpha, l1_ratio, tol, max_iter)
    W = np.zeros((Xc.shape[0], Hc.shape[0]), dtype=np.float32)
    if Xc.shape[0] == 0:
        return W
    _nmf_call(Xc, W, Hc, float(alpha), float(l1_ratio), float(tol), int(max_iter), False, device, stats)
    return W


# irspack/utils/__init__.py exports the ID mappers from here (they import retrieve_recommend_from_score above)
from .id_mapping import IDMapper, ItemIDMapper  # noqa: E402,F401
# the row-wise hold-out split (util.hpp:72-156) with convert_randomstate and df_to_sparse
from ._split import (convert_randomstate, df_to_sparse, rowwise_train_test_split,  # noqa: E402,F401
                     rowwise_train_test_split_by_fixed_n, rowwise_train_test_split_by_ratio)
