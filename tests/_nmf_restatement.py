"""numpy / scipy restatement of what ``sklearn.decomposition.NMF(k, solver="cd", beta_loss="frobenius",
alpha_W=alpha, alpha_H="same", l1_ratio=..., shuffle=False)`` computes once ``W`` and ``H`` are initialised
(``_fit_coordinate_descent`` and the Cython sweep ``_update_cdnmf_fast`` of ``sklearn/decomposition``), its
``random`` initialisation, and ``transform`` (the same loop with ``H`` fixed, ``W`` starting at zero - what
scikit-learn 1.7 does for the ``cd`` solver).  ``dtype=np.float64`` is the arbiter of the GPU tests,
``dtype=np.float32`` casts the matrix, the initial factors and the regularisers to float32 and keeps the
violation sum in double: the reference's arithmetic on float32 input, which sets their bar."""
import numpy as np
import scipy.sparse as sps


def regularisers(shape, alpha, l1_ratio):
    """``(l1_W, l2_W, l1_H, l2_H)`` of ``_compute_regularization`` with ``alpha_H = "same"``"""
    n_users, n_items = shape
    return (n_items * alpha * l1_ratio, n_items * alpha * (1.0 - l1_ratio),
            n_users * alpha * l1_ratio, n_users * alpha * (1.0 - l1_ratio))


def random_init(X, n_components, random_state=42, dtype=np.float64):
    """``_initialize_nmf(init="random")``: ``H`` is drawn first"""
    avg = np.sqrt(X.mean() / n_components)
    rng = np.random.RandomState(random_state)
    H = avg * rng.standard_normal(size=(n_components, X.shape[1])).astype(dtype, copy=False)
    W = avg * rng.standard_normal(size=(X.shape[0], n_components)).astype(dtype, copy=False)
    return np.abs(W), np.abs(H)


def half_step(A, W, Ht, l1, l2):
    """One call of ``_update_coordinate_descent(A, W, Ht, l1, l2, shuffle=False)``: ``W`` is updated in place,
    the violation comes back as a double.  Rows are independent, so a coordinate is swept over all rows at once;
    the violation is added coordinate by coordinate, rows ascending, as the Cython loop adds it."""
    dtype = W.dtype
    k = Ht.shape[1]
    HHt = Ht.T @ Ht
    XHt = np.asarray(A @ Ht)
    if l2 != 0.0:
        HHt.flat[:: k + 1] += dtype.type(l2)
    if l1 != 0.0:
        XHt -= dtype.type(l1)
    violation = 0.0
    for t in range(k):
        grad = W @ HHt[t] - XHt[:, t]
        pg = np.where(W[:, t] == 0, np.minimum(grad, 0), grad)
        violation += float(np.abs(pg).astype(np.float64).sum())
        hess = HHt[t, t]
        if hess != 0:
            W[:, t] = np.maximum(W[:, t] - grad / hess, 0)
    return violation


def nmf_cd(X, W0, H0, alpha=0.0, l1_ratio=0.0, tol=1e-4, max_iter=200, dtype=np.float64, update_H=True):
    """``_fit_coordinate_descent``.  Returns ``(W, H, n_iter, violations)``, the factors in ``dtype`` and the
    per-iteration violation sums as a float64 array of length ``n_iter``."""
    dtype = np.dtype(dtype)
    X = sps.csr_matrix(X, dtype=dtype)
    Xt = X.T.tocsr()
    W = np.array(W0, dtype=dtype, order="C")
    Ht = np.array(np.asarray(H0).T, dtype=dtype, order="C")
    l1_W, l2_W, l1_H, l2_H = regularisers(X.shape, alpha, l1_ratio)
    history = []
    n_iter = 0
    for n_iter in range(1, max_iter + 1):
        violation = half_step(X, W, Ht, l1_W, l2_W)
        if update_H:
            violation += half_step(Xt, Ht, W, l1_H, l2_H)
        history.append(violation)
        if history[0] == 0:
            break
        if violation / history[0] <= tol:
            break
    return W, np.ascontiguousarray(Ht.T), n_iter, np.asarray(history, dtype=np.float64)


def nmf_transform(X, H, alpha=0.0, l1_ratio=0.0, tol=1e-4, max_iter=200, dtype=np.float64):
    """``NMF.transform``: ``H`` fixed, ``W`` from zero.  scikit-learn scales the regularisers by the shape of the
    matrix handed to ``transform``; returns ``(W, n_iter, violations)``."""
    W0 = np.zeros((X.shape[0], np.asarray(H).shape[0]), dtype=dtype)
    W, _, n_iter, history = nmf_cd(X, W0, H, alpha, l1_ratio, tol, max_iter, dtype, update_H=False)
    return W, n_iter, history


def factor_errors(W, H, W64, H64):
    """max abs differences of ``W @ H``, ``W`` and ``H`` from the float64 ones, each with the largest
    magnitude of the float64 array: ``((e_WH, top_WH), (e_W, top_W), (e_H, top_H))``"""
    W, H = np.asarray(W, dtype=np.float64), np.asarray(H, dtype=np.float64)
    S64 = W64 @ H64
    return ((float(np.abs(W @ H - S64).max()), float(np.abs(S64).max())),
            (float(np.abs(W - W64).max()), float(np.abs(W64).max())),
            (float(np.abs(H - H64).max()), float(np.abs(H64).max())))


def frobenius_objective(X, W, H):
    """``0.5 * ||X - W H||_F^2`` in float64 (dense: test shapes only)"""
    R = np.asarray(sps.csr_matrix(X, dtype=np.float64).todense()) - np.asarray(W, np.float64) @ np.asarray(H, np.float64)
    return 0.5 * float((R * R).sum())
