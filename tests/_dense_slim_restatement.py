"""numpy restatement of the EASE / EDLAE weights (no test in here), written from the formula

    G = X^T X,   P = G + diag(lam),   lam_j = diag_scale * G_jj + reg,   B = P^-1,
    W_ij = -B_ij / B_jj  (i != j),   W_jj = 0.

``dtype=np.float64``: ``np.linalg.inv``, the arbiter of the GPU tests.  ``dtype=np.float32``:
``scipy.linalg.inv`` of a float32 ``P`` (LAPACK's single-precision LU), the arithmetic of the reference's
recommenders; its distance from float64 sets the bar of a configuration."""
import numpy as np
import scipy.linalg
import scipy.sparse as sps


def regularised_gram(X, reg, diag_scale=0.0, dtype=np.float64):
    """P as a dense array of ``dtype``; ``diag_scale`` and ``reg`` are rounded to ``dtype`` first and every
    operation on the diagonal is rounded to ``dtype`` (numpy's evaluation of ``scale * diag + reg``)."""
    Xd = sps.csr_matrix(X).astype(dtype)
    P = np.asarray((Xd.T @ Xd).todense(), dtype=dtype)
    idx = np.arange(P.shape[0])
    lam = dtype(diag_scale) * P[idx, idx] + dtype(reg)
    P[idx, idx] += lam
    return P


def weights_from_inverse(B):
    W = -B / np.diag(B)[np.newaxis, :]
    np.fill_diagonal(W, 0)
    return W


def ease_weights(X, reg, diag_scale=0.0, dtype=np.float64):
    P = regularised_gram(X, reg, diag_scale, dtype)
    if P.shape[0] == 0:
        return P
    B = np.linalg.inv(P) if dtype == np.float64 else scipy.linalg.inv(P)
    assert B.dtype == dtype
    return weights_from_inverse(B)


def worst_column_error(W, W64):
    """max over ALL columns of ||W[:, j] - W64[:, j]|| / ||W64[:, j]||; a column that is exactly zero in
    float64 counts 0 when it is exactly zero in W and inf otherwise."""
    W, W64 = np.asarray(W, dtype=np.float64), np.asarray(W64, dtype=np.float64)
    assert W.shape == W64.shape
    if W64.size == 0:
        return 0.0
    num, den = np.linalg.norm(W - W64, axis=0), np.linalg.norm(W64, axis=0)
    zero_ok = ~np.asarray(W != 0).any(axis=0)
    err = np.where(den > 0, num / np.where(den > 0, den, 1.0), np.where(zero_ok, 0.0, np.inf))
    return float(err.max())


def optimality_residual(P64, W):
    """max over i != j of |(P W)_ij - P_ij| / max|P| (W = I - B diag(B)^-1, so P W = P - diag(B)^-1)"""
    P64, W = np.asarray(P64, dtype=np.float64), np.asarray(W, dtype=np.float64)
    if P64.size == 0:
        return 0.0
    R = P64 @ W - P64
    np.fill_diagonal(R, 0.0)
    return float(np.abs(R).max() / np.abs(P64).max())
