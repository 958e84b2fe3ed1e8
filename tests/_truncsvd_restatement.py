"""numpy / scipy restatement of what ``sklearn.decomposition.TruncatedSVD(k, random_state=s).fit_transform``
computes on its randomized branch (``sklearn.utils.extmath._randomized_svd`` with ``n_iter=5``,
``n_oversamples=10``, ``transpose="auto"``, LU-normalised power iterations - none for ``n_iter <= 2`` - an
economic QR of the last block, ``scipy.linalg.svd`` of the projected matrix, the sign flip on the rows of
``components_`` and ``z = X @ components_.T``).  ``dtype=np.float64`` is the arbiter of the GPU tests,
``dtype=np.float32`` the reference's own arithmetic on float32 input, which sets their bar."""
import numpy as np
import scipy.linalg
import scipy.sparse as sps


def randomized_truncated_svd(X, n_components, random_seed=0, dtype=np.float64, n_iter=5, n_oversamples=10):
    """Returns ``(z, singular_values, components)`` in ``dtype``."""
    X = sps.csr_matrix(X, dtype=dtype)
    A = X.T if X.shape[0] < X.shape[1] else X
    rng = np.random.RandomState(random_seed)
    Q = rng.normal(size=(A.shape[1], n_components + n_oversamples)).astype(dtype, copy=False)
    if n_iter <= 2:
        normalizer = lambda x: (x, None)  # noqa: E731
    else:
        normalizer = lambda x: scipy.linalg.lu(x, permute_l=True, check_finite=False)  # noqa: E731
    for _ in range(n_iter):
        Q, _ = normalizer(A @ Q)
        Q, _ = normalizer(A.T @ Q)
    Q, _ = scipy.linalg.qr(A @ Q, mode="economic", check_finite=False)
    B = Q.T @ A
    Uhat, s, Vt = scipy.linalg.svd(B, full_matrices=False, lapack_driver="gesdd")
    U = Q @ Uhat
    if A is not X:
        U, s, Vt = Vt[:n_components, :].T, s[:n_components], U[:, :n_components].T
    else:
        U, s, Vt = U[:, :n_components], s[:n_components], Vt[:n_components, :]
    rows = np.arange(Vt.shape[0])
    signs = np.sign(Vt[rows, np.argmax(np.abs(Vt), axis=1)])
    Vt = Vt * signs[:, np.newaxis]
    z = X @ Vt.T
    return np.asarray(z), s, Vt


def range_gram(A, omega, n_iter, dtype=np.float64):
    """What ``irs_truncsvd_range(omega, l, n_iter)`` hands back, restated in ``dtype``: the device's own power
    iteration, not sklearn's.  ``Q = omega``; ``n_iter`` times ``Y = A Q``, normalise, ``Q = A^T Y``, normalise;
    then ``Y = A Q`` and ``G = Y^T Y``.  Normalise a block ``B`` of ``l`` columns: ``G = B^T B + d I`` with
    ``d = 1e-5 * trace(B^T B) / l``, its Cholesky factor ``L`` (unique, so the result can be compared element by
    element), ``W = L^-1`` and ``B <- B W^T``."""
    A = sps.csr_matrix(A, dtype=dtype)
    At = A.T.tocsr()
    Q = np.ascontiguousarray(omega, dtype=dtype)
    l = Q.shape[1]
    eye = np.eye(l, dtype=dtype)

    def normalise(B):
        G = B.T @ B
        d = dtype(1e-5) * np.trace(G) / dtype(l)
        L = np.linalg.cholesky(G + d * eye)
        W = scipy.linalg.solve_triangular(L, eye, lower=True, check_finite=False)
        return B @ W.T

    for _ in range(n_iter):
        Q = normalise(np.asarray(A @ Q))
        Q = normalise(np.asarray(At @ Q))
    Y = np.asarray(A @ Q)
    G = Y.T @ Y
    assert G.dtype == dtype
    return G


def score_error(z, components, z64, components64):
    """max abs difference of the score matrices ``z @ components`` and the largest magnitude of the float64 one"""
    S = np.asarray(z, dtype=np.float64) @ np.asarray(components, dtype=np.float64)
    S64 = z64 @ components64
    return float(np.abs(S - S64).max()), float(np.abs(S64).max())


def sigma_error(sigma, sigma64):
    """max difference of the singular values over ``sigma_1``"""
    return float(np.abs(np.asarray(sigma, dtype=np.float64) - sigma64).max() / sigma64[0])
