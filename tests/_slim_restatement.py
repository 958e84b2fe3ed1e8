"""numpy restatement of the SLIM coordinate descent on the Gram matrix: the arbiter of the GPU tests
(float64) and their yardstick for what single precision costs (the same code in float32).

One update of coordinate ``f != j`` of target ``j`` (``q = G w`` is the running product)::

    lin  = q_f - G_fj - G_ff * w_f ;  quad = G_ff + l2
    plus = (-lin - l1) / quad ;  minus = (-lin + l1) / quad
    w_f' = plus if plus > 0, minus if (not positive_only) and minus < 0, else 0
    if w_f' != w_f:  q += G[:, f] * (w_f' - w_f)

coordinates in ascending order, every sweep; a sweep whose largest ``|w_f' - w_f|`` is ``< tol`` is the
last one; at most ``n_iter`` sweeps.  ``slim_column_plain`` is that loop, one Python step per coordinate;
``slim_column`` evaluates a chunk of coordinates at once from the current ``q`` and applies the first
change - the coordinates before it are final - which is the same arithmetic in the same order
(``tests/test_slim_surface.py`` holds the two equal bit for bit)."""
import numpy as np


def gram(X, dtype=np.float64) -> np.ndarray:
    Xd = np.asarray(X.toarray() if hasattr(X, "toarray") else X, dtype=np.float64)
    return np.ascontiguousarray((Xd.T @ Xd).astype(dtype))


def _sweep_plain(G, j, w, q, gj, d, l2, l1, positive_only):
    """one sweep, one Python step per coordinate; returns (largest change, number of changes)"""
    dt = G.dtype.type
    delta, n_changed = dt(0), 0
    for f in range(G.shape[0]):
        if f == j:
            continue
        lin = q[f] - gj[f] - d[f] * w[f]
        quad = d[f] + l2
        plus, minus = (-lin - l1) / quad, (-lin + l1) / quad
        new = plus if plus > 0 else (minus if (not positive_only and minus < 0) else dt(0))
        if new != w[f]:
            diff = dt(new - w[f])
            q += G[:, f] * diff
            w[f] = new
            delta = max(delta, abs(diff))
            n_changed += 1
    return delta, n_changed


def _sweep_chunked(G, j, w, q, gj, d, l2, l1, positive_only, chunk):
    """the same sweep: a chunk of coordinates evaluated at once from the current q, the first change
    applied (everything before it is final), the rest of the chunk evaluated again"""
    dt = G.dtype.type
    n = G.shape[0]
    quad = d + l2
    delta, n_changed = dt(0), 0
    for base in range(0, n, chunk):
        lo, hi = base, min(base + chunk, n)
        while lo < hi:
            s = slice(lo, hi)
            lin = q[s] - gj[s] - d[s] * w[s]
            plus, minus = (-lin - l1) / quad[s], (-lin + l1) / quad[s]
            new = np.where(plus > 0, plus, dt(0))
            if not positive_only:
                new = np.where(plus > 0, plus, np.where(minus < 0, minus, dt(0)))
            changed = new != w[s]
            if lo <= j < hi:
                changed[j - lo] = False
            hit = np.flatnonzero(changed)
            if hit.size == 0:
                break
            f = lo + int(hit[0])
            diff = dt(new[hit[0]] - w[f])
            q += G[:, f] * diff
            w[f] = new[hit[0]]
            delta = max(delta, abs(diff))
            n_changed += 1
            lo = f + 1
    return delta, n_changed


def _descend(G, j, l2, l1, n_iter, tol, positive_only, chunk, dense_fraction):
    dt = G.dtype.type
    n = G.shape[0]
    l2, l1, tol = dt(l2), dt(l1), dt(tol)
    w, q, gj, d = np.zeros(n, dtype=dt), np.zeros(n, dtype=dt), G[:, j].copy(), np.diag(G).copy()
    n_changed = 0
    with np.errstate(divide="ignore", invalid="ignore"):
        for _ in range(n_iter):
            # (a sweep that changes many coordinates is cheaper one coordinate at a time)
            if chunk <= 1 or n_changed > dense_fraction * n:
                delta, n_changed = _sweep_plain(G, j, w, q, gj, d, l2, l1, positive_only)
            else:
                delta, n_changed = _sweep_chunked(G, j, w, q, gj, d, l2, l1, positive_only, chunk)
            if delta < tol:
                break
    return w


def slim_column_plain(G, j, l2, l1, n_iter, tol, positive_only):
    return _descend(G, j, l2, l1, n_iter, tol, positive_only, 1, 0.0)


def slim_column(G, j, l2, l1, n_iter, tol, positive_only, chunk=256, dense_fraction=0.1):
    """``dense_fraction``: a sweep that follows one with more than this share of the coordinates changed
    runs as the plain loop (which is then the faster of the two equal forms)"""
    return _descend(G, j, l2, l1, n_iter, tol, positive_only, chunk, dense_fraction)


def kkt_residual(G64, j, w, l2, l1, positive_only) -> float:
    """Largest violation of the optimality conditions of column j, in float64."""
    w = np.asarray(w, dtype=np.float64)
    g = G64 @ w - G64[:, j] + l2 * w
    on = w != 0
    res = np.where(on, np.abs(g + l1 * np.sign(w)),
                   np.maximum(0.0, -g - l1) if positive_only else np.maximum(0.0, np.abs(g) - l1))
    res[j] = 0.0
    return float(res.max())
