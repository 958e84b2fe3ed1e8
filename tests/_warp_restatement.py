"""The WARP trainer's arithmetic restated in plain numpy ("WARP"): the yardstick of the GPU
tests, next to ``_bpr_restatement.py`` whose state, data and measures it shares.

``warp_search`` is the search of one synchronous batch on the caller's candidates: per position the first candidate
``t`` with ``x- > x+ - 1`` (``j = -1`` and ``t = max_sampled`` where there is none), and the margins it examined.
``warp_step`` is the batch itself: the search, then BPR's update with the weight ``w_t`` in place of the sigmoid on
the positions that found a violation.  Its float32 form takes ``(j, t)`` from the float64 search and does only the
update arithmetic in float32 - a float32 flip of a margin would make "what float32 loses" a different batch.
``warp_fit`` is a whole fit with numpy's generator in place of the library's.
"""
import math

import numpy as np
import scipy.sparse as sps

from _bpr_restatement import TABLES, initial_state

MAX_LOSS = 10.0


def warp_weights(n_items, max_sampled):
    """``w_t = min(ln(max(1, (n_items - 1) // t)), 10)`` for ``t = 1 .. max_sampled``, in double"""
    return np.array([min(math.log(max(1, (int(n_items) - 1) // t)), MAX_LOSS) for t in range(1, int(max_sampled) + 1)],
                    dtype=np.float64)


def warp_search(state, users, pos, cand, dtype=np.float64):
    """``(neg, tries, margins)``: ``margins[p, t - 1] = x- - (x+ - 1)`` of every examined candidate, NaN elsewhere"""
    U, V, b = (np.asarray(state[n], dtype=dtype) for n in ("U", "V", "b"))
    users, pos = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (users, pos))
    cand = np.asarray(cand, dtype=np.int64).reshape(users.size, -1)
    n, max_sampled = cand.shape
    pu = U[users]
    xp = (pu * V[pos]).sum(axis=1, dtype=dtype) + b[pos]
    xn = np.einsum("nk,ntk->nt", pu, V[cand]).astype(dtype) + b[cand]
    margin = xn - (xp[:, None] - dtype(1))
    hit = margin > 0
    found = hit.any(axis=1)
    first = np.where(found, hit.argmax(axis=1), max_sampled - 1)
    neg = np.where(found, cand[np.arange(n), first], -1).astype(np.int64)
    tries = (first + 1).astype(np.int64)
    margins = np.where(np.arange(max_sampled)[None, :] < tries[:, None], margin, np.nan)
    return neg, tries, margins


def warp_step(state, users, pos, cand, user_alpha, item_alpha, lr, dtype=np.float64, choice=None, n_items=None):
    """the state after one batch; ``state`` is not changed.  The search runs in float64 on ``state`` whatever
    ``dtype`` is, unless the caller hands in the ``choice = (neg, tries)`` of another run."""
    users, pos = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (users, pos))
    cand = np.asarray(cand, dtype=np.int64).reshape(users.size, -1)
    neg, tries = warp_search(state, users, pos, cand, np.float64)[:2] if choice is None else choice
    U, V, b, GU, GV, Gb = (np.array(state[n], dtype=dtype) for n in TABLES)
    weights = warp_weights(V.shape[0] if n_items is None else n_items, cand.shape[1])
    sel = np.asarray(neg) >= 0
    u, i, j = users[sel], pos[sel], np.asarray(neg, dtype=np.int64)[sel]
    w = weights[np.asarray(tries, dtype=np.int64)[sel] - 1].astype(dtype)
    ua, ia, lr = dtype(user_alpha), dtype(item_alpha), dtype(lr)
    d = V[i] - V[j]
    pu = U[u]
    gU, gV, gb = np.zeros_like(U), np.zeros_like(V), np.zeros_like(b)
    np.add.at(gU, u, -w[:, None] * d)
    np.add.at(gV, i, -w[:, None] * pu)
    np.add.at(gV, j, w[:, None] * pu)
    np.add.at(gb, i, -w)
    np.add.at(gb, j, w)
    tu, ti = np.unique(u), np.unique(np.concatenate([i, j]))
    for theta, G, g, rows, alpha in ((U, GU, gU, tu, ua), (V, GV, gV, ti, ia), (b, Gb, gb, ti, ia)):
        gr = g[rows] + alpha * theta[rows]
        theta[rows] -= lr * gr / np.sqrt(G[rows])  # (G is read before it is updated)
        G[rows] += gr * gr
    return dict(zip(TABLES, (U, V, b, GU, GV, Gb)), epoch=state.get("epoch", 0))


def touched_rows(users, pos, neg):
    """``(user rows, item rows)`` that a batch with these choices touches"""
    users, pos, neg = (np.asarray(a, dtype=np.int64) for a in (users, pos, neg))
    sel = neg >= 0
    return set(users[sel].tolist()), set(pos[sel].tolist()) | set(neg[sel].tolist())


def warp_fit(X, k, user_alpha=1e-9, item_alpha=1e-9, lr=0.05, batch_size=4096, epochs=20, seed=42, max_sampled=10,
             dtype=np.float64, stats=None):
    """a whole fit on the entries > 0 of ``X``: every epoch uses every positive of a user with an unseen item once, in
    a random order, each with ``max_sampled`` candidates uniform over the user's unseen items.  ``stats``, a list,
    receives ``(mean tries, share of positions without a violation, max |theta|)`` per epoch."""
    X = sps.csr_matrix(X)
    X = X.multiply(X > 0).tocsr()
    X.eliminate_zeros()
    X.sort_indices()
    n_users, n_items = X.shape
    rng = np.random.RandomState(seed)
    state = initial_state(n_users, n_items, k, rng, dtype)
    deg = np.diff(X.indptr)
    seen = np.zeros((n_users, n_items), dtype=bool)
    rows = np.repeat(np.arange(n_users), deg)
    seen[rows, X.indices] = True
    unseen = np.argsort(seen, axis=1, kind="stable")  # per user: the unseen items in order, then the seen ones
    use = deg[rows] < n_items
    pu, pi = rows[use], X.indices[use].astype(np.int64)
    for _ in range(epochs):
        order = rng.permutation(pu.size)
        u, i = pu[order], pi[order]
        free = (n_items - deg[u])[:, None]
        r = np.minimum((rng.random_sample((u.size, max_sampled)) * free).astype(np.int64), free - 1)
        cand = unseen[u[:, None], r]
        n_tries = n_none = 0
        for first in range(0, u.size, batch_size):
            sl = slice(first, first + batch_size)
            choice = warp_search(state, u[sl], i[sl], cand[sl], np.float64)[:2]
            n_tries += int(choice[1].sum())
            n_none += int((choice[0] < 0).sum())
            state = warp_step(state, u[sl], i[sl], cand[sl], user_alpha, item_alpha, lr, dtype, choice=choice)
        state["epoch"] += 1
        if stats is not None:
            stats.append((n_tries / max(u.size, 1), n_none / max(u.size, 1),
                          max(float(np.abs(state[n]).max()) for n in ("U", "V", "b"))))
    return state
