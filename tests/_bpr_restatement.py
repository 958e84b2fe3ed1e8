"""The BPR trainer's arithmetic restated in plain numpy: the yardstick of the GPU tests.

``bpr_step`` is one synchronous batch - every triple reads the parameters as the batch found them, the per-row
gradient sums are ``np.add.at`` in the order of the triples, the L2 term and Adagrad go to the touched rows once -
runnable in float64 (the arbiter) and in float32 (what a plain float32 implementation loses).  ``bpr_fit`` is a
whole fit with numpy's generator in place of the library's: the same model of the data, another random stream.
``planted_split`` is the data of the quality tests, ``ndcg_at`` their measure (the evaluator's nDCG, on the host).
"""
import numpy as np
import scipy.sparse as sps

TABLES = ("U", "V", "b", "GU", "GV", "Gb")


def bpr_step(state, users, pos, neg, user_alpha, item_alpha, lr, dtype=np.float64):
    """the state after one batch on the triples; ``state`` is not changed"""
    U, V, b, GU, GV, Gb = (np.array(state[n], dtype=dtype) for n in TABLES)
    users, pos, neg = (np.asarray(a, dtype=np.int64) for a in (users, pos, neg))
    ua, ia, lr = dtype(user_alpha), dtype(item_alpha), dtype(lr)
    d = V[pos] - V[neg]
    pu = U[users]
    with np.errstate(over="ignore"):
        x = (pu * d).sum(axis=1, dtype=dtype) + b[pos] - b[neg]
        w = (dtype(1) / (dtype(1) + np.exp(x))).astype(dtype)
    gU, gV, gb = np.zeros_like(U), np.zeros_like(V), np.zeros_like(b)
    np.add.at(gU, users, -w[:, None] * d)
    np.add.at(gV, pos, -w[:, None] * pu)
    np.add.at(gV, neg, w[:, None] * pu)
    np.add.at(gb, pos, -w)
    np.add.at(gb, neg, w)
    tu, ti = np.unique(users), np.unique(np.concatenate([pos, neg]))
    for theta, G, g, rows, alpha in ((U, GU, gU, tu, ua), (V, GV, gV, ti, ia), (b, Gb, gb, ti, ia)):
        gr = g[rows] + alpha * theta[rows]
        theta[rows] -= lr * gr / np.sqrt(G[rows])  # (G is read before it is updated)
        G[rows] += gr * gr
    return dict(zip(TABLES, (U, V, b, GU, GV, Gb)), epoch=state.get("epoch", 0))


def initial_state(n_users, n_items, k, rng, dtype=np.float64):
    """LightFM's start: embeddings uniform in (-0.5, 0.5) / k, zero biases, accumulators 1"""
    U = ((rng.random_sample((n_users, k)) - 0.5) / k).astype(dtype)
    V = ((rng.random_sample((n_items, k)) - 0.5) / k).astype(dtype)
    return dict(U=U, V=V, b=np.zeros(n_items, dtype), GU=np.ones_like(U), GV=np.ones_like(V),
                Gb=np.ones(n_items, dtype), epoch=0)


def unseen_by_rank(row, r):
    """the r-th (from 0) column that the sorted ``row`` does not hold: ``r + #{m : row[m] - m <= r}``"""
    row = np.asarray(row, dtype=np.int64)
    return int(r + np.count_nonzero(row - np.arange(row.size) <= r))


def bpr_fit(X, k, user_alpha=1e-9, item_alpha=1e-9, lr=0.05, batch_size=4096, epochs=20, seed=42, dtype=np.float64):
    """a whole fit on the entries > 0 of ``X``; every epoch uses every positive of a user with an unseen item once,
    in a random order, each with one negative uniform over the user's unseen items"""
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
        r = np.minimum((rng.random_sample(u.size) * (n_items - deg[u])).astype(np.int64), n_items - deg[u] - 1)
        j = unseen[u, r]
        for first in range(0, u.size, batch_size):
            sl = slice(first, first + batch_size)
            state = bpr_step(state, u[sl], i[sl], j[sl], user_alpha, item_alpha, lr, dtype)
        state["epoch"] += 1
    return state


def scores(state):
    return np.asarray(state["U"], np.float64) @ np.asarray(state["V"], np.float64).T + \
        np.asarray(state["b"], np.float64)[None, :]


def planted_matrix():
    """600 users x 400 items in 8 groups: 20 items of the user's own group and 5 anywhere"""
    rng = np.random.RandomState(0)
    n_users, n_items, n_groups = 600, 400, 8
    gu = rng.randint(0, n_groups, n_users)
    gi = np.arange(n_items) % n_groups
    rows, cols = [], []
    for u in range(n_users):
        own = np.flatnonzero(gi == gu[u])
        items = np.unique(np.concatenate([rng.choice(own, 20, replace=False), rng.randint(0, n_items, 5)]))
        rows.append(np.full(items.size, u))
        cols.append(items)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    return sps.csr_matrix((np.ones(rows.size), (rows, cols)), shape=(n_users, n_items))


_planted = []


def planted_split():
    """``(X_train, X_test)`` of the planted matrix by ``synthetic.holdout_split`` at its defaults (computed once)"""
    if not _planted:
        from irspack_amd.synthetic import holdout_split

        _planted.append(holdout_split(planted_matrix()))
    return _planted[0]


def ndcg_at(score, X_train, X_test, cutoff=20):
    """mean nDCG@cutoff over the users with a test item, seen items removed (the evaluator's definition)"""
    S = np.array(score, dtype=np.float64)
    S[sps.csr_matrix(X_train).nonzero()] = -np.inf
    X_test = sps.csr_matrix(X_test)
    top = np.argsort(-S, axis=1, kind="stable")[:, :cutoff]
    discount = 1.0 / np.log2(np.arange(cutoff) + 2.0)
    total, n = 0.0, 0
    for u in range(S.shape[0]):
        truth = X_test.indices[X_test.indptr[u]:X_test.indptr[u + 1]]
        if truth.size == 0:
            continue
        hit = np.isin(top[u], truth)
        total += float((hit * discount).sum() / discount[:min(truth.size, cutoff)].sum())
        n += 1
    return total / max(n, 1)
