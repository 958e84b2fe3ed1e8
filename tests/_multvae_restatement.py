"""The Mult-VAE trainer's arithmetic restated in plain numpy: the yardstick of the GPU tests.

``forward`` / ``gradients`` / ``adam_step`` are one update on dense rows, runnable in float64 (the arbiter) and in
float32 (what a plain float32 implementation loses).  The device's generator is not restated: the order of the rows,
the dropout ``keep`` and the Gaussian ``eps`` are inputs.  ``fit`` is a whole fit with numpy's generator in their
place: the same model of the data, another random stream.  ``eval_scores`` is the evaluation forward pass.
"""
import numpy as np
import scipy.sparse as sps

TABLES = ("W1", "b1", "W2", "b2", "W3", "b3", "W4", "b4")
STATE_TABLES = TABLES + tuple("m" + n for n in TABLES) + tuple("v" + n for n in TABLES)


def shapes(n_items, H, L, Hd):
    return {"W1": (n_items, H), "b1": (H,), "W2": (H, 2 * L), "b2": (2 * L,), "W3": (L, Hd), "b3": (Hd,),
            "W4": (Hd, n_items), "b4": (n_items,)}


def initial_state(n_items, H, L, Hd, rng, dtype=np.float64):
    """biases 0, weights truncated normal at +-2 sigma with sigma = 1 / sqrt(fan_in), zero moments"""
    state = {}
    for name, shape in shapes(n_items, H, L, Hd).items():
        if name.startswith("b"):
            state[name] = np.zeros(shape, dtype)
            continue
        z = rng.standard_normal(shape)
        bad = np.abs(z) > 2.0
        while bad.any():
            z[bad] = rng.standard_normal(int(bad.sum()))
            bad = np.abs(z) > 2.0
        state[name] = (z / np.sqrt(shape[0])).astype(dtype)
    for name in TABLES:
        state["m" + name] = np.zeros_like(state[name])
        state["v" + name] = np.zeros_like(state[name])
    state["n_updates"], state["epoch"] = 0, 0
    return state


def kl_coefficient(goal, update, anneal_end_epoch, n_users, minibatch_size):
    total = anneal_end_epoch * n_users / minibatch_size
    return goal if total <= 0 else goal * min(1.0, update / total)


def _log_softmax(logit):
    mx = logit.max(axis=1, keepdims=True)
    return logit - (mx + np.log(np.exp(logit - mx).sum(axis=1, keepdims=True, dtype=logit.dtype)))


def forward(state, x, keep, eps, dropout_p, dtype=np.float64):
    """the training forward pass on dense raw rows ``x``; ``keep`` (0 / 1, the shape of ``x``) and ``eps`` (n, L)"""
    p = {n: np.asarray(state[n], dtype=dtype) for n in TABLES}
    x = np.asarray(x, dtype=dtype)
    L = p["W3"].shape[0]
    xn = x / np.sqrt((x * x).sum(axis=1, dtype=dtype) + dtype(1e-8))[:, None]
    xd = xn * np.asarray(keep, dtype=dtype) / dtype(1.0 - dropout_p)
    h1 = np.tanh(xd @ p["W1"] + p["b1"])
    ml = h1 @ p["W2"] + p["b2"]
    mu, lv = ml[:, :L], ml[:, L:]
    std = np.exp(lv / dtype(2))
    z = mu + np.asarray(eps, dtype=dtype) * std
    h2 = np.tanh(z @ p["W3"] + p["b3"])
    logit = h2 @ p["W4"] + p["b4"]
    lsm = _log_softmax(logit)
    nll = -(lsm * x).sum(axis=1, dtype=dtype)
    kl = (dtype(0.5) * (-lv + std * std + mu * mu - dtype(1))).sum(axis=1, dtype=dtype)
    return dict(p=p, x=x, xd=xd, h1=h1, mu=mu, lv=lv, std=std, z=z, h2=h2, lsm=lsm, eps=np.asarray(eps, dtype=dtype),
                nll=nll.mean(dtype=dtype), kl=kl.mean(dtype=dtype))


def loss(state, x, keep, eps, dropout_p, klc, dtype=np.float64):
    f = forward(state, x, keep, eps, dropout_p, dtype)
    return f["nll"] + dtype(klc) * f["kl"]


def gradients(state, x, keep, eps, dropout_p, klc, dtype=np.float64):
    """the eight gradient tables of ``loss`` (and the forward pass they came from)"""
    f = forward(state, x, keep, eps, dropout_p, dtype)
    p, n, klc = f["p"], dtype(x.shape[0]), dtype(klc)
    g = (np.exp(f["lsm"]) * f["x"].sum(axis=1, dtype=dtype)[:, None] - f["x"]) / n
    grads = {"W4": f["h2"].T @ g, "b4": g.sum(axis=0, dtype=dtype)}
    da3 = (g @ p["W4"].T) * (dtype(1) - f["h2"] * f["h2"])
    grads["W3"], grads["b3"] = f["z"].T @ da3, da3.sum(axis=0, dtype=dtype)
    dz = da3 @ p["W3"].T
    dmu = dz + klc * f["mu"] / n
    dlv = dz * f["eps"] * f["std"] / dtype(2) + klc * (f["std"] * f["std"] - dtype(1)) / (dtype(2) * n)
    dml = np.concatenate([dmu, dlv], axis=1)
    grads["W2"], grads["b2"] = f["h1"].T @ dml, dml.sum(axis=0, dtype=dtype)
    da1 = (dml @ p["W2"].T) * (dtype(1) - f["h1"] * f["h1"])
    grads["W1"], grads["b1"] = f["xd"].T @ da1, da1.sum(axis=0, dtype=dtype)
    f["da1"] = da1
    return {k: np.asarray(v, dtype=dtype) for k, v in grads.items()}, f


def adam_step(state, grads, lr, dtype=np.float64):
    """optax's ``adam(lr)`` on every element of every table; ``state`` is not changed"""
    t = int(state["n_updates"])
    c1, c2 = dtype(1.0 - 0.9 ** (t + 1)), dtype(1.0 - 0.999 ** (t + 1))
    new = dict(n_updates=t + 1, epoch=state.get("epoch", 0))
    for n in TABLES:
        g = np.asarray(grads[n], dtype=dtype)
        m = dtype(0.9) * np.asarray(state["m" + n], dtype=dtype) + dtype(0.1) * g
        v = dtype(0.999) * np.asarray(state["v" + n], dtype=dtype) + dtype(0.001) * g * g
        new["m" + n], new["v" + n] = m, v
        new[n] = np.asarray(state[n], dtype=dtype) - dtype(lr) * (m / c1) / (np.sqrt(v / c2) + dtype(1e-8))
    return new


def step(state, x, keep, eps, dropout_p, klc, lr, dtype=np.float64):
    """``(new state, gradients, forward)`` of one update"""
    grads, f = gradients(state, x, keep, eps, dropout_p, klc, dtype)
    return adam_step(state, grads, lr, dtype), grads, f


def dense_keep(X, users, keep_bytes):
    """the device's per-stored-entry ``keep`` bytes of the rows ``users`` as a dense 0 / 1 matrix"""
    X = sps.csr_matrix(X)
    out = np.zeros((len(users), X.shape[1]))
    at = 0
    for r, u in enumerate(users):
        cols = X.indices[X.indptr[u]:X.indptr[u + 1]]
        out[r, cols] = keep_bytes[at:at + cols.size]
        at += cols.size
    return out


def eval_hidden(state, x, dtype=np.float64):
    """``(h2, logit)`` of the evaluation forward pass: no dropout, z = mu"""
    p = {n: np.asarray(state[n], dtype=dtype) for n in TABLES}
    x = np.asarray(x, dtype=dtype)
    L = p["W3"].shape[0]
    xn = x / np.sqrt((x * x).sum(axis=1, dtype=dtype) + dtype(1e-8))[:, None]
    mu = (np.tanh(xn @ p["W1"] + p["b1"]) @ p["W2"] + p["b2"])[:, :L]
    h2 = np.tanh(mu @ p["W3"] + p["b3"])
    return h2, h2 @ p["W4"] + p["b4"]


def eval_scores(state, x, dtype=np.float64):
    """log-softmax scores of the evaluation forward pass"""
    return _log_softmax(eval_hidden(state, x, dtype)[1])


def fit(X, dim_z=16, enc_hidden=64, dec_hidden=None, dropout_p=0.5, kl_anneal_goal=0.2, anneal_end_epoch=50,
        minibatch_size=100, learning_rate=1e-2, epochs=10, seed=42, dtype=np.float64):
    """a whole fit with numpy's generator for the initial tables, the order, the dropout and eps"""
    D = np.asarray(sps.csr_matrix(X).todense(), dtype=dtype)
    n_users, n_items = D.shape
    rng = np.random.RandomState(seed)
    state = initial_state(n_items, enc_hidden, dim_z, dec_hidden or enc_hidden, rng, dtype)
    for _ in range(epochs):
        order = rng.permutation(n_users)
        for first in range(0, n_users, minibatch_size):
            rows = order[first:first + minibatch_size]
            x = D[rows]
            keep = rng.random_sample(x.shape) >= dropout_p
            eps = rng.standard_normal((rows.size, dim_z))
            klc = kl_coefficient(kl_anneal_goal, state["n_updates"], anneal_end_epoch, n_users, minibatch_size)
            epoch = state["epoch"]
            state = step(state, x, keep, eps, dropout_p, klc, learning_rate, dtype)[0]
            state["epoch"] = epoch
        state["epoch"] += 1
    return state
