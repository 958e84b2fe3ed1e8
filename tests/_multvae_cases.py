"""The inputs of the Mult-VAE single-update, scoring and divergence tests (``test_gpu_multvae.py``), built from numpy,
scipy and the restatement alone, so that ``test_multvae_case_inputs.py`` can check them without a device: the batch
matrices, the starts, the explicit noise, the case tables and the slab counts the cases are named after."""
import numpy as np
import scipy.sparse as sps

import _multvae_restatement as R
from _multvae_restatement import TABLES

LR = 1e-2
DH2_SLAB_UNIT, DH2_MAX_SLABS, DW4_SLAB = 512, 64, 256  # (multvae_host_prep.hpp)


def dh2_slab(n_items):
    """items per K-slab of dh2, restated from multvae_host_prep.hpp: 512, times a factor that keeps the slabs <= 64"""
    factor = -(-n_items // (DH2_SLAB_UNIT * DH2_MAX_SLABS))
    return DH2_SLAB_UNIT * max(1, factor)


# ---- the data of the single-update tests ---------------------------------------------------------------------------
def batch_matrix(n, n_items, seed):
    """n rows: non-binary values at density 0.15; row 0 empty; row 1 with every item but item 3, which no row has
    (the row is long enough for every wave of the encoder kernel); an explicit zero stored in row 2"""
    rng = np.random.default_rng(seed)
    D = (rng.random((n, n_items)) < 0.15) * rng.choice([0.5, 1.0, 2.0, 3.0], (n, n_items))
    if n >= 3:
        D[0] = 0
    D[min(1, n - 1)] = rng.choice([0.5, 1.0, 2.0], n_items)
    D[:, 3] = 0
    X = sps.csr_matrix(D.astype(np.float32))
    if n >= 3 and X.indptr[3] > X.indptr[2]:
        X.data[X.indptr[2]] = 0.0  # (stays stored)
    return X


def random_start(n_items, H, L, Hd, seed, moments=True):
    """float32 tables at their initial scale, biases and moments that are not zero, three updates done"""
    rng = np.random.RandomState(seed)
    state = R.initial_state(n_items, H, L, Hd, rng, np.float32)
    for n in TABLES:
        if n.startswith("b"):
            state[n] = (0.1 * rng.standard_normal(state[n].shape)).astype(np.float32)
        if moments:
            state["m" + n] = (1e-3 * rng.standard_normal(state[n].shape)).astype(np.float32)
            state["v" + n] = (1e-5 * rng.random_sample(state[n].shape)).astype(np.float32)
    state["n_updates"] = 3 if moments else 0
    return state


MIN_ACTIVATION = 3e-3


def least_activation(start, X, users, keep, eps, p):
    """the smallest norm over the batch of a column of h1, z or h2 in the float64 forward pass"""
    f = R.forward(start, np.asarray(X[users].todense()), R.dense_keep(X, users, keep), eps, p)
    return min(float(np.linalg.norm(f[k], axis=0).min()) for k in ("h1", "z", "h2"))


def conditioned_start(X, users, keep, eps, p, n_items, H, L, Hd, seed):
    """``random_start`` at the first seed (``seed``, ``seed + 1000``, ...) whose float64 forward pass has no column
    of h1, z or h2 of norm below ``MIN_ACTIVATION`` over the batch.  Such a column multiplies a whole row of a weight
    gradient (with one batch row: dW4[j] = h2[j] g), and a float32 activation is known to 2^-24 of its inputs'
    magnitude (about 1) however it was summed - so the row is relatively off by about 1e-7 / |activation| in ANY
    float32 implementation, the restatement's included, and which of two is nearer to float64 there is chance.
    3e-3 keeps that a third of the bar's 1e-4.  The rule looks at the float64 restatement alone."""
    x, dense = np.asarray(X[users].todense()), R.dense_keep(X, users, keep)
    for attempt in range(200):
        start = random_start(n_items, H, L, Hd, seed + 1000 * attempt)
        f = R.forward(start, x, dense, eps, p)
        if min(float(np.linalg.norm(f[k], axis=0).min()) for k in ("h1", "z", "h2")) >= MIN_ACTIVATION:
            return start
    raise AssertionError("no well-conditioned start found")


def explicit_noise(X, users, L, p, seed, drop_row=None):
    rng = np.random.default_rng(seed)
    deg = np.diff(X.indptr)[users]
    keep = (rng.random(int(deg.sum())) >= p).astype(np.uint8) if p > 0 else np.ones(int(deg.sum()), np.uint8)
    if drop_row is not None and p > 0:
        at = int(deg[:drop_row].sum())
        keep[at:at + deg[drop_row]] = 0
    return keep, rng.standard_normal((len(users), L)).astype(np.float32)


# ---- the case tables ------------------------------------------------------------------------------------------------
def update_cases(dh2_slab, dw4_slab):
    """a covering selection of (I, H, Hd, L, n, dropout_p, klc): every value of every axis the issue names, the item
    counts with the ragged fourth dh2 slab and the batch with two dW4 slabs and a remainder from the slab sizes"""
    i_big, n_big = 3 * dh2_slab + 37, 2 * dw4_slab + 9
    return [
        (70, 1, 1, 1, 1, 0.0, 0.0), (70, 5, 33, 3, 7, 0.5, 0.2), (70, 33, 5, 16, 100, 0.5, 0.0),
        (70, 64, 130, 65, 7, 0.0, 0.2), (70, 130, 64, 1, 100, 0.5, 0.2), (70, 130, 1, 65, 100, 0.0, 0.2),
        (70, 64, 64, 3, 1, 0.5, 0.2), (257, 1, 5, 3, 100, 0.5, 0.2), (257, 5, 1, 16, 1, 0.5, 0.0),
        (257, 33, 64, 65, 7, 0.5, 0.2), (257, 64, 33, 1, 100, 0.0, 0.0), (257, 130, 130, 16, 100, 0.5, 0.2),
        (257, 1, 130, 3, 7, 0.0, 0.2), (257, 64, 64, 16, n_big, 0.5, 0.2), (257, 5, 130, 1, n_big, 0.0, 0.0),
        (i_big, 33, 130, 3, 7, 0.5, 0.2), (i_big, 64, 64, 16, 100, 0.0, 0.2), (i_big, 5, 5, 1, n_big, 0.5, 0.0),
        (i_big, 130, 33, 65, 1, 0.5, 0.2), (i_big, 1, 64, 16, 100, 0.5, 0.2),
    ]


def wide_cases(dh2_slab, dw4_slab):
    """(I, H, Hd, L, n, dropout_p, klc) past the widths, the slab counts and the exact edges of ``update_cases``:
    every pass count of the two sparse kernels (Hp = 256 | 260, 512 | 516, 576), the latent kernel's second pass
    (L = 256 | 257), 2 L of five column tiles, Hd of five row tiles, n and I at a slab, a tile or a BK step and one
    past, the 64 dh2 slabs there can be at most and the first doubled slab.  No case has fewer than 7 rows: with one
    row and 574 columns no start passes ``conditioned_start``."""
    return [
        (70, 256, 5, 3, 7, 0.5, 0.2), (70, 257, 5, 16, 7, 0.5, 0.2), (257, 300, 574, 16, 7, 0.5, 0.2),
        (70, 512, 513, 256, 16, 0.0, 0.2), (257, 513, 257, 257, 100, 0.5, 0.2), (70, 574, 574, 300, 7, 0.5, 0.2),
        (129, 33, 64, 16, dw4_slab, 0.5, 0.2), (128, 64, 33, 3, dw4_slab + 1, 0.5, 0.0),
        (dh2_slab, 5, 130, 16, 17, 0.5, 0.2), (dh2_slab + 1, 130, 5, 65, 2 * dw4_slab, 0.0, 0.2),
        (64 * dh2_slab, 5, 33, 3, 7, 0.5, 0.2), (64 * dh2_slab + 1, 33, 5, 3, 7, 0.5, 0.2),
    ]


# (dh2 slabs, items in the last; dW4 slabs, rows in the last) of every wide case, as the issue's table claims them
WIDE_SLABS = [(1, 70, 1, 7), (1, 70, 1, 7), (1, 257, 1, 7), (1, 70, 1, 16), (1, 257, 1, 100), (1, 70, 1, 7),
              (1, 129, 1, 256), (1, 128, 2, 1), (1, 512, 1, 17), (2, 1, 2, 256), (64, 512, 1, 7), (33, 1, 1, 7)]


def slab_counts(n_items, n):
    slab = dh2_slab(n_items)
    a, b = -(-n_items // slab), -(-n // DW4_SLAB)
    return a, n_items - (a - 1) * slab, b, n - (b - 1) * DW4_SLAB


CONTRIB_CAP = 256.0  # (multvae_host_prep.hpp: a contribution to the fixed-point sums of [W1; b1] stays below it)
# The multinomial gradient of a row is S (softmax - x / S) / n with S the sum of its values, and its part along the
# logits' own directions does not average out over the items: with the full row of ``batch_matrix`` at 32768 items
# (S = 38000) in a batch of 7, max |da1| of the float64 restatement is 200 .. 550 whatever the seeds (six tried for
# each of the two cases), at and past the cap - the device reports such a step as diverged, as it should.  The
# gradient is linear in the values and the forward pass normalises them away, so the two cases take the same matrix
# with its values times 2^-3: the same entries, rows and kernel paths, contributions of 25 .. 70.
WIDE_VALUE_SCALE = {10: 2.0 ** -3, 11: 2.0 ** -3}


def largest_contribution(start, X, users, keep, eps, p, klc):
    """the largest |xd[r, i] da1[r, h]| and |da1[r, h]| (the bias row) of the float64 restatement: what
    ``mv_dw1_kernel`` adds to the fixed-point sums, and raises the divergence flag for at ``CONTRIB_CAP``"""
    f = R.gradients(start, np.asarray(X[users].todense()), R.dense_keep(X, users, keep), eps, p, klc)[1]
    return float((np.abs(f["da1"]).max(axis=1) * np.maximum(1.0, f["xd"].max(axis=1))).max())


def case_inputs(shape, case, wide):
    """``(X, users, keep, eps, start)`` of one single-update case: the batch, its order, its noise (the first row
    with entries dropped out whole) and its conditioned start, from the case's number alone"""
    I, H, Hd, L, n, p, klc = shape
    matrix, order, start = (500 + case, 100 + case, 700 + case) if wide else (100 + case, case, 200 + case)
    X = batch_matrix(n, I, matrix)
    if wide and case in WIDE_VALUE_SCALE:
        X.data *= np.float32(WIDE_VALUE_SCALE[case])
    users = np.random.default_rng(order).permutation(n).astype(np.int32)
    drop = int(np.argmax(np.diff(X.indptr)[users] > 0)) if n >= 3 else None
    keep, eps = explicit_noise(X, users, L, p, order, drop_row=drop)
    return X, users, keep, eps, conditioned_start(X, users, keep, eps, p, I, H, L, Hd, start)


# ---- a small batch after a larger one ---------------------------------------------------------------------------------
REGROW = dict(I=257, H=33, Hd=64, L=16, p=0.5, klc=0.2, rows=300, first_capacity=8)


def regrowth_inputs():
    """the 300-row matrix and two batches of it, each ``(users, keep, eps, start)``: all 300 rows (two dW4 slabs and
    44 rows) and then 5 rows, the empty and the full one among them"""
    c = REGROW
    X = batch_matrix(c["rows"], c["I"], 31)
    assert X.indptr[1] == 0 and X.indptr[2] - X.indptr[1] == c["I"] - 1
    batches = []
    for users, seed in ((np.random.default_rng(32).permutation(c["rows"]).astype(np.int32), 33),
                        (np.array([17, 0, 250, 1, 99], dtype=np.int32), 35)):
        keep, eps = explicit_noise(X, users, c["L"], c["p"], seed)
        batches.append((users, keep, eps, conditioned_start(X, users, keep, eps, c["p"], c["I"], c["H"], c["L"], c["Hd"], seed + 1)))
    return X, batches


# ---- scoring in ragged chunks -------------------------------------------------------------------------------------
SCORING = dict(I=257, H=33, Hd=64, L=16, users=40, capacity=8, rows=21, empty=(0, 8, 20), full=7)


def ragged_cold_rows():
    """21 rows for a capacity of 8 (chunks of 8, 8 and 5) at density 0.06 with values in {1, 2}: rows 0, 8 (the first
    of the second chunk) and 20 (the last) are empty, row 7 (the last of the first chunk) holds every item"""
    c = SCORING
    rng = np.random.default_rng(41)
    D = (rng.random((c["rows"], c["I"])) < 0.06) * rng.choice([1.0, 2.0], (c["rows"], c["I"]))
    D[list(c["empty"])] = 0
    D[c["full"]] = rng.choice([1.0, 2.0], c["I"])
    return sps.csr_matrix(D.astype(np.float32))


def log_sum_exp(logit):
    mx = logit.max(axis=1)
    return mx + np.log(np.exp(logit - mx[:, None]).sum(axis=1, dtype=logit.dtype))


# ---- the divergence flag ------------------------------------------------------------------------------------------
DIVERGENCE = dict(I=70, H=33, Hd=33, L=3, p=0.0, klc=0.0, cap=256.0)


def divergence_inputs():
    """One batch row at p = 0 and klc = 0: xd <= 1, so the largest contribution to the fixed-point sums of W1 is
    max |db1| = max |da1|, ``m`` at the unscaled values; the gradient is linear in the stored values (the forward
    pass normalises them away), so the row times ``a_lo`` has it in (64, 128] and times ``a_hi`` in [512, 1024),
    a factor of two on either side of the cap.  ``X`` holds the two scaled rows: user 0 legal, user 1 diverging."""
    c = DIVERGENCE
    row = batch_matrix(1, c["I"], 51)
    users = np.zeros(1, dtype=np.int32)
    keep, eps = explicit_noise(row, users, c["L"], c["p"], 52)
    start = conditioned_start(row, users, keep, eps, c["p"], c["I"], c["H"], c["L"], c["Hd"], 53)
    g64 = R.gradients(start, np.asarray(row.todense()), R.dense_keep(row, users, keep), eps, c["p"], c["klc"])[0]
    m = float(np.abs(g64["b1"]).max())
    a_lo = 2.0 ** np.floor(np.log2(0.5 * c["cap"] / m))
    a_hi = 2.0 ** np.ceil(np.log2(2.0 * c["cap"] / m))
    X = sps.vstack([row * np.float32(a_lo), row * np.float32(a_hi)]).tocsr().astype(np.float32)
    return dict(row=row, X=X, keep=keep, eps=eps, start=start, m=m, a_lo=a_lo, a_hi=a_hi)
