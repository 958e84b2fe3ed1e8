"""The inputs of the WARP GPU tests (``tests/test_gpu_warp.py``), built without a device so that the surface test can
check on the CPU what they promise: margins away from zero in the float64 restatement, and a search that ends at
``t = 1``, later, and not at all in fair shares - a state in which everything violates at once does not test it."""
import numpy as np
import scipy.sparse as sps

from _warp_restatement import warp_search

N_USERS, N_ITEMS = 50, 37
K_LIST = [1, 5, 64, 65, 128, 130, 256, 512]
MAX_SAMPLED_LIST = [1, 3, 10]
ALPHAS = [0.0, 0.1]
LR = 2.0 ** -7  # (a float32 value; the weights reach ln 36 = 3.6 and one row collects hundreds of them)
# (search and step_candidates do not look at the matrix: every row full, an epoch of no positions)
X_ANY = sps.csr_matrix(np.ones((N_USERS, N_ITEMS), dtype=np.float32))


def random_state(k, seed, n_users=N_USERS, n_items=N_ITEMS):
    """float32 tables whose scores ``U V^T + b`` have a standard deviation near 4 at every K (the margin of 1 is then
    a fraction of the spread: some positives are beaten at once, some after a few tries, some never), accumulators in
    [1, 4]"""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    sigma = (16.0 / k) ** 0.25
    return dict(U=(sigma * rng.standard_normal((n_users, k))).astype(f32),
                V=(sigma * rng.standard_normal((n_items, k))).astype(f32),
                b=rng.standard_normal(n_items).astype(f32), GU=rng.uniform(1, 4, (n_users, k)).astype(f32),
                GV=rng.uniform(1, 4, (n_items, k)).astype(f32), Gb=rng.uniform(1, 4, n_items).astype(f32), epoch=0)


def search_batch():
    """1,000 positions with 10 candidates each; the first 20 have one candidate repeated (a user with one unseen
    item).  Fewer candidates are the leading columns, smaller batches the leading rows."""
    rng = np.random.default_rng(17)
    users, pos = rng.integers(0, N_USERS, 1000), rng.integers(0, N_ITEMS, 1000)
    cand = rng.integers(0, N_ITEMS, (1000, 10))
    cand[:20] = cand[:20, :1]
    return users.astype(np.int32), pos.astype(np.int32), cand.astype(np.int32)


SEARCH_SIZES = [1, 63, 64, 65, 1000]


def step_cases(k):
    """name -> (start state, list of batches (users, pos, cand) run in a row from it), 10 candidates each"""
    rng = np.random.default_rng(5)

    def rand(n):
        u, i, c = rng.integers(0, N_USERS, n), rng.integers(0, N_ITEMS, n), rng.integers(0, N_ITEMS, (n, 10))
        c = np.where(c == i[:, None], (c + 1) % N_ITEMS, c)  # (a candidate is unseen, so never the position's positive)
        return u.astype(np.int32), i.astype(np.int32), c.astype(np.int32)

    out = {}
    seed = [1000 * k]

    def add(name, runs, state=None):
        seed[0] += 1
        out[name] = (random_state(k, seed[0]) if state is None else state, runs)

    def one_that_violates(state):  # (a position that finds a violation, or the case would touch nothing)
        for _ in range(100):
            u, i, c = rand(1)
            if warp_search(state, u, i, c)[0][0] >= 0:
                return u, i, c
        raise AssertionError("no position with a violation")

    state = random_state(k, seed[0] + 1)
    add("random 1", [one_that_violates(state)], state)
    for n in (63, 64, 65, 1000):
        add(f"random {n}", [rand(n)])
    u, i, c = rand(200)
    add("one user in every position", [(np.full(200, 7, np.int32), i, c)])
    u, i, c = rand(120)
    i[:60] = 11
    c[:60][c[:60] == 11] = 12
    c[60:] = 11  # item 11: the positive of 60 positions and the only candidate of 60 others
    i[60:][i[60:] == 11] = 12
    add("one item as positive and as the only candidate", [(u, i, c)])
    state = random_state(k, seed[0] + 1)
    u, i, c = one_that_violates(state)
    add("identical positions", [(np.repeat(u, 300), np.repeat(i, 300), np.repeat(c, 300, axis=0))], state)
    add("three batches in a row", [rand(65), rand(257), rand(9)])
    # no position finds a violation: item 3 scores 100 above the rest and is every position's positive
    state = random_state(k, seed[0] + 1)
    state["b"][3] = 100.0
    u, i, c = rand(130)
    c[c == 3] = 4
    add("no violation", [(u, np.full(130, 3, np.int32), c)], state)
    return out


def five_item_case(k):
    """``n_items = 5``, ``max_sampled = 10``: the weights are ln 4, ln 2, 0, 0, ...  Item 0 (bias 50) is every
    position's positive, items 1 and 2 its first two candidates (no violation), item 4 (bias 120) the rest: every
    position finds its violation at ``t = 3`` with weight 0."""
    state = random_state(k, 77 + k, n_items=5)
    state["b"][0], state["b"][4] = 50.0, 120.0
    rng = np.random.default_rng(9)
    users = rng.integers(0, N_USERS, 90).astype(np.int32)
    cand = np.full((90, 10), 4, dtype=np.int32)
    cand[:, 0], cand[:, 1] = 1, 2
    return state, (users, np.zeros(90, np.int32), cand)


def many_item_case():
    """``n_items = 30,000``, 8 users, K = 4: ``ln 29,999 = 10.31`` is capped at 10.  Every position's first candidate
    violates (the positive's bias is -100)."""
    n_items = 30000
    state = random_state(4, 31, n_users=8, n_items=n_items)
    rng = np.random.default_rng(3)
    users, pos = rng.integers(0, 8, 40).astype(np.int32), rng.integers(0, 100, 40).astype(np.int32)
    state["b"][:100] = -100.0
    cand = rng.integers(100, n_items, (40, 10)).astype(np.int32)
    return state, (users, pos, cand)
