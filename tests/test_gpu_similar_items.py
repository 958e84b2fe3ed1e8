"""GPU tests of the neighbour calls: ``irs_serve_neighbors`` through ``DeviceRecommender.similar_items`` /
``similar_users``, the bare C entry, and the ``ItemIDMapper`` / ``IDMapper`` methods.

Similarity servers (metric ``weight``, float64 score block): the expected lists are a Python restatement of the
ranking rule (candidates in list order - all entities in index order without a list -, best first, equal scores in
candidate order, stop at -inf, scores narrowed to float32) applied to the row of ``W`` taken from scipy / numpy:
-inf everywhere, then the row's STORED entries (stored zeros included), then -inf for the entity itself and the
forbidden ones.  Equality is exact: the same indices in the same order, the same float32 scores.

Factor servers (float32 MFMA tiles), against float64 over the leading ``k_used`` columns of the float32 table
(``|x|`` is the vector of absolute values, ``n_x`` the float64 norm):

  dot      ``|s - v_q.v_j| <= k_used * 2**-23 * |v_q|.|v_j|`` - the project's bound for a float32 dot product of
           that length in any order (``gamma_k ~ k * 2**-24``, a factor of two over it);
  cosine   ``|s - v_q.v_j / (n_q n_j)| <= (k_used + 4) * 2**-23 * |v_q|.|v_j| / (n_q n_j)`` - the same sum over the
           scaled query, and four more roundings of ``2**-24`` each (the two inverse norms, computed in double and
           rounded once, and the two scalings): ``2 * 2**-23``, doubled for the second-order terms.

Every row is checked as ``check_factor_rows`` of test_gpu_serving.py checks a recommend row (restated here): nothing
excluded, only allowed candidates, no repeats, the length ``min(cutoff, live candidates)``, scores that do not
increase, every listed score within its bound, and no live candidate left out whose float64 score exceeds the last
listed score by more than its bound.  A row of zeros has no direction: under ``cosine`` it is never a candidate and
its own list is empty.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps

from irspack_amd import _lib, serving
from irspack_amd.serving import DeviceRecommender
from irspack_amd.utils import IDMapper

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS = 300, 257
WEIGHT, COSINE, DOT = 0, 1, 2
ZERO, TWIN_A, TWIN_B, TINY, HUGE = 3, 5, 7, 11, 13  # the special rows of make_table


# ---- the ranking rule, restated -------------------------------------------------------------------------------

def restated(score, allowed, cutoff):
    rows, n = score.shape
    out = []
    for r in range(rows):
        if len(allowed) == 0:
            cand = list(range(n))
        else:
            lst = allowed[0] if len(allowed) == 1 else allowed[r]
            cand = [int(i) for i in lst if 0 <= i < n]
        pairs = sorted(((i, score[r, i]) for i in cand), key=lambda t: -t[1])  # stable: ties in candidate order
        res = []
        for i, s in pairs[:cutoff]:
            if s == -np.inf:
                break
            res.append((int(i), float(np.float32(s))))
        out.append(res)
    return out


def as_lists(idx, score, length):
    assert idx.dtype == np.int32 and score.dtype == np.float32 and length.dtype == np.int32
    assert idx.shape == score.shape and length.shape == (idx.shape[0],)
    for r in range(idx.shape[0]):  # the padding
        assert (idx[r, length[r]:] == -1).all() and (idx[r, :length[r]] >= 0).all()
        assert (score[r, length[r]:] == 0).all()
    return [[(int(i), float(s)) for i, s in zip(idx[r, :length[r]], score[r, :length[r]])]
            for r in range(idx.shape[0])]


def weight_scores(W, ids, forbidden=None):
    """the float64 score block of a ``weight`` call: rows ``ids`` of ``W`` (scipy CSR: stored entries only; ndarray:
    the whole row), self and forbidden at -inf"""
    ids = np.asarray(ids)
    n = W.shape[1]
    S = np.full((ids.size, n), -np.inf)
    for r, q in enumerate(ids):
        if sps.issparse(W):
            lo, hi = W.indptr[q], W.indptr[q + 1]
            S[r, W.indices[lo:hi]] = W.data[lo:hi]
        else:
            S[r] = W[q]
        S[r, q] = -np.inf
        if forbidden is not None:
            S[r, list(forbidden[r])] = -np.inf
    return S


def stored(W, q):
    return set(W.indices[W.indptr[q]:W.indptr[q + 1]].tolist())


# ---- factor rows against float64 --------------------------------------------------------------------------------

def check_neighbour_rows(T, ids, k_used, metric, cutoff, idx, score, length, excluded=None, allowed=()):
    """every row of a factor neighbour result against float64 over ``T[:, :k_used]`` (the bounds of the module
    docstring); ``excluded``: one set per row beside the entity itself"""
    ids = np.asarray(ids)
    V = T[:, :k_used].astype(np.float64)
    Q = V[ids]
    s64 = Q @ V.T
    A = np.abs(Q) @ np.abs(V).T
    n = V.shape[0]
    dead = np.zeros(n, dtype=bool)
    if metric == "cosine":
        norm = np.sqrt((V * V).sum(axis=1))
        dead = norm == 0.0
        safe = np.where(dead, 1.0, norm)
        s64 = s64 / (safe[ids][:, None] * safe[None, :])
        B = (k_used + 4) * 2.0 ** -23 * A / (safe[ids][:, None] * safe[None, :])
    else:
        B = k_used * 2.0 ** -23 * A
    got = as_lists(idx, score, length)
    assert len(got) == ids.size
    for r, row in enumerate(got):
        if len(allowed) == 0:
            cand = list(range(n))
        else:
            cand = [int(i) for i in (allowed[0] if len(allowed) == 1 else allowed[r]) if 0 <= i < n]
        out = {int(ids[r])} | set(np.flatnonzero(dead).tolist()) | (set(excluded[r]) if excluded is not None else set())
        if dead[ids[r]]:
            out = set(range(n))  # a query without direction: nothing is listed
        live = [i for i in cand if i not in out]
        items = [i for i, _ in row]
        assert not set(items) & out, r
        assert set(items) <= set(cand), r
        if len(set(cand)) == len(cand):
            assert len(set(items)) == len(items), r
        assert len(items) == min(cutoff, len(live)), (r, len(items), len(live))
        scores = np.array([s for _, s in row], dtype=np.float64)
        assert (np.diff(scores) <= 0).all(), r
        for i, s in row:
            assert abs(s - s64[r, i]) <= B[r, i], (r, i, s, s64[r, i], B[r, i])
        if row and len(items) < len(live):
            last = scores[-1]
            for i in set(live) - set(items):
                assert s64[r, i] <= last + B[r, i], (r, i, s64[r, i], last, B[r, i])
    return got


def make_table(n, k, seed):
    """float32 [n, k] with a row of zeros, two identical rows, a row scaled by 1e-20 and one scaled by 1e19 (the
    float32 sum of its squares overflows from k = 4 on: its norm must be taken in double)"""
    rng = np.random.default_rng(seed)
    T = rng.standard_normal((n, k)).astype(np.float32)
    T[ZERO] = 0.0
    T[TWIN_B] = T[TWIN_A]
    T[TINY] *= np.float32(1e-20)
    T[HUGE] *= np.float32(1e19)
    assert np.isfinite(T).all() and (T[TINY] != 0).any()
    return T


def hand_factor_model(users, items):
    """an NMF recommender with hand-made tables: ``users`` [n_users, k], ``items`` [n_items, k]"""
    from irspack_amd.recommenders.nmf import NMFRecommender

    model = NMFRecommender(sps.csr_matrix((users.shape[0], items.shape[0]), dtype=np.float64),
                           n_components=items.shape[1])
    model.W = np.ascontiguousarray(users, dtype=np.float32)
    model.H = np.ascontiguousarray(items.T, dtype=np.float32)
    return model


def queries(n):
    if n <= 70:
        return np.arange(n)
    return np.array([0, ZERO, TWIN_A, TWIN_B, TINY, HUGE, 1, 63, 64, 65, n // 2, n - 2, n - 1, TWIN_A, 0])


def check_twins(got, ids):
    """the two identical rows score the same bits and come in candidate (index) order"""
    for r, row in enumerate(got):
        if ids[r] in (TWIN_A, TWIN_B):
            continue
        at = {i: p for p, (i, _) in enumerate(row)}
        if TWIN_A in at and TWIN_B in at:
            assert row[at[TWIN_A]][1] == row[at[TWIN_B]][1], r
            assert at[TWIN_A] < at[TWIN_B], r


# ---- 1. factor servers against float64 --------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 5, 33, 64, 576])
@pytest.mark.parametrize("n", [70, 257, 1000])
def test_factor_neighbours_within_the_derived_bounds(n, k):
    T = make_table(n, k, seed=100 * k + n)
    dev = DeviceRecommender(hand_factor_model(T[:4], T))
    ids = queries(n)
    for metric in ("cosine", "dot"):
        for cutoff in (7, n):
            out = dev.similar_items_arrays(ids, cutoff, metric=metric)
            got = check_neighbour_rows(T, ids, k, metric, cutoff, *out)
            check_twins(got, ids)
            if metric == "cosine":
                zero_rows = [r for r, q in enumerate(ids) if q == ZERO]
                assert zero_rows and all(got[r] == [] for r in zero_rows)
                assert all(ZERO not in [i for i, _ in row] for row in got)
    # (the default metric of a factor model is the cosine)
    assert dev.similar_items(ids[:5], 7) == dev.similar_items(ids[:5], 7, metric="cosine")
    dev.close()


# ---- bare C entry -------------------------------------------------------------------------------------------------

def neighbours_c(h, n, ids, metric, k_used, cutoff, excl=None, lists=()):
    """``irs_serve_neighbors`` as it stands: (status, idx, score, length)"""
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    rows, width = ids.size, max(min(cutoff, n), 0)
    idx, sc = np.full((rows, width), -1, dtype=np.int32), np.zeros((rows, width), dtype=np.float32)
    ln = np.zeros(rows, dtype=np.int32)
    lptr = np.zeros(len(lists) + 1, dtype=np.int64)
    for i, l in enumerate(lists):
        lptr[i + 1] = lptr[i] + len(l)
    litems = np.array([i for l in lists for i in l] + [0], dtype=np.int64)
    ep = ei = None
    if excl is not None:
        ep = np.concatenate([[0], np.cumsum([len(e) for e in excl])]).astype(np.int64)
        ei = np.array([i for e in excl for i in e] + [0], dtype=np.int32)
    ptr = _lib.ptr
    status = _lib.lib().irs_serve_neighbors(
        h, C.c_int64(rows), ptr(ids, C.c_int64), C.c_int32(metric), C.c_int32(k_used),
        ptr(ep, C.c_int64) if ep is not None else None, ptr(ei, C.c_int32) if ei is not None else None,
        C.c_int64(len(lists)), ptr(lptr, C.c_int64), ptr(litems, C.c_int64), C.c_int64(cutoff), ptr(idx, C.c_int32),
        ptr(sc, C.c_float), ptr(ln, C.c_int32))
    return status, idx, sc, ln


class Server:
    """a bare ``irs_server`` made through the C constructors"""

    def __init__(self, table=None, csr=None, shape=None):
        self.h = C.c_void_p()
        dev, ptr = C.c_int32(_lib.default_device()), _lib.ptr
        if table is not None:
            table = np.ascontiguousarray(table, dtype=np.float32)
            _lib.check(_lib.lib().irs_serve_create_factors(
                C.c_int64(table.shape[0]), C.c_int32(table.shape[1]), ptr(table, C.c_float), dev, C.byref(self.h)))
        else:
            indptr, indices, data = csr
            self.keep = (np.ascontiguousarray(indptr, dtype=np.int64), np.ascontiguousarray(indices, dtype=np.int32),
                         np.ascontiguousarray(data, dtype=np.float64))
            _lib.check(_lib.lib().irs_serve_create_similarity(
                C.c_int64(shape[0]), C.c_int64(shape[1]), ptr(self.keep[0], C.c_int64), ptr(self.keep[1], C.c_int32),
                ptr(self.keep[2], C.c_double), dev, C.byref(self.h)))

    def close(self):
        h, self.h = self.h, C.c_void_p()
        if h.value:
            _lib.lib().irs_serve_destroy(h)


# ---- 2. k_used < k ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width", [65, 34])  # [V | b]: 64 + 1 columns (KP 96 against 64) and 33 + 1 (KP 64 both)
def test_leading_columns_only(width):
    n = 257
    T = make_table(n, width, seed=width)
    T[:, -1] = np.float32(50.0) * np.random.default_rng(1).standard_normal(n).astype(np.float32)  # a bias-like column
    T[ZERO, -1] = 7.0  # (the embedding of the zero row is still zero)
    ids = queries(n)
    with_bias, without = Server(table=T), Server(table=T[:, :width - 1])
    for code, metric in ((COSINE, "cosine"), (DOT, "dot"), (COSINE, "cosine")):
        status, *out = neighbours_c(with_bias.h, n, ids, code, width - 1, 20)
        assert status == 0
        got = check_neighbour_rows(T, ids, width - 1, metric, 20, *out)
        status, *ref = neighbours_c(without.h, n, ids, code, width - 1, 20)
        assert status == 0
        check_neighbour_rows(T[:, :width - 1], ids, width - 1, metric, 20, *ref)
        if metric == "cosine":
            assert got[list(ids).index(ZERO)] == []
    # the whole table is another answer, and the inverse norms follow k_used from call to call
    status, *full = neighbours_c(with_bias.h, n, ids, COSINE, width, 20)
    assert status == 0
    check_neighbour_rows(T, ids, width, "cosine", 20, *full)
    status, *again = neighbours_c(with_bias.h, n, ids, COSINE, width - 1, 20)
    assert status == 0
    check_neighbour_rows(T, ids, width - 1, "cosine", 20, *again)
    with_bias.close()
    without.close()


# ---- 3. sparse W, exact -------------------------------------------------------------------------------------------

def hand_csr(n, seed):
    """CSR rows in shuffled column order with negative weights, ties and stored zeros; row 2 is empty, row 4 stores
    only itself, row 6 stores every column"""
    rng = np.random.default_rng(seed)
    indptr, indices, data = [0], [], []
    for r in range(n):
        count = {2: 0, 4: 1, 6: n}.get(r, int(rng.integers(1, min(n, 40))))
        cols = rng.choice(n, size=count, replace=False)
        if r == 4:
            cols = np.array([4])
        indices += cols.tolist()
        data += rng.choice([-2.0, -0.5, 0.0, 0.25, 0.5, 1.0, 3.0], size=count).tolist()
        indptr.append(len(indices))
    W = sps.csr_matrix((np.array(data), np.array(indices, dtype=np.int32), np.array(indptr, dtype=np.int32)), shape=(n, n))
    assert not W.has_sorted_indices or n < 3
    return W


@pytest.mark.parametrize("n", [70, 257, 1031])
def test_sparse_rows_by_hand_are_exact(n):
    W = hand_csr(n, seed=n)
    assert (W.data == 0).any() and (W.data < 0).any()
    srv = Server(csr=(W.indptr, W.indices, W.data), shape=(n, n))
    ids = np.arange(n) if n <= 70 else np.array([0, 2, 4, 6, 1, n - 1, 6, n // 2, 63, 64, 65])
    for cutoff in (1, 7, 65, n):
        status, *out = neighbours_c(srv.h, n, ids, WEIGHT, 0, cutoff)
        assert status == 0
        got = as_lists(*out)
        assert got == restated(weight_scores(W, ids), [], cutoff)
        for r, q in enumerate(ids):  # an item without a stored weight never appears; nor does the item itself
            assert {i for i, _ in got[r]} <= stored(W, q) - {int(q)}
    assert got[list(ids).index(2)] == [] and got[list(ids).index(4)] == []
    assert len(got[list(ids).index(6)]) == n - 1  # (stored zeros and negative weights are listed)
    srv.close()


@pytest.fixture(scope="module")
def X():
    rng = np.random.default_rng(11)
    D = (rng.random((N_USERS, N_ITEMS)) < 0.05).astype(np.float64)
    D[0] = 0.0
    return sps.csr_matrix(D)


@pytest.fixture(scope="module")
def sim_models(X):
    from irspack_amd.recommenders.dense_slim import DenseSLIMRecommender
    from irspack_amd.recommenders.knn import CosineKNNRecommender
    from irspack_amd.recommenders.slim import SLIMRecommender
    from irspack_amd.recommenders.user_knn import CosineUserKNNRecommender

    return {
        "item_knn": CosineKNNRecommender(X, top_k=5).learn(),
        "slim": SLIMRecommender(X, alpha=0.01, l1_ratio=0.1, n_iter=10).learn(),
        "ease": DenseSLIMRecommender(X, reg=5.0).learn(),
        "user_knn": CosineUserKNNRecommender(X, top_k=5).learn(),
    }


@pytest.fixture(scope="module")
def sim_servers(sim_models):
    return {name: DeviceRecommender(m) for name, m in sim_models.items()}


def canonical(W):
    """what the Python layer uploads: float64 CSR with sorted rows (stored entries as the model has them)"""
    out = sps.csr_matrix(W, dtype=np.float64, copy=True)
    out.sort_indices()
    return out


ITEMS = np.array([0, 5, 17, 5, 256, 42, 42, 101, 250, 64, 65, 128, 255, 1])


@pytest.mark.parametrize("name", ["item_knn", "slim"])
def test_fitted_sparse_models_are_exact(sim_models, sim_servers, name):
    W = canonical(sim_models[name].W)
    dev = sim_servers[name]
    everything = np.arange(N_ITEMS)
    for ids, cutoff in ((everything, 20), (ITEMS, 1), (ITEMS, 300)):
        got = as_lists(*dev.similar_items_arrays(ids, cutoff))
        assert got == restated(weight_scores(W, ids), [], cutoff)
        for r, q in enumerate(ids):
            assert {i for i, _ in got[r]} <= stored(W, q) - {int(q)}
    assert dev.similar_items(ITEMS, 20, metric="weight") == dev.similar_items(ITEMS, 20)
    if name == "item_knn":  # top_k = 5: a row stores five weights at the most
        assert max(len(row) for row in dev.similar_items(everything, 20)) <= 5


# ---- 4. dense W, exact --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [70, 257, 260])  # (260: rows of four columns per lane; the others: single elements)
def test_dense_rows_are_exact(n, dtype):
    from irspack_amd.recommenders.base import BaseSimilarityRecommender

    rng = np.random.default_rng(n)
    W = rng.choice([-1.5, 0.0, 0.25, 0.5, 1.0], size=(n, n)).astype(dtype)  # ties everywhere
    W += (rng.random((n, n)) < 0.2) * rng.standard_normal((n, n)).astype(dtype)
    model = BaseSimilarityRecommender(sps.csr_matrix((rng.random((9, n)) < 0.1).astype(np.float64)))
    model._W = np.ascontiguousarray(W)
    dev = DeviceRecommender(model)
    assert dev.kind == "dense_similarity"
    ids = np.arange(n) if n <= 70 else np.array([0, 1, 2, 3, 4, n - 1, n - 2, n - 3, n - 4, 128, 129, 130, 131, 64, 0])
    for cutoff in (7, n):
        got = as_lists(*dev.similar_items_arrays(ids, cutoff))
        assert got == restated(weight_scores(W.astype(np.float64), ids), [], cutoff)
        assert all(len(row) == min(cutoff, n - 1) for row in got)
    dev.close()


def test_fitted_ease_is_exact(sim_models, sim_servers):
    W = sim_models["ease"].W
    got = as_lists(*sim_servers["ease"].similar_items_arrays(ITEMS, 20))
    assert got == restated(weight_scores(np.asarray(W, dtype=np.float64), ITEMS), [], 20)


# ---- 5. lists and exclusions --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def factor_pair():
    """a hand-made pair of tables (k = 33): ``(model, users [300, 33], items [257, 33])``"""
    items = make_table(N_ITEMS, 33, seed=5)
    users = make_table(N_USERS, 33, seed=6)
    return hand_factor_model(users, items), users, items


@pytest.fixture(scope="module")
def factor_server(factor_pair):
    return DeviceRecommender(factor_pair[0])


def list_cases(ids, n, seed):
    rng = np.random.default_rng(seed)
    common = [5, 3, 3, n - 1, n, -1, 77, 0, 100, 101, 102, 3, 900, int(ids[0]), TWIN_B, TWIN_A]
    per = [[int(q)] + list(rng.integers(-3, n + 5, size=rng.integers(0, 60))) for q in ids]  # each names its query
    per[2] = []
    per[3] = [int(ids[3])]  # nothing but the query itself
    forbidden = [list(rng.integers(0, n, size=rng.integers(0, 20))) for _ in ids]
    forbidden[1] = list(range(n))
    return common, per, forbidden


def test_lists_and_exclusions_on_similarity_servers(sim_models, sim_servers):
    for name in ("item_knn", "ease"):
        W = sim_models[name].W
        W = canonical(W) if sps.issparse(W) else np.asarray(W, dtype=np.float64)
        dev = sim_servers[name]
        common, per, forbidden = list_cases(ITEMS, N_ITEMS, seed=3)
        for cutoff in (3, 65):
            got = as_lists(*dev.similar_items_arrays(ITEMS, cutoff, allowed=common, forbidden=forbidden))
            assert got == restated(weight_scores(W, ITEMS, forbidden), [common], cutoff)
            assert got[1] == []
            # (per-row lists take precedence over the common one)
            got = as_lists(*dev.similar_items_arrays(ITEMS, cutoff, allowed=common, per_item_allowed=per))
            assert got == restated(weight_scores(W, ITEMS), per, cutoff)
            assert got[2] == [] and got[3] == []
            assert all(int(q) not in [i for i, _ in row] for q, row in zip(ITEMS, got))


def test_lists_and_exclusions_on_a_factor_server(factor_pair, factor_server):
    _, _, T = factor_pair
    common, per, forbidden = list_cases(ITEMS, N_ITEMS, seed=4)
    for metric in ("cosine", "dot"):
        for cutoff in (3, 65):
            out = factor_server.similar_items_arrays(ITEMS, cutoff, allowed=common, forbidden=forbidden, metric=metric)
            got = check_neighbour_rows(T, ITEMS, 33, metric, cutoff, *out, excluded=[set(f) for f in forbidden],
                                       allowed=[common])
            assert got[1] == []
            out = factor_server.similar_items_arrays(ITEMS, cutoff, per_item_allowed=per, metric=metric)
            got = check_neighbour_rows(T, ITEMS, 33, metric, cutoff, *out, allowed=per)
            assert got[2] == [] and got[3] == []
    with pytest.raises(ValueError):
        factor_server.similar_items(ITEMS, 5, per_item_allowed=per[:-1])
    with pytest.raises(ValueError):
        factor_server.similar_items(ITEMS, 5, forbidden=forbidden[:-1])
    with pytest.raises(ValueError):
        factor_server.similar_items(ITEMS[:1], 5, forbidden=[[N_ITEMS]])


# ---- 6. chunking --------------------------------------------------------------------------------------------------

def test_three_chunks_equal_one(sim_servers, factor_server, monkeypatch):
    rng = np.random.default_rng(2)
    ids = rng.integers(0, N_ITEMS, size=600)  # (with repeats)
    per = [list(rng.integers(-2, N_ITEMS + 2, size=rng.integers(0, 30))) for _ in ids]
    forbidden = [list(rng.integers(0, N_ITEMS, size=rng.integers(0, 5))) for _ in ids]
    calls = [(sim_servers["item_knn"], {}), (sim_servers["slim"], dict(per_item_allowed=per, forbidden=forbidden)),
             (factor_server, dict(metric="cosine")), (factor_server, dict(metric="dot", forbidden=forbidden)),
             (factor_server, dict(metric="cosine", per_item_allowed=per))]
    monkeypatch.delenv("IRSPACK_AMD_SERVE_BLOCK", raising=False)
    whole = [dev.similar_items_arrays(ids, 7, **kw) for dev, kw in calls]
    monkeypatch.setenv("IRSPACK_AMD_SERVE_BLOCK", "256")  # (read per call): 256 + 256 + 88 rows
    for (dev, kw), want in zip(calls, whole):
        got = dev.similar_items_arrays(ids, 7, **kw)
        for a, b in zip(got, want):
            assert a.tobytes() == b.tobytes()
    assert (whole[0][2] > 0).any() and (whole[2][2] == 7).any()


# ---- 7. cutoff edges ----------------------------------------------------------------------------------------------

def test_cutoff_edges(sim_models, sim_servers, factor_pair, factor_server):
    _, _, T = factor_pair
    for dev in (sim_servers["item_knn"], sim_servers["ease"], factor_server):
        idx, sc, ln = dev.similar_items_arrays(ITEMS, 0)
        assert idx.shape == sc.shape == (ITEMS.size, 0) and (ln == 0).all()
        for cutoff in (0, 5):
            idx, sc, ln = dev.similar_items_arrays([], cutoff)
            assert idx.shape == sc.shape == (0, cutoff) and ln.shape == (0,)
        assert dev.similar_items([], 5) == []
        with pytest.raises(TypeError):
            dev.similar_items(ITEMS, -1)
    for cutoff in (N_ITEMS - 1, N_ITEMS, N_ITEMS + 50):
        out = factor_server.similar_items_arrays(ITEMS, cutoff, metric="dot")
        assert out[0].shape == (ITEMS.size, min(cutoff, N_ITEMS))
        check_neighbour_rows(T, ITEMS, 33, "dot", cutoff, *out)
        assert (out[2] == N_ITEMS - 1).all()  # everything but the item itself
        W = np.asarray(sim_models["ease"].W, dtype=np.float64)
        got = as_lists(*sim_servers["ease"].similar_items_arrays(ITEMS, cutoff))
        assert got == restated(weight_scores(W, ITEMS), [], cutoff)


def test_cutoff_above_2048():
    """2500 items, k = 5, cutoff 2400: the ranking keeps its lists in global scratch, the output stage walks 38 steps"""
    T = make_table(2500, 5, seed=9)
    dev = DeviceRecommender(hand_factor_model(T[:4], T))
    ids = np.array([0, 2499, ZERO, 1234])
    for metric in ("cosine", "dot"):
        out = dev.similar_items_arrays(ids, 2400, metric=metric)
        check_neighbour_rows(T, ids, 5, metric, 2400, *out)
        assert out[2][0] == 2400 and out[2][1] == 2400
    dev.close()


# ---- 8. determinism -----------------------------------------------------------------------------------------------

def test_two_calls_give_identical_arrays_between_recommend_calls(sim_servers, factor_server):
    users = np.array([5, 17, 5, 299, 0])
    for dev in (sim_servers["item_knn"], sim_servers["ease"], factor_server):
        before = dev.recommend_known_arrays(users, 65)
        a = dev.similar_items_arrays(ITEMS, 65)
        between = dev.recommend_known_arrays(users, 65)
        b = dev.similar_items_arrays(ITEMS, 65)
        after = dev.recommend_known_arrays(users, 65)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        for other in (between, after):
            for x, y in zip(before, other):
                assert x.tobytes() == y.tobytes()
    d1 = factor_server.similar_items_arrays(ITEMS, 20, metric="dot")
    c1 = factor_server.similar_items_arrays(ITEMS, 20, metric="cosine")
    d2 = factor_server.similar_items_arrays(ITEMS, 20, metric="dot")
    for x, y in zip(d1, d2):
        assert x.tobytes() == y.tobytes()
    assert c1[1].tobytes() != d1[1].tobytes()


# ---- 9. errors ----------------------------------------------------------------------------------------------------

def refused(status):
    assert status == 1
    with pytest.raises(ValueError) as err:
        _lib.check(status)
    assert str(err.value)


def test_argument_errors_leave_the_server_usable(sim_servers, factor_server):
    fh, sh, dh = factor_server._h, sim_servers["item_knn"]._h, sim_servers["ease"]._h
    good = np.array([1, 2, 3])

    def ok(h, metric, k_used):
        status, idx, sc, ln = neighbours_c(h, N_ITEMS, good, metric, k_used, 5)
        assert status == 0 and (ln > 0).any()

    for bad_ids in ([1, N_ITEMS, 3], [-1], [2 ** 40]):  # an id out of range
        refused(neighbours_c(fh, N_ITEMS, bad_ids, COSINE, 33, 5)[0])
        ok(fh, COSINE, 33)
        refused(neighbours_c(sh, N_ITEMS, bad_ids, WEIGHT, 0, 5)[0])
        ok(sh, WEIGHT, 0)
    for h, metric, k_used in ((fh, WEIGHT, 33), (fh, 3, 33), (fh, -1, 33), (sh, COSINE, 0), (sh, DOT, 0),
                              (dh, COSINE, 0), (dh, 7, 0)):  # a metric that does not fit the server
        refused(neighbours_c(h, N_ITEMS, good, metric, k_used, 5)[0])
    ok(fh, DOT, 33)
    ok(dh, WEIGHT, 0)
    for k_used in (0, -1, 34, 576):  # k_used outside 1 .. k on a factor server
        refused(neighbours_c(fh, N_ITEMS, good, COSINE, k_used, 5)[0])
        ok(fh, COSINE, 1)
    for h in (sh, dh):  # k_used on a similarity server
        refused(neighbours_c(h, N_ITEMS, good, WEIGHT, 1, 5)[0])
        ok(h, WEIGHT, 0)
    # a non-square sparse W: a fine server for recommend calls, none for neighbours
    W = sps.random(40, 50, density=0.2, format="csr", random_state=1)
    srv = Server(csr=(W.indptr, W.indices, W.data), shape=(40, 50))
    refused(neighbours_c(srv.h, 50, good, WEIGHT, 0, 5)[0])
    srv.close()
    # the Python layer: IndexError for an index, ValueError for a metric
    for dev in (factor_server, sim_servers["item_knn"]):
        with pytest.raises(IndexError):
            dev.similar_items([0, N_ITEMS], 5)
        with pytest.raises(IndexError):
            dev.similar_items([-1], 5)
        with pytest.raises(ValueError):
            dev.similar_items([0], 5, metric="euclid")
    with pytest.raises(ValueError):
        factor_server.similar_items([0], 5, metric="weight")
    with pytest.raises(ValueError):
        sim_servers["item_knn"].similar_items([0], 5, metric="cosine")
    with pytest.raises(ValueError):
        sim_servers["ease"].similar_items([0], 5, metric="dot")
    assert factor_server.similar_items([0], 5) and sim_servers["ease"].similar_items([0], 5)


# ---- 10. the user side --------------------------------------------------------------------------------------------

USERS = np.array([5, 0, ZERO, TWIN_A, TWIN_B, TINY, HUGE, 299, 5, 150])


def test_similar_users_of_a_factor_pair(factor_pair, factor_server):
    _, U, _ = factor_pair
    for metric in ("cosine", "dot"):
        for cutoff in (7, N_USERS):
            out = factor_server.similar_users_arrays(USERS, cutoff, metric=metric)
            assert out[0].shape == (USERS.size, min(cutoff, N_USERS))
            got = check_neighbour_rows(U, USERS, 33, metric, cutoff, *out)
            check_twins(got, USERS)
    rng = np.random.default_rng(12)
    per = [[int(u)] + list(rng.integers(-3, N_USERS + 5, size=rng.integers(0, 60))) for u in USERS]
    forbidden = [list(rng.integers(0, N_USERS, size=rng.integers(0, 20))) for _ in USERS]
    out = factor_server.similar_users_arrays(USERS, 9, per_user_allowed=per)
    check_neighbour_rows(U, USERS, 33, "cosine", 9, *out, allowed=per)
    out = factor_server.similar_users_arrays(USERS, 9, forbidden=forbidden, metric="dot")
    check_neighbour_rows(U, USERS, 33, "dot", 9, *out, excluded=[set(f) for f in forbidden])
    with pytest.raises(IndexError):
        factor_server.similar_users([N_USERS], 5)
    # the item side of the same recommender is untouched by the second handle
    assert factor_server.similar_items(ITEMS, 5) == factor_server.similar_items(ITEMS, 5)


def test_similar_users_of_a_fitted_user_knn(sim_models, sim_servers):
    model, dev = sim_models["user_knn"], sim_servers["user_knn"]
    U = canonical(model.U)
    users = np.array([5, 0, 17, 5, 299, 42, 150])
    for cutoff in (1, 20):
        got = as_lists(*dev.similar_users_arrays(users, cutoff))
        assert got == restated(weight_scores(U, users), [], cutoff)
        for r, q in enumerate(users):
            assert {i for i, _ in got[r]} <= stored(U, q) - {int(q)}
    assert any(got)
    with pytest.raises(ValueError):
        dev.similar_users(users, 5, metric="cosine")


def test_sides_that_do_not_exist(sim_servers):
    with pytest.raises(NotImplementedError):
        sim_servers["user_knn"].similar_items([0], 5)
    for name in ("item_knn", "slim", "ease"):
        with pytest.raises(NotImplementedError):
            sim_servers[name].similar_users([0], 5)


# ---- 11. fitted factor models -------------------------------------------------------------------------------------

def fitted(name, X):
    """(model, item table [I, k], user table [U, k], k_used)"""
    from irspack_amd.recommenders.bpr import BPRFMRecommender
    from irspack_amd.recommenders.ials import IALSRecommender
    from irspack_amd.recommenders.multvae import MultVAERecommender
    from irspack_amd.recommenders.nmf import NMFRecommender
    from irspack_amd.recommenders.truncsvd import TruncatedSVDRecommender

    if name == "ials":
        m = IALSRecommender(X, n_components=64, alpha0=0.1, reg=1e-2, train_epochs=3).learn()
        return m, m.get_item_embedding(), m.get_user_embedding(), 64
    if name == "bpr":
        m = BPRFMRecommender(X, n_components=8, train_epochs=3).learn()
        users, items = m.factor_tables()
        assert items.shape[0] == 9
        return m, np.ascontiguousarray(items.T), users, 8
    if name == "multvae":
        m = MultVAERecommender(X, train_epochs=3, enc_hidden_dims=64, dec_hidden_dims=8, dim_z=16).learn()
        users, items = m.factor_tables()
        assert items.shape[0] == 10
        return m, np.ascontiguousarray(items.T), users, 8
    if name == "svd":
        m = TruncatedSVDRecommender(X, n_components=33).learn()
        return m, np.ascontiguousarray(m.decomposer.components_.T), m.z, 33
    m = NMFRecommender(X, n_components=8).learn()
    return m, np.ascontiguousarray(m.H.T), m.W, 8


@pytest.mark.parametrize("name", ["ials", "bpr", "multvae", "svd", "nmf"])
def test_fitted_factor_models(X, name):
    model, V, U, k_used = fitted(name, X)
    assert V.dtype == np.float32 and U.dtype == np.float32
    assert serving.embedding_width(model) == k_used
    dev = DeviceRecommender(model)
    users = np.array([5, 0, 17, 5, 299])
    for metric in ("cosine", "dot"):
        out = dev.similar_items_arrays(ITEMS, 20, metric=metric)
        check_neighbour_rows(V, ITEMS, k_used, metric, 20, *out)
        out = dev.similar_users_arrays(users, 20, metric=metric)
        check_neighbour_rows(U, users, k_used, metric, 20, *out)
    dev.close()


# ---- 12. ItemIDMapper and IDMapper --------------------------------------------------------------------------------

def test_id_mappers_equal_the_device_recommender(sim_models, sim_servers, factor_pair, factor_server):
    user_ids = [f"user-{u}" for u in range(N_USERS)]
    item_ids = [f"item-{i}" for i in range(N_ITEMS)]
    mapper = IDMapper(user_ids, item_ids)
    items, allowed = [5, 17, 5, 256, 0], [3, 9, 200, 77, 13, 14, 15, 16, 5]
    forbidden = [[1, 2], [], [77], [9], [3]]
    per = [[10, 11, 12], [], [], [256, 255], [0, 0, 1]]
    for model, dev in ((sim_models["item_knn"], sim_servers["item_knn"]), (sim_models["ease"], sim_servers["ease"]),
                       (factor_pair[0], factor_server)):
        got = mapper.similar_items_batch(
            model, [item_ids[i] for i in items], cutoff=6, allowed_item_ids=[item_ids[i] for i in allowed] + ["nope"],
            forbidden_item_ids=[[item_ids[i] for i in f] + ["unknown"] for f in forbidden])
        want = dev.similar_items(items, 6, allowed=allowed, forbidden=forbidden)
        assert got == [[(item_ids[i], s) for i, s in row] for row in want]
        got = mapper.similar_items_batch(
            model, [item_ids[i] for i in items], allowed_item_ids=[item_ids[1]],
            per_item_allowed_item_ids=[[item_ids[i] for i in p] + ["nope"] for p in per])
        want = dev.similar_items(items, 20, per_item_allowed=per)
        assert got == [[(item_ids[i], s) for i, s in row] for row in want]
        # one item: the same call with one row, whatever the batch threshold of the kind
        got = mapper.similar_items(model, item_ids[17], cutoff=4, forbidden_item_ids=[item_ids[5], "unknown"])
        want = dev.similar_items([17], 4, forbidden=[[5]])[0]
        assert got == [(item_ids[i], s) for i, s in want]
        assert 5 not in [i for i, _ in want] and 17 not in [i for i, _ in want]
        with pytest.raises(RuntimeError, match="not found"):
            mapper.similar_items(model, "item-9999")
        with pytest.raises(RuntimeError, match="not found"):
            mapper.similar_items_batch(model, [item_ids[0], "item-9999"])
    model = factor_pair[0]
    got = mapper.similar_items(model, item_ids[17], metric="dot")
    assert got == [(item_ids[i], s) for i, s in factor_server.similar_items([17], 20, metric="dot")[0]]
    users = [5, 299, 5]
    got = mapper.similar_users_batch(model, [user_ids[u] for u in users], cutoff=6,
                                     allowed_user_ids=[user_ids[u] for u in (1, 2, 5, 250, 299)] + ["nobody"],
                                     forbidden_user_ids=[[user_ids[1]], ["nobody"], []])
    want = factor_server.similar_users(users, 6, allowed=[1, 2, 5, 250, 299], forbidden=[[1], [], []])
    assert got == [[(user_ids[u], s) for u, s in row] for row in want]
    got = mapper.similar_users(model, user_ids[42], cutoff=3, metric="dot")
    assert got == [(user_ids[u], s) for u, s in factor_server.similar_users([42], 3, metric="dot")[0]]
    with pytest.raises(RuntimeError, match="not found"):
        mapper.similar_users(model, "nobody")
    knn = sim_models["user_knn"]
    got = mapper.similar_users_batch(knn, [user_ids[u] for u in users], cutoff=4)
    assert got == [[(user_ids[u], s) for u, s in row] for row in sim_servers["user_knn"].similar_users(users, 4)]
    with pytest.raises(NotImplementedError):
        mapper.similar_users(sim_models["item_knn"], user_ids[1])
    with pytest.raises(NotImplementedError):
        mapper.similar_items(knn, item_ids[1])


def test_id_mapper_remakes_the_user_side_after_an_edit_in_place():
    """the user table of a factor model is read where it lies by the recommend calls, so an edit in place leaves
    the cached DeviceRecommender alone; its user-side copy is a snapshot and has to be remade"""
    from irspack_amd.utils import id_mapping

    items, users = make_table(N_ITEMS, 8, seed=21), make_table(N_USERS, 8, seed=22)
    model = hand_factor_model(users, items)
    mapper = IDMapper(list(range(N_USERS)), list(range(N_ITEMS)))
    first = mapper.similar_users_batch(model, [1, 2, 42], cutoff=5, metric="dot")
    served = id_mapping._recommenders[model].served
    handle = served._user_side
    assert handle is not None and handle.h.value
    assert mapper.similar_users_batch(model, [1, 2, 42], cutoff=5, metric="dot") == first
    assert served._user_side is handle  # (kept while the table is unchanged)
    model.W *= np.float32(2.0)  # edited in place: same object, other content
    second = mapper.similar_users_batch(model, [1, 2, 42], cutoff=5, metric="dot")
    assert id_mapping._recommenders[model].served is served
    assert served._user_side is not handle and served._user_side.h.value
    assert [[u for u, _ in row] for row in second] == [[u for u, _ in row] for row in first]
    assert [[s for _, s in row] for row in second] == [[float(np.float32(4.0) * np.float32(s)) for _, s in row] for row in first]
    check_neighbour_rows(model.W, [1, 2, 42], 8, "dot", 5, *served.similar_users_arrays([1, 2, 42], 5, metric="dot"))
