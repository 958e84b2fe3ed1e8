"""GPU tests of the serving path: ``irspack_amd.serving.DeviceRecommender`` (``irs_serve_*``) and the batch methods
of ``irspack_amd.utils.IDMapper``.

Similarity models (sparse and dense weights): the expected lists are a Python restatement of
``retrieve_recommend_from_score`` (util.hpp:426-504: candidates in list order, best first, equal scores in candidate
order, stop at -inf, scores narrowed to float32) applied to scipy's own float64 product ``profiles[u] @ W`` with the
excluded items set to -inf.  Equality is exact: the same indices in the same order, the same float32 scores.

Factor models (float32 MFMA tiles): with ``s64`` the float64 product of the float32 tables, every returned score
must lie within ``B(u, i) = k * 2**-23 * sum_j |u_j v_j|`` of ``s64`` - the a-priori bound of a length-``k`` float32
dot product in any summation order (``gamma_k ~ k * 2**-24``), with a factor of two over it - and every row is
checked: no excluded item, only allowed ones, no repeats, the length ``min(cutoff, candidates)``, scores that do not
increase, and no candidate left out whose ``s64`` exceeds the last returned score by more than its ``B``.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps

from irspack_amd import _lib
from irspack_amd.serving import DeviceRecommender
from irspack_amd.utils import IDMapper

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS = 300, 257
CUTOFFS = [1, 7, 64, 65, 300]
EMPTY_USER = 0  # a user without history


def restated(score, allowed, cutoff):
    rows, n_items = score.shape
    out = []
    for r in range(rows):
        if len(allowed) == 0:
            cand = list(range(n_items))
        else:
            lst = allowed[0] if len(allowed) == 1 else allowed[r]
            cand = [i for i in lst if 0 <= i < n_items]
        pairs = sorted(((i, score[r, i]) for i in cand), key=lambda t: -t[1])  # stable: ties in candidate order
        res = []
        for i, s in pairs[:cutoff]:
            if s == -np.inf:
                break
            res.append((int(i), float(np.float32(s))))
        out.append(res)
    return out


def host_scores(profiles, W, seen, forbidden=None):
    """scipy's own product, float64, seen (nonzero) and forbidden items at -inf"""
    S = profiles @ W
    S = np.asarray(S.toarray() if sps.issparse(S) else S, dtype=np.float64)
    S[seen.nonzero()] = -np.inf
    if forbidden is not None:
        for r, f in enumerate(forbidden):
            S[r, list(f)] = -np.inf
    return S


def as_lists(idx, score, length):
    assert idx.dtype == np.int32 and score.dtype == np.float32 and length.dtype == np.int32
    assert idx.shape == score.shape and length.shape == (idx.shape[0],)
    for r in range(idx.shape[0]):  # the padding
        assert (idx[r, length[r]:] == -1).all() and (idx[r, :length[r]] >= 0).all()
    return [[(int(i), float(s)) for i, s in zip(idx[r, :length[r]], score[r, :length[r]])]
            for r in range(idx.shape[0])]


@pytest.fixture(scope="module")
def X():
    rng = np.random.default_rng(11)
    D = (rng.random((N_USERS, N_ITEMS)) < 0.05).astype(np.float64)
    D[EMPTY_USER] = 0.0
    return sps.csr_matrix(D)


@pytest.fixture(scope="module")
def models(X):
    from irspack_amd.recommenders.dense_slim import DenseSLIMRecommender
    from irspack_amd.recommenders.knn import CosineKNNRecommender
    from irspack_amd.recommenders.slim import SLIMRecommender
    from irspack_amd.recommenders.user_knn import CosineUserKNNRecommender

    out = {
        "item_knn": CosineKNNRecommender(X, top_k=30).learn(),
        "user_knn": CosineUserKNNRecommender(X, top_k=30).learn(),
        "slim": SLIMRecommender(X, alpha=0.01, l1_ratio=0.1, n_iter=10).learn(),
        "ease": DenseSLIMRecommender(X, reg=5.0).learn(),
    }
    assert out["slim"].W.dtype == np.float32 and isinstance(out["ease"].W, np.ndarray)
    return out


@pytest.fixture(scope="module")
def servers(models):
    return {name: DeviceRecommender(m) for name, m in models.items()}


def operands(model):
    """(profiles, W) of the host product"""
    if hasattr(model, "U_"):
        return model.U.tocsr(), model.X_train_all
    return model.X_train_all, model.W


def expected_known(model, users, cutoff, allowed=(), forbidden=None):
    P, W = operands(model)
    S = host_scores(P[users], W, model.X_train_all[users], forbidden)
    return restated(S, list(allowed), cutoff)


USERS = np.array([5, EMPTY_USER, 17, 5, 299, 42, 42, 42, 101, 250, 7, 8, 9, 200, 150, 3, 298, 64, 65, 128, 255, 1, 2])


@pytest.mark.parametrize("name", ["item_knn", "user_knn", "slim", "ease"])
@pytest.mark.parametrize("cutoff", CUTOFFS)
def test_similarity_models_are_exact(models, servers, name, cutoff):
    model, dev = models[name], servers[name]
    everything = list(range(N_ITEMS))
    forbidden = [[] for _ in USERS]
    forbidden[4] = everything  # exclusions that cover the whole catalogue: an empty list
    forbidden[2] = [0, 1, 2, 200]
    got = as_lists(*dev.recommend_known_arrays(USERS, cutoff, forbidden=forbidden))
    want = expected_known(model, USERS, cutoff, forbidden=forbidden)
    assert got == want
    assert got[4] == []
    assert got[0] == got[3] and got[5] == got[6] == got[7]  # repeated user indices
    if name in ("item_knn", "slim", "ease"):  # no history: all scores 0, the first candidates in order
        assert got[1] == [(i, 0.0) for i in range(min(cutoff, N_ITEMS))]
    for users in (USERS[:1], USERS[:3]):  # rows 1 and 3
        assert dev.recommend_known(users, cutoff) == expected_known(model, users, cutoff)


@pytest.mark.parametrize("name", ["item_knn", "ease"])
def test_three_chunks_with_a_ragged_last_one(models, servers, name, monkeypatch):
    monkeypatch.setenv("IRSPACK_AMD_SERVE_BLOCK", "256")  # (read per call)
    rng = np.random.default_rng(2)
    users = rng.integers(0, N_USERS, size=601)
    per_user = [list(rng.integers(-2, N_ITEMS + 2, size=rng.integers(0, 30))) for _ in users]
    got = as_lists(*servers[name].recommend_known_arrays(users, 7))
    assert got == expected_known(models[name], users, 7)
    got = as_lists(*servers[name].recommend_known_arrays(users, 7, per_user_allowed=per_user))
    assert got == expected_known(models[name], users, 7, allowed=per_user)


@pytest.mark.parametrize("name", ["item_knn", "user_knn", "ease"])
def test_allowed_and_forbidden_lists(models, servers, name):
    model, dev = models[name], servers[name]
    rng = np.random.default_rng(4)
    glob = [5, 3, 3, 256, 257, -1, 77, 0, 100, 101, 102, 3, 900]  # duplicates kept, out-of-range ids dropped
    forbidden = [list(rng.integers(0, N_ITEMS, size=rng.integers(0, 20))) for _ in USERS]
    for cutoff in (1, 7, 64):
        got = as_lists(*dev.recommend_known_arrays(USERS, cutoff, allowed=glob, forbidden=forbidden))
        assert got == expected_known(model, USERS, cutoff, allowed=[glob], forbidden=forbidden)
    per = [list(rng.integers(-3, N_ITEMS + 5, size=rng.integers(0, 120))) for _ in USERS]
    per[6] = []
    for cutoff in (7, 65, 300):
        # (per-user lists take precedence over the global one)
        got = as_lists(*dev.recommend_known_arrays(USERS, cutoff, allowed=glob, per_user_allowed=per))
        assert got == expected_known(model, USERS, cutoff, allowed=per)
        assert got[6] == []


def hand_model(n_users, n_items, seed, density=0.03):
    """a similarity model with hand-built weights out of {0.25, 0.5, 1.0}: scores tie everywhere"""
    from irspack_amd.recommenders.base import BaseSimilarityRecommender

    rng = np.random.default_rng(seed)
    Xh = sps.csr_matrix((rng.random((n_users, n_items)) < 0.04).astype(np.float64))
    W = sps.random(n_items, n_items, density=density, format="csr", random_state=seed,
                   data_rvs=lambda n: rng.choice([0.25, 0.5, 1.0], size=n))
    model = BaseSimilarityRecommender(Xh)
    model._W = W
    return model


@pytest.mark.parametrize("cutoff", [7, 65, 300])
def test_wide_catalogue_with_ties(cutoff):
    model = hand_model(60, 1031, seed=1)
    dev = DeviceRecommender(model)
    users = np.arange(60)
    got = as_lists(*dev.recommend_known_arrays(users, cutoff))
    want = expected_known(model, users, cutoff)
    assert got == want
    assert any(len({s for _, s in row}) < len(row) for row in want)  # (the case has ties)
    lst = [1030, 5, 5, 700, 1031, 3, 2, 1, 0, 512, 513]
    assert dev.recommend_known(users[:9], cutoff, allowed=lst) == expected_known(model, users[:9], cutoff, allowed=[lst])


def test_cutoff_above_2048():
    """cutoff 2100 of 2500 items: the ranking keeps its lists in global scratch, the output stage walks 33 steps"""
    model = hand_model(6, 2500, seed=2, density=0.4)
    dev = DeviceRecommender(model)
    users = np.array([0, 3, 5, 3])
    got = as_lists(*dev.recommend_known_arrays(users, 2100))
    assert got == expected_known(model, users, 2100)
    assert max(len(g) for g in got) > 2048


def test_duplicate_column_in_a_row_of_W():
    """The C call refuses it; the Python layer uploads a canonical copy (duplicates summed - exact for these dyadic
    weights, so the lists are scipy's) and leaves the model's matrix alone."""
    from irspack_amd.recommenders.base import BaseSimilarityRecommender

    n = 40
    rng = np.random.default_rng(6)
    Xh = sps.csr_matrix((rng.random((25, n)) < 0.2).astype(np.float64))
    rows = np.repeat(np.arange(n), 4)
    cols = rng.integers(0, n, size=4 * n)
    cols[0:4] = [7, 3, 7, 9]  # row 0 stores column 7 twice
    vals = rng.choice([0.25, 0.5, 1.0, 2.0], size=4 * n)
    indptr = np.arange(0, 4 * n + 1, 4, dtype=np.int64)
    W = sps.csr_matrix((vals, cols.astype(np.int32), indptr.astype(np.int32)), shape=(n, n))
    assert W.nnz == 4 * n  # (duplicates are stored)
    h = C.c_void_p()
    cols32, vals64 = cols.astype(np.int32), vals.astype(np.float64)
    status = _lib.lib().irs_serve_create_similarity(
        C.c_int64(n), C.c_int64(n), _lib.ptr(indptr, C.c_int64), _lib.ptr(cols32, C.c_int32),
        _lib.ptr(vals64, C.c_double), C.c_int32(_lib.default_device()), C.byref(h))
    assert status == 1 and not h.value
    with pytest.raises(ValueError, match="duplicate column in a row of W"):
        _lib.check(status)
    model = BaseSimilarityRecommender(Xh)
    model._W = W
    before = (W.indptr.copy(), W.indices.copy(), W.data.copy())
    users = np.arange(25)
    assert DeviceRecommender(model).recommend_known(users, 10) == expected_known(model, users, 10)
    assert all(np.array_equal(a, b) for a, b in zip(before, (W.indptr, W.indices, W.data)))


@pytest.mark.parametrize("name", ["item_knn", "slim", "ease"])
def test_new_user_profiles(models, servers, name):
    model, dev = models[name], servers[name]
    rng = np.random.default_rng(8)
    rows = []
    for r in range(12):
        items = rng.choice(N_ITEMS, size=rng.integers(0, 15), replace=False)  # storage order: not sorted
        rows.append({int(i): float(rng.choice([0.0, 1.0, 2.5])) for i in items})  # (0.0: a stored zero, not excluded)
    indptr = np.cumsum([0] + [len(r) for r in rows])
    Xn = sps.csr_matrix((np.array([v for r in rows for v in r.values()], dtype=np.float64),
                         np.array([i for r in rows for i in r], dtype=np.int32), indptr.astype(np.int32)),
                        shape=(12, N_ITEMS))
    forbidden = [[int(rng.integers(0, N_ITEMS))] for _ in rows]
    for cutoff in (7, 65):
        got = as_lists(*dev.recommend_profiles_arrays(Xn, cutoff, forbidden=forbidden))
        assert got == restated(host_scores(Xn, model.W, Xn, forbidden), [], cutoff)
    # a repeated item inside a profile: the whole call takes the host path, the lists are scipy's
    Xd = sps.csr_matrix((np.array([1.0, 1.0, 1.0, 2.0]), np.array([4, 9, 4, 30], dtype=np.int32),
                         np.array([0, 3, 4], dtype=np.int32)), shape=(2, N_ITEMS))
    want = restated(model.get_score_cold_user_remove_seen(Xd.copy()), [], 7)
    assert dev.recommend_profiles(Xd, 7) == want


def test_user_similarity_has_no_new_user_path(servers):
    with pytest.raises(NotImplementedError):
        servers["user_knn"].recommend_profiles(sps.csr_matrix((1, N_ITEMS)), 5)


# ---- factor models ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def factor_models(X):
    from irspack_amd.recommenders.ials import IALSRecommender
    from irspack_amd.recommenders.nmf import NMFRecommender
    from irspack_amd.recommenders.truncsvd import TruncatedSVDRecommender

    rng = np.random.default_rng(13)
    wide = NMFRecommender(X, n_components=576)  # a hand-made pair of tables at the largest k
    wide.W = rng.standard_normal((N_USERS, 576)).astype(np.float32)
    wide.H = rng.standard_normal((576, N_ITEMS)).astype(np.float32)
    return {
        "ials64": IALSRecommender(X, n_components=64, alpha0=0.1, reg=1e-2, train_epochs=3).learn(),
        "svd5": TruncatedSVDRecommender(X, n_components=5).learn(),
        "svd33": TruncatedSVDRecommender(X, n_components=33).learn(),
        "nmf8": NMFRecommender(X, n_components=8).learn(),
        "hand576": wide,
    }


@pytest.fixture(scope="module")
def factor_servers(factor_models):
    return {name: DeviceRecommender(m) for name, m in factor_models.items()}


def tables(name, model):
    """(user table (U, k), item table (I, k)) as float32"""
    if name.startswith("ials"):
        return model.get_user_embedding(), model.get_item_embedding()
    if name.startswith("svd"):
        return model.z, model.decomposer.components_.T
    return model.W, model.H.T


def check_factor_rows(U, V, excluded, allowed, cutoff, idx, score, length):
    """every row of a factor-model result against the float64 product of the float32 tables"""
    k = U.shape[1]
    U64, V64 = U.astype(np.float64), V.astype(np.float64)
    s64 = U64 @ V64.T
    B = k * 2.0 ** -23 * (np.abs(U64) @ np.abs(V64).T)
    n_items = V.shape[0]
    got = as_lists(idx, score, length)
    for r, row in enumerate(got):
        if len(allowed) == 0:
            cand = list(range(n_items))
        else:
            cand = [i for i in (allowed[0] if len(allowed) == 1 else allowed[r]) if 0 <= i < n_items]
        live = [i for i in cand if i not in excluded[r]]
        items = [i for i, _ in row]
        assert not set(items) & excluded[r], r
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


@pytest.mark.parametrize("name", ["ials64", "svd5", "svd33", "nmf8", "hand576"])
@pytest.mark.parametrize("cutoff", CUTOFFS)
def test_factor_models_within_the_fp32_bound(X, factor_models, factor_servers, name, cutoff):
    model, dev = factor_models[name], factor_servers[name]
    U, V = tables(name, model)
    assert U.dtype == np.float32 and V.dtype == np.float32
    rng = np.random.default_rng(cutoff)
    users = USERS
    forbidden = [list(rng.integers(0, N_ITEMS, size=rng.integers(0, 10))) for _ in users]
    forbidden[4] = list(range(N_ITEMS))
    excluded = [set(X[u].indices.tolist()) | set(f) for u, f in zip(users, forbidden)]
    out = dev.recommend_known_arrays(users, cutoff, forbidden=forbidden)
    check_factor_rows(U[users], V, excluded, [], cutoff, *out)
    assert out[2][4] == 0
    glob = [5, 3, 256, 257, -1, 77, 0, 100, 101, 102, 900, 200, 201]
    out = dev.recommend_known_arrays(users, cutoff, allowed=glob)
    check_factor_rows(U[users], V, [set(X[u].indices.tolist()) for u in users], [glob], cutoff, *out)
    per = [list(rng.choice(N_ITEMS, size=rng.integers(0, 90), replace=False)) for _ in users]
    per[6] = []
    out = dev.recommend_known_arrays(users, cutoff, per_user_allowed=per)
    check_factor_rows(U[users], V, [set(X[u].indices.tolist()) for u in users], per, cutoff, *out)
    assert out[2][6] == 0


def test_factor_models_three_chunks(X, factor_models, factor_servers, monkeypatch):
    monkeypatch.setenv("IRSPACK_AMD_SERVE_BLOCK", "256")
    users = np.random.default_rng(3).integers(0, N_USERS, size=601)
    for name in ("ials64", "svd33"):
        U, V = tables(name, factor_models[name])
        out = factor_servers[name].recommend_known_arrays(users, 7)
        check_factor_rows(U[users], V, [set(X[u].indices.tolist()) for u in users], [], 7, *out)


@pytest.mark.parametrize("name", ["ials64", "svd5", "nmf8"])
def test_factor_models_new_users(X, factor_models, factor_servers, name):
    model, dev = factor_models[name], factor_servers[name]
    Xn = sps.csr_matrix(X[100:117])
    if name == "ials64":
        F = model.compute_user_embedding(Xn)
    elif name == "svd5":
        F = model.decomposer.transform(Xn)
    else:
        F = model.nmf_model.transform(Xn)
    F = np.ascontiguousarray(F, dtype=np.float32)
    V = tables(name, model)[1]
    out = dev.recommend_profiles_arrays(Xn, 20)
    check_factor_rows(F, V, [set(Xn[r].indices.tolist()) for r in range(Xn.shape[0])], [], 20, *out)


# ---- IDMapper ------------------------------------------------------------------------------------------------

def test_id_mapper_batches_equal_the_device_recommender(models, servers, factor_models, factor_servers):
    user_ids = [f"user-{u}" for u in range(N_USERS)]
    item_ids = [f"item-{i}" for i in range(N_ITEMS)]
    mapper = IDMapper(user_ids, item_ids)
    users = [5, 17, 5, 299, EMPTY_USER]
    allowed = [3, 9, 200, 77, 13, 14, 15, 16]
    forbidden = [[1, 2], [], [77], [9], [3]]
    profiles = [[item_ids[i] for i in (4, 9, 30)], {item_ids[7]: 2.0, "unknown": 1.0, item_ids[8]: 0.0}, []]
    Xn = mapper.list_of_user_profile_to_matrix(profiles)
    for model, dev in ((models["item_knn"], servers["item_knn"]), (models["ease"], servers["ease"]),
                       (factor_models["svd5"], factor_servers["svd5"])):
        got = mapper.recommend_for_known_user_batch(
            model, [user_ids[u] for u in users], cutoff=6, allowed_item_ids=[item_ids[i] for i in allowed] + ["nope"],
            forbidden_item_ids=[[item_ids[i] for i in f] for f in forbidden])
        want = dev.recommend_known(users, 6, allowed=allowed, forbidden=forbidden)
        assert got == [[(item_ids[i], s) for i, s in row] for row in want]
        per = [[item_ids[i] for i in (10, 11, 12)], [], ["nope"], [item_ids[256]], [item_ids[0], item_ids[0]]]
        got = mapper.recommend_for_known_user_batch(model, [user_ids[u] for u in users],
                                                    allowed_item_ids=[item_ids[1]], per_user_allowed_item_ids=per)
        want = dev.recommend_known(users, 20, per_user_allowed=[[10, 11, 12], [], [], [256], [0, 0]])
        assert got == [[(item_ids[i], s) for i, s in row] for row in want]
        got = mapper.recommend_for_new_user_batch(model, profiles, cutoff=9)
        want = dev.recommend_profiles(Xn, 9)
        assert got == [[(item_ids[i], s) for i, s in row] for row in want]
        assert all(len(row) == 9 for row in got)


def test_id_mapper_two_step_path_for_an_unrecognised_model(X):
    from irspack_amd.recommenders.base import BaseRecommender
    from irspack_amd.utils import retrieve_recommend_from_score

    scores = np.random.default_rng(9).standard_normal((N_USERS, N_ITEMS))
    item_item = np.random.default_rng(10).standard_normal((N_ITEMS, N_ITEMS))

    class Fixed(BaseRecommender):
        def get_score(self, user_indices):
            return scores[user_indices].copy()

        def get_score_cold_user(self, Xc):
            return np.asarray(sps.csr_matrix(Xc).dot(item_item))

    model = Fixed(X)
    mapper = IDMapper(list(range(N_USERS)), [f"i{i}" for i in range(N_ITEMS)])
    users = [3, 8, 3]
    got = mapper.recommend_for_known_user_batch(model, users, cutoff=5, forbidden_item_ids=[["i1"], [], ["i2"]])
    S = model.get_score_remove_seen(np.array(users))
    S[0, 1] = S[2, 2] = -np.inf
    want = retrieve_recommend_from_score(S, [], 5, 1)
    assert got == [[(f"i{i}", s) for i, s in row] for row in want]
    got = mapper.recommend_for_new_user_batch(model, [["i4", "i9"], ["i0"]], cutoff=3)
    Xn = mapper.list_of_user_profile_to_matrix([["i4", "i9"], ["i0"]])
    want = retrieve_recommend_from_score(model.get_score_cold_user_remove_seen(Xn), [], 3, 1)
    assert got == [[(f"i{i}", s) for i, s in row] for row in want]
    with pytest.raises(ValueError, match="float32 or float64"):
        mapper.score_to_recommended_items_batch(np.zeros((2, N_ITEMS), dtype=np.float16), 3)
    # the host-scores form writes -inf into the caller's array, as the reference does
    S = np.zeros((2, N_ITEMS), dtype=np.float32)
    mapper.score_to_recommended_items_batch(S, 3, forbidden_item_ids=[["i5"], []])
    assert S[0, 5] == -np.inf and np.isfinite(S[1]).all()


def test_id_mapper_notices_a_changed_model(models):
    """the device copy is kept per model and remade when an operand's content changes"""
    from irspack_amd.recommenders.base import BaseSimilarityRecommender
    from irspack_amd.utils import id_mapping

    model = BaseSimilarityRecommender(models["item_knn"].X_train_all)
    model._W = models["item_knn"].W.copy()
    mapper = IDMapper(list(range(N_USERS)), list(range(N_ITEMS)))
    first = mapper.recommend_for_known_user_batch(model, [5, 17], cutoff=4)
    held = id_mapping._recommenders[model].served
    assert mapper.recommend_for_known_user_batch(model, [5, 17], cutoff=4) == first
    assert id_mapping._recommenders[model].served is held
    model._W.data *= 2.0  # edited in place: same object, other content
    second = mapper.recommend_for_known_user_batch(model, [5, 17], cutoff=4)
    assert id_mapping._recommenders[model].served is not held
    assert [[i for i, _ in row] for row in second] == [[i for i, _ in row] for row in first]
    assert [[s for _, s in row] for row in second] == [[float(np.float32(2.0 * s)) for _, s in row] for row in first]


def test_id_mapper_lets_go_of_a_dropped_model(models):
    """the cached device copy must not keep its model alive: the entry and the handle go with the model"""
    import gc
    import weakref

    from irspack_amd.recommenders.base import BaseSimilarityRecommender
    from irspack_amd.utils import id_mapping

    model = BaseSimilarityRecommender(models["item_knn"].X_train_all)
    model._W = models["item_knn"].W.copy()
    mapper = IDMapper(list(range(N_USERS)), list(range(N_ITEMS)))
    before = len(id_mapping._recommenders)
    want = DeviceRecommender(model).recommend_known([5, 17], 4)
    assert mapper.recommend_for_known_user_batch(model, [5, 17], cutoff=4) == want
    served = id_mapping._recommenders[model].served
    assert len(id_mapping._recommenders) == before + 1 and served._h.value
    gone = weakref.ref(model)
    del model
    gc.collect()
    assert gone() is None and len(id_mapping._recommenders) == before
    assert not served._h.value  # closed
    with pytest.raises(ReferenceError):
        served.recommend_known([5], 4)


def test_host_path_keeps_ties_in_candidate_order(models, servers):
    """a profile row with a repeated column takes the host path; equal scores inside an UNSORTED allowed list must
    still come in the order of the list, as on the device"""
    dev = servers["item_knn"]
    Xd = sps.csr_matrix((np.array([1.0, 1.0]), np.array([4, 4], dtype=np.int32), np.array([0, 2, 2], dtype=np.int32)),
                        shape=(2, N_ITEMS))  # row 1 is empty: every score 0
    allowed = [200, 3, 256, 3, 17, 999, 5]
    S = models["item_knn"].get_score_cold_user_remove_seen(Xd.copy())
    assert dev.recommend_profiles(Xd, 4, allowed=allowed) == restated(S, [allowed], 4)
    assert [i for i, _ in dev.recommend_profiles(Xd, 4, allowed=allowed)[1]] == [200, 3, 256, 3]
    # the same lists with a profile the device scores
    Xs = sps.csr_matrix((2, N_ITEMS))
    assert [i for i, _ in dev.recommend_profiles(Xs, 4, allowed=allowed)[1]] == [200, 3, 256, 3]


def test_negative_first_offsets_are_argument_errors(servers):
    """the row, exclusion and list arrays are read by absolute offset: a negative first offset is refused"""
    lib, ptr = _lib.lib(), _lib.ptr
    h = servers["item_knn"]._h
    ok_ptr, bad_ptr = np.array([0, 1], dtype=np.int64), np.array([-1, 0], dtype=np.int64)
    cols, vals = np.array([3], dtype=np.int32), np.array([1.0])
    items = np.array([5], dtype=np.int64)
    idx, sc, ln = np.zeros((1, 2), dtype=np.int32), np.zeros((1, 2), dtype=np.float32), np.zeros(1, dtype=np.int32)

    def call(xp, ep, n_lists, lp):
        return lib.irs_serve_recommend_profiles(
            h, C.c_int64(1), ptr(xp, C.c_int64), ptr(cols, C.c_int32), ptr(vals, C.c_double),
            ptr(ep, C.c_int64) if ep is not None else None, ptr(cols, C.c_int32) if ep is not None else None,
            C.c_int64(n_lists), ptr(lp, C.c_int64), ptr(items, C.c_int64), C.c_int64(2), ptr(idx, C.c_int32),
            ptr(sc, C.c_float), ptr(ln, C.c_int32))

    assert call(ok_ptr, ok_ptr, 1, ok_ptr) == 0 and ln[0] == 1 and idx[0, 0] == 5
    for args in ((bad_ptr, None, 0, ok_ptr), (ok_ptr, bad_ptr, 0, ok_ptr), (ok_ptr, None, 1, bad_ptr)):
        status = call(*args)
        assert status == 1
        with pytest.raises(ValueError):
            _lib.check(status)


# ---- determinism -------------------------------------------------------------------------------------------------

def test_two_calls_give_identical_arrays(servers, factor_servers):
    for dev in list(servers.values()) + list(factor_servers.values()):
        a = dev.recommend_known_arrays(USERS, 65)
        b = dev.recommend_known_arrays(USERS, 65)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()


# ---- row pointers that do not start at 0 -------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["item_knn", "ease"])
def test_rows_and_exclusions_of_a_larger_matrix_without_rebasing(X, servers, name, monkeypatch):
    """``recommend_profiles`` through the C ABI with ``x_indptr[0] > 0`` and ``excl_indptr[0] > 0``: 40 rows out of
    the middle of a larger CSR, their pointers as they stand (the profile entries are read at those offsets, the
    exclusion entries from the first one of the call) - the same three arrays as with the pointers rebased to 0."""
    monkeypatch.setenv("IRSPACK_AMD_SERVE_BLOCK", "256")  # (read per call)
    lib, ptr = _lib.lib(), _lib.ptr
    h = servers[name]._h
    rows, first, cutoff = 40, 100, 7
    xp = np.ascontiguousarray(X.indptr[first:first + rows + 1], dtype=np.int64)
    xi, xd = np.ascontiguousarray(X.indices, dtype=np.int32), np.ascontiguousarray(X.data, dtype=np.float64)
    E = sps.csr_matrix((np.random.default_rng(5).random(X.shape) < 0.1).astype(np.float64))
    ep = np.ascontiguousarray(E.indptr[first + 20:first + 20 + rows + 1], dtype=np.int64)
    ei = np.ascontiguousarray(E.indices[ep[0]:ep[-1]], dtype=np.int32)
    assert xp[0] > 0 and ep[0] > 0 and xp[-1] > xp[0] and ep[-1] > ep[0]
    no_list = np.zeros(1, dtype=np.int64)

    def call(xp_, xi_, xd_, ep_):
        idx, sc = np.full((rows, cutoff), -7, dtype=np.int32), np.full((rows, cutoff), -7, dtype=np.float32)
        ln = np.full(rows, -7, dtype=np.int32)
        _lib.check(lib.irs_serve_recommend_profiles(
            h, C.c_int64(rows), ptr(xp_, C.c_int64), ptr(xi_, C.c_int32), ptr(xd_, C.c_double), ptr(ep_, C.c_int64),
            ptr(ei, C.c_int32), C.c_int64(0), ptr(no_list, C.c_int64), ptr(no_list, C.c_int64), C.c_int64(cutoff),
            ptr(idx, C.c_int32), ptr(sc, C.c_float), ptr(ln, C.c_int32)))
        return idx, sc, ln

    got = call(xp, xi, xd, ep)
    want = call(xp - xp[0], np.ascontiguousarray(xi[xp[0]:]), np.ascontiguousarray(xd[xp[0]:]), ep - ep[0])
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()
    assert (got[2] == cutoff).all() and (got[0] >= 0).all()
    excluded = E[first + 20:first + 20 + rows].toarray() != 0
    assert not excluded[np.arange(rows)[:, None], got[0]].any()
