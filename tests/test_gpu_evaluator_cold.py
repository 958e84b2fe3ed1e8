"""``EvaluatorWithColdUser`` on the device: fold-in, scores, mask and ranking without the host block loop
(``cold_user_operands``; the ``*_scored`` model calls with a scored width below the evaluator's; the truncated SVD's
device fold-in ``irs_truncsvd_transform``).

The comparison target is always the same evaluator with ``fused=False`` - the model's own host scores ``mb_size``
users at a time, padded with ``-inf`` for the feature-only items, masked and ranked on the device.  "Equal" is
``assert_equal`` of test_gpu_evaluator_models.py: ``item_cnt``, ``valid_user`` and ``total_user`` identical, the five
float64 sums to ``rel=1e-12`` (identical terms in another order) and, with ``mb_size=128`` for the dense and factor
kinds, to the last bit.  In every case the model's ``get_score_cold_user`` is replaced ON THE INSTANCE by a function
that raises before the device path runs: the host loop did not run."""
import copy

import numpy as np
import pytest
import scipy.sparse as sps
from test_gpu_evaluator_models import assert_equal, metrics_of

from irspack_amd.evaluation import EvaluatorWithColdUser
from irspack_amd.evaluation._core_evaluator import EvaluatorCore, MaskRows, Metrics
from irspack_amd.synthetic import holdout_split, make_interactions
from irspack_amd.utils import truncated_svd_transform

pytestmark = pytest.mark.gpu

CUTOFFS = [5, 20]


def trap(model):
    def get_score_cold_user(*args, **kwargs):
        raise AssertionError("the host cold-user scores ran")

    model.get_score_cold_user = get_score_cold_user  # (on the instance: the class's scoring is what it was)


def untrap(model):
    del model.get_score_cold_user


def compare(model, path, same_sums, what, *args, **kwargs):
    """the device path against the block loop of the same evaluator; returns the block loop's ``Metrics``"""
    plain = EvaluatorWithColdUser(*args, fused=False, **kwargs)
    fused = EvaluatorWithColdUser(*args, **kwargs)
    assert fused._device_path(model) == path and plain._device_path(model) == "blocks", what
    want = metrics_of(plain, model, CUTOFFS)
    if path != "blocks":
        trap(model)
    try:
        got = metrics_of(fused, model, CUTOFFS)
    finally:
        if path != "blocks":
            untrap(model)
    assert_equal(got, want, what, same_sums=same_sums)
    assert want[0].total_user == args[0].shape[0]
    return want


def cold_problem(rns, n_users, n_warm, n_cold, density, empty=(0, 1, 2)):
    """binary cold profiles (some empty), a ground truth over all ``n_warm + n_cold`` columns with hits placed in the
    feature-only columns, an ``n_warm``-wide mask of its own and the features of the feature-only items"""
    lil = sps.lil_matrix((rns.rand(n_users, n_warm) < density).astype(np.float64))
    for r in empty:
        lil.rows[r], lil.data[r] = [], []
    cold = sps.csr_matrix(lil)
    cold.sort_indices()
    truth = (rns.rand(n_users, n_warm + n_cold) < max(0.01, 8.0 / n_warm)).astype(np.float64)
    truth[:, n_warm:] = rns.rand(n_users, n_cold) < 0.5
    own_mask = sps.csr_matrix((rns.rand(n_users, n_warm) > 0.95).astype(np.float64))
    features = np.ones((n_cold, 3), dtype=np.float32) if n_cold else None
    return cold, sps.csr_matrix(truth), own_mask, features


def variants(rns, n_users, n_warm, n_cold, own_mask):
    """the keyword sets of the issue's list: default mask, an n_warm-wide mask of the caller's (the constructor
    widens it), recall_with_cutoff, a shared candidate list that holds feature-only columns, per-user lists"""
    n_items = n_warm + n_cold
    shared = sorted(set(rns.randint(0, n_warm, n_warm // 3).tolist()) | set(range(n_warm, n_items)))
    per_user = [sorted(set(rns.randint(0, n_items, 60).tolist()) | set(range(n_warm, n_items))) for _ in range(n_users)]
    return [("default mask", {}), ("own mask", dict(masked_interactions=own_mask)),
            ("recall_with_cutoff", dict(recall_with_cutoff=True)), ("shared list", dict(recommendable_items=shared)),
            ("per-user lists", dict(per_user_recommendable_items=per_user))]


# --------------------------------------------------------------------------------------- 1. sparse similarity
_knn = {}


def knn_model(n_warm):
    from irspack_amd.recommenders import CosineKNNRecommender

    if n_warm not in _knn:
        rns = np.random.RandomState(n_warm)
        X = sps.csr_matrix((rns.rand(400, n_warm) < 0.02).astype(np.float64))
        _knn[n_warm] = CosineKNNRecommender(X, top_k=20).learn()
    return _knn[n_warm]


@pytest.mark.parametrize("n_warm, n_cold", [(2040, 0), (2040, 20), (2048, 1)])
def test_sparse_similarity_model(n_warm, n_cold):
    """The scored width ends inside the first 2,048-column tile of ``sim_score_kernel`` with the unscored columns
    running into the second, and exactly at the tile's edge; 300 users cross 128 and 256."""
    model = knn_model(n_warm)
    rns = np.random.RandomState(10 * n_warm + n_cold)
    cold, truth, own_mask, features = cold_problem(rns, 300, n_warm, n_cold, 0.02)
    for what, kw in variants(rns, 300, n_warm, n_cold, own_mask):
        want = compare(model, "similarity", False, f"{n_warm}+{n_cold} {what}", cold, truth,
                       cold_item_features=features, **kw)
        # a feature-only item is never recommended: both evaluators leave those columns at -inf
        assert all(m.item_cnt[n_warm:].sum() == 0 for m in want) and want[0].valid_user > 0


def test_float32_profiles_against_float64_sparse_weights():
    model = knn_model(2040)
    assert model.W.dtype == np.float64
    rns = np.random.RandomState(77)
    cold, truth, _, features = cold_problem(rns, 300, 2040, 20, 0.02)
    compare(model, "similarity", False, "float32 profiles", cold.astype(np.float32), truth, cold_item_features=features)


# ---------------------------------------------------------------------------------------- 2. dense similarity
_dense = {}


def dense_model(n_warm):
    from irspack_amd.recommenders import DenseSLIMRecommender

    if n_warm not in _dense:
        rns = np.random.RandomState(n_warm)
        X = sps.csr_matrix((rns.rand(300, n_warm) < 0.06).astype(np.float64))
        _dense[n_warm] = DenseSLIMRecommender(X, reg=5.0).learn()
        assert _dense[n_warm].W.dtype == np.float32
    return _dense[n_warm]


@pytest.mark.parametrize("n_warm, n_cold", [(250, 0), (250, 10), (256, 1)])
def test_dense_similarity_model(n_warm, n_cold, monkeypatch):
    """The scored width ends inside a 256-column strip of ``dense_sim_score_kernel`` and at its edge; 200 users, in
    the middle case in two device blocks (128 + 72: the last one short); ``mb_size=128``, so the float64 sums are the
    block loop's to the last bit."""
    model = dense_model(n_warm)
    rns = np.random.RandomState(10 * n_warm + n_cold + 1)
    cold, truth, own_mask, features = cold_problem(rns, 200, n_warm, n_cold, 0.06)
    if n_cold == 10:
        monkeypatch.setenv("IRSPACK_AMD_EVAL_SIM_BLOCK_ROWS", "128")
    for what, kw in variants(rns, 200, n_warm, n_cold, own_mask):
        want = compare(model, "dense_similarity", True, f"{n_warm}+{n_cold} {what}", cold, truth,
                       cold_item_features=features, mb_size=128, **kw)
        assert all(m.item_cnt[n_warm:].sum() == 0 for m in want) and want[0].valid_user > 0
    # float32 profiles against the float32 W: a float32 product on the host, which stays there
    compare(model, "blocks", True, "float32 profiles", cold.astype(np.float32), truth, cold_item_features=features,
            mb_size=128)


# ------------------------------------------------------------------------------- 3. the factor call, exact
@pytest.mark.parametrize("n_scored, n_items", [(70, 70), (70, 75), (64, 65)])
@pytest.mark.parametrize("k", [3, 33])
def test_factor_call_with_a_scored_width_on_integer_factors(k, n_scored, n_items):
    """Integer-valued factors (test_factor_kernel_on_integer_factors): every order of the float32 sums gives the same
    block, so the call equals the exact host product padded with ``-inf`` and ranked by ``get_metrics_masked``, sums
    to the last bit.  The scored width ends inside a 64-column MFMA tile, at its edge with one unscored column, and
    covers the block; 300 users: the last 128-user chunk is short.  Handing the users over in two calls, the second
    continuing the sums of the first, gives the same bits."""
    rns = np.random.RandomState(100 * k + n_items)
    n_users = 300
    A = rns.randint(-8, 9, (n_users, k)).astype(np.float32)
    B = rns.randint(-8, 9, (n_scored, k)).astype(np.float32)
    truth = rns.rand(n_users, n_items) < 0.05
    truth[:, n_scored:] = rns.rand(n_users, n_items - n_scored) < 0.5
    core = EvaluatorCore(sps.csr_matrix(truth.astype(np.float64)), [])
    mask = MaskRows(sps.csr_matrix((rns.rand(n_users, n_items) > 0.9).astype(np.float64)), n_items)
    want = [Metrics(n_items) for _ in CUTOFFS]
    for b in range(0, n_users, 128):
        e = min(b + 128, n_users)
        block = np.full((e - b, n_items), -np.inf, dtype=np.float32)
        block[:, :n_scored] = A[b:e] @ B.T
        for total, part in zip(want, core.get_metrics_masked(block, mask, b, CUTOFFS, b, 1, True)):
            total.merge(part)
    got = core.get_metrics_factors_scored(A, B, 0, n_users, mask, 0, CUTOFFS, 0, True, n_scored=n_scored)
    assert_equal(got, want, "one call", same_sums=True)
    assert all(m.item_cnt[n_scored:].sum() == 0 for m in got) and got[0].valid_user > 0
    first = core.get_metrics_factors_scored(A[:256], B, 0, 256, mask, 0, CUTOFFS, 0, True, n_scored=n_scored)
    both = core.get_metrics_factors_scored(A[256:], B, 0, n_users - 256, mask, 256, CUTOFFS, 256, True,
                                           n_scored=n_scored, running=first)
    assert_equal(both, want, "two calls", same_sums=True)


def test_argument_errors_of_the_scored_calls():
    rns = np.random.RandomState(3)
    U, I, k = 50, 40, 8
    core = EvaluatorCore(sps.csr_matrix((rns.rand(U, I) > 0.9).astype(np.float64)), [])
    X = sps.csr_matrix((rns.rand(U, 30) > 0.8).astype(np.float64))
    A, B = rns.randn(U, k).astype(np.float32), rns.randn(30, k).astype(np.float32)
    W = rns.randn(30, 30).astype(np.float32)
    factors = lambda B_=B, n=30: core.get_metrics_factors_scored(A, B_, 0, U, None, 0, [5], 0, n_scored=n)  # noqa: E731
    assert factors()[0].total_user == U
    for n in (0, -1, I + 1):
        with pytest.raises(ValueError, match="n_scored must lie in"):
            factors(n=n)
        with pytest.raises(ValueError, match="n_scored must lie in"):
            core.get_metrics_dense_similarity_scored(X, W, 0, U, None, 0, [5], 0, n_scored=n)
        with pytest.raises(ValueError, match="n_scored must lie in"):
            core.get_metrics_similarity_scored(X, sps.csr_matrix(W.astype(np.float64)), 0, U, None, 0, [5], 0, n_scored=n)
    for wrong in (B[:-1].copy(), np.zeros((I, k), dtype=np.float32)):  # an item table of the wrong height
        with pytest.raises(ValueError, match="item_factors must be n_scored"):
            factors(B_=wrong)
    with pytest.raises(ValueError, match="W must be X.shape\\[1\\] x n_scored"):
        core.get_metrics_dense_similarity_scored(X, W[:, :-1].copy(), 0, U, None, 0, [5], 0, n_scored=30)
    with pytest.raises(ValueError, match="one Metrics per cutoff"):
        core.get_metrics_factors_scored(A, B, 0, U, None, 0, [5, 10], 0, n_scored=30, running=[Metrics(I)])
    # the library's own check, reached without the Python one
    import ctypes as C

    from irspack_amd import _lib
    st, cnt, cut = (_lib.MetricsStruct * 1)(), np.zeros(I, dtype=np.int64), np.array([5], dtype=np.int64)
    f = lambda a: _lib.ptr(a, C.c_float)  # noqa: E731
    for n in (0, I + 1):
        assert _lib.lib().irs_eval_get_metrics_factors_scored(
            core._h, 0, U, U, k, f(A), f(B), n, None, None, None, 1, _lib.ptr(cut, C.c_int64), 0, 0, st,
            _lib.ptr(cnt, C.c_int64)) == 1
        assert "n_scored must lie in 1 .. n_items." in _lib.lib().irs_last_error().decode()
    assert factors()[0].total_user == U  # and the evaluator still works


# ------------------------------------------------------------------------------------- 4. the fold-in, parity
@pytest.mark.parametrize("rows", [1, 129])
@pytest.mark.parametrize("k", [1, 32, 67])
def test_truncated_svd_fold_in_against_the_float64_product(rows, k):
    """``|z - Z64| <= 2^-24 |Z64| + nnz_row 2^-52 (|X| @ |C|.T)`` per element: one float32 rounding plus the worst
    case of a double sum.  Row 0 stores every column (3,000 entries: three segments of the product kernel, so the
    split-row reduce runs), row 1 none; two calls give equal bytes."""
    I = 3000
    rns = np.random.RandomState(1000 * rows + k)
    dense = (rns.rand(rows, I) < 0.03) * rns.randint(1, 25, (rows, I)) / 8.0  # float32 values that are not all 1
    dense[0] = rns.randint(1, 25, I) / 8.0
    if rows > 1:
        dense[1] = 0.0
    X = sps.csr_matrix(dense)
    C_ = rns.randn(k, I).astype(np.float32)
    z = truncated_svd_transform(X, C_)
    assert z.shape == (rows, k) and z.dtype == np.float32
    Z64 = X @ C_.T.astype(np.float64)
    nnz_row = np.diff(X.indptr)[:, None]
    assert nnz_row[0, 0] == I and (rows == 1 or nnz_row[1, 0] == 0)
    bound = 2.0 ** -24 * np.abs(Z64) + nnz_row * 2.0 ** -52 * (abs(X) @ np.abs(C_.T.astype(np.float64)))
    excess = np.abs(z.astype(np.float64) - Z64) - bound
    print(f"rows={rows} k={k}: largest error / bound = {np.max(np.abs(z - Z64) / np.maximum(bound, 1e-300)):.3f}")
    assert (excess <= 0).all(), float(excess.max())
    if rows > 1:
        assert not z[1].any()
    assert z.tobytes() == truncated_svd_transform(X, C_).tobytes()
    # the storage order of a row does not matter: the call takes canonical rows
    indices, data = X.indices.copy(), X.data.copy()
    for b, e in zip(X.indptr[:-1], X.indptr[1:]):
        order = b + rns.permutation(e - b)
        indices[b:e], data[b:e] = X.indices[order], X.data[order]
    shuffled = sps.csr_matrix((data, indices, X.indptr.copy()), shape=X.shape)
    assert not shuffled.has_sorted_indices and truncated_svd_transform(shuffled, C_).tobytes() == z.tobytes()


# ------------------------------------------------------------------------- 5. real fits on the ML-100K shape
_ml100k = {}


def ml100k_cold():
    """the first 700 users train the model; the other 243 are cold: their input and ground truth"""
    if not _ml100k:
        X = sps.csr_matrix(make_interactions("ml100k"), dtype=np.float64)
        cold, truth = holdout_split(X[700:])
        _ml100k.update(train=X[:700], cold=cold, truth=truth)
    return _ml100k["train"], _ml100k["cold"], _ml100k["truth"]


def near_tied(Z, Ct, seen, terms, depth=22, columns=slice(None)):
    """the rule of test_gpu_evaluator_models.without_near_ties with the bound's factor as an argument: a user is
    near-tied when the float64 scores ``Z @ Ct`` (seen items removed; ranked among ``columns``) hold two adjacent
    scores among the top ``depth`` closer than ``terms 2^-24 max_j sum_i |z_ui c_ij|``"""
    Z, Ct = Z.astype(np.float64), Ct.astype(np.float64)
    S = Z @ Ct
    bound = terms * 2.0 ** -24 * (np.abs(Z) @ np.abs(Ct)).max(axis=1)
    S[seen.nonzero()] = -np.inf
    top = -np.sort(-S[:, columns], axis=1)[:, :depth]
    with np.errstate(invalid="ignore"):
        gaps = top[:, :-1] - top[:, 1:]
    gaps[~np.isfinite(gaps)] = np.inf
    return gaps.min(axis=1) < bound


def without_near_ties(Z, Ct, seen, truth, terms, also=None):
    """the ground truth with the rows of the near-tied users emptied - they leave BOTH evaluations and count in
    ``total_user`` only - and the share removed (``truth`` may be wider than the scored columns: the columns behind
    them are never ranked; ``also``: users that leave for a reason of the caller's)"""
    near = near_tied(Z, Ct, seen, terms)
    if also is not None:
        near = near | also
    gt = sps.lil_matrix(truth)
    for u in np.flatnonzero(near):
        gt.rows[u], gt.data[u] = [], []
    return sps.csr_matrix(gt), float(near.mean())


@pytest.mark.parametrize("kind", ["truncsvd", "nmf", "ials", "multvae"])
def test_fitted_factor_models(kind):
    """Float32 scores depend on the order of their sums, so users whose ranking could turn on it leave the ground
    truth before BOTH evaluations - at most 5 % of the cold users, a condition on the fit (change the seed or ``k``,
    never the cap).  The bound is ``4 k 2^-24 max_j sum |z c|``, and ``(4 k + 2) 2^-24 ...`` for the truncated SVD,
    whose device fold-in differs from the host's float64 one by one float32 rounding per factor."""
    from irspack_amd.recommenders import IALSRecommender, MultVAERecommender, NMFRecommender, TruncatedSVDRecommender

    train, cold, truth = ml100k_cold()
    if kind == "truncsvd":
        model = TruncatedSVDRecommender(train, n_components=32).learn()
        Z, Ct, terms = model.decomposer.transform(cold), model.decomposer.components_, 4 * 32 + 2
    elif kind == "nmf":
        model = NMFRecommender(train, n_components=32).learn()
        Z, Ct, terms = model.nmf_model.transform(cold), model.H, 4 * 32
    elif kind == "ials":
        model = IALSRecommender(train, n_components=32, alpha0=0.1, reg=1e-2, train_epochs=5,
                                solver_type="CHOLESKY").learn()
        Z, Ct, terms = model.compute_user_embedding(cold), model.get_item_embedding().T, 4 * 32
    else:
        model = MultVAERecommender(train, train_epochs=10, enc_hidden_dims=64, dec_hidden_dims=8, dim_z=16,
                                   minibatch_size=100, learning_rate=1e-2).learn()
        Z, Ct, terms = model.profile_factors(cold), model.factor_tables()[1], 4 * (8 + 2)
    gt, share = without_near_ties(Z, Ct, cold, truth, terms)
    print(f"{kind}: near-tied cold users removed: {share:.4f}")
    assert share <= 0.05
    want = compare(model, "factors", True, kind, cold, gt, mb_size=128)
    assert want[0].valid_user > 200
    compare(model, "factors", True, kind + " own mask", cold, gt, mb_size=128, recall_with_cutoff=True,
            masked_interactions=sps.csr_matrix((np.random.RandomState(9).rand(*cold.shape) > 0.9).astype(np.float64)))


def test_fold_in_chunks_continue_the_sums(monkeypatch):
    """Two fold-ins of 128 and 115 users instead of one of 243: the second call continues the sums of the first, so
    the float64 sums stay the block loop's at ``mb_size=128`` to the last bit."""
    from irspack_amd.recommenders import NMFRecommender

    train, cold, truth = ml100k_cold()
    model = NMFRecommender(train, n_components=32).learn()
    gt, share = without_near_ties(model.nmf_model.transform(cold), model.H, cold, truth, 4 * 32)
    monkeypatch.setattr(EvaluatorWithColdUser, "fold_in_rows", 128)
    compare(model, "factors", True, "two fold-ins", cold, gt, mb_size=128)


# ------------------------------------------------------- 6. iALS with item features and feature-only items
def test_ials_with_item_features_scores_the_feature_only_items():
    from irspack_amd.recommenders import IALSRecommender

    rns = np.random.RandomState(6)
    U, n_warm, n_cold, K = 300, 120, 9, 16
    X = sps.csr_matrix((rns.rand(U, n_warm) >= 0.85).astype(np.float64))
    features = rns.randn(n_warm + n_cold, 6).astype(np.float32)
    cold, truth, own_mask, _ = cold_problem(rns, 60, n_warm, n_cold, 0.15)
    args = dict(n_components=K, alpha0=0.1, reg=1e-2, train_epochs=3, solver_type="CHOLESKY")
    aware = IALSRecommender(X, item_features=features[:n_warm], lambda_item_feature=1.0, **args).learn()
    plain = IALSRecommender(X, **args).learn()
    for model, n_scored in ((aware, n_warm + n_cold), (plain, n_warm)):
        Z = model.compute_user_embedding(cold)
        items = model.get_item_embedding()
        if n_scored > n_warm:
            items = np.concatenate([items, model.compute_item_embedding_from_features(features[n_warm:])], axis=0)
        # (the near-tie rule over the columns the model scores; the mask is the cold users' own input)
        seen = sps.csr_matrix((cold.data, cold.indices, cold.indptr), shape=(60, n_scored))
        # (the last variant ranks the feature-only items alone: near ties among them count too)
        among_cold = near_tied(Z, items.T, seen, 4 * K, columns=slice(n_warm, None)) if n_scored > n_warm else None
        gt, share = without_near_ties(Z, items.T, seen, truth, 4 * K, also=among_cold)
        print(f"n_scored={n_scored}: near-tied cold users removed: {share:.4f}")
        assert share <= 0.05
        only_cold = dict(recommendable_items=list(range(n_warm, n_warm + n_cold)))
        for what, kw in (("default mask", {}), ("own mask", dict(masked_interactions=own_mask, recall_with_cutoff=True)),
                         ("the feature-only items alone", only_cold)):
            want = compare(model, "factors", True, f"n_scored={n_scored} {what}", cold, gt,
                           cold_item_features=features[n_warm:], mb_size=128, **kw)
        # ranked alone, the nine items fill the list of every user with a ground truth when the model scores them,
        # and none when they stay at -inf
        filled = [m.valid_user * min(c, n_cold) * (n_scored > n_warm) for m, c in zip(want, CUTOFFS)]
        assert [int(m.item_cnt.sum()) for m in want] == filled and want[0].valid_user > 40


# -------------------------------------------------------------------------------------------- 7. fallbacks
def test_fallbacks_to_the_block_loop():
    from irspack_amd.recommenders import BPRFMRecommender, CosineKNNRecommender

    model = knn_model(2040)
    rns = np.random.RandomState(8)
    cold, truth, _, _ = cold_problem(rns, 150, 2040, 0, 0.02)
    # a subclass with cold-user scores of its own
    own = copy.copy(model)
    own.__class__ = type("OwnScores", (CosineKNNRecommender,), {
        "get_score_cold_user": lambda self, X: CosineKNNRecommender.get_score_cold_user(self, X)})
    fused, plain = EvaluatorWithColdUser(cold, truth), EvaluatorWithColdUser(cold, truth, fused=False)
    assert fused._device_path(own) == "blocks" and fused._device_path(model) == "similarity"
    assert_equal(metrics_of(fused, own, CUTOFFS), metrics_of(plain, model, CUTOFFS), "own scores")
    # a profile row that stores a column twice
    indptr, indices = cold.indptr.copy(), cold.indices.copy()
    row = int(np.flatnonzero(np.diff(indptr) >= 2)[0])
    indices[indptr[row] + 1] = indices[indptr[row]]
    twice = sps.csr_matrix((cold.data.copy(), indices, indptr), shape=cold.shape)
    dup, dup_plain = EvaluatorWithColdUser(twice, truth), EvaluatorWithColdUser(twice, truth, fused=False)
    assert dup._device_path(model) == "blocks"
    assert_equal(metrics_of(dup, model, CUTOFFS), metrics_of(dup_plain, model, CUTOFFS), "a duplicated column")
    # a model without cold-user scores raises from the block loop as before
    bpr = BPRFMRecommender(sps.csr_matrix((rns.rand(60, 2040) < 0.02).astype(np.float64)), n_components=4)
    with pytest.raises(NotImplementedError, match="get_score_cold_user is not implemented"):
        fused.get_scores(bpr, CUTOFFS)
    # fused=False runs the model's own scorer: the trap's error
    trap(model)
    try:
        with pytest.raises(AssertionError, match="host cold-user scores ran"):
            plain.get_scores(model, CUTOFFS)
        fused.get_scores(model, CUTOFFS)
    finally:
        untrap(model)
