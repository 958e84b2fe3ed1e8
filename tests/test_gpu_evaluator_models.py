"""``Evaluator`` on the device for the models that used to take the host block loop: dense item weights
(DenseSLIM / EASE, EDLAE: ``irs_eval_get_metrics_dense_similarity``), SLIM's float32 sparse weights (cast to
float64, ``irs_eval_get_metrics_similarity``) and factor models (truncated SVD, NMF:
``irs_eval_get_metrics_factors``).

The comparison target is the same evaluator's block loop - the model's own host scores, uploaded, masked and
ranked per 128 users (``fused=False``).  "Equal" means: ``item_cnt``, ``valid_user`` and ``total_user`` identical,
the five float64 sums to ``rel=1e-12`` (sums of identical terms in another order)."""
import numpy as np
import pytest
import scipy.sparse as sps

from irspack_amd.evaluation import Evaluator
from irspack_amd.evaluation._core_evaluator import EvaluatorCore, MaskRows, Metrics
from irspack_amd.synthetic import holdout_split, make_interactions

pytestmark = pytest.mark.gpu

SUMS = ("hit", "recall", "ndcg", "precision", "map")


def assert_equal(got, want, what="", same_sums=False):
    """``same_sums``: the float64 sums to the last bit as well - the device calls add the users' terms in the
    order of the host loop at its default ``mb_size`` (128-user blocks merged in sequence)"""
    assert len(got) == len(want) and len(got) > 0
    for c, (a, b) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(a.item_cnt, b.item_cnt, err_msg=f"{what} cutoff #{c}")
        assert (a.valid_user, a.total_user) == (b.valid_user, b.total_user), (what, c)
        for name in SUMS:
            assert getattr(a, name) == pytest.approx(getattr(b, name), rel=1e-12, abs=0.0), (what, c, name)
            if same_sums:
                assert getattr(a, name) == getattr(b, name), (what, c, name)


def block_loop(core, score_block, begin, end, mask, mask_begin, cutoffs, offset, rwc, mb=128):
    """what ``Evaluator(fused=False)`` does: host scores of ``mb`` users at a time, masked and ranked per block,
    the blocks merged in order"""
    totals = [Metrics(core.n_items) for _ in cutoffs]
    for b in range(begin, end, mb):
        e = min(b + mb, end)
        block = np.ascontiguousarray(score_block(b, e))
        part = core.get_metrics_masked(block, mask, mask_begin + (b - begin), cutoffs, offset + (b - begin), 1, rwc)
        for t, p in zip(totals, part):
            t.merge(p)
    return totals


def metrics_of(evaluator, model, cutoffs):
    """the ``Metrics`` per cutoff behind ``evaluator.get_scores(model, cutoffs)``"""
    seen, summarise = [], evaluator._with_coverage
    evaluator._with_coverage = lambda m: (seen.append(m), summarise(m))[1]
    try:
        evaluator.get_scores(model, cutoffs)
    finally:
        del evaluator._with_coverage
    return seen


def trap(model):
    def get_score_block(begin, end):
        raise AssertionError("the host block loop ran")

    model.get_score_block = get_score_block  # (on the instance: the class's scoring is what it was)


# ------------------------------------------------------------------------------------- 1. the dense kernel, exact
N_USERS = 200


def unsorted_profiles(I, rns):
    """float64 CSR built from (data, indices, indptr): non-binary values, every row in shuffled storage order;
    row lengths at the edges of the kernel's loops (0, 1, the 64-entry fetch, the in-flight batch of 8) and,
    where the width allows it, one row of 1,000 entries.  A row longer than ``I`` repeats columns (legal CSR:
    scipy and the kernel add the entries one by one)."""
    lengths = [0, 1, 64, 65, 130, 7, 8, 9, 63, 128] + [1000 if I > 1000 else 16]
    lengths += list(rns.randint(0, min(I, 40) + 1, N_USERS - len(lengths)))
    rows = []
    for n in lengths:
        rows.append(rns.choice(I, n, replace=False) if n <= I else rns.randint(0, I, n))
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    indices = np.concatenate(rows).astype(np.int32)
    data = rns.uniform(0.5, 3.0, indices.size) * rns.choice([-1.0, 1.0], indices.size)
    X = sps.csr_matrix((data, indices, indptr), shape=(N_USERS, I))
    return X, indices.copy(), data.copy()


_dense_problems = {}


def dense_problem(I):
    if I not in _dense_problems:
        rns = np.random.RandomState(1000 + I)
        X, idx, dat = unsorted_profiles(I, rns)
        W = rns.randn(I, I).astype(np.float32)
        gt = sps.csr_matrix((rns.rand(N_USERS, I) < max(0.02, 1.5 / I)).astype(np.float64))
        M = sps.csr_matrix((rns.rand(N_USERS, I) > 0.9).astype(np.float64))
        _dense_problems[I] = (X, idx, dat, W, gt, M)
    return _dense_problems[I]


def mask_variant(kind, X, M, I):
    """(begin, offset, mask, mask_begin): an explicit mask indexed like the ground truth; a window of the users
    from 37 masked with the profiles' own rows; no mask"""
    if kind == "explicit":
        return 0, 0, MaskRows(M, I), 0
    if kind == "offset":
        return 37, 37, MaskRows(X, I), 37
    return 0, 0, None, 0


@pytest.mark.parametrize("kind, rwc, restricted", [("explicit", False, False), ("offset", True, False),
                                                   ("none", False, False), ("none", True, False),
                                                   ("explicit", True, True), ("offset", False, True)])
@pytest.mark.parametrize("I", [1, 63, 257, 300, 2049])
def test_dense_kernel_is_the_host_product(I, kind, rwc, restricted):
    """``get_metrics_dense_similarity`` on a random float32 ``W``: the device block is ``X[b:e].dot(W)`` bit for
    bit (storage order of the profile, product and sum rounded separately), so the ranking - full of
    comparisons of float64 scores - equals the block loop's.  ``I % 4 != 0``, ``I`` below one 256-column strip
    and one past a strip boundary; the profile matrix is read as it is and left as it is."""
    X, idx, dat, W, gt, M = dense_problem(I)
    cutoffs = [c for c in (1, 5, 20) if c <= I]
    allowed = [sorted(set(np.random.RandomState(5).randint(0, I, max(1, I // 2)).tolist()))] if restricted else []
    if restricted:
        cutoffs = [c for c in cutoffs if c <= len(allowed[0])] or [1]
    core = EvaluatorCore(gt, allowed)
    begin, offset, mask, mask_begin = mask_variant(kind, X, M, I)
    got = core.get_metrics_dense_similarity(X, W, begin, N_USERS, mask, mask_begin, cutoffs, offset, rwc)
    want = block_loop(core, lambda b, e: X[b:e].dot(W), begin, N_USERS, mask, mask_begin, cutoffs, offset, rwc)
    assert_equal(got, want, f"I={I} {kind}", same_sums=True)
    assert got[0].total_user == N_USERS - begin
    assert np.array_equal(X.indices, idx) and np.array_equal(X.data, dat)  # neither sorted nor rewritten


def test_dense_kernel_in_several_blocks_and_float64_weights(monkeypatch):
    X, _, _, W, gt, M = dense_problem(300)
    core = EvaluatorCore(gt, [])
    mask = MaskRows(M, 300)
    want = block_loop(core, lambda b, e: X[b:e].dot(W), 0, N_USERS, mask, 0, [1, 5, 20], 0, False)
    monkeypatch.setenv("IRSPACK_AMD_EVAL_SIM_BLOCK_ROWS", "17")
    assert_equal(core.get_metrics_dense_similarity(X, W, 0, N_USERS, mask, 0, [1, 5, 20], 0), want, "17-row blocks")
    W64 = np.random.RandomState(2).randn(300, 300)
    want = block_loop(core, lambda b, e: X[b:e].dot(W64), 0, N_USERS, mask, 0, [1, 5, 20], 0, False)
    assert_equal(core.get_metrics_dense_similarity(X, W64, 0, N_USERS, mask, 0, [1, 5, 20], 0), want, "float64 W")


# ------------------------------------------------------------------- 2. / 3. through the similarity recommenders
_split = {}


def split(shape):
    if shape not in _split:
        X = sps.csr_matrix(make_interactions(shape), dtype=np.float64)
        _split[shape] = holdout_split(X)
    return _split[shape]


def check_model_on_device(model, X_test, path, cutoffs=(5, 20)):
    cutoffs = list(cutoffs)
    same = path != "similarity"  # (the sparse call keeps the summation order it had: equal to rounding)
    fused, plain = Evaluator(X_test, cutoff=10), Evaluator(X_test, cutoff=10, fused=False)
    assert fused._device_path(model) == path and plain._device_path(model) == "blocks"
    want = metrics_of(plain, model, cutoffs)
    assert_equal(metrics_of(fused, model, cutoffs), want, path, same_sums=same)
    assert want[0].valid_user > 0
    # with a mask of its own, over a window of the users
    n = X_test.shape[0] - 21
    own = sps.csr_matrix((np.random.RandomState(9).rand(n, X_test.shape[1]) > 0.9).astype(np.float64))
    a = Evaluator(X_test[21:], offset=21, masked_interactions=own, recall_with_cutoff=True)
    b = Evaluator(X_test[21:], offset=21, masked_interactions=own, recall_with_cutoff=True, fused=False)
    assert_equal(metrics_of(a, model, cutoffs), metrics_of(b, model, cutoffs), path + " window", same_sums=same)
    trap(model)
    with pytest.raises(AssertionError, match="host block loop"):
        plain.get_scores(model, cutoffs)
    assert_equal(metrics_of(fused, model, cutoffs), want, path + " without the host scores")


@pytest.mark.parametrize("kind", ["dense_slim", "edlae"])
def test_dense_recommenders_are_scored_on_the_device(kind):
    from irspack_amd.recommenders import DenseSLIMRecommender, EDLAERecommender

    X_train, X_test = split("tiny")
    model = (DenseSLIMRecommender(X_train, reg=5.0) if kind == "dense_slim"
             else EDLAERecommender(X_train, reg=2.0, dropout_p=0.2)).learn()
    assert isinstance(model.W, np.ndarray) and model.W.dtype == np.float32
    check_model_on_device(model, X_test, "dense_similarity")


def test_slim_is_scored_on_the_device():
    from irspack_amd.recommenders import SLIMRecommender

    X_train, X_test = split("tiny")
    model = SLIMRecommender(X_train, alpha=0.01, l1_ratio=0.01, n_iter=10).learn()
    assert sps.issparse(model.W) and model.W.dtype == np.float32 and model.W.nnz > 0
    W = model.W.copy()
    check_model_on_device(model, X_test, "similarity")
    assert model.W.format == W.format and np.array_equal(model.W.indices, W.indices) and \
        np.array_equal(model.W.data, W.data)  # the model's weights are as the fit left them


# ---------------------------------------------------------------------- 4. the factor kernel, exact on integers
FACTOR_USERS = 300
FACTOR_VARIANTS = [("explicit", False, False), ("offset", True, False), ("none", False, True), ("offset", False, True),
                   ("explicit", True, True)]
_factor_items = {}


def factor_items(I):
    if I not in _factor_items:
        rns = np.random.RandomState(2000 + I)
        gt = sps.csr_matrix((rns.rand(FACTOR_USERS, I) < 0.03).astype(np.float64))
        X = sps.csr_matrix((rns.rand(FACTOR_USERS, I) > 0.85).astype(np.float64))
        M = sps.csr_matrix((rns.rand(FACTOR_USERS, I) > 0.9).astype(np.float64))
        _factor_items[I] = (gt, X, M)
    return _factor_items[I]


@pytest.mark.parametrize("I", [63, 300, 1000])
@pytest.mark.parametrize("k", [1, 31, 32, 33, 64, 100, 576])
def test_factor_kernel_on_integer_factors(k, I, monkeypatch):
    """Factors drawn as integers in [-8, 8], stored as float32: every product and partial sum is an integer
    below 576 * 64 < 2^24, so every summation order gives the same float32 and the device block equals
    ``A[b:e] @ B.T`` exactly; the rows are full of exact ties (lower index first).  Mask, offset, cutoff and
    candidate variants as for the dense kernel, one per (k, I); k = 64 also in two device blocks."""
    gt, X, M = factor_items(I)
    rns = np.random.RandomState(k * 7 + I)
    A = rns.randint(-8, 9, (FACTOR_USERS, k)).astype(np.float32)
    B = rns.randint(-8, 9, (I, k)).astype(np.float32)
    kind, rwc, restricted = FACTOR_VARIANTS[(k + I) % len(FACTOR_VARIANTS)]
    allowed = [sorted(set(rns.randint(0, I, I // 2).tolist()))] if restricted else []
    cutoffs = [1, 5, 20]
    core = EvaluatorCore(gt, allowed)
    begin, offset, mask, mask_begin = mask_variant(kind, X, M, I)
    want = block_loop(core, lambda b, e: A[b:e] @ B.T, begin, FACTOR_USERS, mask, mask_begin, cutoffs, offset, rwc)
    assert want[0].total_user == FACTOR_USERS - begin
    if k == 64:
        monkeypatch.setenv("IRSPACK_AMD_EVAL_BLOCK", "256")
    got = core.get_metrics_factors(A, B, begin, FACTOR_USERS, mask, mask_begin, cutoffs, offset, rwc)
    assert_equal(got, want, f"k={k} I={I} {kind}", same_sums=True)


# -------------------------------------------------------------------------------- 5. the factor path on real fits
def without_near_ties(model_users, model_items, X_train, X_test, k, depth=22):
    """the ground truth with the rows of near-tied users emptied (they count in ``total_user`` only): a user is
    near-tied when, in the float64 product of the fitted factors with the seen items removed, two adjacent
    scores among the top ``depth`` differ by less than 4 k 2^-24 max_j sum_i |z_ui c_ij| - twice the
    worst-case float32 dot-product error of two scores.  Returns the ground truth and the share removed."""
    Z, Ct = model_users.astype(np.float64), model_items.astype(np.float64)  # (U, k), (k, I)
    S = Z @ Ct
    bound = 4.0 * k * 2.0 ** -24 * (np.abs(Z) @ np.abs(Ct)).max(axis=1)
    S[X_train.nonzero()] = -np.inf
    top = -np.sort(-S, axis=1)[:, :depth]
    with np.errstate(invalid="ignore"):
        gaps = top[:, :-1] - top[:, 1:]
    gaps[~np.isfinite(gaps)] = np.inf
    near = gaps.min(axis=1) < bound
    gt = sps.lil_matrix(X_test)
    for u in np.flatnonzero(near):
        gt.rows[u], gt.data[u] = [], []
    return sps.csr_matrix(gt), float(near.mean())


@pytest.mark.parametrize("kind", ["truncsvd", "nmf"])
def test_factor_recommenders_are_scored_on_the_device(kind):
    """Float32 scores depend on the order of the sum, so users whose ranking could turn on it leave the ground
    truth before BOTH evaluations (at most 5 % of them: scikit-learn's fits at this shape lose 2.5 % / 2.2 %);
    on the others the device path equals the block loop, with and without the host scores."""
    from irspack_amd.recommenders import NMFRecommender, TruncatedSVDRecommender

    X_train, X_test = split("ml100k")
    k = 32
    if kind == "truncsvd":
        model = TruncatedSVDRecommender(X_train, n_components=k).learn()
        users, items = model.z, model.decomposer.components_
    else:
        model = NMFRecommender(X_train, n_components=k).learn()
        users, items = model.W, model.H
    gt, share = without_near_ties(users, items, model.X_train_all, X_test, k)
    print(f"{kind}: near-tied users removed: {share:.4f}")
    assert share <= 0.05
    check_model_on_device(model, gt, "factors")


# ---------------------------------------------------------------------------------------------- 6. validation
def test_argument_errors_of_both_calls():
    rns = np.random.RandomState(3)
    U, I, k = 50, 40, 8
    gt = sps.csr_matrix((rns.rand(U, I) > 0.9).astype(np.float64))
    X = sps.csr_matrix((rns.rand(U, I) > 0.8).astype(np.float64))
    W = rns.randn(I, I).astype(np.float32)
    A, B = rns.randn(U, k).astype(np.float32), rns.randn(I, k).astype(np.float32)
    core = EvaluatorCore(gt, [])
    dense = lambda X_=X, W_=W, end=U, cut=(5,): core.get_metrics_dense_similarity(X_, W_, 0, end, None, 0, list(cut), 0)
    factors = lambda A_=A, B_=B, end=U, cut=(5,): core.get_metrics_factors(A_, B_, 0, end, None, 0, list(cut), 0)
    assert dense()[0].total_user == U and factors()[0].total_user == U
    # a profile column out of range (never dereferenced: the host checks the rows it is about to upload)
    bad = sps.csr_matrix((X.data.copy(), X.indices.copy(), X.indptr.copy()), shape=X.shape)
    bad.indices[3] = I
    with pytest.raises(ValueError, match="column index out of range"):
        dense(X_=bad)
    bad.indices[3] = -1
    with pytest.raises(ValueError, match="column index out of range"):
        dense(X_=bad)
    # W / the item factors of the wrong shape, layout or type
    for wrong in (W[:, :-1].copy(), W[:-1].copy(), np.asfortranarray(W), W.astype(np.float16), W.ravel()):
        with pytest.raises(ValueError, match="W must be"):
            dense(W_=wrong)
    for wrong in (B[:-1].copy(), B[:, :-1].copy()):
        with pytest.raises(ValueError, match="item_factors"):
            factors(B_=wrong)
    # k < 1 and k above what the call takes
    with pytest.raises(ValueError, match="number of factors"):
        factors(A_=np.zeros((U, 0), dtype=np.float32), B_=np.zeros((I, 0), dtype=np.float32))
    with pytest.raises(ValueError, match="number of factors"):
        factors(A_=np.zeros((U, 577), dtype=np.float32), B_=np.zeros((I, 577), dtype=np.float32))
    # users past the model's
    for call in (dense, factors):
        with pytest.raises(ValueError, match="out of bounds"):
            call(end=U + 1)
        with pytest.raises(ValueError, match="cutoff"):
            call(cut=(0,))
    # a mask column out of range that reaches the library (MaskRows checks its own)
    m = MaskRows(X, I)
    m.indices = m.indices.copy()
    m.indices[0] = I + 5
    with pytest.raises(ValueError, match="mask column index out of range"):
        core.get_metrics_dense_similarity(X, W, 0, U, m, 0, [5], 0)
    with pytest.raises(ValueError, match="mask column index out of range"):
        core.get_metrics_factors(A, B, 0, U, m, 0, [5], 0)
    # and the evaluator still works
    assert dense()[0].total_user == U and factors()[0].total_user == U
