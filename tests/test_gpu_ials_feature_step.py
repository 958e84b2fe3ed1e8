"""The native feature-aware epoch (irs_ials_feature_step: prior -> per-row solve -> ridge update of
the feature weights, all on the device) against a float64 numpy restatement of the reference's
IALSTrainer::step (hpp:758-789) at ML-100K size, and its behaviour: warm-up, errors,
reproducibility, the host-ridge A/B path, weight accessors, pickle and the C ABI on its own.

The float64 restatement starts from the trainer's own factors and weights, read back before the
step.  Each half step is judged on its own: the item half and both ridge updates take the GPU's
output of the step before as their input.  ``oracle32`` is the private host-ridge path
(``IALSTrainer._step_host_ridge``) run from the same state.
"""
import ctypes as C
import pickle

import numpy as np
import pytest
import scipy.sparse as sps

from conftest import assert_float64_bar, row_rel_err

from irspack_amd import _lib
from irspack_amd.recommenders._ials_core import (IALSModelConfigBuilder, IALSSolverConfigBuilder,
                                                  IALSTrainer, LossType, SolverType)
from irspack_amd.synthetic import make_interactions

pytestmark = pytest.mark.gpu

ALPHA0, REG, NU, LAM_U, LAM_I = 0.1, 0.05, 1.0, 0.5, 0.3


def config(K, loss=LossType.ORIGINAL, warmup=0, seed=1, alpha0=ALPHA0, reg=REG, nu=NU, lam_u=LAM_U,
           lam_i=LAM_I):
    return (IALSModelConfigBuilder().set_K(K).set_alpha0(alpha0).set_reg(reg).set_nu(nu)
            .set_init_stdev(0.1).set_random_seed(seed).set_loss_type(loss)
            .set_lambda_user_feature(lam_u).set_lambda_item_feature(lam_i)
            .set_feature_warmup_epochs(warmup).build())


def solver(kind, steps=3):
    return (IALSSolverConfigBuilder().set_n_threads(1).set_solver_type(SolverType[kind])
            .set_max_cg_steps(steps).build())


def one_hot(n, f, seed):
    rng = np.random.default_rng(seed)
    return sps.csr_matrix((np.ones(n, np.float32), (np.arange(n), rng.integers(0, f, n))), shape=(n, f))


def ml100k_features(n_users, n_items):
    """users: 32 dense + 200 one-hot columns; items: 20 one-hot columns"""
    rng = np.random.default_rng(7)
    dense = sps.csr_matrix(rng.standard_normal((n_users, 32)).astype(np.float32) * 0.3)
    uf = sps.hstack([dense, one_hot(n_users, 200, 8)], format="csr").astype(np.float32)
    return uf, one_hot(n_items, 20, 9)


def row_reg(nnz, n_other, cfg):
    """Solver::compute_reg in float32, like the library"""
    base = np.float32(cfg.alpha0) * np.float32(n_other) + nnz.astype(np.float32)
    return (np.float32(cfg.reg) * np.power(base, np.float32(cfg.nu), dtype=np.float32)).astype(np.float64)


def half_f64(X, other, start, prior, cfg, kind, max_cg):
    """step_cholesky_with_prior (hpp:333-385) / step_cg with the prior (hpp:170-265) in float64"""
    X = sps.csr_matrix(X)
    K = other.shape[1]
    P = cfg.alpha0 * other.T @ other
    bias = 0.0 if cfg.loss_type == LossType.IALSPP else cfg.alpha0
    regs = row_reg(np.diff(X.indptr), other.shape[0], cfg)
    out = np.empty_like(start)
    steps = K if max_cg == 0 else max_cg
    for r in range(X.shape[0]):
        idx, val = X.indices[X.indptr[r]:X.indptr[r + 1]], X.data[X.indptr[r]:X.indptr[r + 1]].astype(np.float64)
        Y = other[idx]
        A = P + regs[r] * np.eye(K) + Y.T @ (val[:, None] * Y)
        b = regs[r] * prior[r] + Y.T @ (bias + val)
        if kind == "CHOLESKY":
            out[r] = np.linalg.solve(A, b)
            continue
        x = start[r].copy()
        res = b - A @ x
        p = res.copy()
        for _ in range(steps):
            r2 = res @ res
            if r2 <= 1e-20:
                break
            Ap = A @ p
            alpha = r2 / (p @ Ap)
            x += alpha * p
            res -= alpha * Ap
            if res @ res <= 1e-20:
                break
            p = res + (res @ res) / r2 * p
        out[r] = x
    return out


def ridge_f64(F, w, lam, factor):
    """update_feature_weight (hpp:1082-1171): (F^T D F + lambda I)^-1 F^T (D factor)"""
    F = np.asarray(F.todense() if sps.issparse(F) else F, dtype=np.float64)
    G = F.T @ (w[:, None] * F) + lam * np.eye(F.shape[1])
    return np.linalg.solve(G, F.T @ (w[:, None] * factor))


def parity_case(X, uf, itf, cfg, kind, max_cg=3, W_scale=0.05, name=""):
    """one native epoch vs float64 restatement vs the host-ridge path, all from the same state"""
    sc = solver(kind, max_cg)
    a = IALSTrainer(cfg, X, uf, itf)
    b = IALSTrainer(cfg, X, uf, itf)
    rng = np.random.default_rng(3)
    K = cfg.K
    W0 = [None if f is None else (rng.standard_normal((f.shape[1], K)) * W_scale).astype(np.float32)
          for f in (uf, itf)]
    for t in (a, b):
        if W0[0] is not None:
            t.user_feature_weight = W0[0]
        if W0[1] is not None:
            t.item_feature_weight = W0[1]
    user0, item0 = a.user.astype(np.float64), a.item.astype(np.float64)
    np.testing.assert_array_equal(b.user, a.user)
    a.step(sc)
    b._step_host_ridge(sc)
    Xc = sps.csr_matrix(X)
    g_user, g_item = a.user.astype(np.float64), a.item.astype(np.float64)
    truncated = kind == "CG"
    feats = (uf, itf)
    for side, (Xs, other, start, got, orc) in enumerate(
            ((Xc, item0, user0, g_user, b.user), (Xc.T.tocsr(), g_user, item0, g_item, b.item))):
        F = feats[side]
        prior = np.zeros_like(start) if F is None else np.asarray(F @ W0[side].astype(np.float64))
        ref = half_f64(Xs, other, start, prior, cfg, kind, max_cg)
        assert_float64_bar(got, orc, ref, f"{name} side {side} {kind}", test="feature_step",
                           truncated=truncated)
        if F is None:
            continue
        w = row_reg(np.diff(Xs.indptr), other.shape[0], cfg)
        lam = cfg.lambda_user_feature if side == 0 else cfg.lambda_item_feature
        W_ref = ridge_f64(F, w, lam, got)
        W_gpu = a.user_feature_weight if side == 0 else a.item_feature_weight
        W_orc = b.user_feature_weight if side == 0 else b.item_feature_weight
        assert_float64_bar(W_gpu, W_orc, W_ref, f"{name} W side {side} {kind}", test="feature_step_W")
    return a, b


@pytest.fixture(scope="module")
def ml100k():
    X = make_interactions("ml100k")
    return X, ml100k_features(*X.shape)


@pytest.mark.parametrize(("K", "kind"), [(64, "CHOLESKY"), (64, "CG"), (128, "CHOLESKY"), (128, "CG"),
                                         (256, "CHOLESKY"), (256, "CG")])
def test_ml100k_epoch_vs_float64(ml100k, K, kind):
    X, (uf, itf) = ml100k
    assert (X.data == 1).all()  # binary interactions: the unit / bf16x3 rank-update kernels at K = 64
    parity_case(X, uf, itf, config(K), kind, name=f"ml100k K={K}")


def test_split_rows_with_prior():
    """rows of more than 1,024 stored entries go through the split-row path; IALSPP loss (b = 0)"""
    rng = np.random.default_rng(11)
    n_users, n_items = 400, 3000
    X = sps.random(n_users, n_items, density=0.01, random_state=5, format="lil", dtype=np.float32)
    for u in range(6):  # long rows
        cols = rng.choice(n_items, 1100 + 300 * u, replace=False)
        X[u, cols] = 1.0
    X = sps.csr_matrix(X)
    X.data[:] = rng.uniform(0.5, 2.0, X.nnz).astype(np.float32)
    assert np.diff(X.indptr).max() > 1024
    uf = one_hot(n_users, 30, 1)
    itf = sps.csr_matrix(rng.standard_normal((n_items, 8)).astype(np.float32))
    parity_case(X, uf, itf, config(64, loss=LossType.IALSPP), "CHOLESKY", name="split rows")


@pytest.mark.parametrize(("fu", "fi"), [(1, 17), (17, 1)])
def test_feature_counts_off_the_tile(fu, fi):
    X = make_interactions("tiny")
    rng = np.random.default_rng(fu)
    uf = rng.standard_normal((X.shape[0], fu)).astype(np.float32)
    itf = sps.csr_matrix(rng.standard_normal((X.shape[1], fi)).astype(np.float32))
    parity_case(X, uf, itf, config(32), "CHOLESKY", name=f"F={fu}/{fi}")


def test_many_features_one_side_only(ml100k):
    """F = 1,100 (18 Cholesky / substitution blocks) on the users, no item features"""
    X, _ = ml100k
    uf = sps.hstack([one_hot(X.shape[0], 1000, 2), one_hot(X.shape[0], 100, 4)], format="csr")
    parity_case(X, uf, None, config(64), "CHOLESKY", W_scale=0.02, name="F=1100")


def _plain_step(t, sc):
    s = sc._struct()
    _lib.check(_lib.lib().irs_ials_step(t._h, C.byref(s)))


def test_warmup(ml100k):
    X, (uf, itf) = ml100k
    sc = solver("CHOLESKY")
    a = IALSTrainer(config(64, warmup=2), X, uf, itf)
    b = IALSTrainer(config(64, warmup=2), X, uf, itf)
    for _ in range(2):
        a.step(sc)
        _plain_step(b, sc)
    assert not a.user_feature_weight.any() and not a.item_feature_weight.any()
    np.testing.assert_array_equal(a.user, b.user)
    np.testing.assert_array_equal(a.item, b.item)
    a.step(sc)
    assert a.user_feature_weight.any() and a.item_feature_weight.any()


def test_errors_leave_a_working_trainer(ml100k):
    X, (uf, itf) = ml100k
    t = IALSTrainer(config(64), X, uf, itf)
    with pytest.raises(ValueError, match="does not support IALSPP"):
        t.step(IALSSolverConfigBuilder().set_solver_type(SolverType.IALSPP).build())
    t.step(solver("CHOLESKY"))
    assert np.isfinite(t.user).all() and t.user_feature_weight.any()
    # alpha0 = 0 and reg * 0^nu = 0: an empty row has no defined embedding (hpp:639-653)
    Xe = sps.csr_matrix(X)
    Xe = sps.vstack([Xe, sps.csr_matrix((1, X.shape[1]), dtype=np.float32)], format="csr")
    te = IALSTrainer(config(16, alpha0=0.0), Xe, one_hot(Xe.shape[0], 5, 1), None)
    with pytest.raises(ValueError, match="not uniquely defined for an empty interaction row"):
        te.step(solver("CHOLESKY"))
    _plain_step(te, solver("CG"))
    assert np.isfinite(te.item).all()


def _struct_config(K, lam_u, lam_i):
    return _lib.ModelConfigStruct(K, ALPHA0, REG, NU, 0.1, 1, 0, lam_u, lam_i, 0)


def _create(X, cfg):
    lib = _lib.lib()
    Xc, ip, ind, dat = _lib.csr_arrays(X, np.float32)
    h = C.c_void_p()
    _lib.check(lib.irs_ials_create(C.byref(cfg), C.c_int64(X.shape[0]), C.c_int64(X.shape[1]),
                                   _lib.ptr(ip, C.c_int64), _lib.ptr(ind, C.c_int32),
                                   _lib.ptr(dat, C.c_float), C.c_int32(_lib.default_device()), None,
                                   C.byref(h)))
    return h


def _set_features(h, side, F):
    Fc, fp, fi, fd = _lib.csr_arrays(sps.csr_matrix(F), np.float32)
    _lib.check(_lib.lib().irs_ials_set_features(h, C.c_int32(side), C.c_int64(F.shape[0]),
                                                C.c_int64(F.shape[1]), _lib.ptr(fp, C.c_int64),
                                                _lib.ptr(fi, C.c_int32), _lib.ptr(fd, C.c_float)))


def test_singular_ridge_raises_and_trainer_recovers():
    """lambda = 0 with a duplicated feature column and one that no row stores: F^T D F is singular
    (hpp:1104-1105).  (The empty column makes a pivot exactly 0; the duplicate alone leaves a
    rounding-noise pivot whose sign is chance, in float32 Eigen as here.)  The shim rejects
    lambda <= 0, so this goes through the C ABI."""
    X = make_interactions("tiny")
    lib = _lib.lib()
    h = _create(X, _struct_config(32, 0.0, 0.0))
    try:
        col = np.random.default_rng(0).standard_normal((X.shape[0], 1)).astype(np.float32)
        _set_features(h, 0, np.hstack([col, col, np.zeros_like(col)]))
        sc = solver("CHOLESKY")._struct()
        W0 = np.full((3, 32), 7.0, np.float32)
        _lib.check(lib.irs_ials_set_feature_weight(h, 0, _lib.ptr(W0, C.c_float), 3, 32))
        with pytest.raises(RuntimeError, match=r"^Feature ridge Cholesky decomposition failed\.$"):
            _lib.check(lib.irs_ials_feature_step(h, C.byref(sc)))
        W = np.empty((3, 32), np.float32)
        _lib.check(lib.irs_ials_get_feature_weight(h, 0, _lib.ptr(W, C.c_float)))
        np.testing.assert_array_equal(W, W0)  # the weights keep their values, like the reference's
        _lib.check(lib.irs_ials_step(h, C.byref(sc)))  # a valid call still works
    finally:
        lib.irs_ials_destroy(h)


def test_reproducible(ml100k):
    X, (uf, itf) = ml100k
    runs = []
    for _ in range(2):
        t = IALSTrainer(config(64), X, uf, itf)
        for _ in range(3):
            t.step(solver("CG"))
        runs.append((t.user, t.item, t.user_feature_weight, t.item_feature_weight))
    for x, y in zip(*runs):
        np.testing.assert_array_equal(x, y)


def test_native_vs_host_ridge_five_epochs(ml100k):
    X, (uf, itf) = ml100k
    a, b = IALSTrainer(config(64), X, uf, itf), IALSTrainer(config(64), X, uf, itf)
    sc = solver("CHOLESKY")
    for _ in range(5):
        a.step(sc)
        b._step_host_ridge(sc)
    assert row_rel_err(a.user, b.user) < 1e-3
    assert row_rel_err(a.item, b.item) < 1e-3
    assert row_rel_err(a.user_feature_weight, b.user_feature_weight) < 1e-3
    assert row_rel_err(a.item_feature_weight, b.item_feature_weight) < 1e-3


def test_set_weights_reach_the_step_and_pickle(ml100k):
    X, (uf, itf) = ml100k
    a, b = IALSTrainer(config(64), X, uf, itf), IALSTrainer(config(64), X, uf, itf)
    W = (np.random.default_rng(2).standard_normal((uf.shape[1], 64)) * 0.1).astype(np.float32)
    a.user_feature_weight = W
    np.testing.assert_array_equal(a.user_feature_weight, W)
    a.step(solver("CHOLESKY"))
    b.step(solver("CHOLESKY"))
    assert row_rel_err(a.user, b.user) > 1e-2  # the prior F @ W moved the users
    a.step(solver("CHOLESKY"))
    t2 = pickle.loads(pickle.dumps(a))
    np.testing.assert_array_equal(t2.user_feature_weight, a.user_feature_weight)
    np.testing.assert_array_equal(t2.item_feature_weight, a.item_feature_weight)
    np.testing.assert_array_equal(t2.transform_item_feature(itf), a.transform_item_feature(itf))


def test_recommender_learns_through_native_step(ml100k):
    from irspack_amd.recommenders import IALSRecommender

    X, (uf, _) = ml100k
    rec = IALSRecommender(X, n_components=32, alpha0=ALPHA0, reg=REG, nu=NU, solver_type="CHOLESKY",
                          loss_type="ORIGINAL", user_features=uf, lambda_user_feature=LAM_U,
                          train_epochs=4, random_seed=0).learn()
    core = rec.trainer_as_ials.core_trainer
    W = core.user_feature_weight
    assert W.shape == (uf.shape[1], 32) and W.any()
    # the weights are the ridge solution for the trainer's own user factors (last epoch)
    w = row_reg(np.diff(sps.csr_matrix(X).indptr), X.shape[1], config(32))
    want = ridge_f64(uf, w, LAM_U, core.user.astype(np.float64))
    assert row_rel_err(W, want) < 1e-3


def test_c_abi_alone_matches_shim(ml100k):
    """INTEGRATION.md "Option B": create, set_features, feature_step x 2, get_feature_weight"""
    X, (uf, itf) = ml100k
    lib = _lib.lib()
    h = _create(X, _struct_config(64, LAM_U, LAM_I))
    try:
        _set_features(h, 0, uf)
        _set_features(h, 1, itf)
        sc = solver("CG")._struct()
        for _ in range(2):
            _lib.check(lib.irs_ials_feature_step(h, C.byref(sc)))
        Wu = np.empty((uf.shape[1], 64), np.float32)
        Wi = np.empty((itf.shape[1], 64), np.float32)
        _lib.check(lib.irs_ials_get_feature_weight(h, 0, _lib.ptr(Wu, C.c_float)))
        _lib.check(lib.irs_ials_get_feature_weight(h, 1, _lib.ptr(Wi, C.c_float)))
    finally:
        lib.irs_ials_destroy(h)
    mc = (IALSModelConfigBuilder().set_K(64).set_alpha0(ALPHA0).set_reg(REG).set_nu(NU).set_init_stdev(0.1)
          .set_random_seed(1).set_loss_type(LossType.ORIGINAL).set_lambda_user_feature(LAM_U)
          .set_lambda_item_feature(LAM_I).build())
    t = IALSTrainer(mc, X, uf, itf)
    for _ in range(2):
        t.step(solver("CG"))
    np.testing.assert_array_equal(Wu, t.user_feature_weight)
    np.testing.assert_array_equal(Wi, t.item_feature_weight)
