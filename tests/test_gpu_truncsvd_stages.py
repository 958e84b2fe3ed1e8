"""Stage probes of the truncated SVD's kernels (``truncsvd_kernels.hpp``, planned by ``truncsvd_plan.hpp``; the NMF
fit and the evaluator's truncated-SVD path run on the same code), driven through the four C calls as
``utils.truncated_svd`` drives them:

    range(omega, l, n_iter=0)   Y = A omega (SpMM over A), G1 = Y^T Y
    apply(M, l2)                Y2 = Y M (tsvd_apply_kernel<false>), G2 = Y2^T Y2
    project()                   Q = A^T Y2 (SpMM over A^T), G3 = Q^T Q
    finish(rot, k)              V = Q rot or Y2 rot, z = X V (SpMM), signs

With the small integer inputs of ``_truncsvd_probe.py`` every float32 sum of these stages is exact
(``test_truncsvd_probe_inputs.py`` asserts it on the CPU), so the device is compared with the float64 chain for
EQUALITY: a lost, doubled or misplaced entry, a wrong partial slot of a split row, a wrong tile of the last slab or
a stale padding column changes the result, and there is no tolerance to choose.  The one stage that sums past 2^24,
the Gram matrix of ``Q`` where the matrix has rows or columns of a thousand entries, is held to the bound of a
float32 sum of exact products in any order.  The normalisation of the power iterations (Cholesky tiles, triangular
inverse, ``tsvd_apply_kernel<true>``) is not integer arithmetic; it is compared element by element with the float64
restatement of the device's own algorithm at a bar measured on the float32 restatement."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps

import _truncsvd_probe as P
from _truncsvd_restatement import range_gram
from conftest import random_csr, record_parity
from irspack_amd import _lib
from irspack_amd._lib import check, lib, ptr

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
MATRICES = {"probe": P.probe_matrix, "light": P.light_matrix, "tall": P.tall_matrix}


class Handle:
    """one ``irs_truncsvd`` handle; every output array starts as NaN, so an element the call does not write shows"""

    def __init__(self, handle, shape):
        self.handle, (self.n_users, self.n_items) = handle, shape
        self.l = 0

    @staticmethod
    def _f(a):
        return ptr(a, C.c_float)

    def range(self, omega, n_iter=0):
        omega = np.ascontiguousarray(omega, dtype=np.float32)
        n, self.l = omega.shape
        G = np.full((self.l, self.l), np.nan, dtype=np.float32)
        check(lib().irs_truncsvd_range(self.handle, self._f(omega), n, self.l, n_iter, self._f(G)))
        return G

    def apply(self, M):
        M = np.ascontiguousarray(M, dtype=np.float32)
        assert M.shape[0] == self.l
        self.l = M.shape[1]
        G = np.full((self.l, self.l), np.nan, dtype=np.float32)
        check(lib().irs_truncsvd_apply(self.handle, self._f(M), self.l, self._f(G)))
        return G

    def project(self):
        G = np.full((self.l, self.l), np.nan, dtype=np.float32)
        check(lib().irs_truncsvd_project(self.handle, self._f(G)))
        return G

    def finish(self, rot):
        rot = np.ascontiguousarray(rot, dtype=np.float32)
        assert rot.shape[0] == self.l
        k = rot.shape[1]
        z = np.full((self.n_users, k), np.nan, dtype=np.float32)
        c = np.full((k, self.n_items), np.nan, dtype=np.float32)
        check(lib().irs_truncsvd_finish(self.handle, self._f(rot), k, self._f(z), self._f(c)))
        return z, c

    def stats(self):
        st = _lib.TruncSvdStatsStruct()
        check(lib().irs_truncsvd_stats(self.handle, C.cast(C.byref(st), C.c_void_p)))
        return st

    def chain(self, omega, M, rot):
        """the four calls; ``n_spmm`` grows by one per sparse product: range, project, finish"""
        before = self.stats().n_spmm
        out = {"G1": self.range(omega)}
        st = self.stats()
        assert st.l_pad == 64 * -(-omega.shape[1] // 64) and st.n_spmm == before + 1
        out["G2"] = self.apply(M)
        assert self.stats().n_spmm == before + 1
        out["G3"] = self.project()
        assert self.stats().n_spmm == before + 2
        out["z"], out["components"] = self.finish(rot)
        st = self.stats()
        assert st.l_pad == 64 * -(-omega.shape[1] // 64) and st.n_spmm == before + 3
        for a in out.values():
            assert a.dtype == np.float32 and a.flags.c_contiguous
        return out


@contextlib.contextmanager
def truncsvd_handle(X):
    X = sps.csr_matrix(X, dtype=np.float32)
    assert X.has_canonical_format
    indptr = np.ascontiguousarray(X.indptr, dtype=np.int64)
    indices = np.ascontiguousarray(X.indices, dtype=np.int32)
    data = np.ascontiguousarray(X.data, dtype=np.float32)
    handle = C.c_void_p()
    check(lib().irs_truncsvd_create(X.shape[0], X.shape[1], ptr(indptr, C.c_int64), ptr(indices, C.c_int32),
                                    ptr(data, C.c_float), _lib.default_device(), C.byref(handle)))
    try:
        yield Handle(handle, X.shape)
    finally:
        lib().irs_truncsvd_destroy(handle)


def first_difference(got, want):
    at = np.argwhere(got != want)
    return f"{len(at)} elements differ, the first at {tuple(at[0])}: {got[tuple(at[0])]} != {want[tuple(at[0])]}"


def assert_equal(got, ref, keys, what):
    for key in keys:
        assert got[key].shape == ref[key].shape, (what, key, got[key].shape)
        assert np.array_equal(got[key], ref[key]), (what, key, first_difference(got[key], ref[key]))


def assert_gram_within_summation_bound(G, Q, what):
    """``G = Q^T Q`` in float32, ``Q`` exact, summed over ``n`` rows in any order through at most 256 slab
    partials: ``|G - G64| <= 1.01 (n + 256) 2^-24 |Q|^T |Q|`` elementwise, and symmetric to the bit"""
    n = Q.shape[0]
    bound = 1.01 * (n + 256) * EPS * (np.abs(Q).T @ np.abs(Q))
    err = np.abs(G.astype(np.float64) - Q.T @ Q)
    assert np.isfinite(G).all() and (err <= bound).all(), (what, float((err - bound).max()), float(err.max()))
    assert np.array_equal(G, G.T), what


def check_chain(name, transposed, l):
    X = MATRICES[name](transposed)
    omega, M, rot = P.inputs(X, l)
    ref = P.stages(X, omega, M, rot)
    what = f"{name}{' transposed' if transposed else ''} l={l}"
    with truncsvd_handle(X) as h:
        got = h.chain(omega, M, rot)
    exact = ["G1", "G2", "z", "components"]
    if name in P.G3_NOT_EXACT:
        assert got["G3"].shape == ref["G3"].shape
        assert_gram_within_summation_bound(got["G3"], ref["Q"], what)
    else:
        exact.append("G3")
    assert_equal(got, ref, exact, what)
    return X, got


# ------------------------------------------------------------------ 1. every stage at every width
@pytest.mark.parametrize("l", P.WIDTHS)
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("name", ["probe", "light"])
def test_every_stage_at_every_width(name, transposed, l):
    """all five instantiations of the sparse product (l_pad 64: <16,1>; 128: <32,1>; 192, 256: <64,1>; 320 .. 512:
    <64,2>; 576: <64,3>), the full and the partly masked chunk of each, l on both sides of a tile boundary; split
    rows of two and three segments on either side (``probe``), and the Gram of Q compared exactly (``light``)"""
    X, got = check_chain(name, transposed, l)
    empty_user, empty_item = P.empties(transposed)
    assert not got["z"][empty_user].any() and not got["components"][:, empty_item].any()


# ------------------------------------------------------------------ 2. the tall block
@pytest.mark.parametrize("l", P.TALL_WIDTHS)
@pytest.mark.parametrize("transposed", [False, True])
def test_tall_block(transposed, l):
    """20,000 rows: 313 chunks of 64 rows in 157 slabs of two, the last slab one chunk of 32 rows"""
    check_chain("tall", transposed, l)


# ------------------------------------------------------------------ 3. one handle, several widths
_FRESH = {}


def fresh(transposed, l):
    if (transposed, l) not in _FRESH:
        X = P.probe_matrix(transposed)
        with truncsvd_handle(X) as h:
            _FRESH[(transposed, l)] = h.chain(*P.inputs(X, l))
    return _FRESH[(transposed, l)]


@pytest.mark.parametrize("transposed", [False, True])
def test_one_handle_at_several_widths(transposed):
    """``range`` re-sizes and re-points the three blocks: what the wider run left in them, in G, W, the small
    matrix or the partial buffers must not reach a narrower run, nor the narrower run's padding a wider one"""
    X = P.probe_matrix(transposed)
    with truncsvd_handle(X) as h:
        for l in (576, 65, 320):
            got, want = h.chain(*P.inputs(X, l)), fresh(transposed, l)
            for key in ("G1", "G2", "G3", "z", "components"):
                assert got[key].tobytes() == want[key].tobytes(), (l, key, first_difference(got[key], want[key]))
        assert h.stats().n_spmm == 9


# ------------------------------------------------------------------ 4. the normalisation
NORMALISED = {"700 x 600": (700, 600, 0.1, 2), "3000 x 1100": (3000, 1100, 0.02, 3)}
_NORM = {}


def normalised_case(shape, l):
    """``(A, omega)``, shared by the two ``n_iter`` of a case"""
    if (shape, l) not in _NORM:
        A = random_csr(*NORMALISED[shape])
        omega = np.ascontiguousarray(np.random.RandomState(0).normal(size=(A.shape[1], l)), dtype=np.float32)
        _NORM[(shape, l)] = (A, omega)
    return _NORM[(shape, l)]


@pytest.mark.parametrize("n_iter", [1, 2])
@pytest.mark.parametrize("shape,l", [("700 x 600", 40), ("700 x 600", 310), ("700 x 600", 510),
                                     ("3000 x 1100", 130), ("3000 x 1100", 576)])
def test_normalised_power_iterations(shape, l, n_iter):
    """``range(omega, l, n_iter)``: Gram, shift, tiled Cholesky, triangular inverse and ``tsvd_apply_kernel<true>``
    on both blocks of every iteration.  The shifted Cholesky factor is unique, so the Gram matrix that comes home
    is compared element by element: ``max |G - G64| / max |G64|`` against the float64 restatement of the same
    algorithm.  The bar is the float32 restatement's own distance times 4 (the multiple of
    ``test_gpu_truncsvd.compare``), with a floor of 16 float32 roundings (``test_gpu_nmf``'s, for a restatement
    that is nearly exact by accident); never a number taken from the device."""
    A, omega = normalised_case(shape, l)
    G64 = range_gram(A, omega, n_iter, np.float64)
    G32 = range_gram(A, omega, n_iter, np.float32)
    top = float(np.abs(G64).max())
    e_r32 = float(np.abs(G32.astype(np.float64) - G64).max() / top)
    assert G32.dtype == np.float32 and e_r32 <= 1e-4, e_r32  # precondition: otherwise change the case
    bar = max(4.0 * e_r32, 16.0 * EPS)
    with truncsvd_handle(A) as h:
        G = h.range(omega, n_iter)
        st = h.stats()
    assert G.dtype == np.float32 and G.shape == (l, l) and np.isfinite(G).all()
    e_gpu = float(np.abs(G.astype(np.float64) - G64).max() / top)
    record_parity("test_normalised_power_iterations", f"{shape} l={l} n_iter={n_iter}", err_gpu=e_gpu, err_r32=e_r32,
                  bar=bar, ratio=e_gpu / max(e_r32, 1e-300), gram_max=top, cond=float(np.linalg.cond(G64)))
    assert st.l_pad == 64 * -(-l // 64) and st.n_spmm == 2 * n_iter + 1
    assert np.array_equal(G, G.T)
    assert e_gpu <= bar, (e_gpu, e_r32, bar)
