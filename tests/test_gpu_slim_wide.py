"""GPU tests of the SLIM descent at its wide launch shapes: 512 and 1024 threads, LDS above 64 KiB, and the edge
between the running vector in LDS and in a global scratch row (``slim_host_plan.hpp`` decides, ``slim_kernels.hpp``
runs it).  ``tests/test_gpu_slim.py`` never leaves 256 threads.

What differs between the shapes: the first-change search over 8 or 16 wave slots, the two alternating slot
buffers behind one barrier, ``tid == first`` with ``first >= 256``, the look-ahead load ``w[f + nthr]`` and its
guard at the last chunk, chunk seams at multiples of 512 and 1024, LDS above 64 KiB.

The input makes a wide catalogue cheap to arbitrate.  Of ``I`` items only ``T`` (1,019 at a chunk width ``B`` of
512, 1,531 at 1,024, 761 at the 256 of the first catalogue past the LDS edge) have interactions; an item without interactions never moves (``G_ff = 0``, ``l2 > 0``), so by
the embedding lemma (``tests/test_slim_surface.py``, on the restatement) the fit restricted to the touched items
is the fit of the compacted ``500 x T`` matrix, bit for bit.  The compacted fit runs 256 threads with the vector
in LDS, the shape the existing tests arbitrate; the float64 restatement arbitrates a few columns directly.  The
touched items are placed where the wide shapes differ: the run ``[B - 200, 2B + 300)`` covers every lane of every
wave of one full chunk and crosses two seams; then items 0, 63, 64, the last item of the penultimate chunk, the
first of the last chunk, ``I - 2`` and ``I - 1``.  ``n_iter = 4`` with ``tol = 0`` is unconverged on purpose: only
the ascending order passes.

Every case first asserts the launch shape the library reports (``irs_slim_last_launch``), so a case that ran
another shape fails instead of passing vacuously."""
import time

import numpy as np
import pytest
import scipy.sparse as sps

from _slim_restatement import gram, slim_column
from conftest import record_parity
from irspack_amd.utils import slim_weight_allow_negative, slim_weight_positive_only

pytestmark = pytest.mark.gpu

N_USERS, N_ITER, L2, L1 = 500, 4, 5.0, 0.5
SLOT_BYTES = 400

# catalogue -> (threads, lds_r, lds_bytes, raise_dynamic_lds): 400 + 4 I bytes of LDS; 256 threads up to 40 KiB,
# 512 up to 80 KiB, 1024 above; the dynamic-LDS limit is raised above 64 KiB
FIXED_CASES = {
    10_141: (512, True, 40_964, False),   # the smallest 8-wave catalogue
    16_285: (512, True, 65_540, True),    # the first size through the raised dynamic-LDS limit
    20_381: (1024, True, 81_924, True),   # the smallest 16-wave catalogue, a partial last chunk
    20_480: (1024, True, 82_320, True),   # no partial chunk: the other side of the f + nthr < n_items guard
}


def fit(X, positive_only, n_iter=N_ITER, tol=0.0, stats=None):
    f = slim_weight_positive_only if positive_only else slim_weight_allow_negative
    return f(X, 1, n_iter, L2, L1, tol, -1, stats=stats)


def same_bytes(A, B):
    return (A.indptr.tobytes() == B.indptr.tobytes() and A.indices.tobytes() == B.indices.tobytes()
            and A.data.tobytes() == B.data.tobytes())


def touched_items(n_items, B):
    last = (-(-n_items // B) - 1) * B  # the first item of the last chunk
    items = set(range(B - 200, 2 * B + 300)) | {0, 63, 64, last - 1, last, n_items - 2, n_items - 1}
    items = np.asarray(sorted(items), dtype=np.int64)
    assert items[0] == 0 and items[-1] == n_items - 1 and last - 1 >= 2 * B + 300 and last < n_items - 2
    return items, last


def sampled_items(n_items, B, last):
    """item 0, the first item of the full chunk and of the chunk behind it (one on each seam), three more targets
    inside the full chunk (its second lane, a lane of a middle wave, its last lane), the first item of the last
    chunk, the last item"""
    return [0, B, B + 1, B + B // 2 + 37, 2 * B - 1, 2 * B, last, n_items - 1]


_COMPACT, _SMALL_FIT, _REFERENCE = {}, {}, {}


def compact(T):
    """the compacted 500 x T matrix (float64 CSR) and its Gram matrix in float64 and float32"""
    if T not in _COMPACT:
        rng = np.random.default_rng(41)
        dense = (rng.random((N_USERS, T)) < 0.05) * rng.integers(1, 6, size=(N_USERS, T))
        assert (dense != 0).sum(axis=0).min() >= 10
        X = sps.csr_matrix(dense.astype(np.float64))
        _COMPACT[T] = (X, gram(X), gram(X, np.float32))
    return _COMPACT[T]


def small_fit(T, positive_only, tol=0.0):
    """the fit of the compacted matrix: 256 threads, the running vector in LDS"""
    key = (T, positive_only, tol)
    if key not in _SMALL_FIT:
        stats = {}
        W = fit(compact(T)[0], positive_only, tol=tol, stats=stats)
        assert (stats["threads"], stats["lds_r"], stats["lds_bytes"]) == (256, True, SLOT_BYTES + 4 * T)
        _SMALL_FIT[key] = (W, stats)
    return _SMALL_FIT[key]


def reference(T, positive_only, cols):
    """{compacted column: (float64 column, error of the float32 restatement)} and the bar that follows"""
    key = (T, positive_only, tuple(cols))
    if key not in _REFERENCE:
        _, G64, G32 = compact(T)
        out = {}
        for c in cols:
            w64 = slim_column(G64, c, L2, L1, N_ITER, 0.0, positive_only)
            w32 = slim_column(G32, c, np.float32(L2), np.float32(L1), N_ITER, 0.0, positive_only).astype(np.float64)
            scale = np.abs(w64).max()
            assert scale > 0, c
            out[c] = (w64, np.abs(w32 - w64).max() / scale)
        f32_worst = max(e for _, e in out.values())
        _REFERENCE[key] = (out, f32_worst, max(4.0 * f32_worst, 1e-5))
    return _REFERENCE[key]


def embed(T, touched, n_items):
    coo = compact(T)[0].tocoo()
    return sps.csr_matrix((coo.data, (coo.row, touched[coo.col])), shape=(N_USERS, n_items))


def shape_of(stats):
    return stats["threads"], stats["lds_r"], stats["lds_bytes"], stats["raise_dynamic_lds"]


def check_case(name, n_items, B, expected, positive_only, may_skip):
    touched, last = touched_items(n_items, B)
    T = touched.size
    big = embed(T, touched, n_items)
    stats = {}
    t0 = time.perf_counter()
    try:
        W_big = fit(big, positive_only, stats=stats)
    except RuntimeError as exc:
        if may_skip and "device memory" in str(exc):
            pytest.skip(f"NOT RUN: {exc}")
        raise
    wall = time.perf_counter() - t0

    # 1. the launch shape
    print(f"{name}: I={n_items} T={T} B={B} positive_only={positive_only} launch={stats} wall_s={wall:.2f}")
    assert shape_of(stats) == expected, (shape_of(stats), expected, stats["lds_per_block"])
    assert stats["threads"] == B

    # 2. the bytes of the compacted fit
    W_small, stats_small = small_fit(T, positive_only)
    assert W_big.shape == (n_items, n_items) and W_big.dtype == np.float32
    assert W_big.nnz == W_small.nnz > 0
    sub = W_big[touched][:, touched].tocsc()
    sub.sort_indices()
    assert same_bytes(sub, W_small)

    # 3. float64 directly
    items = sampled_items(n_items, B, last)
    cols = [int(c) for c in np.searchsorted(touched, items)]
    assert (touched[cols] == items).all()
    ref, f32_worst, bar = reference(T, positive_only, cols)
    chunk = np.flatnonzero((touched >= B) & (touched < 2 * B))  # compacted coordinates of the full chunk
    assert chunk.size == B
    gpu_worst = 0.0
    for item, c in zip(items, cols):
        w64 = ref[c][0]
        # (a condition on the reference alone) the column changes in at least two waves of the full chunk
        waves = {int(w) for w in (touched[chunk][w64[chunk] != 0] - B) // 64}
        assert len(waves) >= 2, (item, waves)
        col = np.asarray(W_big[:, [item]].todense()).ravel().astype(np.float64)
        wg = col[touched]
        assert np.count_nonzero(col) == np.count_nonzero(wg)
        gpu_worst = max(gpu_worst, np.abs(wg - w64).max() / np.abs(w64).max())
        assert (wg[np.abs(w64) > bar] != 0).all(), item
    record_parity(name, f"I={n_items} positive_only={positive_only}", T=int(T), threads=stats["threads"],
                  lds_r=stats["lds_r"], lds_bytes=stats["lds_bytes"], raise_dynamic_lds=stats["raise_dynamic_lds"],
                  n_wg=stats["n_wg"], lds_per_block=stats["lds_per_block"], n_cols=len(cols),
                  gpu_worst_col_err=gpu_worst, f32_restatement_worst_col_err=f32_worst, bar=bar, nnz=int(W_big.nnz),
                  wall_s=wall)
    assert gpu_worst <= bar, (gpu_worst, f32_worst)

    # 4. counters
    assert stats["updates_total"] == stats_small["updates_total"] > 0
    assert stats["sweeps_total"] == n_items * N_ITER and stats_small["sweeps_total"] == T * N_ITER
    return W_big, stats


_AT_20381 = {}


def fit_at_20381(positive_only):
    if positive_only not in _AT_20381:
        _AT_20381[positive_only] = check_case("test_wide_catalogue", 20_381, 1024, FIXED_CASES[20_381], positive_only,
                                              may_skip=False)
    return _AT_20381[positive_only]


@pytest.mark.parametrize("positive_only", [True, False])
@pytest.mark.parametrize("n_items", sorted(FIXED_CASES))
def test_wide_catalogue(n_items, positive_only):
    """512 and 1024 threads with the running vector in LDS; needs at most 3.4 GB of device memory: never skipped.
    20,381 is also DESIGN 9's claim about the ML-20M size (26,744 items): 1024 threads, the vector in LDS."""
    if n_items == 20_381:
        fit_at_20381(positive_only)
        return
    expected = FIXED_CASES[n_items]
    check_case("test_wide_catalogue", n_items, expected[0], expected, positive_only, may_skip=False)


def device_lds_limit():
    """the per-block LDS limit, read back from a small fit"""
    stats = {}
    fit(compact(1019)[0][:, :64], True, n_iter=1, stats=stats)
    assert stats["lds_r"] and stats["threads"] == 256 and stats["lds_bytes"] == SLOT_BYTES + 4 * 64
    return stats["lds_per_block"]


@pytest.mark.parametrize("positive_only", [True, False])
@pytest.mark.parametrize("side", ["last_in_lds", "first_in_global"])
def test_per_block_lds_edge(side, positive_only):
    """``I_max = (limit - 400) / 4`` is the last catalogue whose running vector is in LDS, ``I_max + 1`` the first
    in a global scratch row (256 threads again).  With the 160 KiB an MI355X reports per block that is 40,860 and
    40,861 items and 13.4 GB per call: only these cases may skip, on the library's "device memory" error."""
    limit = device_lds_limit()
    assert limit >= SLOT_BYTES + 4 * 20_381, limit  # else: test_wide_catalogue has failed on the shape already
    i_max = (limit - SLOT_BYTES) // 4
    if side == "last_in_lds":
        n_items, lds_bytes = i_max, SLOT_BYTES + 4 * i_max
        threads = 1024 if lds_bytes > 80 * 1024 else 512 if lds_bytes > 40 * 1024 else 256
        expected = (threads, True, lds_bytes, lds_bytes > 64 * 1024)
    else:
        n_items, expected = i_max + 1, (256, False, SLOT_BYTES, False)
    check_case("test_per_block_lds_edge", n_items, expected[0], expected, positive_only, may_skip=True)


@pytest.mark.parametrize("positive_only", [True, False])
def test_every_column_stops_on_its_own(positive_only):
    """20,381 items, ``tol = 1e-30``: a column of an item without interactions changes nothing in its first sweep
    and stops there; the touched columns run as they do in the compacted fit; the bytes are the ``tol = 0``
    call's."""
    n_items = 20_381
    W0, _ = fit_at_20381(positive_only)
    touched, _ = touched_items(n_items, 1024)
    stats, stats_small = {}, small_fit(touched.size, positive_only, tol=1e-30)[1]
    W = fit(embed(touched.size, touched, n_items), positive_only, tol=1e-30, stats=stats)
    assert shape_of(stats) == FIXED_CASES[n_items]
    assert stats["sweeps_total"] == stats_small["sweeps_total"] + (n_items - touched.size)
    assert touched.size <= stats_small["sweeps_total"] <= touched.size * N_ITER
    assert stats["updates_total"] == stats_small["updates_total"]
    assert same_bytes(W, W0)


@pytest.mark.parametrize("positive_only", [True, False])
def test_two_calls_give_the_same_bytes(positive_only):
    n_items = 20_381
    W0, stats0 = fit_at_20381(positive_only)
    touched, _ = touched_items(n_items, 1024)
    stats = {}
    W = fit(embed(touched.size, touched, n_items), positive_only, stats=stats)
    assert shape_of(stats) == FIXED_CASES[n_items]
    assert same_bytes(W, W0)
    assert (stats["sweeps_total"], stats["updates_total"]) == (stats0["sweeps_total"], stats0["updates_total"])
