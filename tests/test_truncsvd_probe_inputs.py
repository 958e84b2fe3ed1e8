"""The preconditions of the truncated SVD's stage probes (``tests/test_gpu_truncsvd_stages.py``), checked without a
GPU: the planted rows and columns of ``_truncsvd_probe.probe_matrix`` have exactly the stored entries and segments
they are named after, and every stage that the GPU tests compare for equality sums magnitudes of at most 2^24 per
output element, at every width and in both orientations, so that float32 is exact there in any order of addition.
If one of these fails, the input changes (a sparser ``omega``, a lighter background), not the assertion."""
import numpy as np
import pytest

import _truncsvd_probe as P


def check_matrix(X, shape):
    assert X.shape == shape and X.dtype == np.float32 and X.has_canonical_format
    assert set(np.unique(X.data)) == {1.0, 2.0}


@pytest.mark.parametrize("transposed", [False, True])
def test_planted_counts_and_segments(transposed):
    X, L = P.probe_matrix(transposed), P.light_matrix(transposed)
    shape = (P.N_ITEMS, P.N_USERS) if transposed else (P.N_USERS, P.N_ITEMS)
    check_matrix(X, shape)
    check_matrix(L, shape)
    by_user, by_item = np.diff(X.indptr), np.diff(X.tocsc().indptr)
    if transposed:
        by_user, by_item = by_item, by_user
    # (by_user / by_item now index the 3000 x 1100 orientation, whichever way X lies)
    for user, count in P.USER_COUNTS.items():
        assert by_user[user] == count, (user, by_user[user], count)
    for item, count in P.ITEM_COUNTS.items():
        assert by_item[item] == count, (item, by_item[item], count)
    # the full row holds every item that has any entry
    assert by_user[P.FULL_USER] == (by_item > 0).sum()
    assert sorted(np.flatnonzero(by_user > 64)) == sorted(u for u, c in P.USER_COUNTS.items() if c)
    assert sorted(np.flatnonzero(by_item > 64)) == sorted(i for i, c in P.ITEM_COUNTS.items() if c)
    # segments per side, recomputed from indptr
    for indptr, want in zip((X.indptr, X.tocsc().indptr), P.expected_segments(transposed)):
        seg = P.segments(indptr)
        assert {int(r): int(seg[r]) for r in np.flatnonzero(seg != 1)} == want
    # the light matrix: the same background, nothing split, the same empty row and column
    empty_user, empty_item = P.empties(transposed)
    for M in (X, L):
        assert M.indptr[empty_user] == M.indptr[empty_user + 1] and not (M.indices == empty_item).any()
    assert P.segments(L.indptr).max() == 1 and P.segments(L.tocsc().indptr).max() == 1
    assert 0.008 * L.shape[0] * L.shape[1] < L.nnz < 0.012 * L.shape[0] * L.shape[1]
    assert X.nnz < 50000


def test_tall_matrix():
    X, Xt = P.tall_matrix(), P.tall_matrix(True)
    check_matrix(X, (20000, 70))
    check_matrix(Xt, (70, 20000))
    assert not (X != Xt.T).nnz
    assert 2.5 * 20000 < X.nnz < 3.5 * 20000
    assert P.segments(X.indptr).max() == 1 and P.segments(Xt.indptr).max() == 1


def test_small_inputs():
    for l in P.WIDTHS:
        l, l2, k = P.widths_of(l)
        assert 1 <= k <= l2 <= l
        om = P.omega(P.N_ITEMS, l)
        assert om.dtype == np.float32 and om.flags.c_contiguous and set(np.unique(om)) <= {-1.0, 0.0, 1.0}
        if l >= 63:
            assert 0.2 < (om != 0).mean() < 0.3 and (om != 0).any(axis=0).all()
        for M in (P.small(l, l2), P.small(l2, k)):
            assert M.dtype == np.float32 and M.flags.c_contiguous and set(np.unique(M)) <= {-1.0, 0.0, 1.0}
            assert ((M != 0).sum(axis=0) == min(2, M.shape[0])).all()
    assert np.array_equal(P.omega(70, 5), P.omega(70, 5)) and not np.array_equal(P.omega(70, 5), P.omega(70, 64)[:, :5])


def gram_plan(rows, l_pad):
    """``(chunks of 64 rows, chunks per slab, slabs, live rows of the last chunk)`` of a Gram pass, restated from
    ``plan_gram_pass`` and ``gram_slabs`` in sparse_block_plan.hpp"""
    nb = l_pad // 64
    n_tile = nb * (nb + 1) // 2
    chunks = max(1, -(-rows // 64))
    want = min(chunks, min(256, max(1, 2048 // n_tile)))
    per_slab = -(-chunks // want)
    return chunks, per_slab, -(-chunks // per_slab), rows - 64 * (chunks - 1)


def test_the_shapes_cross_the_second_pass_of_the_gram_row_loop():
    assert gram_plan(3000, 576) == (47, 2, 24, 56)  # 45 slabs wanted: two chunks each, the last slab one chunk
    assert gram_plan(20000, 64) == (313, 2, 157, 32) and gram_plan(20000, 128) == (313, 2, 157, 32)
    assert gram_plan(1100, 576) == (18, 1, 18, 12)


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("name", ["probe", "light", "tall"])
def test_every_stage_compared_for_equality_is_exact_in_float32(name, transposed):
    X = {"probe": P.probe_matrix, "light": P.light_matrix, "tall": P.tall_matrix}[name](transposed)
    worst = {}
    for l in P.TALL_WIDTHS if name == "tall" else P.WIDTHS:
        ref = P.stages(X, *P.inputs(X, l))
        for stage, bound in ref["bounds"].items():
            worst[stage] = max(worst.get(stage, 0.0), bound)
            # G3 = Q^T Q, Q = A^T Y2: A^T A has the planted columns' counts on its diagonal (the tall matrix: its
            # 70 columns of about 860 entries), so there the GPU tests hold G3 to a derived bound, not equality
            if stage == "G3" and name in P.G3_NOT_EXACT:
                continue
            assert bound <= P.EXACT, (name, transposed, l, stage, bound)
        for key in ("G1", "G2", "G3", "z", "components"):
            assert np.array_equal(ref[key], np.rint(ref[key])) and np.abs(ref[key]).max() <= 2.0 ** 52
    print(name, "transposed" if transposed else "", {k: f"{v:.3g}" for k, v in worst.items()})


def test_stages_against_integer_arithmetic():
    """the reference chain itself, on a small matrix, against int64 products and a literal sign rule"""
    rng = np.random.default_rng(3)
    for shape in ((9, 6), (6, 9)):
        X = (rng.random(shape) < 0.5) * rng.integers(1, 3, size=shape)
        n, l, l2, k = min(shape), 5, 4, 3
        om, M, rot = P.omega(n, l), P.small(l, l2), P.small(l2, k)
        rot[:, 2] = 0.0  # a zero component keeps sign +1
        ref = P.stages(X, om, M, rot)
        A = X.T if shape[0] < shape[1] else X
        iom, iM, irot = (a.astype(np.int64) for a in (om, M, rot))
        Y = A @ iom
        Y2 = Y @ iM
        Q = A.T @ Y2
        V = (Y2 if shape[0] < shape[1] else Q) @ irot
        z = X @ V
        for j in range(k):
            col = V[:, j]
            first = int(np.flatnonzero(np.abs(col) == np.abs(col).max())[0])
            if col[first] < 0:
                V[:, j], z[:, j] = -V[:, j], -z[:, j]
        for key, want in (("G1", Y.T @ Y), ("G2", Y2.T @ Y2), ("G3", Q.T @ Q), ("z", z), ("components", V.T)):
            assert ref[key].dtype == np.float64 and np.array_equal(ref[key], want), key
        assert not ref["components"][2].any() and not ref["z"][:, 2].any()
        assert ref["bounds"]["Y"] == (np.abs(A) @ np.abs(iom)).max()
        assert ref["bounds"]["G3"] == (np.abs(Q).T @ np.abs(Q)).max()
        assert ref["bounds"]["z"] == (np.abs(X) @ np.abs(V)).max()
