"""The preconditions of the Mult-VAE single-update tests (``tests/test_gpu_multvae.py``), checked without a GPU and
without the library, from ``_multvae_cases`` and the numpy restatement alone: every case finds a conditioned start,
the float32 restatement of every case lies inside 1e-4 of float64 on every row of every table the GPU tests compare
(so the bar the device is held to there is the fixed 1e-4 of ``assert_float64_bar``, not "as far as the oracle"), no
contribution to the fixed-point sums of W1 comes within a factor of two of the cap at which the device reports
divergence, the slab counts the wide cases are named after are what their shapes give, and the two scaled rows of the divergence test
lie a factor of two on either side of the cap.  If one of these fails, the case's seeds change, not its shape and
not the assertion."""
import numpy as np
import pytest

import _multvae_cases as K
import _multvae_restatement as R
from conftest import rows_vs_float64

OLD, WIDE = K.update_cases(512, 256), K.wide_cases(512, 256)


def restatement_worst(X, users, keep, eps, start, p, klc):
    """the float32 restatement's worst row from float64, as ``assert_float64_bar`` measures it, per compared table"""
    x, dense = np.asarray(X[users].todense()), R.dense_keep(X, users, keep)
    new64, g64, _ = R.step(start, x, dense, eps, p, klc, K.LR, np.float64)
    new32, g32, _ = R.step(start, x, dense, eps, p, klc, K.LR, np.float32)
    worst = {}
    for n in R.TABLES:
        rows = (1, -1) if n.startswith("b") else (g64[n].shape[0], -1)
        pairs = [("d" + n, g32[n], g64[n])] + [(pre + n, new32[pre + n], new64[pre + n]) for pre in ("", "m", "v")]
        for name, a32, a64 in pairs:
            assert np.isfinite(a32).all() and np.isfinite(a64).all(), name
            worst[name] = float(rows_vs_float64(a32.reshape(rows), a32.reshape(rows), a64.reshape(rows))[1].max())
    return worst


W1_FAMILY = ("dW1", "W1", "mW1", "vW1")


def check_case(X, users, keep, eps, start, p, klc, what, one_column_w1=False):
    """``one_column_w1`` (H = 1, three of the 20 first cases, whose seeds are fixed): a row of dW1 is ONE element, the
    sum over the batch of signed terms xd[r, i] da1[r], and where they cancel no float32 sum is relatively accurate -
    the float32 restatement's worst such row is 4.7e-3 (case 7), 1.4e-4 (case 19) and 5.4e-5 (case 12, whose mW1
    reaches 1.02e-4) from float64.  There the bar of the GPU test is the restatement's own worst row and not 1e-4,
    for the four W1 tables alone; they are printed and every other table is held to 1e-4 like everywhere else.  No
    wide case has H = 1."""
    worst = restatement_worst(X, users, keep, eps, start, p, klc)
    name = max(worst, key=worst.get)
    grads = max(v for k, v in worst.items() if k.startswith("d"))
    top = K.largest_contribution(start, X, users, keep, eps, p, klc)
    print(f"{what}: float32 restatement worst row {worst[name]:.3g} ({name}), worst gradient row {grads:.3g}, "
          f"largest contribution to the W1 sums {top:.3g}")
    assert top <= 0.5 * K.CONTRIB_CAP, (what, top)  # a legal step, a factor of two inside the device's cap
    for name, err in worst.items():
        if not (one_column_w1 and name in W1_FAMILY):
            assert err < 1e-4, (what, name, err)


def test_the_slab_rule():
    assert K.dh2_slab(1) == K.dh2_slab(70) == K.dh2_slab(32768) == 512
    assert K.dh2_slab(32769) == K.dh2_slab(65536) == 1024 and K.dh2_slab(65537) == 1536
    assert all(-(-i // K.dh2_slab(i)) <= 64 for i in (32768, 32769, 65536, 65537, 10 ** 6, 2 ** 31 - 1))
    assert len(OLD) == 20 and len(WIDE) == 12 and min(c[4] for c in WIDE) == 7 and min(c[1] for c in WIDE) > 1
    assert [c[0] for c in OLD[15:]] == [3 * 512 + 37] * 5 and OLD[13][4] == 2 * 256 + 9


@pytest.mark.parametrize("case", range(20))
def test_old_case(case):
    shape = OLD[case]
    inputs = K.case_inputs(shape, case, wide=False)  # (raises where no start is found)
    check_case(*inputs, shape[5], shape[6], f"case {case} {shape}", one_column_w1=shape[1] == 1)


@pytest.mark.parametrize("case", range(12))
def test_wide_case(case):
    shape = WIDE[case]
    I, H, Hd, L, n, p, klc = shape
    assert K.slab_counts(I, n) == K.WIDE_SLABS[case]
    # the passes of the sparse kernels, the latent kernel and the tiles of the template that the case is named after
    Hp = (H + 3) // 4 * 4
    lanes = min(64, 1 << max(0, (Hp // 4 - 1).bit_length()))
    passes = -(-(Hp // 4) // lanes)
    assert (Hp, passes, -(-L // 256), -(-2 * L // 128), -(-(Hd + 1) // 128)) == [
        (256, 1, 1, 1, 1), (260, 2, 1, 1, 1), (300, 2, 1, 1, 5), (512, 2, 1, 4, 5), (516, 3, 2, 5, 3), (576, 3, 2, 5, 5),
        (36, 1, 1, 1, 1), (64, 1, 1, 1, 1), (8, 1, 1, 1, 2), (132, 1, 1, 2, 1), (8, 1, 1, 1, 1), (36, 1, 1, 1, 1)][case]
    check_case(*K.case_inputs(shape, case, wide=True), p, klc, f"wide case {case} {shape}")


def test_regrowth_batches():
    c = K.REGROW
    X, batches = K.regrowth_inputs()
    assert X.shape == (300, 257) and [b[0].size for b in batches] == [300, 5] and c["first_capacity"] < 300
    assert K.slab_counts(c["I"], 300)[2:] == (2, 44)
    small = batches[1][0]
    degrees = np.diff(X.indptr)[small]
    assert 0 in degrees and c["I"] - 1 in degrees  # the empty row and the full one
    for users, keep, eps, start in batches:
        check_case(X, users, keep, eps, start, c["p"], c["klc"], f"regrowth, {users.size} rows")


def test_ragged_cold_rows():
    c = K.SCORING
    cold = K.ragged_cold_rows()
    degrees = np.diff(cold.indptr)
    assert cold.shape == (21, 257) and cold.has_canonical_format and set(np.unique(cold.data)) == {1.0, 2.0}
    assert [min(c["capacity"], 21 - f) for f in range(0, 21, c["capacity"])] == [8, 8, 5]
    assert not degrees[list(c["empty"])].any() and degrees[c["full"]] == 257
    assert cold.indptr[8] >= 257 and (degrees[[r for r in range(21) if r not in c["empty"]]] > 0).all()


def test_divergence_rows():
    c, d = K.DIVERGENCE, K.divergence_inputs()
    X, users = d["X"], np.zeros(1, dtype=np.int32)
    assert X.shape == (2, 70) and X.dtype == np.float32 and np.isfinite(X.data).all() and np.abs(X.data).max() < 2.0 ** 20
    for user, a, low, high in ((0, d["a_lo"], 64.0, 128.0), (1, d["a_hi"], 512.0, 1024.0)):
        assert np.log2(a) == np.rint(np.log2(a))
        np.testing.assert_array_equal(X[user].toarray(), d["row"].toarray() * np.float32(a))
        x = np.asarray(X[user].todense())
        g, f = R.gradients(d["start"], x, np.ones_like(x), d["eps"], c["p"], c["klc"])
        assert f["xd"].max() <= 1.0  # (so no contribution is larger than the bias row's)
        top = float(np.abs(g["b1"]).max())
        print(f"max |db1| at {a:g} times the row: {top:.6g} (unscaled: {d['m']:.6g})")
        assert (low < top <= high) if user == 0 else (low <= top < high)
        assert top == pytest.approx(a * d["m"], rel=1e-6)  # the gradient is linear in the stored values
    # the legal row is a case like the others: a conditioned start, the float32 restatement inside the bar
    assert K.least_activation(d["start"], X, users, d["keep"], d["eps"], c["p"]) >= K.MIN_ACTIVATION
    check_case(X, users, d["keep"], d["eps"], d["start"], c["p"], c["klc"], "divergence, the legal row")
