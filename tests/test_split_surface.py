"""The hold-out split and the ``irspack_amd.split`` package without a device: the reference's names and defaults, the
C entries, the pandas glue on small frames with known answers, the uniformity of the rule (on its numpy restatement,
``tests/_split_restatement.py``) and the host layer ``split_host_plan.hpp`` under the sanitizers."""
import ctypes as C
import inspect
import itertools
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sps

from _split_restatement import held_out_mask, n_test_of
from irspack_amd import split, utils
from irspack_amd.split import (UserTrainTestInteractionPair, holdout_specific_interactions,
                               split_dataframe_partial_user_holdout, split_last_n_interaction_df)
from irspack_amd.split.userwise import split_train_test_userwise_random, split_train_test_userwise_time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = inspect.Parameter.empty
POS, KWONLY = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY


def _params(fn, kind):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values() if p.kind is kind]


# ---- the surface ---------------------------------------------------------------------------------------------------

def test_signatures_are_the_reference():
    extra = [("device", None), ("stats", None)]
    assert _params(utils.rowwise_train_test_split_by_ratio, POS) == [
        ("X", EMPTY), ("random_seed", EMPTY), ("heldout_ratio", EMPTY), ("n_test_ceil", EMPTY)]
    assert _params(utils.rowwise_train_test_split_by_ratio, KWONLY) == extra
    assert _params(utils.rowwise_train_test_split_by_fixed_n, POS) == [
        ("X", EMPTY), ("random_seed", EMPTY), ("n_held_out", EMPTY)]
    assert _params(utils.rowwise_train_test_split_by_fixed_n, KWONLY) == extra
    assert _params(utils.rowwise_train_test_split, POS) == [
        ("X", EMPTY), ("test_ratio", 0.5), ("n_test", None), ("ceil_n_heldout", False), ("random_state", None)]
    assert _params(utils.rowwise_train_test_split, KWONLY) == extra
    assert _params(utils.convert_randomstate, POS) == [("arg", EMPTY)]
    assert _params(utils.df_to_sparse, POS) == [
        ("df", EMPTY), ("user_column", EMPTY), ("item_column", EMPTY), ("user_ids", None), ("item_ids", None),
        ("rating_column", None)]
    assert _params(UserTrainTestInteractionPair.__init__, POS) == [
        ("self", EMPTY), ("user_ids", EMPTY), ("X_train", EMPTY), ("X_test", EMPTY), ("item_ids", None)]
    assert _params(split_train_test_userwise_random, POS) == [
        ("df_", EMPTY), ("user_column", EMPTY), ("item_column", EMPTY), ("item_ids", EMPTY), ("heldout_ratio", EMPTY),
        ("n_heldout", EMPTY), ("rns", EMPTY), ("rating_column", None), ("ceil_n_heldout", False)]
    assert _params(split_train_test_userwise_time, POS) == [
        ("df_", EMPTY), ("user_column", EMPTY), ("item_column", EMPTY), ("time_column", EMPTY), ("item_ids", EMPTY),
        ("heldout_ratio", EMPTY), ("n_heldout", EMPTY), ("rating_column", None), ("ceil_n_heldout", False)]
    assert _params(split_dataframe_partial_user_holdout, POS) == [
        ("df_all", EMPTY), ("user_column", EMPTY), ("item_column", EMPTY), ("time_column", None),
        ("rating_column", None), ("n_val_user", None), ("n_test_user", None), ("val_user_ratio", 0.1),
        ("test_user_ratio", 0.1), ("heldout_ratio_val", 0.5), ("n_heldout_val", None), ("heldout_ratio_test", 0.5),
        ("n_heldout_test", None), ("ceil_n_heldout", False), ("random_state", None)]
    assert _params(holdout_specific_interactions, POS) == [
        ("df", EMPTY), ("user_column", EMPTY), ("item_column", EMPTY), ("interaction_indicator", EMPTY),
        ("validatable_user_ratio_val", 0.2), ("validatable_user_ratio_test", 0.2), ("random_state", None)]
    assert _params(split_last_n_interaction_df, POS) == [
        ("df", EMPTY), ("user_column", EMPTY), ("timestamp_column", EMPTY), ("n_heldout", None),
        ("heldout_ratio", 0.1), ("ceil_n_heldout", False)]
    # the reference's irspack.split.__all__, and the re-export
    for name in ("UserTrainTestInteractionPair", "split_dataframe_partial_user_holdout",
                 "holdout_specific_interactions", "rowwise_train_test_split", "split_last_n_interaction_df"):
        assert name in split.__all__ and hasattr(split, name)
    assert split.rowwise_train_test_split is utils.rowwise_train_test_split
    import irspack_amd

    assert irspack_amd.rowwise_train_test_split is utils.rowwise_train_test_split
    assert irspack_amd.df_to_sparse is utils.df_to_sparse
    with pytest.raises(AttributeError):
        irspack_amd.no_such_name


def test_header_declares_the_split_entries_and_abi_stays_4():
    from irspack_amd import _lib

    header = open(os.path.join(ROOT, "include", "irspack_amd.h")).read()
    assert re.search(r"#define IRS_ABI_VERSION 4\b", header) and _lib.ABI_VERSION == 4
    declared = set(re.findall(r"\b(irs_[a-z0-9_]*)\(", header))
    for name in ("irs_split_rowwise", "irs_split_nnz", "irs_split_fetch", "irs_split_last_stats", "irs_split_destroy"):
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and name in _lib.ARGTYPES
        assert hasattr(_lib.lib(), name)
    assert "#define IRS_SPLIT_BY_RATIO 0" in header and "#define IRS_SPLIT_BY_FIXED_N 1" in header
    assert (_lib.SPLIT_BY_RATIO, _lib.SPLIT_BY_FIXED_N) == (0, 1)
    # the stats struct, field by field in the header's order
    body = re.search(r"typedef struct \{([^}]*)\} irs_split_stats;", header).group(1)
    fields = re.findall(r"\b(double|int64_t)\s+(\w+);", body)
    assert [(n, {"double": C.c_double, "int64_t": C.c_int64}[t]) for t, n in fields] == _lib.SplitStatsStruct._fields_


def test_importing_utils_does_not_import_pandas():
    code = ("import sys; import irspack_amd.utils, irspack_amd; "
            "assert 'pandas' not in sys.modules, 'pandas was imported'; "
            "from irspack_amd import rowwise_train_test_split, df_to_sparse; "
            "assert 'pandas' not in sys.modules, 'pandas was imported by the lazy exports'")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


# ---- the C entries where no device is needed: the checks come first, empty inputs succeed ---------------------------

def _c_split(indptr, indices, data, rows, cols, elem_bytes=None, seed=1, mode=0, ratio=0.5, ceil=0, n=0):
    from irspack_amd import _lib

    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    data = np.ascontiguousarray(data)
    h = C.c_void_p()
    st = _lib.lib().irs_split_rowwise(
        rows, cols, _lib.ptr(indptr, C.c_int64), _lib.ptr(indices, C.c_int32), data.ctypes.data_as(C.c_void_p),
        data.dtype.itemsize if elem_bytes is None else elem_bytes, seed, mode, ratio, ceil, n, 0, C.byref(h))
    return st, _lib.lib().irs_last_error().decode(), h


def test_argument_checks_come_before_device_work():
    """status 1 (invalid argument) where no device is visible too - a status 2 would mean the device was asked first"""
    ok = dict(indptr=[0, 2, 3], indices=[0, 2, 1], data=np.ones(3, np.float32), rows=2, cols=3)
    for kw, word in [(dict(ratio=1.5), "test_ratio"), (dict(ratio=-0.1), "test_ratio"),
                     (dict(ratio=float("nan")), "test_ratio"), (dict(mode=1, n=-1), "n_held_out"),
                     (dict(mode=7), "mode"), (dict(elem_bytes=3), "width"), (dict(elem_bytes=16), "width"),
                     (dict(indptr=[0, 2, 1]), "indptr"), (dict(indices=[2, 0, 1]), "sorted"),
                     (dict(indices=[1, 1, 0]), "duplicate"), (dict(indices=[0, 3, 1]), "range")]:
        st, msg, h = _c_split(**{**ok, **kw})
        assert st == 1 and word in msg and not h.value, (kw, st, msg)


def test_empty_inputs_succeed_without_a_device():
    from irspack_amd import _lib

    lib = _lib.lib()
    for rows, indptr in [(0, [0]), (3, [0, 0, 0, 0])]:
        st, msg, h = _c_split(indptr, [0], np.zeros(1, np.float64), rows, 5)
        assert st == 0, msg
        a, b = C.c_int64(-1), C.c_int64(-1)
        assert lib.irs_split_nnz(h, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (0, 0)
        tr, te = np.full(rows + 1, -1, np.int64), np.full(rows + 1, -1, np.int64)
        assert lib.irs_split_fetch(h, _lib.ptr(tr, C.c_int64), None, None, _lib.ptr(te, C.c_int64), None, None) == 0
        assert not tr.any() and not te.any()
        stats = _lib.SplitStatsStruct()
        assert lib.irs_split_last_stats(h, C.cast(C.byref(stats), C.c_void_p)) == 0
        assert (stats.rows_empty, stats.rows_wave, stats.rows_lds, stats.rows_stream) == (rows, 0, 0, 0)
        assert lib.irs_split_destroy(h) == 0
    # the Python layer on the same inputs: shapes and dtype kept
    for dtype in (np.float64, np.int64, np.bool_):
        tr, te = utils.rowwise_train_test_split(sps.csr_matrix((3, 5), dtype=dtype), n_test=2, random_state=0)
        assert tr.shape == te.shape == (3, 5) and tr.dtype == te.dtype == dtype and tr.nnz == te.nnz == 0
    with pytest.raises(ValueError, match="test_ratio"):
        utils.rowwise_train_test_split(sps.csr_matrix(np.eye(3)), test_ratio=1.5)
    with pytest.raises(ValueError, match="n_held_out"):
        utils.rowwise_train_test_split(sps.csr_matrix(np.eye(3)), n_test=-1)
    with pytest.raises(ValueError, match="width"):
        utils.rowwise_train_test_split(sps.csr_matrix(np.eye(3), dtype=np.complex128))
    with pytest.raises(ValueError, match="random state"):
        utils.convert_randomstate("seed")
    rs = np.random.RandomState(3)
    assert utils.convert_randomstate(rs) is rs
    assert utils.convert_randomstate(5).randint(1 << 30) == np.random.RandomState(5).randint(1 << 30)


# ---- the pandas glue ----------------------------------------------------------------------------------------------------

def _frame():
    import pandas as pd

    return pd.DataFrame(dict(user=["b", "a", "b", "c", "a", "b"], item=[10, 30, 20, 10, 30, 30],
                             rating=[1.0, 2.0, 3.0, 4.0, 5.0, 6.0], ts=[5, 1, 5, 2, 0, 4]))


def test_df_to_sparse_known_answers():
    df = _frame()
    X, uids, iids = utils.df_to_sparse(df, "user", "item")
    assert list(uids) == ["a", "b", "c"] and list(iids) == [10, 20, 30]
    assert sps.isspmatrix_csr(X) and X.dtype == np.float64
    assert np.array_equal(X.toarray(), [[0, 0, 2], [1, 1, 1], [1, 0, 0]])  # ("a", 30) occurs twice: summed
    X, uids, iids = utils.df_to_sparse(df, "user", "item", rating_column="rating")
    assert np.array_equal(X.toarray(), [[0, 0, 7], [1, 3, 6], [4, 0, 0]])
    # given ids: their order, their number; other users and items are dropped
    X, uids, iids = utils.df_to_sparse(df, "user", "item", user_ids=["c", "zz", "b"], item_ids=[30, 10],
                                       rating_column="rating")
    assert list(uids) == ["c", "zz", "b"] and list(iids) == [30, 10]
    assert np.array_equal(X.toarray(), [[0, 4], [0, 0], [6, 1]])


def test_user_pair_known_answers_and_errors():
    Xtr = sps.csr_matrix(np.array([[1, 0, 2], [0, 0, 3]], dtype=np.float64))
    Xte = sps.csr_matrix(np.array([[0, 5, 0], [4, 0, 0]], dtype=np.float64))
    pair = UserTrainTestInteractionPair(np.array(["u", "v"]), Xtr, Xte, item_ids=[7, 8, 9])
    assert pair.user_ids == ["u", "v"] and (pair.n_users, pair.n_items) == (2, 3)
    assert np.array_equal(pair.X_all.toarray(), [[1, 5, 2], [4, 0, 3]])
    tr, te = pair.df_train(), pair.df_test()
    assert list(tr.columns) == ["user_id", "item_id", "rating"]
    assert tr.values.tolist() == [["u", 7, 1.0], ["u", 9, 2.0], ["v", 9, 3.0]]
    assert te.values.tolist() == [["u", 8, 5.0], ["v", 7, 4.0]]
    # no test part: an empty matrix of the same shape
    alone = UserTrainTestInteractionPair(["u", "v"], Xtr, None)
    assert alone.X_test.shape == (2, 3) and alone.X_test.nnz == 0 and (alone.X_all != Xtr).nnz == 0
    with pytest.raises(RuntimeError, match="item_ids"):
        alone.df_train()
    both = pair.concat(alone)
    assert both.user_ids == ["u", "v", "u", "v"] and both.X_train.shape == (4, 3) and both.item_ids is None
    assert np.array_equal(both.X_test.toarray(), np.vstack([Xte.toarray(), np.zeros((2, 3))]))
    with pytest.raises(ValueError, match="user_ids and X_train"):
        UserTrainTestInteractionPair(["u"], Xtr, Xte)
    with pytest.raises(ValueError, match="X_train and X_test"):
        UserTrainTestInteractionPair(["u", "v"], Xtr, Xte[:, :2])
    with pytest.raises(ValueError, match="item_ids"):
        UserTrainTestInteractionPair(["u", "v"], Xtr, Xte, item_ids=[7, 8])
    with pytest.raises(ValueError, match="n_items"):
        pair.concat(UserTrainTestInteractionPair(["w"], sps.csr_matrix((1, 4)), None))


def test_split_last_n_known_answers_and_tie_order():
    df = _frame()
    # sorted by user, then time; b's two rows at ts = 5 keep the frame's order (item 10 before item 20)
    first, held = split_last_n_interaction_df(df, "user", "ts", n_heldout=1)
    assert held[["user", "item"]].values.tolist() == [["a", 30], ["b", 20], ["c", 10]]
    assert first[["user", "item", "ts"]].values.tolist() == [["a", 30, 0], ["b", 30, 4], ["b", 10, 5]]
    first, held = split_last_n_interaction_df(df, "user", "ts", n_heldout=2)
    assert held[["user", "item"]].values.tolist() == [["a", 30], ["a", 30], ["b", 10], ["b", 20], ["c", 10]]
    assert first[["user", "item"]].values.tolist() == [["b", 30]]
    # ratio 0.5: floor gives a 1, b 1, c 0; ceil gives a 1, b 2, c 1
    first, held = split_last_n_interaction_df(df, "user", "ts", heldout_ratio=0.5)
    assert held[["user", "item"]].values.tolist() == [["a", 30], ["b", 20]] and len(first) == 4
    first, held = split_last_n_interaction_df(df, "user", "ts", heldout_ratio=0.5, ceil_n_heldout=True)
    assert held[["user", "item"]].values.tolist() == [["a", 30], ["b", 10], ["b", 20], ["c", 10]] and len(first) == 2
    first, held = split_last_n_interaction_df(df, "user", "ts")  # the default ratio 0.1: nothing of 1 - 3 rows
    assert len(held) == 0 and len(first) == 6


def test_time_ordered_user_split_needs_no_device():
    import pandas as pd

    rng = np.random.RandomState(0)
    df = pd.DataFrame(dict(u=rng.randint(0, 40, 600), i=rng.randint(0, 30, 600), t=rng.randint(0, 1000, 600)))
    data, items = split_dataframe_partial_user_holdout(df, "u", "i", time_column="t", val_user_ratio=0.25,
                                                       test_user_ratio=0.25, heldout_ratio_val=0.5, n_heldout_test=2,
                                                       random_state=1)
    users = [set(data[k].user_ids) for k in ("train", "val", "test")]
    assert [len(s) for s in users] == [20, 10, 10] and set().union(*users) == set(df.u) and len(items) == df.i.nunique()
    assert not (users[0] & users[1] or users[0] & users[2] or users[1] & users[2])
    dedup = df.drop_duplicates(["u", "i"])
    for k in ("val", "test"):
        pair = data[k]
        want, _, __ = utils.df_to_sparse(dedup, "u", "i", user_ids=pair.user_ids, item_ids=items)
        assert (pair.X_all != want).nnz == 0 and pair.X_train.multiply(pair.X_test).nnz == 0
    m = np.diff(data["val"].X_all.indptr)
    assert np.array_equal(np.diff(data["val"].X_test.indptr), m // 2)
    assert np.array_equal(np.diff(data["test"].X_test.indptr), np.minimum(np.diff(data["test"].X_all.indptr), 2))
    assert data["train"].X_test.nnz == 0
    with pytest.raises(ValueError, match="n_val_user exceeds"):
        split_dataframe_partial_user_holdout(df, "u", "i", time_column="t", n_val_user=41)
    with pytest.raises(ValueError, match="n_val_user \\+ n_test_users"):
        split_dataframe_partial_user_holdout(df, "u", "i", time_column="t", n_val_user=30, n_test_user=11)


def test_holdout_specific_interactions_known_answers():
    import pandas as pd

    df = pd.DataFrame(dict(u=np.repeat(np.arange(10), 4), i=np.tile(np.arange(4), 10)))
    marked = (df.i.values == 3) & (df.u.values < 8)  # users 8 and 9 are not validatable
    items, data = holdout_specific_interactions(df, "u", "i", marked, 0.25, 0.25, random_state=0)
    assert list(items) == [0, 1, 2, 3]
    train, val, test = (set(data[k].user_ids) for k in ("train", "val", "test"))
    assert {8, 9} <= train and len(val) == len(test) == 2 and len(train) == 6
    assert train | val | test == set(range(10)) and not (train & val or train & test or val & test)
    assert data["train"].X_test.nnz == 0 and np.array_equal(data["train"].X_train.toarray(), np.ones((6, 4)))
    for k in ("val", "test"):
        assert np.array_equal(data[k].X_test.toarray(), np.tile([0, 0, 0, 1.0], (2, 1)))
        assert np.array_equal(data[k].X_train.toarray(), np.tile([1.0, 1, 1, 0], (2, 1)))
    with pytest.raises(ValueError, match="exceeds 1"):
        holdout_specific_interactions(df, "u", "i", marked, 0.7, 0.7)


# ---- the rule: counts, ties, uniformity (on the restatement) ---------------------------------------------------------------

def test_restatement_counts_and_tie_break():
    m = np.array([0, 1, 3, 10, 100, 90])
    assert n_test_of(m, ratio=0.3).tolist() == [0, 0, 0, 3, 30, 27]
    # 10 * 0.3 rounds to 3.0 itself in double (its ceil is 3, as in the reference's std::ceil(nnz_row * test_ratio));
    # 100 * 0.07 = 7.000000000000001 and 100 * 0.57 = 56.99999999999999 are where the rounding shows
    assert n_test_of(m, ratio=0.3, ceil=True).tolist() == [0, 1, 1, 3, 30, 27]
    assert n_test_of(np.array([100]), ratio=0.07, ceil=True).tolist() == [8] == [math.ceil(100 * 0.07)]
    assert n_test_of(np.array([100]), ratio=0.57).tolist() == [56] == [math.floor(100 * 0.57)]
    assert n_test_of(np.array([90]), ratio=0.7).tolist() == [62]
    assert n_test_of(m, n_held_out=5).tolist() == [0, 1, 3, 5, 5, 5]
    # injected keys 5 5 1 5 9 in two rows: j = 2 first, then the 5s in the order of j
    keys = np.array([5, 5, 1, 5, 9] * 2, dtype=np.uint64)
    for n, want in enumerate([[0, 0, 0, 0, 0], [0, 0, 1, 0, 0], [1, 0, 1, 0, 0], [1, 1, 1, 0, 0], [1, 1, 1, 1, 0],
                              [1, 1, 1, 1, 1]]):
        assert held_out_mask([0, 5, 10], 0, n_held_out=n, keys=keys).astype(int).tolist() == want * 2


@pytest.mark.parametrize("seed", [1, 42])
@pytest.mark.parametrize("m,n", [(2, 1), (3, 1), (4, 2), (5, 2)])
def test_rule_draws_every_subset_uniformly(m, n, seed):
    from scipy.stats import chi2

    rows = 8192
    held = held_out_mask(np.arange(rows + 1) * m, seed, n_held_out=n).reshape(rows, m)
    assert (held.sum(axis=1) == n).all()
    code = held @ (1 << np.arange(m))
    subsets = [sum(1 << j for j in c) for c in itertools.combinations(range(m), n)]
    counts = np.array([(code == s).sum() for s in subsets])
    assert counts.sum() == rows and (counts > 0).all()
    expected = rows / len(subsets)
    stat = float(((counts - expected) ** 2 / expected).sum())
    print(f"m={m} n={n} seed={seed}: chi2={stat:.3f} p={chi2.sf(stat, len(subsets) - 1):.4f}")
    assert stat < chi2.isf(1e-6, len(subsets) - 1)


# ---- the host layer in a program of its own ----------------------------------------------------------------------------------

_HOST_CXX = shutil.which("g++") or shutil.which("clang++")


@pytest.mark.skipif(_HOST_CXX is None, reason="needs a host C++ compiler")
def test_split_host_plan_under_address_and_ub_sanitizers(tmp_path):
    """irspack_amd/csrc/split_host_plan.hpp - n_test in both modes with the double-rounding edges, the lexicographic
    tie-break with injected equal keys, the class bounds at each boundary, the argument checks, the plan's row lists -
    in a program of its own (tests/host/split_host_plan_main.cpp), every report fatal."""
    exe = str(tmp_path / "split_host_plan_main")
    src = os.path.join(ROOT, "tests", "host", "split_host_plan_main.cpp")
    subprocess.check_call([_HOST_CXX, "-std=c++17", "-O1", "-g", "-pthread", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "split_host_plan ok" in r.stdout
