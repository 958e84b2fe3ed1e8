"""Records, per configuration, which route one ``get_metrics_ials`` call takes and what it returns:
``eval_routes.json``, the golden of tests/test_gpu_evaluator_routes.py.  The evaluator tests compare results with
the oracle; they would not notice a call that left the threshold-filtered path for the two-pass one, scored more
tiles than before or sent other rows to the one-by-one ranking.  Recorded before the host decisions of the fused
call moved into csrc/eval_emit_plan.hpp.

Needs a GPU and the built library:

    python tests/golden/make_eval_routes.py            # writes the golden
    python tests/golden/make_eval_routes.py --print    # prints the same JSON (what the test runs)

Per configuration: ``last_call_stats()``'s path, hard_rows, tiles_total, tiles_scored and sample_items, the seven
metric fields as ``float.hex()`` and a SHA-256 of the item counts.  The factors are small integers set through
``t.user`` / ``t.item``: every score is exact, ties are plentiful, no trained model is involved, and the
fixed-order sums make every field reproducible bit for bit.

Shape: 330 users x 8,250 items - above the 8,192-item floor of the filtered path, with a partial last user tile,
item tile and bitmap word.  User 7 has no ground truth; users 5 and 6 are all zero (every score ties: the
candidate list overflows -> hard rows); users 10 and 11 have seen the 5,000 items of largest norm and every item
that ties with the last of them (no threshold from either sample -> second chance -> hard rows).
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import scipy.sparse as sps

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
GOLDEN = os.path.join(HERE, "eval_routes.json")

N_USERS, N_ITEMS = 330, 8250
NO_GT, ZERO_USERS, SEEN_TOP = 7, (5, 6), (10, 11)
SWITCHES = ("IRSPACK_AMD_EVAL_EMIT", "IRSPACK_AMD_EVAL_BOUND", "IRSPACK_AMD_EVAL_SAMPLE_FUSED",
            "IRSPACK_AMD_EVAL_SAMPLE", "IRSPACK_AMD_EVAL_PASS_ROWS")

# (name, K, cutoff, switches, mask: "cached" | "call" | None, (begin, end), extra all-zero users)
WHOLE = (0, N_USERS)
CONFIGS = (  # (configurations of one model stand together: one model at a time is kept on the device)
    [(f"K{K}", K, 20, {}, "cached", WHOLE, 0) for K in (16, 32, 128, 192, 256, 80, 288, 64)]
    + [("mask_cached_again", 64, 20, {}, "cached", WHOLE, 0)]  # (the mask object of "K64": nothing is uploaded)
    + [(f"cutoff{c}", 64, c, {}, "cached", WHOLE, 0) for c in (5, 24, 32, 33)]
    + [("emit0", 64, 20, {"IRSPACK_AMD_EVAL_EMIT": "0"}, "cached", WHOLE, 0),
       ("bound0", 64, 20, {"IRSPACK_AMD_EVAL_BOUND": "0"}, "cached", WHOLE, 0),
       ("sample_fused0", 64, 20, {"IRSPACK_AMD_EVAL_SAMPLE_FUSED": "0"}, "cached", WHOLE, 0),
       ("sample64", 64, 20, {"IRSPACK_AMD_EVAL_SAMPLE": "64"}, "cached", WHOLE, 0),
       ("pass_rows128", 64, 20, {"IRSPACK_AMD_EVAL_PASS_ROWS": "128"}, "cached", WHOLE, 0),
       ("mask_with_call", 64, 20, {}, "call", WHOLE, 0),
       ("mask_none", 64, 20, {}, None, WHOLE, 0),
       ("users_3_303", 64, 20, {}, "cached", (3, 303), 0),
       ("abandon_1200_zero_users", 16, 20, {}, "cached", (0, N_USERS + 1200), 1200),
       ("two_level_32832_users", 16, 20, {}, None, (0, 32832), 0)]
)


def model(K, n_users, extra_zero):
    """-> (user factors, item factors, mask, ground truth) for `n_users` users, the last `extra_zero` all zero"""
    rng = np.random.default_rng(1000 * K + n_users)
    user = rng.integers(-2, 3, size=(n_users, K)).astype(np.float32)
    item = rng.integers(-2, 3, size=(N_ITEMS, K)).astype(np.float32)
    user[list(ZERO_USERS)] = 0.0
    if extra_zero:
        user[n_users - extra_zero:] = 0.0
    norm2 = (item.astype(np.float64) ** 2).sum(axis=1)  # (exact: small integers)
    seen = np.flatnonzero(norm2 >= np.sort(norm2)[::-1][4999])  # the 5,000 of largest norm and what ties with the last
    unseen = np.flatnonzero(norm2 < np.sort(norm2)[::-1][4999])
    rows = [rng.integers(0, n_users, size=int(0.02 * n_users * N_ITEMS))]
    cols = [rng.integers(0, N_ITEMS, size=rows[0].size)]
    for u in SEEN_TOP:
        rows.append(np.full(seen.size, u))
        cols.append(seen)
    mask = sps.csr_matrix((np.ones(sum(r.size for r in rows), dtype=np.float32),
                           (np.concatenate(rows), np.concatenate(cols))), shape=(n_users, N_ITEMS))
    mask.sum_duplicates()
    mask.data[:] = 1.0
    mask.sort_indices()
    g_rows = rng.integers(0, n_users, size=int(0.003 * n_users * N_ITEMS))
    g_cols = rng.integers(0, N_ITEMS, size=g_rows.size)
    keep = ~np.isin(g_rows, (NO_GT,) + SEEN_TOP)
    g_rows = np.concatenate([g_rows[keep], np.array(ZERO_USERS + SEEN_TOP)])
    g_cols = np.concatenate([g_cols[keep], np.array([17, 18, unseen[3], unseen[40]])])  # (something to find)
    gt = sps.csr_matrix((np.ones(g_rows.size), (g_rows, g_cols)), shape=(n_users, N_ITEMS))
    gt.sum_duplicates()
    gt.data[:] = 1.0
    return user, item, mask, gt


def metrics_with_call_mask(core, t, begin, end, mask, cutoff, offset):
    """The C entry point with the mask rows among its arguments (the wrapper always caches the mask first)."""
    from irspack_amd import _lib
    from irspack_amd._lib import MetricsStruct, check, lib, ptr
    from irspack_amd.evaluation._core_evaluator import Metrics

    core.get_metrics_ials(t, begin, end, None, cutoff, offset)  # (drops a cached mask)
    _, mp, mi, _ = _lib.csr_arrays(mask, np.float32)
    st, cnt = MetricsStruct(), np.zeros(core.n_items, dtype=np.int64)
    check(lib().irs_eval_get_metrics_ials(core._h, t._h, C.c_int64(begin), C.c_int64(end), ptr(mp, C.c_int64),
                                          ptr(mi, C.c_int32), C.c_int64(cutoff), C.c_int64(offset), C.c_int32(0),
                                          C.byref(st), ptr(cnt, C.c_int64)))
    return Metrics._from_struct(core.n_items, st, cnt)


def record():
    from irspack_amd.evaluation._core_evaluator import EvaluatorCore
    from irspack_amd.recommenders._ials_core import IALSModelConfigBuilder, IALSTrainer

    for k in SWITCHES:
        os.environ.pop(k, None)
    built, out = {}, {}
    for name, K, cutoff, switches, mask_mode, (begin, end), extra_zero in CONFIGS:
        n_users = max(N_USERS, end)
        key = (K, n_users)
        if key not in built:
            user, item, mask, gt = model(K, n_users, extra_zero)
            t = IALSTrainer(IALSModelConfigBuilder().set_K(K).build(), sps.csr_matrix((n_users, N_ITEMS), dtype=np.float32))
            t.user, t.item = user, item
            built = {key: (t, mask, {}, EvaluatorCore(gt, []))}  # (one model at a time on the device)
        t, mask, slices, core = built[key]
        if (begin, end) not in slices:  # (the same object again: the wrapper keeps its device copy)
            slices[(begin, end)] = mask if (begin, end) == (0, n_users) else sps.csr_matrix(mask[begin:end])
        os.environ.update(switches)
        try:
            if mask_mode == "call":
                m = metrics_with_call_mask(core, t, begin, end, slices[(begin, end)], cutoff, begin)
            else:
                m = core.get_metrics_ials(t, begin, end, slices[(begin, end)] if mask_mode else None, cutoff, begin)
        finally:
            for k in switches:
                os.environ.pop(k, None)
        stats = core.last_call_stats()
        out[name] = {
            **{k: stats[k] for k in ("path", "hard_rows", "tiles_total", "tiles_scored", "sample_items")},
            **{k: float(getattr(m, k)).hex() for k in ("valid_user", "total_user", "hit", "recall", "ndcg", "precision", "map")},
            "item_cnt_sha256": hashlib.sha256(np.ascontiguousarray(m.item_cnt, dtype=np.int64).tobytes()).hexdigest(),
        }
    return out


if __name__ == "__main__":
    text = json.dumps(record(), indent=1, sort_keys=True)
    if "--print" in sys.argv:
        print(text)
    else:
        with open(GOLDEN, "w") as f:
            f.write(text + "\n")
        print("wrote", GOLDEN)
