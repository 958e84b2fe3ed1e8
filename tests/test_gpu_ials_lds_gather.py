"""The LDS-staged gather of the bf16x3 Cholesky kernel at K <= 64 (``syrk_gather_bf16x3_lds``, ials_kernels.hpp;
``IRSPACK_AMD_IALS_GATHER_LDS``, default on) against the register-staged one it replaces, bit for bit, and against
the float64 arbiter.

The matrix: binary, 2,304 items, user rows of exactly 0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128,
129, 1023, 1024, 1025 and 2,100 entries, twelve of each, shuffled - the empty row, a row whose second group is never
fetched, odd and even group counts, the index-block edge at 64, rounds of the two-group loop with one and two
groups behind them, and the split-row edge at 1,024 with the chunk tasks above it.  The transpose supplies the item
side's lengths (10 .. 60 entries: both sides of one group).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sps

from conftest import assert_float64_bar  # (first: it puts the repository root on sys.path, also for __main__ below)

import _operating_point as OP  # noqa: E402
import oracle as O  # noqa: E402
from irspack_amd.recommenders._ials_core import IALSTrainer

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 1023, 1024, 1025, 2100]
COPIES, N_ITEMS = 12, 2304
SWITCH = "IRSPACK_AMD_IALS_GATHER_LDS"
ALPHA0, REG = 0.1, 1e-2
KEYS = ("user1", "item1", "half_user", "half_item", "user2", "item2")


def make_matrix():
    rng = np.random.default_rng(2304)
    deg = np.repeat(LENGTHS, COPIES)
    rng.shuffle(deg)
    rows = np.repeat(np.arange(deg.size), deg)
    cols = np.concatenate([rng.choice(N_ITEMS, size=d, replace=False) for d in deg])
    X = sps.csr_matrix((np.ones(rows.size, np.float32), (rows, cols)), shape=(deg.size, N_ITEMS))
    X.sort_indices()
    assert np.array_equal(np.diff(X.indptr), deg)
    return X


def run(X, K, switch):
    """One epoch; from its factors one half-step per side (what the arbiter is asked about); then the second
    epoch.  A failed factorisation (err_flag) raises out of step / synchronize."""
    old = os.environ.get(SWITCH)
    if switch is None:
        os.environ.pop(SWITCH, None)
    else:
        os.environ[SWITCH] = switch
    try:
        mc, sc, _, _ = OP.configs(K, "CHOLESKY", ALPHA0, REG)
        t = IALSTrainer(mc, X)  # (the switch is read here)
    finally:
        if old is None:
            os.environ.pop(SWITCH, None)
        else:
            os.environ[SWITCH] = old
    out = {}
    t.step(sc)
    out["user1"], out["item1"] = t.user, t.item
    for side, key in enumerate(("half_user", "half_item")):
        t.user, t.item = out["user1"], out["item1"]
        OP.gpu_half_step(t, side, sc)
        out[key] = t.user if side == 0 else t.item
    t.user, t.item = out["user1"], out["item1"]
    t.step(sc)
    out["user2"], out["item2"] = t.user, t.item
    return out


def check(X, K, on, off, what):
    for key in KEYS:
        assert np.isfinite(on[key]).all(), (what, key)
        assert np.array_equal(on[key], off[key]), (what, key, int((on[key] != off[key]).sum()))
    _, _, omc, osc = OP.configs(K, "CHOLESKY", ALPHA0, REG)
    Xt = OP.transpose_csr(X)
    for Xs, key, tgt0, oth0 in ((X, "half_user", on["user1"], on["item1"]), (Xt, "half_item", on["item1"], on["user1"])):
        want = O.ials_solver_step(tgt0, Xs, oth0, O.ials_gramian(oth0, omc.alpha0, OP.CORES), omc, osc)
        ref64 = O.ials_solver_step_f64(tgt0, Xs, oth0, None, omc, osc, OP.CORES)
        assert_float64_bar(on[key], want, ref64, f"{what} K={K} {key}", test="ials_lds_gather")


@pytest.fixture(scope="module")
def X():
    return make_matrix()


@pytest.mark.parametrize("K", [64, 50])
def test_lds_gather_equals_register_gather_and_meets_float64(X, K):
    check(X, K, run(X, K, None), run(X, K, "0"), "lds gather")


def test_lds_gather_with_chunks_lowered(X, tmp_path):
    """Rows above 256 entries cut into chunks: chunk tasks store LDS-staged partials, the MODE 1 pass sums and
    solves them.  ``IRSPACK_AMD_IALS_CHUNK`` is read once per process, hence a process of its own (this file as a
    program), which leaves both runs' factors for the checks here."""
    out = str(tmp_path / "chunk.npz")
    env = dict(os.environ, IRSPACK_AMD_IALS_CHUNK="256", IRSPACK_AMD_IALS_CHUNK_LONG="512")
    env.pop(SWITCH, None)
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, os.path.abspath(__file__), out], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    z = np.load(out)
    on = {k: z["on_" + k] for k in KEYS}
    off = {k: z["off_" + k] for k in KEYS}
    check(X, 64, on, off, "lds gather, chunk 256")


if __name__ == "__main__":  # the chunk case's own process
    Xm = make_matrix()
    res = {}
    for name, switch in (("on", None), ("off", "0")):
        for k, v in run(Xm, 64, switch).items():
            res[f"{name}_{k}"] = v
    np.savez(sys.argv[1], **res)
