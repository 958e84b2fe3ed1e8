"""What the truncated SVD, the NMF fit, EASE / EDLAE, SLIM, BPR / WARP, Mult-VAE and the iALS feature ridge return,
per configuration, against tests/golden/sparse_block_results.json (recorded by
tests/golden/make_sparse_block_results.py before the host code these fits share moved into csr_checks.hpp,
phase_spans.hpp, sparse_block_plan.hpp, sparse_block.hpp and tile_solver_calls.hpp).  The parity tests of these
modules compare with restatements to a tolerance; a launch with another grid, width or slab count, a product kernel
of the wrong instance or a block column left out of the Cholesky loop could stay inside it.  Every sum on these
paths has a fixed order, so the recorded hashes of every output array are reproducible bit for bit.

One child process runs every configuration (the phase switches are environment variables, read when a handle is
made)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sparse_block_results.json")
RECORDER = os.path.join(ROOT, "tests", "golden", "make_sparse_block_results.py")


@pytest.mark.gpu
def test_every_configuration_returns_the_bytes_it_did_before():
    with open(GOLDEN) as f:
        want = json.load(f)
    r = subprocess.run([sys.executable, RECORDER, "--print"], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-4000:]
    got = json.loads(r.stdout[r.stdout.index("{"):])
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        assert got[name] == want[name], (name, got[name], want[name])
    # the configurations do reach the branches they are there for: every padded width, both orientations
    for m in ("X", "Xt"):
        for l, l_pad in ((1, 64), (64, 64), (65, 128), (129, 192), (257, 320), (513, 576)):
            rec = want[f"svd_{m}_l{l}"]
            assert rec["l_pad"] == l_pad and rec["n_spmm"] == 5, (m, l, rec)  # range 3, project 1, finish 1
        assert len({want[f"svd_{m}_l{l}"]["z"] for l in (1, 64, 65, 129, 257, 513)}) == 6
    # the fit does not depend on whether its phases are timed
    for k in (1, 65, 257, 513):
        for update_H in (0, 1):
            plain, timed = (want[f"nmf_k{k}_updateH{update_H}_stats{s}"] for s in (0, 1))
            assert plain["n_iter"] == timed["n_iter"] == 2
            assert (plain["W"], plain["H"]) == (timed["W"], timed["H"]), (k, update_H)
        assert want[f"nmf_k{k}_updateH0_stats0"]["H"] != want[f"nmf_k{k}_updateH1_stats0"]["H"]
    for trainer in ("bpr", "warp", "multvae"):
        assert want[f"{trainer}_phases0"] == want[f"{trainer}_phases1"], trainer
        assert want[f"{trainer}_phases0"]["epoch"] == 2
    assert len({want[f"ease_{n}items"]["W"] for n in (1, 64, 65, 129, 321)} | {want["edlae_129items"]["W"]}) == 6
    assert want["slim_65items_positive0"] != want["slim_65items_positive1"]
