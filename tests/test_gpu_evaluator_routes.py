"""Which route a ``get_metrics_ials`` call takes and what it returns, per configuration, against
tests/golden/eval_routes.json (recorded by tests/golden/make_eval_routes.py before the host decisions of the fused
call moved into csrc/eval_emit_plan.hpp).  The evaluator tests compare results with the oracle; a call that left the
threshold-filtered path, scored more tiles or ranked other rows one by one would pass them.  Exact-integer factors
and fixed-order sums make every recorded field - the path, the tile and hard-row counts, the seven metric fields as
hex floats, a hash of the item counts - reproducible bit for bit.

One child process runs every configuration (the switches are environment variables, read per call)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "eval_routes.json")
RECORDER = os.path.join(ROOT, "tests", "golden", "make_eval_routes.py")


@pytest.mark.gpu
def test_every_configuration_takes_the_route_and_returns_what_it_did_before():
    with open(GOLDEN) as f:
        want = json.load(f)
    r = subprocess.run([sys.executable, RECORDER, "--print"], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-4000:]
    got = json.loads(r.stdout[r.stdout.index("{"):])
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        assert got[name] == want[name], (name, got[name], want[name])
    # the configurations do reach the routes they are there for
    path = {name: rec["path"] for name, rec in want.items()}
    for name in ("K16", "K32", "K64", "K80", "K128", "K192", "K256", "cutoff5", "cutoff24", "cutoff32", "sample_fused0",
                 "sample64", "pass_rows128", "mask_with_call", "mask_cached_again", "mask_none", "users_3_303",
                 "two_level_32832_users"):
        assert path[name] == "emit_bounded", name
    assert path["bound0"] == "emit"
    # (K = 80 is padded to 128 columns, a width the path has; K = 288 to 320, beyond its widest)
    for name in ("K288", "cutoff33", "emit0", "abandon_1200_zero_users"):
        assert path[name] == "two_pass", name
    assert want["K64"]["hard_rows"] == 4  # the two all-zero users and the two that have seen the largest items
    assert want["mask_none"]["hard_rows"] == 2 and want["sample64"]["hard_rows"] > 4  # (64 items: the second chance runs)
    assert want["sample64"]["sample_items"] == 64 and want["K64"]["sample_items"] == 512
    assert want["bound0"]["tiles_scored"] == want["bound0"]["tiles_total"] == 6 * 129
    for k in ("hard_rows", "tiles_total"):  # three passes of 128 users add up to the single pass
        assert want["pass_rows128"][k] == want["K64"][k]
    for name in ("mask_with_call", "mask_cached_again"):  # however the mask arrives
        assert want[name] == want["K64"], name
