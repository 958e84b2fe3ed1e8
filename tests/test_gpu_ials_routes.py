"""Which kernels one iALS epoch launches, per configuration, against tests/golden/ials_launch_names.json (recorded
by tests/golden/make_ials_launch_names.py before the host decisions moved into csrc/ials_host_plan.hpp).  The factor
tests prove that a half-step's results are right; a route that silently fell back to a slower kernel family would
pass them.  The profile names the regions (solve / split / short / fold / iALS++ / long-row CG, per side) and counts
their launches.

One child process runs every configuration (an epoch each): the chunk size of 64 that lets a 2200-entry row split
and fold is read once per process, before the first trainer."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ials_launch_names.json")
RECORDER = os.path.join(ROOT, "tests", "golden", "make_ials_launch_names.py")


@pytest.mark.gpu
def test_every_configuration_launches_what_it_launched_before():
    with open(GOLDEN) as f:
        want = json.load(f)
    r = subprocess.run([sys.executable, RECORDER, "--print"], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-4000:]
    got = json.loads(r.stdout[r.stdout.index("{"):])
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        assert got[name] == want[name], (name, got[name], want[name])
    # the configurations do reach the families they are there for
    assert "ials_fold_partials" in want["K64_CHOLESKY_binary"] and "ials_split_cg_user" in want["K128_CG_binary"]
    assert "ials_short_cg_item" in want["K16_CG_binary"] and "ials_long_cg_user" in want["K192_CG_binary"]
    assert "ials_ialspp_px" in want["K64_IALSPP_sub64"] and "ials_ialspp_px" not in want["K64_IALSPP_sub16"]
