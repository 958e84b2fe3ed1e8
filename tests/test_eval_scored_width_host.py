"""The host rule of the evaluator's ``*_scored`` model calls - ``0 < n_scored <= n_items`` for an item operand of
``n_scored`` columns in a block of ``n_items`` (irspack_amd/csrc/eval_host_prep.hpp: ``scored_width``) - in a program
of its own (tests/host/eval_scored_width_main.cpp), compiled with the host compiler: under AddressSanitizer + UBSan
with every report fatal, and plain at -O3 as the library is built."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HOST_CXX = shutil.which("g++") or shutil.which("clang++")


def _build_and_run(tmp_path, flags):
    exe = str(tmp_path / "eval_scored_width_main")
    src = os.path.join(ROOT, "tests", "host", "eval_scored_width_main.cpp")
    subprocess.check_call([_HOST_CXX, "-std=c++17", "-pthread", *flags, src, "-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, timeout=600)


@pytest.mark.skipif(_HOST_CXX is None, reason="needs a host C++ compiler")
def test_scored_width_rule_under_address_and_ub_sanitizers(tmp_path):
    r = _build_and_run(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                  "-fno-omit-frame-pointer"])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "eval_scored_width ok" in r.stdout


@pytest.mark.skipif(_HOST_CXX is None, reason="needs a host C++ compiler")
def test_scored_width_rule_plain_optimised_build(tmp_path):
    r = _build_and_run(tmp_path, ["-O3", "-ffp-contract=off"])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "eval_scored_width ok" in r.stdout
