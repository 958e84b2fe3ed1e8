"""The route field of the LDS-staged bf16x3 gather (``SolveRoute::x3_lds``, irspack_amd/csrc/ials_host_plan.hpp) on
the host alone: tests/host/ials_gather_lds_route_main.cpp enumerates sizes, solvers, switches and side facts and
checks the field against its one-sentence rule, and that no other field of the route moves with the switch."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HOST_CXX = shutil.which("g++") or shutil.which("clang++")


@pytest.mark.skipif(_HOST_CXX is None, reason="needs a host C++ compiler")
@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_gather_lds_route(tmp_path, flags):
    exe = str(tmp_path / "ials_gather_lds_route_main")
    src = os.path.join(ROOT, "tests", "host", "ials_gather_lds_route_main.cpp")
    subprocess.check_call([_HOST_CXX, "-std=c++17", "-pthread", "-ffp-contract=off", *flags, src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert "ials_gather_lds_route ok" in r.stdout
