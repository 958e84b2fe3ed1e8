"""The multi-threaded HOST preparation of the library compiled on its own with the host compiler and run under
ThreadSanitizer and AddressSanitizer + UBSan ("race detection").  GPU sanitizers are not
available on the pool; this covers the code that runs on host threads:
- tests/san/host_prep_san.cpp: irspack_amd/csrc/host_prep.hpp (counting-sort transposes, validated CSR copies, the
  parallel libstdc++ random stream) and the construction helpers of knn_host_prep.hpp (host_csr, transpose,
  transpose_pattern, column_counts, the weight tables, for_rows_parallel).  It compares every multi-threaded
  result with a sequential one, and the parallel random stream with std::normal_distribution<float> itself
  (> 2^18 values).
- tests/host/knn_host_prep_main.cpp: the rest of knn_host_prep.hpp, i.e. what a kNN compute call does on the host
  before it launches - entry scan, chunk cuts, the threaded target pass, launch order, variant choice, arena layout.
- tests/host/eval_host_prep_main.cpp: eval_host_prep.hpp, and eval_emit_plan.hpp, i.e. what the evaluator decides on the
  host - the domain and shape of a pass of the threshold-filtered path, the ranking dispatch, the item-histogram
  table (against the former chains of conditions, both sides of every boundary).
- tests/host/ials_host_plan_main.cpp: ials_host_plan.hpp, i.e. what the iALS path decides on the host - the task plan
  of a side (chunks, fold groups, the short tail, the row classes) and the route of a half-step (kernel family and
  instance flags, against the former chains of conditions).
- tests/host/sparse_block_plan_main.cpp: sparse_block_plan.hpp and csr_checks.hpp, i.e. what the truncated SVD and
  the NMF fit decide on the host - the segment plan of a matrix, the slabs of a Gram pass, the width of a product
  kernel (against the former code, written out) - and the checks of a caller's CSR matrix, message by message.
- tests/host/slim_host_plan_main.cpp: slim_host_plan.hpp, i.e. what the SLIM fit decides on the host - where the
  running vector of the descent lives, the workgroup width, the workgroup count and whether the dynamic-LDS limit is
  raised, against expectations written out by hand on both sides of every boundary.
The stream, event and buffer handling of knn.hip itself needs a device and is not compiled here."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "san", "host_prep_san.cpp")


def _build_and_run(tmp_path, flags, env_extra):
    exe = str(tmp_path / "host_prep_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-pthread", *flags, SRC, "-o", exe]
    subprocess.check_call(cmd)
    env = dict(os.environ, **env_extra)
    return subprocess.run([exe], env=env, capture_output=True, text=True, timeout=900)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_preparation_under_thread_sanitizer(tmp_path):
    r = _build_and_run(tmp_path, ["-fsanitize=thread"], {"TSAN_OPTIONS": "halt_on_error=1 second_deadlock_stack=1"})
    if "unexpected memory mapping" in r.stderr or "personality" in r.stderr:
        pytest.skip("ThreadSanitizer cannot map its shadow memory in this container: " + r.stderr[:200])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "WARNING: ThreadSanitizer" not in r.stderr, r.stderr[-4000:]
    assert "host_prep_san ok" in r.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_preparation_under_address_and_ub_sanitizers(tmp_path):
    r = _build_and_run(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                  "-fno-omit-frame-pointer"],
                       {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert r.returncode == 0, r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "host_prep_san ok" in r.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_preparation_plain_optimised_build(tmp_path):
    """The same harness without a sanitizer at -O3: this is the build in which the bulk Mersenne
    Twister runs its AVX2 clones (the sanitizer builds take the plain loops - an ifunc resolver
    runs before a sanitizer's runtime is up), compared word for word with std::mt19937 and
    variate for variate with std::normal_distribution."""
    r = _build_and_run(tmp_path, ["-O3"], {})
    assert r.returncode == 0, r.stderr[-4000:]
    assert "host_prep_san ok" in r.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("san", ["thread", "address"])
def test_cpu_oracle_under_sanitizers(san):
    """`make -C oracle SAN=thread|address san`: the multi-threaded CPU oracle (atomic-cursor row
    dispatch, per-thread Gramian partials; two epochs of each solver on 4 threads)."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), f"SAN={san}", "san"])
    exe = os.path.join(ROOT, "oracle", "_san", f"oracle_san_{san}")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, TSAN_OPTIONS="halt_on_error=1"))
    if "unexpected memory mapping" in r.stderr:
        pytest.skip("ThreadSanitizer cannot map its shadow memory in this container")
    assert r.returncode == 0, r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "oracle_san ok" in r.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("portable", [False, True])
def test_mt19937_jump_ahead_arithmetic(tmp_path, portable):
    """Products modulo MT19937's characteristic polynomial against a bit-by-bit reference, the tabulated
    polynomial against Berlekamp-Massey, jumps against the engine's own sequence - with the carry-less
    multiplier and with the portable product a host without PCLMULQDQ takes (mt_jump.hpp)."""
    exe = str(tmp_path / "mt_jump_check")
    src = os.path.join(ROOT, "tests", "san", "mt_jump_check.cpp")
    flags = ["-DIRS_MTJUMP_NO_CLMUL"] if portable else []
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", *flags, src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "mt_jump_check ok" in r.stdout
    if portable:
        assert "portable product" in r.stdout


_HOST_CXX = shutil.which("g++") or shutil.which("clang++")


def _eval_host_prep(tmp_path, flags):
    exe = str(tmp_path / "eval_host_prep_main")
    src = os.path.join(ROOT, "tests", "host", "eval_host_prep_main.cpp")
    subprocess.check_call([_HOST_CXX, "-std=c++17", "-pthread", *flags, src, "-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, timeout=600)


@pytest.mark.skipif(_HOST_CXX is None, reason="needs a host C++ compiler")
def test_evaluator_host_preparation_under_address_and_ub_sanitizers(tmp_path):
    """irspack_amd/csrc/eval_host_prep.hpp - profile, mask and candidate rows, the launch order, the rows per
    score block (against the five formulas of the entry points, written out), the scan of a sparse W - and
    eval_emit_plan.hpp - the pass plan of the threshold-filtered path, the pass size, the bitmap and abandon rules,
    the ranking dispatch and the histogram table against the former condition chains - in a program of its own
    (tests/host/eval_host_prep_main.cpp), every report fatal."""
    r = _eval_host_prep(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                   "-fno-omit-frame-pointer"])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "eval_host_prep ok" in r.stdout


@pytest.mark.skipif(_HOST_CXX is None, reason="needs a host C++ compiler")
def test_evaluator_host_preparation_plain_optimised_build(tmp_path):
    """The same program without a sanitizer at -O3 with the library's -ffp-contract=off: the build in which the
    plan's integer divisions and the bitmap rule's float64 product run as the library runs them."""
    r = _eval_host_prep(tmp_path, ["-O3", "-ffp-contract=off"])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "eval_host_prep ok" in r.stdout


def _knn_host_prep(tmp_path, flags, env_extra):
    exe = str(tmp_path / "knn_host_prep_main")
    src = os.path.join(ROOT, "tests", "host", "knn_host_prep_main.cpp")
    subprocess.check_call([_HOST_CXX, "-std=c++17", "-O1", "-g", "-pthread", "-ffp-contract=off", *flags,
                           "-fno-omit-frame-pointer", src, "-o", exe])
    return subprocess.run([exe], env=dict(os.environ, **env_extra), capture_output=True, text=True, timeout=600)


@pytest.mark.skipif(_HOST_CXX is None, reason="needs a host C++ compiler")
def test_knn_host_preparation_under_address_and_ub_sanitizers(tmp_path):
    """irspack_amd/csrc/knn_host_prep.hpp - the entry scan, the chunk cuts, the threaded target pass (malformed row
    pointers and indices included: nothing outside the arrays is read), the launch order, the kernel-variant choice
    (against the former chain of conditions, written out), the arena layout - in a program of its own
    (tests/host/knn_host_prep_main.cpp), every report fatal."""
    r = _knn_host_prep(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], {})
    assert r.returncode == 0, r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "knn_host_prep ok" in r.stdout


@pytest.mark.skipif(_HOST_CXX is None, reason="needs a host C++ compiler")
def test_knn_host_preparation_under_thread_sanitizer(tmp_path):
    """The same program under ThreadSanitizer: the target pass on 1, 2 and 5 threads fills its three tables and
    sets its flags without a race."""
    r = _knn_host_prep(tmp_path, ["-fsanitize=thread"], {"TSAN_OPTIONS": "halt_on_error=1 second_deadlock_stack=1"})
    if "unexpected memory mapping" in r.stderr or "personality" in r.stderr:
        pytest.skip("ThreadSanitizer cannot map its shadow memory in this container: " + r.stderr[:200])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "WARNING: ThreadSanitizer" not in r.stderr, r.stderr[-4000:]
    assert "knn_host_prep ok" in r.stdout


def _ials_host_plan(tmp_path, flags, env_extra):
    exe = str(tmp_path / "ials_host_plan_main")
    src = os.path.join(ROOT, "tests", "host", "ials_host_plan_main.cpp")
    subprocess.check_call([_HOST_CXX, "-std=c++17", "-O1", "-g", "-pthread", "-ffp-contract=off", *flags,
                           "-fno-omit-frame-pointer", src, "-o", exe])
    return subprocess.run([exe], env=dict(os.environ, **env_extra), capture_output=True, text=True, timeout=600)


@pytest.mark.skipif(_HOST_CXX is None, reason="needs a host C++ compiler")
def test_ials_host_plan_under_address_and_ub_sanitizers(tmp_path):
    """irspack_amd/csrc/ials_host_plan.hpp - the task plan at the sizes where the chunk rule changes (exact lists for
    hand-made row pointers; tiling, dense slots, fold groups, the short tail that stops at a split row's chunk), the
    regulariser on several threads, the route of a half-step and the iALS++ variant over every switch setting against
    the former chains of conditions - in a program of its own (tests/host/ials_host_plan_main.cpp), every report fatal."""
    r = _ials_host_plan(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], {})
    assert r.returncode == 0, r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "ials_host_plan ok" in r.stdout


@pytest.mark.skipif(_HOST_CXX is None, reason="needs a host C++ compiler")
def test_ials_host_plan_under_thread_sanitizer(tmp_path):
    """The same program under ThreadSanitizer: the regulariser pass on several threads, and the route enumeration
    on eight (there with every 29th switch setting: every access is instrumented)."""
    r = _ials_host_plan(tmp_path, ["-fsanitize=thread"], {"TSAN_OPTIONS": "halt_on_error=1 second_deadlock_stack=1"})
    if "unexpected memory mapping" in r.stderr or "personality" in r.stderr:
        pytest.skip("ThreadSanitizer cannot map its shadow memory in this container: " + r.stderr[:200])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "WARNING: ThreadSanitizer" not in r.stderr, r.stderr[-4000:]
    assert "ials_host_plan ok" in r.stdout


@pytest.mark.skipif(_HOST_CXX is None, reason="needs a host C++ compiler")
def test_ials_host_plan_plain_optimised_build(tmp_path):
    """The same program without a sanitizer at -O3 (with the library's -ffp-contract=off): the build whose float
    arithmetic is the library's."""
    r = _ials_host_plan(tmp_path, ["-O3"], {})
    assert r.returncode == 0, r.stderr[-4000:]
    assert "ials_host_plan ok" in r.stdout


def _sparse_block_plan(tmp_path, flags):
    exe = str(tmp_path / "sparse_block_plan_main")
    src = os.path.join(ROOT, "tests", "host", "sparse_block_plan_main.cpp")
    subprocess.check_call([_HOST_CXX, "-std=c++17", "-pthread", *flags, src, "-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, timeout=600)


@pytest.mark.skipif(_HOST_CXX is None, reason="needs a host C++ compiler")
def test_sparse_block_plan_under_address_and_ub_sanitizers(tmp_path):
    """irspack_amd/csrc/sparse_block_plan.hpp - the segment plan at row lengths round the segment length (split rows,
    their consecutive slots, the stable longest-first order, empty and zero-row matrices), the slabs of a Gram pass
    and the width of a product kernel against the former code, written out - and csr_checks.hpp - every message at
    its first failing condition, their precedence, null arrays at nnz = 0, zero rows - in a program of its own
    (tests/host/sparse_block_plan_main.cpp), every report fatal."""
    r = _sparse_block_plan(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                      "-fno-omit-frame-pointer"])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "sparse_block_plan ok" in r.stdout


@pytest.mark.skipif(_HOST_CXX is None, reason="needs a host C++ compiler")
def test_sparse_block_plan_plain_optimised_build(tmp_path):
    """The same program without a sanitizer at -O3 with the library's -ffp-contract=off: the build whose integer
    divisions run as the library runs them."""
    r = _sparse_block_plan(tmp_path, ["-O3", "-ffp-contract=off"])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "sparse_block_plan ok" in r.stdout


def _slim_host_plan(tmp_path, flags):
    exe = str(tmp_path / "slim_host_plan_main")
    src = os.path.join(ROOT, "tests", "host", "slim_host_plan_main.cpp")
    subprocess.check_call([_HOST_CXX, "-std=c++17", "-pthread", *flags, src, "-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, timeout=600)


@pytest.mark.skipif(_HOST_CXX is None, reason="needs a host C++ compiler")
def test_slim_host_plan_under_address_and_ub_sanitizers(tmp_path):
    """irspack_amd/csrc/slim_host_plan.hpp - the launch decision of the SLIM descent at 1 item, on both sides of the
    40 KiB, 64 KiB and 80 KiB steps, at the last catalogue that fits a per-block limit of 64 KiB and of 160 KiB and
    the first that does not, with the switch off, with fewer and more items than workgroups, and at 2^31 - 1 items
    (the clamp that keeps the byte count inside an int) - in a program of its own
    (tests/host/slim_host_plan_main.cpp), every report fatal."""
    r = _slim_host_plan(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                   "-fno-omit-frame-pointer"])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "slim_host_plan ok" in r.stdout


@pytest.mark.skipif(_HOST_CXX is None, reason="needs a host C++ compiler")
def test_slim_host_plan_plain_optimised_build(tmp_path):
    """The same program without a sanitizer at -O3 with the library's -ffp-contract=off: the build whose integer
    divisions run as the library runs them."""
    r = _slim_host_plan(tmp_path, ["-O3", "-ffp-contract=off"])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "slim_host_plan ok" in r.stdout
