"""The host ledger of an index, no GPU: codesearch_amd/csrc/index_ledger.hpp (ids, stored rows, tombstones and the group
table: everything cs_index numbers its rows by) through tests/cpp/index_ledger_test.cpp — random walks of append / remove /
build / set_groups / clear against a model written the slow way, and the directed cases of the emptied index, the reclaim
threshold, the top of the id space, runs of ids across a hole, a remove after the reclaim and clear().  Once as an ordinary
build, once under AddressSanitizer + UBSan (`make -C tests/cpp index_ledger_asan`: a stand-alone program, CPU only)."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
SRC = os.path.join(CPP, "index_ledger_test.cpp")


def _run(exe, env=None):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "index ledger ok", r.stdout + r.stderr


def test_index_ledger_cpp():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "index_ledger_test")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe], check=True)
        _run(exe)


def test_index_ledger_under_sanitizers():
    import fcntl

    with open(os.path.join(CPP, ".asan_build.lock"), "w") as lock:  # pytest-xdist workers build one at a time
        fcntl.flock(lock, fcntl.LOCK_EX)
        subprocess.run(["make", "-s", "-C", CPP, "index_ledger_asan"], check=True)
    _run(os.path.join(CPP, "index_ledger_asan"),
         dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
