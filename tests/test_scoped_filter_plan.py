"""The plan and the route of a scoped search through the int8 filter (codesearch_amd/csrc/scoped_filter_plan.hpp) on the
CPU: tests/cpp/scoped_filter_plan_test.cpp checks, over synthetic ascending row lists, that phase 0's entries and the
filter phases' row ranges cover every list entry exactly once, the phase-0 count, the 1,024-row granule, that every phase
keeps plan_filter's kernel choice, and the route predicate with its forced routes; no GPU involved."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "scoped_filter_plan_test.cpp")


def test_scoped_filter_plan_covers_every_list_entry_once():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "scoped_filter_plan_test")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "scoped filter plan ok" in r.stdout
