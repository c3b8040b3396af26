"""The filter-and-refine plan (codesearch_amd/csrc/filter_plan.hpp) on the CPU: tests/cpp/filter_plan_test.cpp pins the phase
boundaries, filter kernels and launch shapes that scan_filter.hip launches; no GPU involved."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "filter_plan_test.cpp")


def test_filter_plan_matches_recorded_launches():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "filter_plan_test")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "filter plan ok" in r.stdout
