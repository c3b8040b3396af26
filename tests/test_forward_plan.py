"""The route of an encoder forward (codesearch_amd/csrc/forward_plan.hpp) on the CPU: tests/cpp/forward_plan_test.cpp pins which
launch sequence a slice of a mini-batch takes, the kernel of each dense layer, what is fused and how many slices the mini-batch is
cut into for each shape; no GPU involved."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "forward_plan_test.cpp")


def test_forward_plan_matches_recorded_plans():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "forward_plan_test")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "forward plan ok" in r.stdout
