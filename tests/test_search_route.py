"""The route of an index search (codesearch_amd/csrc/search_route.hpp) on the CPU: tests/cpp/search_route_test.cpp pins which
path, query source and prime pass index.hip run_search launches for each shape; no GPU involved."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "search_route_test.cpp")


def test_search_route_matches_recorded_routes():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "search_route_test")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "search route ok" in r.stdout
