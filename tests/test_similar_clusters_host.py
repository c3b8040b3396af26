"""Host side of the similar-clusters search, no GPU: the host plan (codesearch_amd/csrc/clusters_plan.hpp) through
tests/cpp/clusters_plan_test.cpp — once as an ordinary build, once under AddressSanitizer + UBSan, a stand-alone program
both times — the contract as host Python (search.clusters_of_pairs: the GPU tests' reducer) on hand-made graphs, and the
header, both libraries, the Python binding, the C++ wrapper and INTEGRATION.md agreeing on cs_index_similar_clusters."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "clusters_plan_test.cpp")


def _run(exe, env=None):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "clusters plan ok", r.stdout + r.stderr


def test_clusters_plan_cpp():
    assert os.path.exists(os.path.join(ROOT, "codesearch_amd", "csrc", "clusters_plan.hpp"))
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "clusters_plan_test")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe], check=True)
        _run(exe)


def test_clusters_plan_under_sanitizers():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "clusters_plan_asan")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", SRC, "-o", exe], check=True)
        _run(exe, dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
                       UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))


def test_clusters_of_pairs_contract():
    from codesearch_amd.search import clusters_of_pairs

    # no edge: everybody is its own label
    labels, clusters, members = clusters_of_pairs([3, 1, 2], [], [])
    assert labels == {1: 1, 2: 2, 3: 3} and (clusters, members) == (0, 0)
    assert clusters_of_pairs([], [], []) == ({}, 0, 0)
    # a chain given out of order: one component, labelled by its smallest id
    labels, clusters, members = clusters_of_pairs(range(10, 16), [14, 12, 10, 13, 11], [15, 13, 11, 14, 12])
    assert set(labels.values()) == {10} and (clusters, members) == (1, 6)
    # a star around its largest id, and a second component; 7 stays alone
    live = [0, 1, 2, 3, 4, 5, 6, 7, 9]
    labels, clusters, members = clusters_of_pairs(live, [1, 2, 3, 5], [9, 9, 9, 6])
    assert labels == {0: 0, 1: 1, 2: 1, 3: 1, 9: 1, 4: 4, 5: 5, 6: 5, 7: 7} and (clusters, members) == (2, 6)
    # an edge twice, and once the other way round, changes nothing
    again = clusters_of_pairs(live, [1, 2, 3, 5, 9, 2, 6], [9, 9, 9, 6, 1, 9, 5])
    assert again == (labels, clusters, members)
    # two components joined late by one edge between their largest members: the smaller label wins everywhere
    labels, clusters, members = clusters_of_pairs(range(8), [0, 1, 4, 5, 2], [1, 2, 5, 6, 6])
    assert labels == {0: 0, 1: 0, 2: 0, 3: 3, 4: 0, 5: 0, 6: 0, 7: 7} and (clusters, members) == (1, 6)
    # ids that are not live are no vertices: an edge that names one is refused
    with pytest.raises(ValueError, match="not live"):
        clusters_of_pairs([0, 1, 3], [1], [2])
    with pytest.raises(ValueError, match="not live"):
        clusters_of_pairs([0, 1, 3], [7], [1])
    # numpy inputs, as the GPU tests pass them
    labels, clusters, members = clusters_of_pairs(np.arange(100, 105, dtype=np.uint32), np.array([101], np.uint32),
                                                  np.array([104], np.uint32))
    assert labels == {100: 100, 101: 101, 102: 102, 103: 103, 104: 101} and (clusters, members) == (1, 2)
    assert all(type(k) is int and type(v) is int for k, v in labels.items())


def test_header_libraries_and_binding_agree_on_similar_clusters(gpu_lib):
    from codesearch_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "codesearch_gpu.h")).read()
    nc = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"CS_API int32_t cs_index_similar_clusters\s*\(([^;]*?)\)\s*;", nc, re.S)
    assert m, "include/codesearch_gpu.h does not declare cs_index_similar_clusters"
    args = [a.strip() for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["h", "min_cos", "mode", "out_label", "n_labels", "out_clusters",
                                                        "out_members"]
    res, argtypes = _lib.SIGNATURES["cs_index_similar_clusters"]
    assert res is ctypes.c_int32 and len(argtypes) == len(args)
    assert argtypes[1] is ctypes.c_float and argtypes[2] is ctypes.c_int32 and argtypes[3] is _lib.u32p
    assert argtypes[4] is ctypes.c_uint64 and argtypes[5] is _lib.u64p and argtypes[6] is _lib.u64p
    m = re.search(r"CS_API int32_t cs_index_similar_clusters_info\s*\(([^;]*?)\)\s*;", nc, re.S)
    assert m and len(m.group(1).split(",")) == len(_lib.SIGNATURES["cs_index_similar_clusters_info"][1]) == 6
    for name in ("cs_index_similar_clusters", "cs_index_similar_clusters_info"):
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
        assert hasattr(ctypes.CDLL(_lib.DIAG_LIB_PATH, mode=ctypes.RTLD_LOCAL), name)
    assert re.search(r"#define\s+CS_NO_ID\s+0xFFFFFFFFu", hdr) and _lib.CS_NO_ID == 0xFFFFFFFF
    wrapper = open(os.path.join(ROOT, "codesearch_amd", "host", "codesearch_gpu.hpp")).read()
    assert "cs_index_similar_clusters(" in wrapper
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "pub fn cs_index_similar_clusters(" in md and "cs_index_similar_clusters_info" not in md  # a diagnostic: no binding
    assert gpu_lib.cs_abi_version() == 6  # only declarations were added
