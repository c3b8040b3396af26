"""Host side of the scoped similar-clusters search, no GPU: the host plan (codesearch_amd/csrc/clusters_scoped_plan.hpp)
through tests/cpp/clusters_scoped_plan_test.cpp — once as an ordinary build, once under AddressSanitizer + UBSan, a
stand-alone program both times — the contract as host Python (search.pairs_between + search.clusters_of_pairs: the GPU
tests' oracle) on hand-made graphs, and the header, both libraries, the Python binding, the C++ wrapper and INTEGRATION.md
agreeing on cs_index_similar_clusters_scoped."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "clusters_scoped_plan_test.cpp")


def _run(exe, env=None):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "clusters scoped plan ok", r.stdout + r.stderr


def test_clusters_scoped_plan_cpp():
    assert os.path.exists(os.path.join(ROOT, "codesearch_amd", "csrc", "clusters_scoped_plan.hpp"))
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "clusters_scoped_plan_test")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe], check=True)
        _run(exe)


def test_clusters_scoped_plan_under_sanitizers():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "clusters_scoped_plan_asan")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", SRC, "-o", exe], check=True)
        _run(exe, dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
                       UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))


def test_plan_header_leaves_its_parents_alone():
    """The plan reuses the two parents' geometry and walk by including them."""
    text = open(os.path.join(ROOT, "codesearch_amd", "csrc", "clusters_scoped_plan.hpp")).read()
    assert '#include "clusters_plan.hpp"' in text and '#include "pairs_scoped_plan.hpp"' in text
    assert "hip/" not in text  # plain C++17


def _scoped(cos, a, b, in_a, in_b):
    """The contract: the scoped pair list reduced to components over the ids of A u B (all live here)."""
    from codesearch_amd.search import clusters_of_pairs, pairs_between

    _c, pa, pb, _n = pairs_between(cos, a, b, in_a, in_b)
    return clusters_of_pairs(sorted(set(in_a) | set(in_b)), pa, pb)


def test_scoped_clusters_contract_on_hand_made_graphs():
    from codesearch_amd.search import clusters_of_pairs

    # the store's graph over ids 0..9: a chain 0-1-2-3, a triangle 5-6-7, and 8-9
    a = np.array([0, 1, 2, 5, 5, 6, 8], np.uint32)
    b = np.array([1, 2, 3, 6, 7, 7, 9], np.uint32)
    cos = np.full(len(a), 0.95, np.float32)
    everything = list(range(10))
    # a scope of every id passed twice: the unscoped answer
    assert _scoped(cos, a, b, everything, everything) == clusters_of_pairs(everything, a, b)
    # NOT A RESTRICTION: the scope holds 0 and 2 but not 1 — unscoped they are one class, here each is alone
    unscoped = clusters_of_pairs(everything, a, b)[0]
    assert unscoped[0] == unscoped[2] == 0
    labels, clusters, members = _scoped(cos, a, b, [0, 2], [0, 2])
    assert labels == {0: 0, 2: 2} and (clusters, members) == (0, 0)
    # ... and with 1 in `other` the rectangle joins all three: 0-1 and 1-2 each have an end on either side
    labels, clusters, members = _scoped(cos, a, b, [0, 2], [1])
    assert labels == {0: 0, 1: 0, 2: 0} and (clusters, members) == (1, 3)
    # between two scopes an edge INSIDE a side connects nothing: 5-6 lies in A, only 5-7 and 6-7 cross
    labels, clusters, members = _scoped(cos, a, b, [5, 6], [7, 8])
    assert labels == {5: 5, 6: 5, 7: 5, 8: 8} and (clusters, members) == (1, 3)
    labels, clusters, members = _scoped(cos, a, b, [5, 6], [8, 9])
    assert labels == {5: 5, 6: 6, 8: 8, 9: 9} and (clusters, members) == (0, 0)
    # overlapping scopes: a vertex of both is one vertex; 1-2 lies inside the overlap and counts
    labels, clusters, members = _scoped(cos, a, b, [0, 1, 2], [1, 2, 3])
    assert labels == {0: 0, 1: 0, 2: 0, 3: 0} and (clusters, members) == (1, 4)
    # swapped arguments, and two "handles" of the same ids against one: the same answer
    assert _scoped(cos, a, b, [1, 2, 3], [0, 1, 2]) == (labels, clusters, members)
    assert _scoped(cos, a, b, [0, 1, 2, 3], list([0, 1, 2, 3])) == _scoped(cos, a, b, [0, 1, 2, 3], [0, 1, 2, 3])
    # the label is the smallest id of the component INSIDE the scopes: 2-3 without 0 and 1 is labelled 2
    labels, clusters, members = _scoped(cos, a, b, [2, 3, 4], [2, 3, 4])
    assert labels == {2: 2, 3: 2, 4: 4} and (clusters, members) == (1, 2)
    # the empty joins: a side without an id, one scope of a single id, the same single id on both sides
    for in_a, in_b in (([], [5, 6, 7]), ([5, 6, 7], []), ([6], [6])):
        labels, clusters, members = _scoped(cos, a, b, in_a, in_b)
        assert labels == {i: i for i in set(in_a) | set(in_b)} and (clusters, members) == (0, 0)


def test_header_libraries_and_binding_agree_on_similar_clusters_scoped(gpu_lib):
    from codesearch_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "codesearch_gpu.h")).read()
    nc = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"CS_API int32_t cs_index_similar_clusters_scoped\s*\(([^;]*?)\)\s*;", nc, re.S)
    assert m, "include/codesearch_gpu.h does not declare cs_index_similar_clusters_scoped"
    args = [x.strip() for x in m.group(1).split(",")]
    assert [x.split()[-1].lstrip("*") for x in args] == ["h", "scope_a", "scope_b", "min_cos", "mode", "out_ids", "out_label",
                                                        "cap", "out_n", "out_clusters", "out_members"]
    res, argtypes = _lib.SIGNATURES["cs_index_similar_clusters_scoped"]
    assert res is ctypes.c_int32 and len(argtypes) == len(args)
    assert argtypes[3] is ctypes.c_float and argtypes[4] is ctypes.c_int32 and argtypes[5] is _lib.u32p
    assert argtypes[6] is _lib.u32p and argtypes[7] is ctypes.c_uint64 and all(t is _lib.u64p for t in argtypes[8:])
    m = re.search(r"CS_API int32_t cs_index_similar_clusters_scoped_info\s*\(([^;]*?)\)\s*;", nc, re.S)
    assert m and [x.split()[-1].lstrip("*") for x in m.group(1).split(",")] == ["pack_ms", "rows_a", "rows_b", "vertices"]
    assert len(_lib.SIGNATURES["cs_index_similar_clusters_scoped_info"][1]) == 4
    for name in ("cs_index_similar_clusters_scoped", "cs_index_similar_clusters_scoped_info"):
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
        assert hasattr(ctypes.CDLL(_lib.DIAG_LIB_PATH, mode=ctypes.RTLD_LOCAL), name)
    # the unscoped call's comment no longer names the scoped form as missing, and points at it
    unscoped = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*#define CS_NO_ID", hdr, re.S).group(1)
    assert "No scoped" not in unscoped and "cs_index_similar_clusters_scoped" in unscoped
    assert "No scoped" not in hdr
    # the contract's own words: not a restriction, never refused
    scoped = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*CS_API int32_t cs_index_similar_clusters_scoped\s*\(", hdr, re.S).group(1)
    assert "NOT A RESTRICTION" in scoped and "a path through a chunk outside" in scoped and "no max_pairs" in scoped
    wrapper = open(os.path.join(ROOT, "codesearch_amd", "host", "codesearch_gpu.hpp")).read()
    assert "cs_index_similar_clusters_scoped(" in wrapper
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "pub fn cs_index_similar_clusters_scoped(" in md
    assert "cs_index_similar_clusters_scoped_info" not in md  # a diagnostic: no binding
    assert gpu_lib.cs_abi_version() == 6  # only declarations were added


def test_other_without_scope_is_a_value_error():
    """Decided in Python before the library or a device is touched."""
    from codesearch_amd import VectorStore

    st = VectorStore.__new__(VectorStore)
    with pytest.raises(ValueError, match="other= needs scope="):
        VectorStore.similar_clusters_raw(st, 0.9, other=object())
