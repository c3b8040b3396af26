"""Host side of the scoped similar-pairs search, no GPU: the host plan (codesearch_amd/csrc/pairs_scoped_plan.hpp) through
tests/cpp/pairs_scoped_plan_test.cpp — once as an ordinary build, once under AddressSanitizer + UBSan, a stand-alone program
both times — the rule as host Python (search.pairs_between: the GPU tests' reducer) on hand-made lists, and the header, both
libraries, the Python binding, the C++ wrapper and INTEGRATION.md agreeing on cs_index_similar_pairs_scoped."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "pairs_scoped_plan_test.cpp")


def _run(exe, env=None):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "pairs scoped plan ok", r.stdout + r.stderr


def test_pairs_scoped_plan_cpp():
    assert os.path.exists(os.path.join(ROOT, "codesearch_amd", "csrc", "pairs_scoped_plan.hpp"))
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "pairs_scoped_plan_test")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe], check=True)
        _run(exe)


def test_pairs_scoped_plan_under_sanitizers():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "pairs_scoped_plan_asan")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", SRC, "-o", exe], check=True)
        _run(exe, dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
                       UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))


def test_pairs_between_rule():
    from codesearch_amd.search import pairs_between

    # an unscoped answer over ids 0..9, already in (cosine desc, a asc, b asc) order; three pairs tie at 0.95
    cos = np.array([0.99, 0.95, 0.95, 0.95, 0.93, 0.92, 0.91], np.float32)
    a = np.array([2, 0, 0, 1, 4, 3, 8], np.uint32)
    b = np.array([5, 1, 2, 2, 9, 7, 9], np.uint32)
    pairs = lambda r: list(zip(r[1].tolist(), r[2].tolist()))
    everything = range(10)
    # every id on both sides: the unscoped answer, bytes and all
    full = pairs_between(cos, a, b, everything, everything)
    assert full[3] == 7 and full[0].tobytes() == cos.tobytes() and full[1].tobytes() == a.tobytes() and full[2].tobytes() == b.tobytes()
    assert full[0].dtype == np.float32 and full[1].dtype == np.uint32 and full[2].dtype == np.uint32
    # inside one scope: both ids in it; the ties keep their (a, b) order
    inside = pairs_between(cos, a, b, [0, 1, 2, 5], [0, 1, 2, 5])
    assert pairs(inside) == [(2, 5), (0, 1), (0, 2), (1, 2)] and inside[3] == 4
    assert inside[0].tobytes() == cos[:4].tobytes()
    # disjoint scopes: one id in each, either way round (the lower id may sit in B); pairs inside a side are not reported
    A, B = [0, 1, 7, 9], [2, 3, 4, 8]
    between = pairs_between(cos, a, b, A, B)
    assert pairs(between) == [(0, 2), (1, 2), (4, 9), (3, 7), (8, 9)] and between[3] == 5
    swapped = pairs_between(cos, a, b, B, A)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(between[:3], swapped[:3])) and swapped[3] == 5
    # overlapping scopes: (0, 1) lies inside the intersection {0, 1} and comes once; (1, 2) has 1 in both and 2 in A only;
    # (2, 5) lies in A \ B entirely and is not a pair between the two
    over = pairs_between(cos, a, b, [0, 1, 2, 5], [0, 1, 9, 4])
    assert pairs(over) == [(0, 1), (0, 2), (1, 2)] and over[3] == 3
    # B a subset of A: every pair with an end in B and the other in A — inside B included
    sub = pairs_between(cos, a, b, range(6), [1, 2])
    assert pairs(sub) == [(2, 5), (0, 1), (0, 2), (1, 2)]
    # an empty side, and a side that names ids no pair carries
    for r in (pairs_between(cos, a, b, [], everything), pairs_between(cos, a, b, everything, []),
              pairs_between(cos, a, b, [100, 101], everything)):
        assert r[3] == 0 and len(r[0]) == len(r[1]) == len(r[2]) == 0
    assert pairs_between([], [], [], [1], [2])[3] == 0
    # numpy id arrays, unsorted and repeated: sets, not lists
    again = pairs_between(cos, a, b, np.array([5, 2, 1, 0, 0], np.uint32), np.array([0, 1, 2, 5], np.uint32))
    assert pairs(again) == pairs(inside)


def test_header_libraries_and_binding_agree_on_similar_pairs_scoped(gpu_lib):
    from codesearch_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "codesearch_gpu.h")).read()
    nc = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"CS_API int32_t cs_index_similar_pairs_scoped\s*\(([^;]*?)\)\s*;", nc, re.S)
    assert m, "include/codesearch_gpu.h does not declare cs_index_similar_pairs_scoped"
    args = [x.strip() for x in m.group(1).split(",")]
    assert [x.split()[-1].lstrip("*") for x in args] == ["h", "scope_a", "scope_b", "min_cos", "mode", "max_pairs", "out_a",
                                                        "out_b", "out_cos", "out_total"]
    res, argtypes = _lib.SIGNATURES["cs_index_similar_pairs_scoped"]
    assert res is ctypes.c_int32 and len(argtypes) == len(args)
    assert argtypes[3] is ctypes.c_float and argtypes[4] is ctypes.c_int32 and argtypes[5] is ctypes.c_uint32
    assert argtypes[9] is _lib.u64p
    for name in ("cs_index_similar_pairs_scoped", "cs_index_similar_pairs_scoped_info"):
        assert name in _lib.SIGNATURES
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
        assert hasattr(ctypes.CDLL(_lib.DIAG_LIB_PATH, mode=ctypes.RTLD_LOCAL), name)
    unscoped = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*#define CS_MAX_PAIRS", hdr, re.S).group(1)
    assert "No scoped" not in unscoped and "cs_index_similar_pairs_scoped" in unscoped
    wrapper = open(os.path.join(ROOT, "codesearch_amd", "host", "codesearch_gpu.hpp")).read()
    assert "cs_index_similar_pairs_scoped(" in wrapper
    assert "cs_index_similar_pairs_scoped(" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert gpu_lib.cs_abi_version() == 6  # only declarations were added


def test_other_without_scope_is_a_value_error():
    """Decided in Python before the library or a device is touched."""
    from codesearch_amd import VectorStore

    st = VectorStore.__new__(VectorStore)
    with pytest.raises(ValueError, match="other= needs scope="):
        VectorStore.similar_pairs_raw(st, 0.9, other=object())
