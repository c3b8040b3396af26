"""Host side of the similar-chunk search, no GPU: the contract as host Python (search.drop_excluded: the GPU tests' ground
truth) on hand-made cases, the resolution of source ids (codesearch_amd/csrc/similar_sources.hpp) through
tests/cpp/similar_sources_test.cpp — once as an ordinary build, once under AddressSanitizer + UBSan, a stand-alone program
both times — and the header, the library and the Python binding agreeing on cs_index_search_similar."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from codesearch_amd.search import NO_GROUP, drop_excluded
from codesearch_amd.vector_store import cos_to_score, score_to_cos

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "similar_sources_test.cpp")


def _run(exe, env=None):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "similar sources ok", r.stdout + r.stderr


def test_similar_sources_cpp():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "similar_sources_test")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe], check=True)
        _run(exe)


def test_similar_sources_under_sanitizers():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "similar_sources_asan")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", SRC, "-o", exe], check=True)
        _run(exe, dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
                       UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))


def _drop(rows, src_id, src_group, mode, min_cos, k):
    """rows: (cos, id, group) already in (cosine desc, id asc) order -> kept ids."""
    cos, ids, groups = zip(*rows) if rows else ((), (), ())
    kc, ki = drop_excluded(cos, ids, groups, src_id, src_group, mode, min_cos, k)
    assert kc == [cos[ids.index(i)] for i in ki]
    return ki


def test_drop_excluded_contract():
    #        cos  id group          the source is id 4 (group 7); ids 1 and 2 tie, id 3 ties the source
    rows = [(1.0, 3, 2), (1.0, 4, 7), (0.8, 1, 7), (0.8, 2, NO_GROUP), (0.7, 9, 3), (0.6, 0, NO_GROUP), (0.5, 5, 7),
            (0.4, 6, NO_GROUP), (0.3, 8, 3)]
    every = [r[1] for r in rows]
    assert _drop(rows, 4, 7, "none", None, 20) == every               # nothing dropped: the source is there, second
    assert _drop(rows, 4, 7, "none", None, 2) == [3, 4]               # an identical row with a lower id wins the tie
    assert _drop(rows, 4, 7, "self", None, 20) == [3, 1, 2, 9, 0, 5, 6, 8]
    assert _drop(rows, 4, 7, "self", None, 2) == [3, 1]               # a tie at the k-th slot: the lower id
    assert _drop(rows, 4, 7, "file", None, 20) == [3, 2, 9, 0, 6, 8]  # the file goes, ungrouped rows stay
    assert _drop(rows, 4, 7, "file", None, 3) == [3, 2, 9]
    # a source without a group: "file" is "self" — the ungrouped rows are not one file
    assert _drop(rows, 2, NO_GROUP, "file", None, 20) == [3, 4, 1, 9, 0, 5, 6, 8]
    assert _drop(rows, 2, NO_GROUP, "file", None, 20) == _drop(rows, 2, NO_GROUP, "self", None, 20)
    # the bound is strict, and it applies after the exclusion
    assert _drop(rows, 4, 7, "self", 0.7, 20) == [3, 1, 2]
    assert _drop(rows, 4, 7, "self", 0.69, 20) == [3, 1, 2, 9]
    assert _drop(rows, 4, 7, "file", 0.6, 20) == [3, 2, 9]
    assert _drop(rows, 4, 7, "self", 1.0, 20) == []
    assert _drop(rows, 4, 7, "none", 0.99, 20) == [3, 4]
    assert _drop(rows, 4, 7, "self", float("-inf"), 20) == _drop(rows, 4, 7, "self", None, 20)
    # k larger than what is left, nothing left, nothing there
    assert _drop(rows, 4, 7, "file", None, 1000) == [3, 2, 9, 0, 6, 8]
    one_file = [(1.0 - i / 100, i, 5) for i in range(30)]
    assert _drop(one_file, 0, 5, "file", None, 10) == []
    assert _drop(one_file, 0, 5, "self", None, 10) == list(range(1, 11))
    assert _drop([], 4, 7, "self", None, 10) == []
    # a source that is not among the rows (deleted rows never are): nothing to drop by id, its group still goes
    assert _drop(rows, 77, 3, "file", None, 20) == [3, 4, 1, 2, 0, 5, 6]
    with pytest.raises(ValueError, match="mode"):
        drop_excluded([], [], [], 0, 0, "group", None, 1)
    # numpy inputs, as the GPU tests pass them: the cosines come back with their bits
    kc, ki = drop_excluded(np.array([0.5, 0.4, 0.3], np.float32), np.array([7, 8, 9], np.uint32),
                           np.array([1, 1, NO_GROUP], np.uint32), 7, 1, "file", np.float32(0.25), 5)
    assert ki == [9] and np.asarray(kc, np.float32).tobytes() == np.array([0.3], np.float32).tobytes()


def test_score_to_cos_inverts_cos_to_score():
    cos = np.array([-1.0, -0.25, 0.0, 0.5, 0.75, 1.0], np.float32)  # exact in both scales
    assert np.array_equal(score_to_cos(cos_to_score(cos)), cos)
    assert float(score_to_cos(0.95)) == pytest.approx(0.9, abs=1e-6)


def test_header_library_and_binding_agree_on_the_similar_search(gpu_lib):
    from codesearch_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "codesearch_gpu.h")).read()
    nc = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"CS_API int32_t cs_index_search_similar\s*\(([^;]*?)\)\s*;", nc, re.S)
    assert m, "include/codesearch_gpu.h does not declare cs_index_search_similar"
    args = [a.strip() for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["h", "ids", "nq", "k", "exclude", "min_cos", "out_cos", "out_ids",
                                                        "out_counts"]
    res, argtypes = _lib.SIGNATURES["cs_index_search_similar"]
    assert res is ctypes.c_int32 and len(argtypes) == len(args)
    assert argtypes[4] is ctypes.c_int32 and argtypes[5] is ctypes.c_float
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "cs_index_search_similar")
    assert hasattr(ctypes.CDLL(_lib.DIAG_LIB_PATH, mode=ctypes.RTLD_LOCAL), "cs_index_search_similar")
    for name, value in (("NONE", 0), ("SELF", 1), ("GROUP", 2)):
        assert re.search(r"#define\s+CS_SIMILAR_EXCLUDE_%s\s+%d\b" % (name, value), hdr)
        assert getattr(_lib, "CS_SIMILAR_EXCLUDE_" + name) == value
    assert gpu_lib.cs_abi_version() == 6  # only declarations were added
