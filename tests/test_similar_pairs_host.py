"""Host side of the similar-pairs search, no GPU: the host plan (codesearch_amd/csrc/pairs_plan.hpp) through
tests/cpp/pairs_plan_test.cpp — once as an ordinary build, once under AddressSanitizer + UBSan, a stand-alone program both
times — the contract as host Python (search.pairs_above: the GPU tests' reducer) on hand-made cases, and the header, both
libraries and the Python binding agreeing on cs_index_similar_pairs."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "pairs_plan_test.cpp")


def _run(exe, env=None):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "pairs plan ok", r.stdout + r.stderr


def test_pairs_plan_cpp():
    assert os.path.exists(os.path.join(ROOT, "codesearch_amd", "csrc", "pairs_plan.hpp"))
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "pairs_plan_test")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe], check=True)
        _run(exe)


def test_pairs_plan_under_sanitizers():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "pairs_plan_asan")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", SRC, "-o", exe], check=True)
        _run(exe, dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
                       UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))


def test_pairs_above_contract():
    from codesearch_amd.search import NO_GROUP, pairs_above

    groups = {0: 7, 1: 7, 2: 3, 3: NO_GROUP, 4: NO_GROUP, 5: 3}
    look = lambda ids: [groups.get(int(i), NO_GROUP) for i in ids]
    # a symmetric table of cosines over ids 0..5; (0,1), (2,5) share a file, (3,4) are both ungrouped; three pairs tie at 0.9
    c = {(0, 1): 0.9, (0, 2): 0.9, (1, 2): 0.9, (2, 5): 0.95, (3, 4): 0.8, (0, 3): 0.5, (1, 4): 0.5, (0, 5): 0.25,
         (2, 3): float("nan"), (4, 5): float("inf"), (1, 5): float("-inf")}
    cos = lambda a, b: 1.0 if a == b else c.get((min(a, b), max(a, b)), 0.0)
    ids = list(range(6))
    # every source's list holds every id, the source itself and lower ids included: only b > a counts
    orders = {a: ([cos(a, b) for b in ids], ids) for a in ids}
    kc, ka, kb, total = pairs_above(orders, look, "all", None, 100)
    finite = [(0, 1), (0, 2), (1, 2), (2, 5), (3, 4), (0, 3), (1, 4), (0, 5)]
    zeros = [(a, b) for a in ids for b in ids if a < b and (a, b) not in c]
    assert total == len(finite) + len(zeros) == 15 - 3  # the NaN and the two infinite cosines are never pairs
    # (cosine desc, a asc, b asc): the three pairs at 0.9 come ordered by a, then b
    assert list(zip(ka, kb))[:8] == [(2, 5), (0, 1), (0, 2), (1, 2), (3, 4), (0, 3), (1, 4), (0, 5)]
    assert kc[:8] == [0.95, 0.9, 0.9, 0.9, 0.8, 0.5, 0.5, 0.25]
    assert list(zip(ka, kb))[8:] == sorted(zeros)
    # the bound is strict, None and -inf mean none
    assert pairs_above(orders, look, "all", 0.9, 100)[1:] == ([2], [5], 1)
    assert pairs_above(orders, look, "all", 0.89, 100)[3] == 4
    assert pairs_above(orders, look, "all", 0.0, 100)[3] == 8
    assert pairs_above(orders, look, "all", float("-inf"), 100) == pairs_above(orders, look, "all", None, 100)
    assert pairs_above(orders, look, "all", 1.0, 100) == ([], [], [], 0)
    # other_group: (0,1) and (2,5) are one file each; (3,4) are both ungrouped and stay
    kc, ka, kb, total = pairs_above(orders, look, "other_group", 0.4, 100)
    assert list(zip(ka, kb)) == [(0, 2), (1, 2), (3, 4), (0, 3), (1, 4)] and total == 5
    no_groups = lambda ids: [NO_GROUP] * len(ids)
    assert pairs_above(orders, no_groups, "other_group", 0.4, 100) == pairs_above(orders, look, "all", 0.4, 100)
    # truncation keeps the full total
    kc, ka, kb, total = pairs_above(orders, look, "all", 0.4, 3)
    assert list(zip(ka, kb)) == [(2, 5), (0, 1), (0, 2)] and total == 7
    # partial lists are enough when they hold every hit that matters; a pair is taken from its lower id only
    part = {0: ([0.9, 0.9], [2, 1]), 2: ([0.95, 0.9], [5, 0]), 5: ([0.95], [2])}
    assert pairs_above(part, look, "all", 0.5, 10)[1:] == ([2, 0, 0], [5, 1, 2], 3)
    assert pairs_above({}, look, "all", None, 10) == ([], [], [], 0)
    with pytest.raises(ValueError, match="mode"):
        pairs_above(orders, look, "file", None, 10)
    # numpy inputs, as the GPU tests pass them: the cosines come back with their bits
    kc, ka, kb, total = pairs_above({7: (np.array([0.5, 0.3], np.float32), np.array([8, 9], np.uint32))}, no_groups, "all",
                                    np.float32(0.25), 5)
    assert (ka, kb, total) == ([7, 7], [8, 9], 2)
    assert np.asarray(kc, np.float32).tobytes() == np.array([0.5, 0.3], np.float32).tobytes()


def test_header_libraries_and_binding_agree_on_similar_pairs(gpu_lib):
    from codesearch_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "codesearch_gpu.h")).read()
    nc = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"CS_API int32_t cs_index_similar_pairs\s*\(([^;]*?)\)\s*;", nc, re.S)
    assert m, "include/codesearch_gpu.h does not declare cs_index_similar_pairs"
    args = [a.strip() for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["h", "min_cos", "mode", "max_pairs", "out_a", "out_b", "out_cos",
                                                        "out_total"]
    res, argtypes = _lib.SIGNATURES["cs_index_similar_pairs"]
    assert res is ctypes.c_int32 and len(argtypes) == len(args)
    assert argtypes[1] is ctypes.c_float and argtypes[2] is ctypes.c_int32 and argtypes[3] is ctypes.c_uint32
    assert argtypes[7] is _lib.u64p
    for name in ("cs_index_similar_pairs", "cs_index_similar_pairs_info"):
        assert name in _lib.SIGNATURES
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
        assert hasattr(ctypes.CDLL(_lib.DIAG_LIB_PATH, mode=ctypes.RTLD_LOCAL), name)
    assert re.search(r"#define\s+CS_MAX_PAIRS\s+4194304u", hdr) and _lib.CS_MAX_PAIRS == 4194304 == 1 << 22
    for name, value in (("ALL", 0), ("OTHER_GROUP", 1)):
        assert re.search(r"#define\s+CS_PAIRS_%s\s+%d\b" % (name, value), hdr)
        assert getattr(_lib, "CS_PAIRS_" + name) == value
    wrapper = open(os.path.join(ROOT, "codesearch_amd", "host", "codesearch_gpu.hpp")).read()
    assert "cs_index_similar_pairs(" in wrapper
    assert "cs_index_similar_pairs" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert gpu_lib.cs_abi_version() == 6  # only declarations were added
