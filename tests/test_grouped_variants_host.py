"""Host side of the grouped scoped and grouped variants searches, no GPU: the capped variants merge of
codesearch_amd/csrc/grouped_plan.hpp through tests/cpp/grouped_variants_test.cpp — once as an ordinary build, once as the
same stand-alone program under AddressSanitizer + UBSan — the contract as host Python (search.merge_variants_capped,
search.high_confidence: the GPU tests' ground truth) on hand-made cases, and the argument rule of the Python store."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from codesearch_amd.search import NO_GROUP, cap_per_group, high_confidence, merge_variants_capped

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "grouped_variants_test.cpp")
FLAGS = ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"]


def _build_and_run(extra, env=None):
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "grouped_variants_test")
        subprocess.run(["g++"] + FLAGS + extra + [SRC, "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "grouped variants ok", r.stdout + r.stderr


def test_grouped_variants_cpp():
    _build_and_run([])


def test_grouped_variants_cpp_under_sanitizers():
    _build_and_run(["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"],
                   dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
                        UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))


def _groups(table):
    return lambda ids: [table.get(int(i), NO_GROUP) for i in ids]


def test_merge_variants_capped_contract():
    g = _groups({1: 7, 2: 7, 3: 7, 4: 3, 5: 3})
    a = ([0.9, 0.8, 0.7, 0.6, 0.5, 0.4], [1, 2, 3, 4, 5, 6])       # one variant, full order
    b = ([0.95, 0.85, 0.6, 0.55, 0.3, 0.2], [3, 5, 4, 6, 1, 2])    # another: other best cosines for 3, 5 and 6
    # best per id: 3 -> .95, 1 -> .9, 5 -> .85, 2 -> .8, 4 -> .6, 6 -> .55
    assert merge_variants_capped([a, b], g, 10, 10) == ([0.95, 0.9, 0.85, 0.8, 0.6, 0.55], [3, 1, 5, 2, 4, 6])
    assert merge_variants_capped([a, b], g, 10, 1) == ([0.95, 0.85, 0.55], [3, 5, 6])   # ungrouped 6 is never capped
    assert merge_variants_capped([a, b], g, 10, 2) == ([0.95, 0.9, 0.85, 0.6, 0.55], [3, 1, 5, 4, 6])
    assert merge_variants_capped([a, b], g, 2, 2) == ([0.95, 0.9], [3, 1])                # stop at k
    assert merge_variants_capped([a, a], g, 3, 1) == merge_variants_capped([a], g, 3, 1) == ([0.9, 0.6, 0.4], [1, 4, 6])
    assert merge_variants_capped([a], g, 4, 2) == tuple(cap_per_group(a[0], a[1], g(a[1]), 4, 2))
    assert merge_variants_capped([], g, 4, 2) == ([], [])
    # a tie across ids after the merge: the lower id first
    t = merge_variants_capped([([0.5, 0.4], [9, 8]), ([0.5, 0.1], [8, 9])], _groups({}), 5, 1)
    assert t == ([0.5, 0.5], [8, 9])
    # capping the merged UNCAPPED lists is not the contract: top-2 per variant, k = 2, one row per group
    v = ([0.9, 0.8, 0.7], [1, 2, 4])
    full = merge_variants_capped([v, v], g, 2, 1)
    assert full == ([0.9, 0.7], [1, 4])
    cut = ([0.9, 0.8], [1, 2])
    assert merge_variants_capped([cut, cut], g, 2, 1) == ([0.9], [1])
    # numpy inputs keep their float32 bits
    c = np.array([0.3, 0.2], np.float32)
    kc, ki = merge_variants_capped([(c, np.array([5, 4], np.uint32))], g, 5, 1)
    assert ki == [5] and np.asarray(kc, np.float32).tobytes() == c[:1].tobytes()


def test_high_confidence_predicate():
    assert high_confidence([1.0, 0.9, 0.8, 0.75, 0.71])          # distance (1 - c) / 2 < 0.15  <=>  c > 0.7
    assert not high_confidence([1.0, 0.9, 0.8, 0.75, 0.69])
    assert high_confidence([1.0, 0.9, 0.8, 0.75, 0.71, 0.0])     # only the first five count
    assert high_confidence([0.99])                               # fewer than five: all of them
    assert not high_confidence([])
    assert not high_confidence([0.7])                            # (1 - 0.7) / 2 is not below 0.15 in float32


def test_per_file_goes_with_a_scope_but_not_with_chunk_ids():
    from codesearch_amd.vector_store import _filters_ok, _one_of

    _filters_ok(None, None, None)
    _filters_ok(None, object(), 3)      # the new pair
    _filters_ok(None, object(), None)
    _filters_ok([1], None, None)
    _filters_ok(None, None, 2)
    with pytest.raises(ValueError, match="exclusive"):
        _filters_ok([1], None, 3)
    with pytest.raises(ValueError, match="exclusive"):
        _filters_ok([1], object(), 3)
    with pytest.raises(ValueError, match="exclusive"):
        _filters_ok([1], object(), None)
    # _one_of itself is what it was
    _one_of(None, None, 3)
    _one_of([1], None, None)
    with pytest.raises(ValueError, match="exclusive"):
        _one_of([1], None, 3)
    with pytest.raises(ValueError, match="exclusive"):
        _one_of(None, object(), 1)
